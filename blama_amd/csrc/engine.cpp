// Engine host code: the decode context -- its buffers, the batch-1 decode schedule captured
// into HIP graphs, sampling reads, the KV cache and state (the model: model.cpp; prompt batches:
// batch.cpp).
//
// Reference anchors (the llama.h functions this replaces):
//   llama_init_from_model       /root/reference/inference/code/llama/Instance.cpp:36
//   llama_decode                /root/reference/inference/code/llama/Session.cpp:388
//   llama_get_logits_ith        /root/reference/inference/code/llama/Session.cpp:24
//   llama_kv_self_*             /root/reference/inference/code/llama/Session.cpp:53,341-361
//   llama_state_*               /root/reference/inference/code/llama/Session.cpp:291-304
//   llama_apply_adapter_cvec    /root/reference/inference/code/llama/Instance.cpp:74
//   llama_set_adapter_lora      /root/reference/inference/code/llama/Instance.cpp:52-61 (lora.cpp)
//   llama_get_embeddings_ith    /root/reference/inference/code/llama/InstanceEmbedding.cpp:24-32,113-164
#include "engine.h"

#include <atomic>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>

namespace mi {

// =============================================================== context ===
namespace {
struct DevChain {
    std::mutex mu;
    std::atomic<int> nctx{0};  // live contexts on the device (attention co-residency budget)
};
DevChain& dev_chain(int device) {
    static std::mutex mu;
    static std::map<int, std::unique_ptr<DevChain>> chains;
    std::lock_guard<std::mutex> lk(mu);
    auto& c = chains[device];
    if (!c) c.reset(new DevChain());
    return *c;
}
const char* const kEmbdMode = "the context is in embeddings mode: no logits (mi_ctx_set_embeddings)";
// unspecified pooling: the model's {arch}.pooling_type when it names a type served here, else NONE
int model_pooling(const HParams& hp) {
    return hp.pooling_type >= MI_POOLING_NONE && hp.pooling_type < MI_POOLING_RANK ? hp.pooling_type : MI_POOLING_NONE;
}
}  // namespace
int dev_chain_contexts(int device) { return dev_chain(device).nctx.load(); }

int act_fmt(std::initializer_list<int> types) {
    int f = 0;
    for (int t : types) f |= takes_q80(t) ? 2 : 1;
    return f;
}

void ensure_kernel_attributes(int device) {
    static std::vector<int> done(64, 0);
    if (device >= 0 && device < (int)done.size() && !done[device]) {
        init_kernel_attributes();
        done[device] = 1;
    }
}

int mmqs_token_limit() {
    const char* e = getenv("MI_MMQS_MAX");
    return e ? std::min(MMQS_MAX, std::max(0, atoi(e))) : MMQS_MAX;
}

GemvSeg seg_of(const QMat& A, int pair, int epi, float* out) {
    GemvSeg g;
    std::memset(&g, 0, sizeof(g));
    g.A = A;
    g.B = A;
    g.pair = pair;
    g.epi = epi;
    g.expA = g.expB = -1;
    g.out = out;
    return g;
}

void moe_gate_up_segs(GemvParams& p, const QMat& gate, const QMat& up, const int* sel, const float* selw, float* h,
                      float* h2) {
    p.sel = sel;   // expert ids/weights: only MoE launches wait for them
    p.selw = selw;
    p.nseg = 2;
    for (int k = 0; k < 2; ++k) {
        p.seg[k] = seg_of(gate, PAIR_AB, EPI_SWIGLU, k == 0 ? h : h2);
        p.seg[k].B = up;
        p.seg[k].expA = p.seg[k].expB = k;
    }
}

void moe_down_seg(GemvParams& p, const QMat& down, const int* sel, const float* selw, const float* h2, float* x,
                  const float* addend) {
    p.sel = sel;
    p.selw = selw;
    p.nslots = 2;
    p.x[1] = h2;
    p.nseg = 1;
    p.seg[0] = seg_of(down, PAIR_AB, EPI_MOE_DOWN, x);
    p.seg[0].expA = 0;
    p.seg[0].expB = 1;
    p.seg[0].actB = 1;
    p.seg[0].resid = x;
    p.seg[0].addend = addend;
}

// ---- CtxMem ----
void* CtxMem::dev_bytes(size_t bytes, bool zero) {
    dev_ptrs.reserve(dev_ptrs.size() + 1);   // (no throw between the allocation and its record)
    void* p = nullptr;
    MI_HIP(hipMalloc(&p, bytes));
    dev_ptrs.push_back(p);
    if (zero) MI_HIP(hipMemset(p, 0, bytes));
    return p;
}
void* CtxMem::host_bytes(size_t bytes, unsigned flags) {
    host_ptrs.reserve(host_ptrs.size() + 1);
    void* p = nullptr;
    MI_HIP(hipHostMalloc(&p, bytes, flags));
    host_ptrs.push_back(p);
    return p;
}
void CtxMem::free_one(void* p) {
    if (!p) return;
    auto d = std::find(dev_ptrs.begin(), dev_ptrs.end(), p);
    if (d != dev_ptrs.end()) {
        dev_ptrs.erase(d);
        hipFree(p);
        return;
    }
    auto h = std::find(host_ptrs.begin(), host_ptrs.end(), p);
    if (h == host_ptrs.end()) throw Error("CtxMem: not a buffer of this context");
    host_ptrs.erase(h);
    hipHostFree(p);
}
hipStream_t CtxMem::stream() {
    if (!stream_) MI_HIP(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
    return stream_;
}
hipEvent_t CtxMem::event() {
    events.reserve(events.size() + 1);
    hipEvent_t e = nullptr;
    MI_HIP(hipEventCreate(&e));
    events.push_back(e);
    return e;
}
CtxMem::~CtxMem() {
    for (hipEvent_t e : events) hipEventDestroy(e);
    for (void* p : dev_ptrs) hipFree(p);
    for (void* p : host_ptrs) hipHostFree(p);
    if (stream_) hipStreamDestroy(stream_);
}

Ctx::Ctx(Model* model, uint32_t nctx, uint32_t nbatch, uint32_t nubatch) : m(model) {
    if (m->vocab_only) throw Error("cannot create a context on a vocab-only model");
    device = m->device;
    MI_HIP(hipSetDevice(device));
    n_ctx = nctx ? nctx : (uint32_t)m->hp.n_ctx_train;
    n_batch = std::min(nbatch ? nbatch : 2048u, n_ctx);   // "may be silently truncated to ctxSize"
    n_ubatch = nubatch ? std::min(nubatch, n_batch) : n_batch;
    const HParams& hp = m->hp;
    kv_dim = hp.n_head_kv * hp.head_dim;
    pooling = model_pooling(hp);
    ensure_kernel_attributes(device);
    stream = mem.stream();
    if (hp.arch == ARCH_BERT) {   // an encoder context: no KV cache, no decode step (enc.cpp)
        enc_init();
        dev_chain(device).nctx++;
        return;
    }
    const size_t kvn = (size_t)hp.n_layer * n_ctx * kv_dim;
    kcache = mem.dev<__half>(kvn);
    vcache = mem.dev<__half>(kvn);
    MI_HIP(hipMemset(kcache, 0, kvn * sizeof(__half)));
    MI_HIP(hipMemset(vcache, 0, kvn * sizeof(__half)));
    cell_pos = mem.dev<int>(n_ctx, true);
    tokpos = mem.dev<int>(4, true);
    const int big = std::max(hp.n_embd, hp.n_ff);
    x = mem.dev<float>(hp.n_embd);
    q = mem.dev<float>(hp.n_embd);
    attn = mem.dev<float>(hp.n_embd);
    h = mem.dev<float>(big);
    h2 = mem.dev<float>(big);
    logits = mem.dev<float>(hp.n_vocab);
    cand = mem.dev<unsigned long long>((size_t)topk_blocks(hp.n_vocab) * TOPK_MAX);
    part_o = mem.dev<float>((size_t)ATTN_SMAX * hp.n_head * hp.head_dim);
#ifdef MI_STAMPS
    stamps = mem.dev<unsigned long long>((size_t)kStampLaunches * kStampWgs * 8, true);
#endif
    const bool gpt2 = hp.arch == ARCH_GPT2;
    batch_ok = getenv("MI_NO_BATCH") == nullptr;
    // GPT-2: physical batches on the tiled int8-MFMA GEMM only (ubatch_gpt2), for a model whose four
    // matrices per layer are mmq32-capable and whose fused attn_qkv splits into whole row tiles;
    // any other GPT-2 model keeps one decode step per token
    if (gpt2) {
        batch_ok = batch_ok && getenv("MI_NO_MMQ") == nullptr && hp.n_embd % 32 == 0 && hp.n_ff % 32 == 0 &&
                   kv_dim == hp.n_embd;
        for (const Layer& L : m->layers)
            for (const QMat* q : {&L.qkv[0], &L.wo, &L.up, &L.down}) batch_ok = batch_ok && mmq32_supported(q->type);
    }
    if (batch_ok) {
        // MFMA batch path (decode_ubatch / mmq32) when every layer matrix is mmq32-capable (each
        // matrix reads the activation format of its type: Q8_0 activations for Q8_0 weights, Q8_K
        // for the k-quants); otherwise prompt chunks on the v_dot4 GEMM (decode_batch, dense only)
        mmq_ok = getenv("MI_NO_MMQ") == nullptr;
        bool any_k = false, any_0 = false;
        for (const Layer& L : m->layers)
            for (const QMat* q : {&L.wq, &L.wk, &L.wv, &L.wo, &L.gate, &L.up, &L.down}) {
                mmq_ok = mmq_ok && mmq32_supported(q->type);
                (takes_q80(q->type) ? any_0 : any_k) = true;
            }
        // the gate/up pair shares one MFMA-order copy (16 gate + 16 up rows per tile)
        for (const Layer& L : m->layers)
            mmq_ok = mmq_ok && L.gate.type == L.up.type && L.gate.rows == L.up.rows;
        const int NB = kBatchRows;
        // MoE: a row per (token, slot), each expert's rows padded to whole 32-row tiles
        const int hrows = hp.n_expert > 0 ? moe_rows_cap(NB * hp.n_expert_used, hp.n_expert) : NB;
        xb = mem.dev<float>((size_t)NB * hp.n_embd);
        qb = mem.dev<float>((size_t)NB * hp.n_embd);
        attnb = mem.dev<float>((size_t)NB * hp.n_embd);
        hb = mem.dev<float>((size_t)hrows * hp.n_ff);
        tokpos_b = mem.dev<int>((size_t)NB * 4);
        h_tokpos_b = mem.host<int>((size_t)kTokbRing * NB * 4);
        const int kmax = std::max(hp.n_embd, hp.n_ff);
        if (mmq_ok) {
            // ub_q / ub_dT / ub_bsb: the k-quant (Q8_K) activations, or the Q8_0 ones when every
            // matrix is Q8_0; a model mixing both (Mixtral's Q8_0 attn_k / attn_v) has a second
            // set ub_q0 / ub_dT0 for Q8_0
            ub_q80 = !any_k;
            // no room for the copy: prompt batches fall back to the v_dot4 GEMM
            mmq_ok = m->ensure_mmq_copies();
            out_mmq = mmq_ok && mmq32_supported(m->output.type);
            attn_mfma = attn_mfma_supported(hp.head_dim);
            ub_q = mem.dev<int8_t>((size_t)UB_MAX * kmax);
            ub_dT = mem.dev<float>((size_t)UB_MAX * (kmax / 32));   // Q8_0: per 32
            ub_bsb = mem.dev<int8_t>((size_t)UB_MAX * (kmax / 256) * 16);
            if (any_k && any_0) {
                ub_q0 = mem.dev<int8_t>((size_t)UB_MAX * kmax);
                ub_dT0 = mem.dev<float>((size_t)UB_MAX * (kmax / 32));
            }
            if (hp.n_expert > 0) {   // routing of a physical batch, grouped rows, expert down outputs
                if (hp.n_expert > MOE_GROUP_MAXE) throw Error("MoE prompt batches: at most 16 experts");
                const int ns = NB * hp.n_expert_used;
                const int cap = moe_rows_cap(ns, hp.n_expert);
                yb = mem.dev<float>((size_t)cap * hp.n_embd);
                sel_b = mem.dev<int>(ns);
                selw_b = mem.dev<float>(ns);
                moe_rows = mem.dev<int>(cap);
                moe_rowsel = mem.dev<int>(cap);
                moe_pos = mem.dev<int>(ns);
                moe_grp = mem.dev<int>(2 * MOE_GROUP_MAXE + 1);
                moe_q = mem.dev<int8_t>((size_t)cap * kmax);
                moe_dT = mem.dev<float>((size_t)cap * (kmax / 32));
                moe_bsb = mem.dev<int8_t>((size_t)cap * (kmax / 256) * 16);
            }
            ub_rope = mem.dev<float2>((size_t)UB_MAX * std::max(1, hp.n_rot / 2));
            // split-K partials of the residual GEMMs (WO, FFN down) of dense models
            // (GPT-2: no split-K, no short-batch form -- every batch on the tiled GEMM)
            if (!gpt2) ub_part = mem.dev<float>((size_t)2 * UB_MAX * hp.n_embd);
            mmqs_max = gpt2 ? 0 : mmqs_token_limit();
            // MoE: short batches when every expert matrix has the grouped form (k-quants)
            moe_short = hp.n_expert > 0;
            for (const Layer& L : m->layers)
                moe_short = moe_short && mmqs_grouped_supported(L.gate.type) && L.up.type == L.gate.type &&
                            mmqs_grouped_supported(L.down.type);
            if (mmqs_max > 0 && (hp.n_expert == 0 || moe_short)) {
                const size_t qkv = (size_t)hp.n_embd + 2 * (size_t)kv_dim;
                size_t per = std::max({(size_t)mmqs_parts(hp.n_embd) * std::max({qkv, (size_t)hp.n_embd, 2 * (size_t)hp.n_ff}),
                                       (size_t)mmqs_parts(hp.n_ff) * hp.n_embd});
                if (out_mmq) per = std::max(per, (size_t)mmqs_parts(hp.n_embd) * hp.n_vocab);
                size_t tot = per * MMQS_MAX;
                if (moe_short)   // the experts' parts over the MoE rows of MMQS_MAX tokens
                    tot = std::max(tot, std::max((size_t)mmqs_parts(hp.n_embd) * 2 * hp.n_ff, (size_t)mmqs_parts(hp.n_ff) * hp.n_embd) *
                                            (size_t)moe_rows_cap(MMQS_MAX * hp.n_expert_used, hp.n_expert));
                ub_spart = mem.dev<float>(tot);
            } else {
                moe_short = false;
                mmqs_max = 0;
            }
        }
        // MoE prompts need the MFMA path (the v_dot4 GEMM has no routed-expert form)
        // (and so do GPT-2 prompts: no copy, no batch -- the per-token loop)
        if ((hp.n_expert > 0 || gpt2) && !mmq_ok) batch_ok = false;
    }
    if (m->f16) f16_init();
    attn_smax = mem.dev<float>((size_t)ATTN_SMAX * hp.n_head);
    attn_scores = mem.dev<float>((size_t)hp.n_head * n_ctx);
    attn_xflags = mem.dev<unsigned>((size_t)hp.n_head * ATTN_SMAX * 32, true);
    attn_xmax = mem.dev<float>((size_t)hp.n_head * ATTN_SMAX);
    attn_xsum = mem.dev<double>((size_t)hp.n_head * ATTN_SMAX);
    step_ctr = mem.dev<unsigned>(4, true);
    const unsigned mapped = hipHostMallocMapped | hipHostMallocCoherent;
    h_attn_xerr = mem.host<unsigned>(4, mapped);
    *h_attn_xerr = 0;
    MI_HIP(hipHostGetDevicePointer(reinterpret_cast<void**>(&d_attn_xerr), h_attn_xerr, 0));
    topk_ids = mem.dev<int>(TOPK_MAX);
    topk_vals = mem.dev<float>(TOPK_MAX);
    sel = mem.dev<int>(64, true);
    selw = mem.dev<float>(64, true);
    gather_ids = mem.dev<int>(4096);
    gather_out = mem.dev<float>(4096);
    cell_delta = mem.dev<int>(n_ctx);
    move_src = mem.dev<int>(n_ctx);
    h_tokpos = mem.host<int>(kTokRing * 4);
    // the top-k kernel writes its result straight into these (coherent, mapped)
    h_topk_ids = mem.host<int>(TOPK_MAX, mapped);
    h_topk_vals = mem.host<float>(TOPK_MAX, mapped);
    MI_HIP(hipHostGetDevicePointer(reinterpret_cast<void**>(&d_h_topk_ids), h_topk_ids, 0));
    MI_HIP(hipHostGetDevicePointer(reinterpret_cast<void**>(&d_h_topk_vals), h_topk_vals, 0));
    h_logits = mem.host<float>(hp.n_vocab);
    h_gather = mem.host<float>(4096);
    h_cell_pos.assign(n_ctx, 0);
    sp_ok = sp_setup();
    dev_chain(device).nctx++;   // last: a constructor that throws leaves the count as it was
}

Ctx::~Ctx() {
    dev_chain(device).nctx--;
    hipSetDevice(device);
    if (stream) hipStreamSynchronize(stream);
    invalidate_graphs();
}   // (mem releases the events, the buffers and the stream)

void Ctx::invalidate_graphs() {
    for (int m = 0; m < 2; ++m) {
        for (hipGraphExec_t* g : {&g_full[m], &g_nolog[m], &g_embd[m], &g_seg[m][0], &g_seg[m][1], &g_seg[m][2]}) {
            if (*g) hipGraphExecDestroy(*g);
            *g = nullptr;
        }
    }
}

void Ctx::set_down_quant(int form) {
    if (!sp_ok || m->hp.n_expert > 0) throw Error("down_quant: no streaming dense decode step in this context");
    if (form < HQ_LAUNCH || form > HQ_WG16) throw Error("down_quant: form");
    MI_HIP(hipSetDevice(device));
    sync();
    std::vector<SpLayer> old = sp;
    for (SpLayer& b : sp) b.hq = form;
    for (int l = 0; l < m->hp.n_layer; ++l)
        if (!dgemv_supported(down_params_sp(l))) {
            sp = std::move(old);
            throw Error("down_quant: no compiled variant for this form");
        }
    invalidate_graphs();    // the next step re-captures with the other launches
}

void Ctx::apply_cvec(const float* data, size_t len, int n_embd, int il_start, int il_end) {
    const HParams& hp = m->hp;
    if (enc) throw Error("apply_cvec: encoder models take no control vector");
    if (data && n_embd != hp.n_embd) throw Error("apply_cvec: the control vector's n_embd differs from the model's");
    MI_HIP(hipSetDevice(device));
    sync();                 // steps in flight still read the old rows
    invalidate_graphs();    // the next step re-captures with the new arguments
    cvec_on.clear();
    if (!data) return;
    std::vector<char> on(hp.n_layer, 0);
    bool any = false;
    for (int il = std::max(1, il_start); il < hp.n_layer && il <= il_end; ++il)
        if ((size_t)il * hp.n_embd <= len) on[il] = 1, any = true;
    if (!any) return;
    if (!cvec) cvec = mem.dev<float>((size_t)hp.n_layer * hp.n_embd, true);
    for (int il = 1; il < hp.n_layer; ++il)
        if (on[il])
            MI_HIP(hipMemcpy(cvec + (size_t)il * hp.n_embd, data + (size_t)(il - 1) * hp.n_embd,
                             (size_t)hp.n_embd * sizeof(float), hipMemcpyHostToDevice));
    cvec_on = std::move(on);
}

long long Ctx::ffn_bytes() const {
    if (enc) return 0;
    const Layer& L = m->layers[0];
    auto mb = [](const QMat& q) {
        if (q.type == T_F16) return (long long)q.rows * q.K * 2;
        return (long long)q.rows * q.nb * ((long long)block_bytes(q.type) * 256 / block_elems(q.type));
    };
    const HParams& hp = m->hp;
    const long long w = hp.n_expert > 0 ? 2 * (mb(L.gate) + mb(L.up)) : mb(L.gate) + mb(L.up);
    if (sp_ok)   // streaming path: x and the norm weight read (by every workgroup, L2-served), h written
        return w + (long long)hp.n_embd * 4 * 2 + (long long)hp.n_ff * 4;
    const long long act = (long long)hp.n_embd * 4 * 2 + (long long)hp.n_ff * 4 * (hp.n_expert > 0 ? 2 : 1);
    return w + act;   // weights + x and norm weight read + h written
}

// ======================================================== decode launches ===
// The parameter block of every launch of a batch-1 decode step for the token in tokpos.  Both
// steps (the streaming one on dgemv_kernel, the r04 one on gemv_kernel), both architectures and
// sp_setup's dry check build their launches here; a GPT-2 layer (llm_build_gpt2) is the LLaMA one
// with LayerNorm for RMSNorm, projection biases, no RoPE and up -> GELU for the gate/up pair.
GemvParams Ctx::gemv_base() const {
    GemvParams p;
    std::memset(&p, 0, sizeof(p));
    p.tokpos = tokpos;
    p.cell_pos = cell_pos;
    p.head_dim = m->hp.head_dim;
    p.kv_dim = kv_dim;
    p.eps = m->hp.eps;
    p.nslots = 1;
    return p;
}

ActOut Ctx::act_out(int role, int fmt, int K, const float* norm_w) const {
    return ActOut{K, fmt & 1, fmt >> 1, sp_act[role], norm_w, m->hp.eps};
}

// How p's activation arrives: quantised at sp_act[role], or the fp32 row xin (normed with norm_w /
// norm_b when set) through gemv_kernel's prologue or quantised in the dgemv launch itself.  fmt:
// the formats the launch's matrices read (dgemv).
void Ctx::set_act(GemvParams& p, ActSrc src, int role, int fmt, const float* xin, const float* norm_w,
                  const float* norm_b) const {
    if (src == ACT_QUANT) {
        p.act_in = sp_act[role];
    } else {
        p.x[0] = xin;
        p.norm_w = norm_w;
    }
    if (src == ACT_PRO) {
        p.pro = !norm_w ? PRO_PLAIN : m->hp.arch == ARCH_GPT2 ? PRO_LAYERNORM : PRO_RMSNORM;
        p.norm_b = norm_b;
    } else {
        p.act_q8k = fmt & 1;
        p.act_q80 = fmt >> 1;
    }
}

// Q/K/V projections + RoPE + KV append: one launch per pair of row groups a kernel variant can carry
int Ctx::qkv_params(int l, ActSrc src, GemvParams out[3]) const {
    const HParams& hp = m->hp;
    const Layer& L = m->layers[l];
    GemvParams p = gemv_base();
    p.K = hp.n_embd;
    set_act(p, src, 0, src == ACT_PRO ? 0 : sp[l].fA, x, L.attn_norm, L.attn_norm_b);
    if (hp.arch == ARCH_LLAMA) {   // (GPT-2: learned positions, n_rot 0)
        p.theta_scale = theta_scale();
        p.freq_scale = hp.freq_scale;
        p.n_rot = hp.n_rot;
        p.freq_factors = m->rope_freqs;
    }
    p.kcache = k_layer(l);
    p.vcache = v_layer(l);
    int n = 0, row0 = 0;   // row0: the group's first row among [Q | K | V]
    for (int g = 0; g < L.n_qkv; ++n) {
        p.nseg = 0;
        for (; g < L.n_qkv && p.nseg < GEMV_MAX_SEG; ++g) {
            if (p.nseg == 1 && !gemv_pair_supported(p.seg[0].A.type, L.qkv[g].type)) break;
            GemvSeg& sg = p.seg[p.nseg++];
            sg = seg_of(L.qkv[g], PAIR_ADJ, EPI_QKV, q);
            sg.nq = L.qkv_nq[g];
            sg.nk = L.qkv_nk[g];
            sg.bias = L.bqkv;   // GPT-2 (its one fused group)
            // LoRA: folded into the streaming launch (ranges Q, K, V: a segment picks its own);
            // gemv_kernel adds the term precomputed in lora_pre, rows [Q | K | V]
            if (src != ACT_PRO) sg.lora = lora_fold(l, 0);
            else if (lora_group(l, 0)) sg.pre = lora_pre + row0;
            row0 += L.qkv[g].rows;
        }
        out[n] = p;
    }
    return n;
}

// Attention over the layer's cache (attn.hip; attn_plan chooses the kernel from what is set here).
// Up to ATTN_SHORT cells one launch, which for the streaming step (quant_out) also quantises its
// output for WO; past that the split kernels -- LLaMA: with the exchange of the single-launch
// attn_long_kernel -- whose partials the WO prologue (r04 step) or attn_combine_quant (streaming
// step) adds in split order.
AttnParams Ctx::attn_params(int l, bool quant_out) const {
    const HParams& hp = m->hp;
    AttnParams a{q, k_layer(l), v_layer(l), tokpos, cell_pos, attn_scores, attn_smax, part_o, hp.n_head, hp.n_head_kv,
                 hp.head_dim, kv_dim, (int)n_ctx, kq_scale()};
    a.fused = attn_fused;
    if (attn_fused) {
        if (quant_out) a.act_out = act_out(1, sp[l].fB, hp.n_embd, nullptr);
    } else if (hp.arch == ARCH_LLAMA) {
        a.xflags = attn_xflags;
        a.xmax = attn_xmax;
        a.xsum = attn_xsum;
        a.step = step_ctr;
        a.layer = l;
        a.n_layer = hp.n_layer;
        a.xerr = d_attn_xerr;
        a.long_share = dev_chain(device).nctx.load();
        a.long_off = attn_long_off ? 1 : 0;
    }
    return a;
}

// output projection + residual, in place (ACT_PRO: the prologue adds the attention splits)
GemvParams Ctx::wo_params(int l, ActSrc src) const {
    const HParams& hp = m->hp;
    const Layer& L = m->layers[l];
    GemvParams p = gemv_base();
    p.K = hp.n_embd;
    if (src == ACT_PRO) {
        p.pro = PRO_ATTN;
        p.attn = AttnPartials{part_o, hp.n_head, hp.head_dim};
        p.attn_nsplit = attn_fused ? 1 : 0;   // the split graph reads the count from the cell count
    } else {
        set_act(p, ACT_QUANT, 1, sp[l].fB, nullptr, nullptr, nullptr);
    }
    p.nseg = 1;
    p.seg[0] = seg_of(L.wo, PAIR_ADJ, EPI_ADD, x);
    p.seg[0].resid = x;
    p.seg[0].bias = L.bo;
    if (src != ACT_PRO) p.seg[0].lora = lora_fold(l, 1);   // LoRA: before the residual add
    else if (lora_group(l, 1)) p.seg[0].pre = lora_pre;
    return p;
}

// FFN gate/up + SwiGLU into h (MoE, ACT_PRO only: the two routed experts into h and h2; GPT-2:
// up + bias + GELU)
GemvParams Ctx::gate_up_params(int l, ActSrc src) const {
    const HParams& hp = m->hp;
    const Layer& L = m->layers[l];
    GemvParams p = gemv_base();
    p.K = hp.n_embd;
    set_act(p, src, 2, src == ACT_PRO ? 0 : sp[l].fC, x, L.ffn_norm, L.ffn_norm_b);
    if (hp.arch == ARCH_GPT2) {
        p.gelu_tab = m->gelu_tab;
        p.nseg = 1;
        p.seg[0] = seg_of(L.up, PAIR_ADJ, EPI_GELU, h);
        p.seg[0].bias = L.bup;
        return p;
    }
    if (hp.n_expert > 0) {
        moe_gate_up_segs(p, L.gate, L.up, sel, selw, h, h2);
        return p;
    }
    p.nseg = 1;
    p.seg[0] = seg_of(L.gate, PAIR_AB, EPI_SWIGLU, h);
    p.seg[0].B = L.up;
    if (src != ACT_PRO) p.seg[0].lora = lora_fold(l, 2);   // ranges gate, up
    else if (lora_group(l, 2)) {
        p.seg[0].pre = lora_pre;   // [gate rows | up rows]
        p.seg[0].pre_up = hp.n_ff;
    }
    return p;
}

// FFN down + residual, in place (MoE, ACT_PRO only: the two experts' rows weighted and added)
GemvParams Ctx::down_params(int l, ActSrc src) const {
    const HParams& hp = m->hp;
    const Layer& L = m->layers[l];
    GemvParams p = gemv_base();
    p.K = hp.n_ff;
    set_act(p, src, 3, src == ACT_PRO ? 0 : sp[l].fD, h, nullptr, nullptr);
    if (hp.n_expert > 0) {
        moe_down_seg(p, L.down, sel, selw, h2, x, cvec_for(l));
        return p;
    }
    p.nseg = 1;
    p.seg[0] = seg_of(L.down, PAIR_ADJ, EPI_ADD, x);
    p.seg[0].bias = L.bdown;
    if (src != ACT_PRO) p.seg[0].lora = lora_fold(l, 3);
    else if (lora_group(l, 3)) p.seg[0].pre = lora_pre;
    p.seg[0].resid = x;
    p.seg[0].addend = cvec_for(l);   // build_cvec: after the FFN residual add
    return p;
}

// the streaming step's FFN down launch: h quantised by a dv_quant launch, or by the launch's own
// workgroups of 8 or 16 waves (sp[l].hq)
GemvParams Ctx::down_params_sp(int l) const {
    GemvParams p = down_params(l, sp[l].hq == HQ_LAUNCH ? ACT_QUANT : ACT_RAW);
    p.act_wide = sp[l].hq == HQ_WG16;
    return p;
}

// final norm + output head of one residual row
GemvParams Ctx::head_params(ActSrc src, const float* xrow) const {
    GemvParams p = gemv_base();
    p.K = m->hp.n_embd;
    set_act(p, src, 4, sp_fH, xrow, m->output_norm, m->output_norm_b);
    p.nseg = 1;
    p.seg[0] = seg_of(m->output, PAIR_ADJ, EPI_STORE, logits);
    return p;
}

// ---- the profiling gate ----
unsigned long long* Ctx::next_stamp() {   // (the r04 step's launches only)
    if (!stamps || sp_ok || enq_launch >= kStampLaunches) return nullptr;
    return stamps + (size_t)(enq_launch++) * kStampWgs * 8;
}

// One GEMV launch of the step being enqueued, on the kernel its activation form selects.  The
// gate/up launch of prof_layer is segment 1 on its own (always eager) and carries the event pair.
void Ctx::run_gemv(GemvParams p, int l, bool gate_up) {
    const bool prof = gate_up && l == prof_layer;
    if (prof) enq_seg = 1;
    const bool timed = prof && seg_filter == 1;
    const bool streaming = p.act_q8k || p.act_q80;
    if (!streaming) p.stamps = next_stamp();
    if (seg_on())
        (streaming ? launch_dgemv : launch_gemv)(p, stream, timed ? prof_ev[0] : nullptr, timed ? prof_ev[1] : nullptr);
    if (prof) enq_seg = 2;
}

void Ctx::run_attn(AttnParams a) {
    a.stamps = next_stamp();
    a.stamps2 = next_stamp();
    if (seg_on()) launch_attn(a, stream);
}

// The routed experts of layer l on gemv_kernel (both steps), x in place
void Ctx::enqueue_moe_ffn(int l) {
    const HParams& hp = m->hp;
    const Layer& L = m->layers[l];
    RouterParams rp{x, L.ffn_norm, hp.eps, L.router, hp.n_embd, hp.n_expert, hp.n_expert_used, sel, selw, 0};
    if (seg_on()) launch_router(rp, stream);
    run_gemv(gate_up_params(l, ACT_PRO), l, true);
    run_gemv(down_params(l, ACT_PRO));
}

// The streaming decode step's buffers (LLaMA; DESIGN.md §4 "dgemv"), and whether every launch of
// the step has a compiled variant (GPT-2 keeps the gemv_kernel graph; MoE experts run on it).
bool Ctx::sp_setup() {
    const HParams& hp = m->hp;
    if (hp.arch != ARCH_LLAMA || m->f16) return false;   // (an F16 model: enqueue_step_f16)
    const bool moe = hp.n_expert > 0;   // MoE: the attention half streams, the experts keep gemv_kernel
    if (hp.n_embd % 256 || hp.n_ff % 256 || hp.n_head * hp.head_dim != hp.n_embd) return false;
    if (!attn_quant_supported(hp.n_head, hp.n_head_kv, hp.head_dim)) return false;   // (the launch's own plan)
    const int nl = hp.n_layer;
    sp.assign(nl, SpLayer{});
    sp_fH = act_fmt({m->output.type});
    size_t act_n = dv_act_bytes(hp.n_embd, sp_fH & 1, sp_fH >> 1), act_f = 0;
    for (int l = 0; l < nl; ++l) {
        const Layer& L = m->layers[l];
        SpLayer& b = sp[l];
        b.fA = 0;
        for (int g = 0; g < L.n_qkv; ++g) b.fA |= act_fmt({L.qkv[g].type});
        b.fB = act_fmt({L.wo.type});
        b.fC = act_fmt({L.gate.type, L.up.type});
        b.fD = act_fmt({L.down.type});
        for (int f : {b.fA, b.fB, b.fC}) act_n = std::max(act_n, dv_act_bytes(hp.n_embd, f & 1, f >> 1));
        act_f = std::max(act_f, dv_act_bytes(hp.n_ff, b.fD & 1, b.fD >> 1));
    }
    // The FFN down launch quantises h in every workgroup itself (no dv_quant launch before it): one
    // launch fewer per layer.  Which workgroup shape does it is by measurement, decode tok/s on one
    // box, dv_quant launch / 8-wave / 16-wave workgroups (profiles/r07_hq16_ab.txt):
    //   tiny-q4_k_m       7397-7420 / 7651-7715 / 7263-7677
    //   TinyLlama Q8_0    1540-1552 / 1644-1649 / 1572-1575
    //   7B Q4_K_M          651-653  /  635-636  /  649-653;  6 runs each: 625.3-626.7 / - / 626.8-629.8
    //   Llama-3-8B Q6_K    512-513  /  477-478  /  515-516;  6 runs each: 490.6-499.9 / - / 490.1-503.2
    // Small models (the redundant work, n_ff elements in each of n_embd / 8 workgroups, is small) keep
    // the 8-wave form; the others take the 16-wave one, which halves that work: no slower than the
    // launch, +0.4 % at the median for 7B -- inside the run-to-run spread.
    const bool small = (long long)hp.n_ff * hp.n_embd <= (1LL << 24);
    for (int l = 0; l < nl; ++l) sp[l].hq = small ? HQ_WG8 : HQ_WG16;
    // The same rule for the normed inputs of Q/K/V and gate/up (dense models): their workgroups
    // build rms_norm(x) * norm_w and quantise it themselves, bit-identical to dv_quant_kernel. That
    // removes two more launches per layer: TinyLlama 1407-1412 -> 1639-1653 tok/s, but 7B 637-643 ->
    // 579-589 and Llama-3-8B 511 -> 470-480 (profiles/r06_nq_ab.txt).
    sp_nq_in = small && !moe && hp.n_embd <= 8192;
    act_n = (act_n + 255) / 256 * 256;
    act_f = (act_f + 255) / 256 * 256;
    sp_mem = mem.dev<char>(4 * act_n + act_f, true);
    sp_act[0] = sp_mem;
    sp_act[1] = sp_mem + act_n;
    sp_act[2] = sp_mem + 2 * act_n;
    sp_act[4] = sp_mem + 3 * act_n;
    sp_act[3] = sp_mem + 4 * act_n;
    if (!moe)   // (a down matrix without a 16-wave variant keeps the dv_quant launch)
        for (int l = 0; l < nl; ++l)
            if (sp[l].hq == HQ_WG16 && !dgemv_supported(down_params_sp(l))) sp[l].hq = HQ_LAUNCH;
    // every launch must have a variant: the parameter blocks enqueue_step_sp will launch, dry
    const ActSrc in = sp_nq_in ? ACT_RAW : ACT_QUANT;
    bool ok = dgemv_supported(head_params(ACT_QUANT, nullptr));
    for (int l = 0; l < nl && ok; ++l) {
        const Layer& L = m->layers[l];
        GemvParams qkv[3];
        const int n = qkv_params(l, in, qkv);
        for (int i = 0; i < n; ++i) ok = ok && dgemv_supported(qkv[i]);
        ok = ok && dgemv_supported(wo_params(l, ACT_QUANT));
        if (moe) continue;
        ok = ok && L.gate.type == L.up.type && dgemv_supported(gate_up_params(l, in)) &&
             dgemv_supported(down_params_sp(l));
    }
    if (!ok) {   // the r04 step serves this model
        mem.release(sp_mem);
        for (char*& a : sp_act) a = nullptr;
        sp.clear();
    }
    return ok;
}

// The layers of one batch-1 decode step on the streaming kernels (any context length): per layer
// dv_quant(rms_norm(x) * attn_norm) -> QKV -> attention (its output also quantised; past ATTN_SHORT
// cells the split attention + attn_combine_quant) -> WO + residual -> dv_quant(rms_norm
// * ffn_norm) -> gate/up -> dv_quant(h) -> down + residual; small models quantise inside the
// consuming launch instead (sp_nq_in); who quantises h is chosen per layer (SpLayer::hq).
void Ctx::enqueue_step_sp(bool with_logits) {
    const HParams& hp = m->hp;
    const bool moe = hp.n_expert > 0;
    const ActSrc in = sp_nq_in ? ACT_RAW : ACT_QUANT;
    auto quant = [&](const float* src, const ActOut& t) {
        if (seg_on()) launch_dv_quant(src, t, stream);
    };
    // the residual quantised for its next reader: layer l's Q/K/V, or (l == n_layer) the output head
    auto quant_x_for = [&](int l) {
        if (l == hp.n_layer) {
            if (with_logits && !embeddings) quant(x, act_out(4, sp_fH, hp.n_embd, m->output_norm));   // (the embedding tail reads x)
        } else if (!sp_nq_in) {
            quant(x, act_out(0, sp[l].fA, hp.n_embd, m->layers[l].attn_norm));
        }
    };
    quant_x_for(0);
    for (int l = 0; l < hp.n_layer; ++l) {
        // LoRA (build_lora_mm): one shrink per activation an adapter reads -- rms_norm(x) * norm_w
        // rebuilt from x (the step keeps it only quantised), the attention output, h -- its B product
        // folded into the consuming launch, ahead of its epilogue
        const LoraGroup *lq = lora_group(l, 0), *lo = lora_group(l, 1), *lg = lora_group(l, 2), *ld = lora_group(l, 3);
        if (lq) lora_shrink(*lq, x, hp.n_embd, hp.n_embd, 1, m->layers[l].attn_norm);
        GemvParams qkv[3];
        const int n = qkv_params(l, in, qkv);
        for (int i = 0; i < n; ++i) run_gemv(qkv[i]);
        AttnParams ap = attn_params(l, true);
        if (lo && attn_fused) ap.out_f32 = part_o;   // the fp32 output too: split 0's slot
        run_attn(ap);
        if (!attn_fused && seg_on()) {
            launch_attn_combine_quant(AttnPartials{part_o, hp.n_head, hp.head_dim}, tokpos,
                                      act_out(1, sp[l].fB, hp.n_embd, nullptr), stream);
            if (lo) launch_attn_combine(AttnPartials{part_o, hp.n_head, hp.head_dim}, tokpos, attn, stream);
        }
        if (lo) lora_shrink(*lo, attn_fused ? part_o : attn, hp.n_embd, hp.n_embd, 1, nullptr);
        run_gemv(wo_params(l, ACT_QUANT));
        if (moe) {
            enqueue_moe_ffn(l);
        } else {
            if (lg) lora_shrink(*lg, x, hp.n_embd, hp.n_embd, 1, m->layers[l].ffn_norm);
            if (!sp_nq_in) quant(x, act_out(2, sp[l].fC, hp.n_embd, m->layers[l].ffn_norm));
            run_gemv(gate_up_params(l, in), l, true);
            if (ld) lora_shrink(*ld, h, hp.n_ff, hp.n_ff, 1, nullptr);
            if (sp[l].hq == HQ_LAUNCH) quant(h, act_out(3, sp[l].fD, hp.n_ff, nullptr));
            run_gemv(down_params_sp(l));
        }
        quant_x_for(l + 1);
    }
}

// ================================================== unquantised F16 models ===
void Ctx::f16_init() {
    const HParams& hp = m->hp;
    f_xn = mem.dev<float>(hp.n_embd);
    attn_mfma = attn_mfma_supported(hp.head_dim);
    if (!batch_ok) return;
    fb_xn = mem.dev<float>((size_t)kBatchRows * hp.n_embd);
    fb_t_stride = std::max(hp.n_embd + 2 * kv_dim, 2 * hp.n_ff);
    fb_t = mem.dev<float>((size_t)kBatchRows * fb_t_stride);
    ub_rope = mem.dev<float2>((size_t)UB_MAX * std::max(1, hp.n_rot / 2));
}

// rms_norm(x) * w of nt rows to f32 rows (the matrix launch that reads them rounds to f16)
void Ctx::f16_norm(const float* xrows, int nt, const float* w, float* out) {
    const HParams& hp = m->hp;
    launch_embd_norm(EmbdNorm{xrows, hp.n_embd, nt, hp.n_embd, w, nullptr, hp.eps, out, hp.n_embd}, stream);
}

namespace {
FgemvParams fgemv_of(int role, const QMat& A, const float* x, float* out) {
    FgemvParams p;
    std::memset(&p, 0, sizeof(p));
    p.role = role;
    p.w[0] = reinterpret_cast<const __half*>(A.p[0]);
    p.rows[0] = A.rows;
    p.nmat = 1;
    p.K = A.K;
    p.x = x;
    p.out = out;
    return p;
}
}  // namespace

// Q/K/V of the normed row + RoPE + KV append: the three matrices in one launch
FgemvParams Ctx::fqkv_params(int l) const {
    const HParams& hp = m->hp;
    const Layer& L = m->layers[l];
    FgemvParams p = fgemv_of(FG_QKV, L.wq, f_xn, q);
    p.w[1] = reinterpret_cast<const __half*>(L.wk.p[0]);
    p.rows[1] = L.wk.rows;
    p.w[2] = reinterpret_cast<const __half*>(L.wv.p[0]);
    p.rows[2] = L.wv.rows;
    p.nmat = 3;
    p.nq = L.wq.rows;
    p.nk = L.wk.rows;
    p.tokpos = tokpos;
    p.cell_pos = cell_pos;
    p.theta_scale = theta_scale();
    p.freq_scale = hp.freq_scale;
    p.n_rot = hp.n_rot;
    p.head_dim = hp.head_dim;
    p.freq_factors = m->rope_freqs;
    p.kcache = k_layer(l);
    p.vcache = v_layer(l);
    p.kv_dim = kv_dim;
    return p;
}

// output projection of the attention output (the fused launch's one split in part_o, else the
// splits' sum in attn) + residual, in place
FgemvParams Ctx::fwo_params(int l) const {
    FgemvParams p = fgemv_of(FG_ADD, m->layers[l].wo, attn_fused ? part_o : attn, x);
    p.resid = x;
    return p;
}

FgemvParams Ctx::fgate_up_params(int l) const {
    const Layer& L = m->layers[l];
    FgemvParams p = fgemv_of(FG_SWIGLU, L.gate, f_xn, h);
    p.w[1] = reinterpret_cast<const __half*>(L.up.p[0]);
    p.rows[1] = L.up.rows;
    p.nmat = 2;
    return p;
}

// FFN down + residual, in place, then the control vector's row (build_cvec)
FgemvParams Ctx::fdown_params(int l) const {
    FgemvParams p = fgemv_of(FG_ADD, m->layers[l].down, h, x);
    p.resid = x;
    p.addend = cvec_for(l);
    return p;
}

FgemvParams Ctx::fhead_params() const { return fgemv_of(FG_STORE, m->output, f_xn, logits); }

// (the gate/up launch of prof_layer: segment 1 on its own, with the event pair -- as run_gemv)
void Ctx::run_fgemv(const FgemvParams& p, int l, bool gate_up) {
    const bool prof = gate_up && l == prof_layer;
    if (prof) enq_seg = 1;
    const bool timed = prof && seg_filter == 1;
    if (seg_on()) launch_fgemv(p, stream, timed ? prof_ev[0] : nullptr, timed ? prof_ev[1] : nullptr);
    if (prof) enq_seg = 2;
}

// The layers and the tail of one batch-1 decode step of an F16 model (the embedding row is in x)
void Ctx::enqueue_step_f16(bool with_logits) {
    const HParams& hp = m->hp;
    for (int l = 0; l < hp.n_layer; ++l) {
        const Layer& L = m->layers[l];
        if (seg_on()) f16_norm(x, 1, L.attn_norm, f_xn);
        run_fgemv(fqkv_params(l));
        run_attn(attn_params(l, false));
        if (!attn_fused && seg_on()) launch_attn_combine(AttnPartials{part_o, hp.n_head, hp.head_dim}, tokpos, attn, stream);
        run_fgemv(fwo_params(l));
        if (seg_on()) f16_norm(x, 1, L.ffn_norm, f_xn);
        run_fgemv(fgate_up_params(l), l, true);
        run_fgemv(fdown_params(l));
    }
    if (!with_logits || !seg_on()) return;
    if (embeddings) {   // embeddings mode: result_norm of this token, no head
        enqueue_embd_norm(x, 1, embd_step());
        return;
    }
    f16_norm(x, 1, m->output_norm, f_xn);
    launch_fgemv(fhead_params(), stream);
    run_topk(logits);
}

// One decode step for the token in tokpos (batch 1): the llm_build_llama / llm_build_gpt2 graph,
// on the streaming kernels (sp_ok) or on gemv_kernel.
void Ctx::enqueue_step(bool with_logits) {
    const HParams& hp = m->hp;
    enq_seg = 0;
    enq_launch = 0;
    EmbedParams ep{m->tok_embd, tokpos, x, hp.n_embd, m->pos_embd, hp.arch == ARCH_GPT2 ? 1 : 0, step_ctr};
    if (seg_on()) launch_embed(ep, stream);
    if (m->f16) {
        enqueue_step_f16(with_logits);
        return;
    }
    if (sp_ok) {
        enqueue_step_sp(with_logits);
    } else {
        for (int l = 0; l < hp.n_layer; ++l) {
            // LoRA on gemv_kernel (dense LLaMA geometries the streaming step does not serve): the
            // terms precomputed into lora_pre ahead of the launch that adds them before its epilogue
            const Layer& L = m->layers[l];
            lora_pre_terms(l, 0, x, hp.n_embd, 1, L.attn_norm);
            GemvParams qkv[3];
            const int n = qkv_params(l, ACT_PRO, qkv);
            for (int i = 0; i < n; ++i) run_gemv(qkv[i]);
            run_attn(attn_params(l, false));
            if (lora_group(l, 1)) {   // the attention output in fp32: the fused launch's one split, or the splits' sum
                if (!attn_fused && seg_on()) launch_attn_combine(AttnPartials{part_o, hp.n_head, hp.head_dim}, tokpos, attn, stream);
                lora_pre_terms(l, 1, attn_fused ? part_o : attn, hp.n_embd, 1, nullptr);
            }
            run_gemv(wo_params(l, ACT_PRO));
            if (hp.n_expert > 0) {
                enqueue_moe_ffn(l);
            } else {
                lora_pre_terms(l, 2, x, hp.n_embd, 1, L.ffn_norm);
                run_gemv(gate_up_params(l, ACT_PRO), l, true);
                lora_pre_terms(l, 3, h, hp.n_ff, 1, nullptr);
                run_gemv(down_params(l, ACT_PRO));
            }
        }
    }
    if (with_logits && seg_on()) {
        if (embeddings) enqueue_embd_norm(x, 1, embd_step());   // embeddings mode: result_norm of this token, no head
        else enqueue_output(sp_ok ? ACT_QUANT : ACT_PRO, x, next_stamp());
    }
}

// the output head of one residual row (ACT_QUANT: quantised at sp_act[4] already), then the top-k
void Ctx::enqueue_output(ActSrc src, const float* xrow, unsigned long long* stamps_slab) {
    GemvParams p = head_params(src, xrow);
    p.stamps = stamps_slab;
    (src == ACT_PRO ? launch_gemv : launch_dgemv)(p, stream, nullptr, nullptr);
    run_topk(logits);
}

void Ctx::run_topk(const float* src) {
    TopkParams tp{src, m->hp.n_vocab, cand, topk_ids, topk_vals, d_h_topk_ids, d_h_topk_vals};
    launch_topk(tp, stream);
}

hipGraphExec_t Ctx::build_graph(bool with_logits, int seg) {
    hipGraph_t g = nullptr;
    seg_filter = seg;
    MI_HIP(hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal));
    try {
        enqueue_step(with_logits);
    } catch (...) {
        seg_filter = -1;
        hipStreamEndCapture(stream, &g);
        if (g) hipGraphDestroy(g);
        throw;
    }
    seg_filter = -1;
    MI_HIP(hipStreamEndCapture(stream, &g));
    hipGraphExec_t ex = nullptr;
    MI_HIP(hipGraphInstantiate(&ex, g, nullptr, nullptr, 0));
    MI_HIP(hipGraphDestroy(g));
    return ex;
}

int Ctx::decode(const int32_t* tokens, int n, bool all) {
    MI_HIP(hipSetDevice(device));
    if (n <= 0) throw Error("decode: empty batch");
    if (!unsynced) {   // the state a failed long-context exchange rolls back to
        undo_cells = n_cells;
        undo_pos = pos_max;
    }
    unsynced = true;
    for (int i = 0; i < n; ++i)
        if (tokens[i] < 0 || tokens[i] >= m->hp.n_vocab) throw Error("decode: token id out of range");
    if (enc) {
        batch_path = 5;
        return decode_enc(tokens, n, all);
    }
    if (n_cells + n > (int)n_ctx) return 1;   // no KV slot (llama_decode returns 1)
    if (m->hp.arch == ARCH_GPT2 && pos_max + n >= m->hp.n_ctx_train)
        throw Error("decode: gpt2 position past the learned position embeddings (n_ctx_train)");
    if (all && n > (int)n_batch) throw Error("decode: MI_OUT_ALL takes at most n_batch tokens");
    out_rows = 0;
    topk_row = -1;
    const bool pooled = embeddings && pooling != MI_POOLING_NONE;
    if (pooled && n > (int)n_batch) throw Error("decode: a pooled embeddings call takes at most n_batch tokens");
    if (embeddings) {   // the rows of this call (a pooled call yields one row whatever out_mode says)
        if (!embd) {    // [n_batch] token rows, the pooled row, the step's row: allocated once
            embd = mem.dev<float>(((size_t)n_batch + 2) * m->hp.n_embd);
            h_embd = mem.host<float>(m->hp.n_embd);
        }
        embd_n = n;
        embd_all = all && !pooled;
        embd_rows = 0;
        embd_valid = false;
        logits_valid = false;   // no head runs
    }
    if (all && !embeddings && logits_all_cap < n) {   // every token's logits: [n_batch][n_vocab], allocated once
        mem.release(logits_all);
        logits_all = mem.dev<float>((size_t)n_batch * m->hp.n_vocab);
        logits_all_cap = (int)n_batch;
    }
    // an F16 model: any call of two tokens or more on the F16 MFMA GEMM (the MFMA attention over any
    // number of cells; head sizes it does not serve: the fused form within ATTN_SHORT cells)
    if (m->f16 && n >= 2 && batch_ok && prof_layer < 0 && (attn_mfma || n_cells + n <= ATTN_SHORT)) {
        batch_path = 4;
        decode_f16_batch(tokens, n, all);
        if (all && !embeddings) out_rows = n;
        return 0;
    }
    // prompt ingestion through the batched GEMM when the context stays within the fused
    // attention's reach (dense models; MI_NO_BATCH=1 forces token-by-token decode)
    const bool fits = n >= 2 && batch_ok && !m->f16 && hp_dense() && m->hp.arch == ARCH_LLAMA && n_cells + n <= ATTN_SHORT &&
                      prof_layer < 0;
    // the MFMA batch path attends over any number of cells with the MFMA attention kernel
    const bool ub = n >= 2 && batch_ok && mmq_ok && prof_layer < 0 && (attn_mfma || n_cells + n <= ATTN_SHORT);
    if (ub && (!all || out_mmq || embeddings)) {
        decode_ubatch(tokens, n, all);
        if (all && !embeddings) out_rows = n;
        return 0;
    }
    if (fits && (!all || embeddings)) {
        batch_path = 1;
        decode_batch(tokens, n);
        return 0;
    }
    batch_path = 0;   // one decode step per token
    for (int i = 0; i < n; ++i) {
        // embeddings mode: the steps whose row the call's result needs end in the embedding row
        const bool last = i == n - 1 || (all && !pooled) || (pooled && (pooling == MI_POOLING_MEAN || (pooling == MI_POOLING_CLS && i == 0)));
        const int pos = pos_max + 1, cell = n_cells;
        attn_fused = cell + 1 <= ATTN_SHORT ? 1 : 0;   // this step attends over cell + 1 cells
        const long long slot = tok_slot++ % kTokRing;
        if (slot == 0 && tok_slot > 1) MI_HIP(hipStreamSynchronize(stream));
        int* hp = h_tokpos + slot * 4;
        hp[0] = tokens[i];
        hp[1] = pos;
        hp[2] = cell;
        hp[3] = 0;
        MI_HIP(hipMemcpyAsync(tokpos, hp, 4 * sizeof(int), hipMemcpyHostToDevice, stream));
        if (last && prof_layer >= 0 && prof_layer < m->hp.n_layer) {
            for (int k = 0; k < 2; ++k)
                if (!prof_ev[k]) prof_ev[k] = mem.event();
            // graph up to the profiled launch, the launch itself eagerly with
            // hipExtLaunchKernel start/stop events, graph for the rest
            for (int k = 0; k < 3; ++k) {
                if (use_graphs && k != 1) {
                    if (!g_seg[attn_fused][k]) g_seg[attn_fused][k] = build_graph(true, k);
                    MI_HIP(hipGraphLaunch(g_seg[attn_fused][k], stream));
                } else {
                    seg_filter = k;
                    enqueue_step(true);
                    seg_filter = -1;
                }
            }
            prof_pending = true;
            prof_bytes = ffn_bytes();
        } else if (!use_graphs) {
            enqueue_step(last);
        } else {
            hipGraphExec_t& g = !last ? g_nolog[attn_fused] : embeddings ? g_embd[attn_fused] : g_full[attn_fused];
            if (!g) g = build_graph(last, -1);
            MI_HIP(hipGraphLaunch(g, stream));
        }
        if (embeddings) {   // this token's embedding -> row i
            if (last && (embd_all || pooled))
                MI_HIP(hipMemcpyAsync(embd + (size_t)i * m->hp.n_embd, embd_step(), (size_t)m->hp.n_embd * sizeof(float),
                                      hipMemcpyDeviceToDevice, stream));
        } else if (all)   // this token's logits -> row i
            MI_HIP(hipMemcpyAsync(logits_all + (size_t)i * m->hp.n_vocab, logits, (size_t)m->hp.n_vocab * sizeof(float),
                                  hipMemcpyDeviceToDevice, stream));
        h_cell_pos[cell] = pos;
        n_cells++;
        pos_max = pos;
    }
    if (embeddings) {
        if (pooled) embd_pool_rows(0, n);
        else if (embd_all) embd_rows = n;
        embd_valid = true;
        return 0;
    }
    if (all) out_rows = n;
    logits_valid = true;
    return 0;
}

void Ctx::sync() {
    MI_HIP(hipSetDevice(device));
    MI_HIP(hipStreamSynchronize(stream));
    const bool was_unsynced = unsynced;
    unsynced = false;
    if (h_attn_xerr && *h_attn_xerr) {   // an attention exchange gave up: the step's logits are invalid
        *h_attn_xerr = 0;
        logits_valid = false;
        embd_valid = false;
        // the cells decoded since the last good sync hold KV rows built from a wrong attention
        // output: drop them, and use the two-launch split kernels from now on
        if (was_unsynced) {
            n_cells = undo_cells;
            pos_max = undo_pos;
        }
        invalidate_graphs();
        attn_long_off = true;
        throw Error("long-context attention: the splits of a head were not co-resident (exchange timed out); "
                    "the step was rolled back and this context now uses the two-launch kernels");
    }
}

const float* Ctx::out_row(int row) const {
    if (row == -1) return logits;
    if (row < 0 || row >= std::max(out_rows, 1)) throw Error("output row out of range");
    if (out_rows == 0) return logits;   // MI_OUT_LAST: row 0 is the last token's
    return logits_all + (size_t)row * m->hp.n_vocab;
}

// ---- embeddings ----

void Ctx::set_embeddings(bool on, int pooling_type) {
    if (pooling_type < MI_POOLING_UNSPECIFIED || pooling_type > MI_POOLING_RANK)
        throw Error("set_embeddings: pooling type out of range (-1 .. 3)");
    if (pooling_type == MI_POOLING_RANK)
        throw Error("set_embeddings: RANK pooling needs a classification head, which this engine does not load");
    if (pooling_type == MI_POOLING_UNSPECIFIED) pooling_type = model_pooling(m->hp);
    if (enc && !on) throw Error("set_embeddings: encoder models have no output head (the context stays in embeddings mode)");
    MI_HIP(hipSetDevice(device));
    sync();                 // steps in flight still write the old mode's outputs
    invalidate_graphs();    // the step graphs end in the other tail
    embeddings = on;
    pooling = pooling_type;
    embd_valid = false;
    embd_rows = 0;
    if (on) logits_valid = false;
}

void Ctx::enqueue_embd_norm(const float* xrows, int nt, float* out) {
    const HParams& hp = m->hp;
    if (hp.arch == ARCH_GPT2 && !m->output_norm_b) throw Error("embeddings: gpt2 without output_norm.bias");
    launch_embd_norm(EmbdNorm{xrows, hp.n_embd, nt, hp.n_embd, m->output_norm, hp.arch == ARCH_GPT2 ? m->output_norm_b : nullptr,
                              hp.eps, out, hp.n_embd},
                     stream);
}

void Ctx::embd_pool_rows(int r0, int nt) {
    const int ne = m->hp.n_embd, n = embd_n;
    EmbdPool p{embd + (size_t)r0 * ne, ne, 0, ne, 1.0f / (float)n, r0 > 0 ? 1 : 0, embd_pooled()};
    if (pooling == MI_POOLING_MEAN) {
        p.nt = nt;
    } else if (pooling == MI_POOLING_CLS) {
        if (r0 > 0) return;
    } else {   // LAST
        if (r0 + nt < n) return;
        p.rows = embd + (size_t)(n - 1) * ne;
    }
    launch_embd_pool(p, stream);
}

void Ctx::embd_tail(const float* xrows, int nt, int c0) {
    const int ne = m->hp.n_embd, n = embd_n;
    const bool last = c0 + nt == n;
    if (pooling == MI_POOLING_NONE) {
        if (embd_all) enqueue_embd_norm(xrows, nt, embd + (size_t)c0 * ne);
        else if (last) enqueue_embd_norm(xrows + (size_t)(nt - 1) * ne, 1, embd_step());
        if (last && embd_all) embd_rows = n;
    } else {
        // the rows the pooled row reads: all of them (MEAN), the call's first (CLS) or last (LAST)
        if (pooling == MI_POOLING_MEAN) enqueue_embd_norm(xrows, nt, embd + (size_t)c0 * ne);
        else if (pooling == MI_POOLING_CLS && c0 == 0) enqueue_embd_norm(xrows, 1, embd);
        else if (pooling == MI_POOLING_LAST && last) enqueue_embd_norm(xrows + (size_t)(nt - 1) * ne, 1, embd + (size_t)(n - 1) * ne);
        embd_pool_rows(c0, nt);
    }
    if (last) embd_valid = true;
}

const float* Ctx::embeddings_host(int row) {
    if (!embeddings) throw Error("embeddings: the context is not in embeddings mode (mi_ctx_set_embeddings)");
    if (!embd_valid) throw Error("no embeddings: decode since the mode was set first");
    const int ne = m->hp.n_embd;
    const float* src;
    if (pooling != MI_POOLING_NONE) {
        if (row != 0 && row != -1) throw Error("embeddings: a pooled context has one row (0 or -1)");
        src = embd_pooled();
    } else if (embd_rows > 0) {
        if (row < -1 || row >= embd_rows) throw Error("embeddings: output row out of range");
        src = embd + (size_t)(row < 0 ? embd_rows - 1 : row) * ne;
    } else {
        if (row != 0 && row != -1) throw Error("embeddings: output row out of range");
        src = embd_step();
    }
    MI_HIP(hipSetDevice(device));
    MI_HIP(hipMemcpyAsync(h_embd, src, (size_t)ne * sizeof(float), hipMemcpyDeviceToHost, stream));
    sync();
    return h_embd;
}

int Ctx::topk(int row, int k, int32_t* ids, float* vals) {
    if (embeddings) throw Error(kEmbdMode);
    if (!logits_valid) throw Error("no logits: decode a token first");
    if (k < 0 || k > TOPK_MAX) throw Error("topk: k must be in [0, 64]");
    if (out_rows > 0 && row == out_rows - 1) row = -1;   // the last row's top-k is already computed
    const float* src = out_row(row);
    if (src != logits || topk_row != -1) {   // another row than the mapped buffers hold
        MI_HIP(hipSetDevice(device));
        run_topk(src);
        topk_row = src == logits ? -1 : row;
    }
    sync();
    for (int i = 0; i < k; ++i) {
        ids[i] = h_topk_ids[i];
        vals[i] = h_topk_vals[i];
    }
    return k;
}

int Ctx::gather(int row, const int32_t* ids, int n, float* out) {
    if (embeddings) throw Error(kEmbdMode);
    if (!logits_valid) throw Error("no logits: decode a token first");
    const float* src = out_row(row);
    if (n < 0 || n > 4096) throw Error("gather: n must be in [0, 4096]");
    for (int i = 0; i < n; ++i)
        if (ids[i] < 0 || ids[i] >= m->hp.n_vocab) throw Error("gather: id out of range");
    if (n == 0) return 0;
    MI_HIP(hipSetDevice(device));
    MI_HIP(hipMemcpyAsync(gather_ids, ids, n * sizeof(int), hipMemcpyHostToDevice, stream));
    launch_gather(src, gather_ids, n, gather_out, stream);
    MI_HIP(hipMemcpyAsync(h_gather, gather_out, n * sizeof(float), hipMemcpyDeviceToHost, stream));
    sync();
    std::memcpy(out, h_gather, n * sizeof(float));
    return n;
}

// Logits of rows row0..row0+nrows-1 at k ids each (ids [nrows][k]): the batched form of gather
// for a verification pass -- one copy in, one kernel, one copy out.
int Ctx::gather_rows(int row0, int nrows, const int32_t* ids, int k, float* out) {
    if (embeddings) throw Error(kEmbdMode);
    if (!logits_valid) throw Error("no logits: decode a token first");
    if (nrows < 0 || k < 0) throw Error("gather_rows: negative count");
    const size_t n = (size_t)nrows * k;
    if (n == 0) return 0;
    const int avail = out_rows > 0 ? out_rows : 1;
    if (row0 < 0 || row0 + nrows > avail) throw Error("gather_rows: output rows out of range");
    for (size_t i = 0; i < n; ++i)
        if (ids[i] < 0 || ids[i] >= m->hp.n_vocab) throw Error("gather_rows: id out of range");
    MI_HIP(hipSetDevice(device));
    if (n > grows_cap) {
        mem.release(grows_ids);
        mem.release(grows_out);
        mem.release(h_grows);
        grows_cap = 0;
        grows_ids = mem.dev<int>(n);
        grows_out = mem.dev<float>(n);
        h_grows = mem.host<float>(n);
        grows_cap = n;
    }
    const float* base = out_rows > 0 ? logits_all + (size_t)row0 * m->hp.n_vocab : logits;
    MI_HIP(hipMemcpyAsync(grows_ids, ids, n * sizeof(int), hipMemcpyHostToDevice, stream));
    launch_gather_rows(base, m->hp.n_vocab, grows_ids, (int)n, k, grows_out, stream);
    MI_HIP(hipMemcpyAsync(h_grows, grows_out, n * sizeof(float), hipMemcpyDeviceToHost, stream));
    sync();
    std::memcpy(out, h_grows, n * sizeof(float));
    return (int)n;
}

const float* Ctx::logits_host(int row) {
    if (embeddings) throw Error(kEmbdMode);
    if (!logits_valid) throw Error("no logits: decode a token first");
    const float* src = out_row(row);
    MI_HIP(hipSetDevice(device));
    MI_HIP(hipMemcpyAsync(h_logits, src, (size_t)m->hp.n_vocab * sizeof(float), hipMemcpyDeviceToHost, stream));
    sync();
    return h_logits;
}

void Ctx::kv_clear() {
    if (enc) return;   // no cache: every call is stateless
    n_cells = 0;
    pos_max = -1;
    out_rows = 0;      // rows of the last MI_OUT_ALL pass belong to the cleared cache
    topk_row = -1;
}

// Remove cells with pos in [p0, p1); the survivors keep their order and are
// compacted to the front of the cache.
int Ctx::kv_seq_rm(int p0, int p1) {
    if (enc) throw Error("kv_seq_rm: an encoder context has no KV cache");
    if (p0 < 0) p0 = 0;
    if (p1 < 0) p1 = INT_MAX;
    std::vector<int> keep;
    keep.reserve(n_cells);
    for (int c = 0; c < n_cells; ++c)
        if (h_cell_pos[c] < p0 || h_cell_pos[c] >= p1) keep.push_back(c);
    bool prefix = true;
    for (int j = 0; j < (int)keep.size(); ++j)
        if (keep[j] != j) { prefix = false; break; }
    if (!prefix) {
        MI_HIP(hipSetDevice(device));
        const HParams& hp = m->hp;
        if (!kv_scratch) kv_scratch = mem.dev<__half>((size_t)hp.n_layer * n_ctx * kv_dim);
        MI_HIP(hipMemcpyAsync(move_src, keep.data(), keep.size() * sizeof(int), hipMemcpyHostToDevice, stream));
        launch_kv_move(kcache, hp.n_layer, n_ctx, kv_dim, move_src, (int)keep.size(), kv_scratch, stream);
        launch_kv_move(vcache, hp.n_layer, n_ctx, kv_dim, move_src, (int)keep.size(), kv_scratch, stream);
        std::vector<int> np(keep.size());
        for (size_t j = 0; j < keep.size(); ++j) np[j] = h_cell_pos[keep[j]];
        for (size_t j = 0; j < keep.size(); ++j) h_cell_pos[j] = np[j];
        MI_HIP(hipMemcpyAsync(cell_pos, h_cell_pos.data(), keep.size() * sizeof(int), hipMemcpyHostToDevice, stream));
        sync();
    }
    n_cells = (int)keep.size();
    pos_max = -1;
    for (int c = 0; c < n_cells; ++c) pos_max = std::max(pos_max, h_cell_pos[c]);
    return 0;
}

// seq_add (div == 0: pos += delta) / seq_div (pos /= div) over [p0, p1):
// positions change and cached K is re-rotated by the delta (K-shift).
int Ctx::kv_seq_shift(int p0, int p1, int delta, int div) {
    if (enc) throw Error("kv_seq_add / kv_seq_div: an encoder context has no KV cache");
    if (p0 < 0) p0 = 0;
    if (p1 < 0) p1 = INT_MAX;
    if (p0 == p1) return 0;
    if (div == 0 && delta == 0) return 0;
    if (div == 1) return 0;
    std::vector<int> dlt(n_cells, 0);
    bool any = false, neg = false;
    for (int c = 0; c < n_cells; ++c) {
        const int ps = h_cell_pos[c];
        if (ps >= p0 && ps < p1) {
            const int np = div ? ps / div : ps + delta;
            dlt[c] = np - ps;
            h_cell_pos[c] = np;
            any = any || dlt[c] != 0;
            neg = neg || np < 0;
        }
    }
    if (any) {
        MI_HIP(hipSetDevice(device));
        const HParams& hp = m->hp;
        MI_HIP(hipMemcpyAsync(cell_delta, dlt.data(), n_cells * sizeof(int), hipMemcpyHostToDevice, stream));
        KvShiftParams kp{kcache, hp.n_layer, (int)n_ctx, kv_dim, hp.head_dim, hp.n_rot, cell_delta, n_cells,
                         theta_scale(), hp.freq_scale, m->rope_freqs};
        launch_kv_shift(kp, stream);
        MI_HIP(hipMemcpyAsync(cell_pos, h_cell_pos.data(), n_cells * sizeof(int), hipMemcpyHostToDevice, stream));
        sync();
    }
    if (neg) return kv_seq_rm(INT_MIN, 0);   // cells shifted below 0 are removed (llama.cpp semantics)
    pos_max = -1;
    for (int c = 0; c < n_cells; ++c) pos_max = std::max(pos_max, h_cell_pos[c]);
    return 0;
}

// ---- state: header | cell positions | K rows | V rows | last logits ----
namespace {
struct StateHdr {
    char magic[8];
    int32_t version, n_layer, kv_dim, n_vocab, n_cells, pos_max, logits_valid, pad;
};
}  // namespace

size_t Ctx::state_size() const {
    if (enc) return 0;   // nothing survives an encoder call
    const HParams& hp = m->hp;
    return sizeof(StateHdr) + (size_t)n_cells * sizeof(int) +
           2 * (size_t)hp.n_layer * n_cells * kv_dim * sizeof(__half) + (size_t)hp.n_vocab * sizeof(float);
}

size_t Ctx::state_get(uint8_t* dst, size_t size) {
    if (enc) return 0;
    const size_t need = state_size();
    if (size < need) throw Error("state_get: buffer too small");
    const HParams& hp = m->hp;
    StateHdr hd{};
    std::memcpy(hd.magic, "MISTATE1", 8);
    hd.version = 1;
    hd.n_layer = hp.n_layer;
    hd.kv_dim = kv_dim;
    hd.n_vocab = hp.n_vocab;
    hd.n_cells = n_cells;
    hd.pos_max = pos_max;
    hd.logits_valid = logits_valid ? 1 : 0;
    uint8_t* o = dst;
    std::memcpy(o, &hd, sizeof(hd));
    o += sizeof(hd);
    std::memcpy(o, h_cell_pos.data(), n_cells * sizeof(int));
    o += n_cells * sizeof(int);
    MI_HIP(hipSetDevice(device));
    sync();
    const size_t row = (size_t)n_cells * kv_dim * sizeof(__half);
    for (__half* cache : {kcache, vcache})
        for (int l = 0; l < hp.n_layer; ++l) {
            if (row) MI_HIP(hipMemcpy(o, cache + (size_t)l * n_ctx * kv_dim, row, hipMemcpyDeviceToHost));
            o += row;
        }
    if (logits_valid) MI_HIP(hipMemcpy(o, logits, (size_t)hp.n_vocab * sizeof(float), hipMemcpyDeviceToHost));
    else std::memset(o, 0, (size_t)hp.n_vocab * sizeof(float));
    return need;
}

size_t Ctx::state_set(const uint8_t* src, size_t size) {
    if (enc) return 0;
    const HParams& hp = m->hp;
    StateHdr hd;
    if (size < sizeof(hd)) throw Error("state_set: truncated state");
    std::memcpy(&hd, src, sizeof(hd));
    if (std::memcmp(hd.magic, "MISTATE1", 8) != 0 || hd.n_layer != hp.n_layer || hd.kv_dim != kv_dim ||
        hd.n_vocab != hp.n_vocab)
        throw Error("state_set: state does not match this model");
    if (hd.n_cells < 0 || hd.n_cells > (int)n_ctx) throw Error("state_set: too many cells for this context");
    const size_t need = sizeof(hd) + (size_t)hd.n_cells * sizeof(int) +
                        2 * (size_t)hp.n_layer * hd.n_cells * kv_dim * sizeof(__half) + (size_t)hp.n_vocab * sizeof(float);
    if (size < need) throw Error("state_set: truncated state");
    const uint8_t* s = src + sizeof(hd);
    n_cells = hd.n_cells;
    pos_max = hd.pos_max;
    out_rows = 0;      // only the restored last-token row (-1 / 0) is valid after a restore
    topk_row = -1;
    std::memcpy(h_cell_pos.data(), s, n_cells * sizeof(int));
    s += n_cells * sizeof(int);
    MI_HIP(hipSetDevice(device));
    sync();
    if (n_cells) MI_HIP(hipMemcpy(cell_pos, h_cell_pos.data(), n_cells * sizeof(int), hipMemcpyHostToDevice));
    const size_t row = (size_t)n_cells * kv_dim * sizeof(__half);
    for (__half* cache : {kcache, vcache})
        for (int l = 0; l < hp.n_layer; ++l) {
            if (row) MI_HIP(hipMemcpy(cache + (size_t)l * n_ctx * kv_dim, s, row, hipMemcpyHostToDevice));
            s += row;
        }
    logits_valid = hd.logits_valid != 0;
    if (logits_valid) {
        MI_HIP(hipMemcpy(logits, s, (size_t)hp.n_vocab * sizeof(float), hipMemcpyHostToDevice));
        run_topk(logits);
        sync();
    }
    return need;
}

int Ctx::prof_read(float* us, int n) {
    if (!prof_pending || n < 1) return 0;
    sync();
    float ms = 0.0f;
    MI_HIP(hipEventElapsedTime(&ms, prof_ev[0], prof_ev[1]));
    us[0] = ms * 1000.0f;
    prof_pending = false;
    return 1;
}

}  // namespace mi
