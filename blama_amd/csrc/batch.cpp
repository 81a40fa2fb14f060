// Engine host code: the prompt-batch paths of the decode context -- prompt chunks on the v_dot4
// GEMM (decode_batch), physical batches on the tiled int8-MFMA GEMM (decode_ubatch) and short
// batches on the split-K streaming GEMM (ubatch_layers_short) -- over one builder per launch.
#include "engine.h"

#include <algorithm>
#include <cstring>

namespace mi {

// ========================================================= batch launches ===
void Ctx::upload_batch(const int32_t* tokens, int nt) {
    const long long slot = tokb_slot++ % kTokbRing;
    if (slot == 0 && tokb_slot > 1) MI_HIP(hipStreamSynchronize(stream));
    int* hpos = h_tokpos_b + slot * kBatchRows * 4;
    for (int t = 0; t < nt; ++t) {
        const int pos = pos_max + 1, cell = n_cells;
        hpos[t * 4 + 0] = tokens[t];
        hpos[t * 4 + 1] = pos;
        hpos[t * 4 + 2] = cell;
        hpos[t * 4 + 3] = 0;
        h_cell_pos[cell] = pos;
        n_cells++;
        pos_max = pos;
    }
    MI_HIP(hipMemcpyAsync(tokpos_b, hpos, nt * 4 * sizeof(int), hipMemcpyHostToDevice, stream));
}

GemmParams Ctx::gemm_base(int l, int nt, bool vdot4) const {
    const HParams& hp = m->hp;
    GemmParams p;
    std::memset(&p, 0, sizeof(p));
    p.ntok = nt;
    p.tokpos = tokpos_b;
    p.cell_pos = cell_pos;
    p.head_dim = hp.head_dim;
    p.kcache = k_layer(l);
    p.vcache = v_layer(l);
    p.kv_dim = kv_dim;
    if (vdot4) {   // (n_rot: on the Q and K launches only)
        p.theta_scale = theta_scale();
        p.freq_scale = hp.freq_scale;
        p.freq_factors = m->rope_freqs;
        p.eps = hp.eps;
    } else {
        p.n_rot = hp.n_rot;
    }
    return p;
}

GemmParams mmq32_params(const QMat& A, const QMat* B, int ntok, const int* tokpos, float* out, int out_stride,
                        const int* grp, int grp_max) {
    GemmParams p;
    std::memset(&p, 0, sizeof(p));
    p.A = A;
    if (B) p.B = *B;
    p.pair = B ? PAIR_AB : PAIR_ADJ;
    p.epi = B ? EPI_SWIGLU : EPI_STORE;
    p.K = A.K;
    p.ntok = ntok;
    p.tokpos = tokpos;
    p.out = out;
    p.out_stride = out_stride;
    if (grp) {
        p.grp = grp;
        p.grp_n = A.n_exp;
        p.grp_max = grp_max;
        p.grp_stride = A.sw_expert_stride;
    }
    return p;
}

// Q, K or V projection (+ RoPE, KV append) into qb
GemmParams Ctx::bqkv_params(int l, int nt, bool vdot4, int i, const float* pre) const {
    const Layer& L = m->layers[l];
    const int epis[3] = {EPI_ROPE_Q, EPI_ROPE_K, EPI_V};
    GemmParams p = gemm_base(l, nt, vdot4);
    p.A = i == 0 ? L.wq : i == 1 ? L.wk : L.wv;
    p.pair = PAIR_ADJ;
    p.epi = epis[i];
    p.K = m->hp.n_embd;
    p.out = qb;
    p.out_stride = m->hp.n_embd;
    if (vdot4 && i < 2) p.n_rot = m->hp.n_rot;
    set_pre(p, pre, l, 0, i);   // LoRA: added before RoPE and the KV append
    return p;
}

// output projection + residual, in place
GemmParams Ctx::bwo_params(int l, int nt, bool vdot4, const float* pre) const {
    GemmParams p = gemm_base(l, nt, vdot4);
    p.A = m->layers[l].wo;
    p.pair = PAIR_ADJ;
    p.epi = EPI_ADD;
    p.K = m->hp.n_embd;
    p.out = xb;
    p.resid = xb;
    p.out_stride = m->hp.n_embd;
    p.bias = m->layers[l].bo;   // GPT-2 (mmq32): (y + b) + x
    set_pre(p, pre, l, 1, 0);   // before the residual add
    return p;
}

// FFN gate/up + SwiGLU into hb
GemmParams Ctx::bgate_up_params(int l, int nt, bool vdot4, const float* pre) const {
    GemmParams p = gemm_base(l, nt, vdot4);
    p.A = m->layers[l].gate;
    p.B = m->layers[l].up;
    p.pair = PAIR_AB;
    p.epi = EPI_SWIGLU;
    p.K = m->hp.n_embd;
    p.out = hb;
    p.out_stride = m->hp.n_ff;
    set_pre(p, pre, l, 2, 0);   // the gate and up terms, before SwiGLU
    return p;
}

// FFN down + residual, in place, then the control vector's row (build_cvec)
GemmParams Ctx::bdown_params(int l, int nt, bool vdot4, const float* pre) const {
    GemmParams p = gemm_base(l, nt, vdot4);
    p.A = m->layers[l].down;
    p.pair = PAIR_ADJ;
    p.epi = EPI_ADD;
    p.K = m->hp.n_ff;
    p.out = xb;
    p.resid = xb;
    p.addend = cvec_for(l);
    p.out_stride = m->hp.n_embd;
    p.bias = m->layers[l].bdown;   // GPT-2 (mmq32): ((y + b) + x), then the control vector's row
    set_pre(p, pre, l, 3, 0);
    return p;
}

// GPT-2: the fused attn_qkv (+ bias, KV append; no rotation) into qb and the caches -- the launch
// takes it as three row segments (launch_mmq32_rows)
GemmParams Ctx::bqkv_gpt2_params(int l, int nt) const {
    GemmParams p = gemm_base(l, nt, false);   // (n_rot 0)
    p.A = m->layers[l].qkv[0];
    p.pair = PAIR_ADJ;
    p.epi = EPI_STORE;
    p.K = m->hp.n_embd;
    p.out = qb;
    p.out_stride = m->hp.n_embd;
    p.bias = m->layers[l].bqkv;
    return p;
}

// GPT-2: FFN up + bias + GELU into hb (LLM_FFN_GELU, LLM_FFN_SEQ)
GemmParams Ctx::bup_gelu_params(int l, int nt) const {
    GemmParams p = gemm_base(l, nt, false);
    p.A = m->layers[l].up;
    p.pair = PAIR_ADJ;
    p.epi = EPI_GELU;
    p.K = m->hp.n_embd;
    p.out = hb;
    p.out_stride = m->hp.n_ff;
    p.bias = m->layers[l].bup;
    p.gelu_tab = m->gelu_tab;
    return p;
}

// causal attention of the batch's tokens, qb -> attnb
AttnParams Ctx::battn_params(int l) const {
    const HParams& hp = m->hp;
    return AttnParams{qb, k_layer(l), v_layer(l), tokpos_b, cell_pos, attn_scores, attn_smax, attnb, hp.n_head, hp.n_head_kv,
                      hp.head_dim, kv_dim, (int)n_ctx, kq_scale()};
}

Ctx::QkvGroups Ctx::qkv_type_groups(const Layer& L) {
    const QMat* mats[3] = {&L.wq, &L.wk, &L.wv};
    QkvGroups G{};
    G.fmt = act_fmt({L.wq.type, L.wk.type, L.wv.type});
    for (int i = 0; i < 3; ++i) {   // (7B: Q/K/V, or Q/K plus a Q6_K V)
        bool first = true;
        for (int j = 0; j < i; ++j) first = first && mats[j]->type != mats[i]->type;
        if (!first) continue;
        for (int j = i; j < 3; ++j)
            if (mats[j]->type == mats[i]->type) G.idx[G.n][G.cnt[G.n]++] = j;
        ++G.n;
    }
    return G;
}

int Ctx::mmqs_one(const QMat& A, bool pair, int nff, const ActQ8& act, int pstride) {
    const QMat* mo[1] = {&A};
    const int pr[1] = {0};
    return launch_mmqs(mo, pr, 1, pair, nff, act, ub_spart, pstride, stream);
}

void Ctx::finish_logits_all(int c0, int nt, bool last) {
    if (!last) return;
    const int nv = m->hp.n_vocab;
    MI_HIP(hipMemcpyAsync(logits, logits_all + (size_t)(c0 + nt - 1) * nv, (size_t)nv * sizeof(float), hipMemcpyDeviceToDevice,
                          stream));
    run_topk(logits);
}

// Prompt ingestion: n tokens in chunks of GEMM_NT, every weight matrix streamed once per
// chunk (launch_gemm), causal attention of the chunk's tokens (launch_attn_multi), the
// output head for the last token only (llama_batch_get_one: logits of the last token).
void Ctx::decode_batch(const int32_t* tokens, int n) {
    const HParams& hp = m->hp;
    // one projection on the v_dot4 GEMM, which quantises its own rows [ntok][K] of x
    auto proj = [&](GemmParams p, const float* x, const float* norm) {
        p.units = p.pair == PAIR_AB ? p.A.rows : (p.A.rows + 1) / 2;
        p.x = x;
        p.x_stride = p.K;
        p.norm_w = norm;
        p.pro = norm ? PRO_RMSNORM : PRO_PLAIN;
        launch_gemm(p, stream);
    };
    for (int c0 = 0; c0 < n; c0 += GEMM_NT) {
        const int nt = std::min(GEMM_NT, n - c0);
        upload_batch(tokens + c0, nt);
        EmbedParams ep{m->tok_embd, tokpos_b, xb, hp.n_embd};
        launch_embed_multi(ep, nt, stream);
        for (int l = 0; l < hp.n_layer; ++l) {
            const Layer& L = m->layers[l];
            // LoRA: each group's terms of the chunk ahead of the launches that add them
            const float* pre = lora_pre_terms(l, 0, xb, hp.n_embd, nt, L.attn_norm);
            for (int i = 0; i < 3; ++i) proj(bqkv_params(l, nt, true, i, pre), xb, L.attn_norm);
            launch_attn_multi(battn_params(l), nt, attnb, stream);
            pre = lora_pre_terms(l, 1, attnb, hp.n_embd, nt, nullptr);
            proj(bwo_params(l, nt, true, pre), attnb, nullptr);
            pre = lora_pre_terms(l, 2, xb, hp.n_embd, nt, L.ffn_norm);
            proj(bgate_up_params(l, nt, true, pre), xb, L.ffn_norm);
            pre = lora_pre_terms(l, 3, hb, hp.n_ff, nt, nullptr);
            proj(bdown_params(l, nt, true, pre), hb, nullptr);
        }
        if (embeddings) embd_tail(xb, nt, c0);   // embeddings mode: the chunk's rows, no head
        else if (c0 + nt == n) enqueue_output(ACT_PRO, xb + (size_t)(nt - 1) * hp.n_embd, nullptr);
    }
    logits_valid = !embeddings;
}

// build_moe_ffn's routing (src/llama-graph.cpp, b5187: softmax gating, top-2, weights normalised)
// over a physical batch, on the device: the router of every token (the decode step's
// router_kernel), the (token, slot) picks grouped by expert (launch_moe_group: tokens ascending
// within an expert, each expert's rows whole 32-row MFMA tiles).  No host round trip.
int Ctx::moe_route(int l, int nt, const float* pend) {
    const HParams& hp = m->hp;
    const Layer& L = m->layers[l];
    const int U = hp.n_expert_used, E = hp.n_expert;
    RouterParams rp{xb, L.ffn_norm, hp.eps, L.router, hp.n_embd, E, U, sel_b, selw_b, hp.n_embd, pend, nt};
    launch_router_multi(rp, nt, stream);
    const int cap = moe_rows_cap(nt * U, E);
    launch_moe_group(sel_b, nt * U, U, E, moe_grp, moe_rows, moe_rowsel, moe_pos, cap, stream);
    return cap;
}

ActQ8 Ctx::moe_act(int K, int cap, bool q80) const {
    ActQ8 a;
    a.q = moe_q;
    a.dT = moe_dT;
    a.bsb = moe_bsb;
    a.K = K;
    a.ntok = cap;
    a.npad = cap;
    a.q80 = q80 ? 1 : 0;
    return a;
}

// ---- what launch_quant_act quantises (engine.h) ----
QuantAct Ctx::qa_rows(const float* x, int K) const {
    QuantAct q{};
    q.x = x;
    q.x_stride = K;
    q.eps = m->hp.eps;
    return q;
}
QuantAct Ctx::qa_norm(const float* x, int K, const float* norm_w, PendParts pend) const {
    QuantAct q = qa_rows(x, K);
    q.norm_w = norm_w;
    if (pend.part) {
        q.part = pend.part;
        q.nks = pend.nks;
        q.addend = pend.addend;
    }
    return q;
}
QuantAct Ctx::qa_layernorm(const float* x, int K, const float* norm_w, const float* norm_b) const {
    QuantAct q = qa_norm(x, K, norm_w);
    q.norm_b = norm_b;
    return q;
}
QuantAct Ctx::qa_swiglu(const float* part, int nks, int K) const {
    QuantAct q{};
    q.x_stride = K;
    q.eps = m->hp.eps;
    q.part = part;
    q.nks = nks;
    q.swiglu = 1;
    return q;
}
// the plain sum of kp parts [kp][ntok][pstride] over `rows` rows into out (the caller adds a
// residual, an addend or SwiGLU by name)
static PartSum part_sum(const float* part, int kp, int ntok, int rows, int pstride, float* out, int ostride) {
    PartSum p{};
    p.part = part;
    p.kp = kp;
    p.ntok = ntok;
    p.rows = rows;
    p.pstride = pstride;
    p.out = out;
    p.ostride = ostride;
    return p;
}

// build_moe_ffn over a physical batch: routing, one quantisation of every row, ONE grouped mmq32
// launch for the experts' gate/up + SwiGLU and one for their down projections (a workgroup per
// (expert, row tile) over that expert's token tiles), then every token's x += w0*y0 + w1*y1 in
// slot order (launch_moe_combine, the decode GEMV's EPI_MOE_DOWN arithmetic).
void Ctx::moe_ffn_batch(int l, int nt, const float* pend) {
    const HParams& hp = m->hp;
    const Layer& L = m->layers[l];
    const int cap = moe_route(l, nt, pend);
    // gate/up + SwiGLU: rms_norm(x) * ffn_norm of each row's token
    const ActQ8 act = moe_act(hp.n_embd, cap, takes_q80(L.gate.type));
    QuantAct q = qa_norm(xb, hp.n_embd, L.ffn_norm);
    q.rows = moe_rows;
    launch_quant_act(q, act, stream);
    launch_mmq32(mmq32_params(L.gate, &L.up, cap, tokpos_b, hb, hp.n_ff, moe_grp, nt), act, ub_rope, stream);
    // down: every row of the FFN output, stored (weighted and summed by the combine)
    const ActQ8 a2 = moe_act(hp.n_ff, cap, takes_q80(L.down.type));
    q = qa_rows(hb, hp.n_ff);
    q.rows = moe_rowsel;
    launch_quant_act(q, a2, stream);
    launch_mmq32(mmq32_params(L.down, nullptr, cap, tokpos_b, yb, hp.n_embd, moe_grp, nt), a2, ub_rope, stream);
    launch_moe_combine(yb, moe_pos, selw_b, xb, nt, hp.n_embd, stream, cvec_for(l));
}

// The same build_moe_ffn over a short batch (<= MMQS_MAX tokens; x already holds the residual) on
// the grouped streaming GEMM: routing, one quantisation of every MoE row, the experts' gate/up
// pair parts (launch_mmqs_grouped: workgroups per (row tile, K-part, expert, 32-row tile), each
// expert's matrix streamed once for the rows routed to it), SwiGLU of the parts quantised for
// down, down's parts, their sum per row, then every token's x += w0*y0 + w1*y1 in slot order.
void Ctx::moe_ffn_short(int l, int nt) {
    const HParams& hp = m->hp;
    const Layer& L = m->layers[l];
    const int E = hp.n_expert;
    const int cap = moe_route(l, nt, nullptr);
    const ActQ8 act = moe_act(hp.n_embd, cap, false);
    QuantAct q = qa_norm(xb, hp.n_embd, L.ffn_norm);
    q.rows = moe_rows;
    launch_quant_act(q, act, stream);
    // an expert receives each token at most once: at most nt rows
    const int kg = launch_mmqs_grouped(L.gate, true, hp.n_ff, act, ub_spart, 2 * hp.n_ff, moe_grp, E, nt, stream);
    const ActQ8 a2 = moe_act(hp.n_ff, cap, false);
    q = qa_swiglu(ub_spart, kg, hp.n_ff);
    q.rows = moe_rowsel;   // (rows[t] < 0: a padding row)
    launch_quant_act(q, a2, stream);
    const int kd = launch_mmqs_grouped(L.down, false, 0, a2, ub_spart, hp.n_embd, moe_grp, E, nt, stream);
    launch_part_sum(part_sum(ub_spart, kd, cap, hp.n_embd, hp.n_embd, yb, hp.n_embd), stream);
    launch_moe_combine(yb, moe_pos, selw_b, xb, nt, hp.n_embd, stream, cvec_for(l));
}

ActQ8 Ctx::ub_act(int K, int ntok, int type) const {
    const bool q80 = takes_q80(type);
    const bool second = q80 && !ub_q80 && ub_q0;   // the Q8_0 set of a mixed model
    ActQ8 a;
    a.q = second ? ub_q0 : ub_q;
    a.dT = second ? ub_dT0 : ub_dT;
    a.bsb = ub_bsb;
    a.K = K;
    a.ntok = ntok;
    a.npad = (ntok + 31) / 32 * 32;
    a.q80 = q80 ? 1 : 0;
    return a;
}

// Prompt ingestion / batched verification in physical batches of up to UB_MAX tokens on the
// int8-MFMA GEMM (mmq.hip): per layer every weight matrix is streamed once per batch; each
// activation is quantised to Q8_K once (RMSNorm fused) and shared by the matrices that read it.
// `all`: the output head runs over every token (rows of logits_all), else over the last one.
void Ctx::decode_ubatch(const int32_t* tokens, int n, bool all) {
    const HParams& hp = m->hp;
    for (int c0 = 0; c0 < n; c0 += UB_MAX) {
        const int nt = std::min(UB_MAX, n - c0);
        upload_batch(tokens + c0, nt);
        if (hp.arch == ARCH_GPT2) {   // llm_build_gpt2: every batch on the tiled form
            if (c0 == 0) batch_path = 2;
            enqueue_ubatch_gpt2(nt, all, c0, c0 + nt == n);
            continue;
        }
        // (a context with a LoRA adapter runs its short batches on the tiled form below, whose
        // epilogues take the adapter's terms; split-K is off for the W_o / down launches an adapter
        // targets, and pending parts are added by the quant_act that precedes every shrink)
        if (mmqs_max > 0 && nt <= mmqs_max && short_ok() && !lora_on()) {   // a short batch (its launches captured as a
            // hipGraph measured no faster: the GPU, not the enqueue, sets the pace)
            if (c0 == 0) batch_path = 3;
            enqueue_ubatch_short(nt, all, c0, c0 + nt == n);
            continue;
        }
        if (c0 == 0) batch_path = 2;
        EmbedParams ep{m->tok_embd, tokpos_b, xb, hp.n_embd};
        launch_embed_multi(ep, nt, stream);
        launch_rope_table(tokpos_b, nt, hp.n_rot, theta_scale(), hp.freq_scale, m->rope_freqs, ub_rope, stream);
        const float* pend = nullptr;   // split-K partials not yet added into xb (the next quant_act does)
        const float* pend_add = nullptr;   // the control-vector row that goes in after them (FFN down's parts)
        // split-K parts of the residual GEMMs: 4 for short batches of dense models (verification
        // of tens of tokens: more workgroups, a quarter of the superblock steps each; 4 x nt rows
        // fit the 2 x UB_MAX partials buffer), else 2 (the MoE router adds 2)
        const int ks = hp_dense() && nt <= 64 ? 4 : 2;   // 4 x 64 rows fit the 2 x UB_MAX partials buffer
        for (int l = 0; l < hp.n_layer; ++l) {
            const Layer& L = m->layers[l];
            // Q / K / V (+ RoPE, KV append) over one quantisation of rms_norm(x) * attn_norm per
            // activation format the three matrices read, the matrices of one type in one launch
            const QMat* mats[3] = {&L.wq, &L.wk, &L.wv};
            const QkvGroups G = qkv_type_groups(L);
            for (int f = 0; f < 2; ++f)
                if (G.fmt >> f & 1) {
                    launch_quant_act(qa_norm(xb, hp.n_embd, L.attn_norm, {pend, ks, pend_add}),
                                     ub_act(hp.n_embd, nt, f ? T_Q8_0 : T_Q4_K), stream);
                    pend = nullptr;
                }
            // LoRA: a group's terms of the batch after the quant_act of its input, before the GEMM
            const float* pre = lora_pre_terms(l, 0, xb, hp.n_embd, nt, L.attn_norm);
            for (int g = 0; g < G.n; ++g) {
                GemmParams ps[3];
                for (int k = 0; k < G.cnt[g]; ++k) ps[k] = bqkv_params(l, nt, false, G.idx[g][k], pre);
                launch_mmq32_multi(ps, G.cnt[g], ub_act(hp.n_embd, nt, mats[G.idx[g][0]]->type), ub_rope, stream);
            }
            if (attn_mfma) launch_attn_mfma(battn_params(l), nt, attnb, stream);
            else launch_attn_multi(battn_params(l), nt, attnb, stream);
            {   // output projection + residual
                const ActQ8 act = ub_act(hp.n_embd, nt, L.wo.type);
                launch_quant_act(qa_rows(attnb, hp.n_embd), act, stream);
                pre = lora_pre_terms(l, 1, attnb, hp.n_embd, nt, nullptr);
                GemmParams p = bwo_params(l, nt, false, pre);
                // parts of K; the FFN's quant_act adds them (not with an adapter on this W_o: its terms
                // go in ahead of the residual add, which a split launch leaves to the next kernel)
                if (ub_part && L.wo.nb >= ks && !pre) {
                    p.ksplit = ks;
                    p.part = ub_part;
                    pend = ub_part;
                }
                launch_mmq32(p, act, ub_rope, stream);
            }
            if (hp.n_expert > 0) {   // routed experts (build_moe_ffn) + residual
                moe_ffn_batch(l, nt, pend);
                pend = nullptr;
                continue;
            }
            {   // FFN gate/up + SwiGLU
                const ActQ8 act = ub_act(hp.n_embd, nt, L.gate.type);
                launch_quant_act(qa_norm(xb, hp.n_embd, L.ffn_norm, {pend, ks}), act, stream);   // (W_o's parts)
                pend = nullptr;
                pre = lora_pre_terms(l, 2, xb, hp.n_embd, nt, L.ffn_norm);
                launch_mmq32(bgate_up_params(l, nt, false, pre), act, ub_rope, stream);
            }
            {   // FFN down + residual
                const ActQ8 act = ub_act(hp.n_ff, nt, L.down.type);
                launch_quant_act(qa_rows(hb, hp.n_ff), act, stream);
                pre = lora_pre_terms(l, 3, hb, hp.n_ff, nt, nullptr);
                GemmParams p = bdown_params(l, nt, false, pre);
                if (ub_part && L.down.nb >= ks && l + 1 < hp.n_layer && !pre) {   // the next layer's quant_act adds them,
                    p.ksplit = ks;                                               // and the control vector's row after them
                    p.part = ub_part;
                    pend = ub_part;
                    pend_add = p.addend;
                    p.addend = nullptr;
                }
                launch_mmq32(p, act, ub_rope, stream);
            }
        }
        if (embeddings) {   // embeddings mode: the batch's result_norm rows (xb is whole: the last layer's down is not split)
            embd_tail(xb, nt, c0);
        } else if (all) {   // final norm + output head over every token of the batch
            const ActQ8 a_out = ub_act(hp.n_embd, nt, m->output.type);   // the head's own activation format
            launch_quant_act(qa_norm(xb, hp.n_embd, m->output_norm), a_out, stream);
            GemmParams p;
            std::memset(&p, 0, sizeof(p));
            p.A = m->output;
            p.pair = PAIR_ADJ;
            p.epi = EPI_STORE;
            p.K = hp.n_embd;
            p.ntok = nt;
            p.tokpos = tokpos_b;
            p.out = logits_all + (size_t)c0 * hp.n_vocab;
            p.out_stride = hp.n_vocab;
            launch_mmq32(p, a_out, ub_rope, stream);
            finish_logits_all(c0, nt, c0 + nt == n);
        } else if (c0 + nt == n) {
            enqueue_output(ACT_PRO, xb + (size_t)(nt - 1) * hp.n_embd, nullptr);
        }
    }
    logits_valid = !embeddings;
}

// One physical batch of a GPT-2 model (tokens uploaded to tokpos_b) on the tiled int8-MFMA GEMM:
// llm_build_gpt2 (b5187) with every matrix streamed once per batch and the arithmetic per token row
// of the decode step.  The rows are token row + position_embd row of the token's position.  Per
// layer, 8 launches:
//   quant_act  layer_norm(x) * attn_norm + attn_norm_b, quantised once
//   mmq2       attn_qkv as three row segments: (y + b) -> Q rows f32 in qb, K and V rows rounded to
//              f16 into the caches (no rotation), cell_pos written
//   attention  attn_mfma (any number of cells), else the fused form within ATTN_SHORT cells
//   quant_act  the attention rows
//   mmq2       attn_output: (y + b) + x, in place
//   quant_act  layer_norm(x) * ffn_norm + ffn_norm_b
//   mmq2       ffn_up: gelu(y + b) through ggml's f16 table into hb
//   quant_act  hb
//   mmq2       ffn_down: ((y + b) + x), then the control vector's row, in place
// No split-K: every residual GEMM writes xb itself.  The output as decode_ubatch's: every row's
// logits through the final LayerNorm and the tied head (`all`), the last row's through the decode
// head, or the embedding tail.
void Ctx::enqueue_ubatch_gpt2(int nt, bool all, int c0, bool last) {
    const HParams& hp = m->hp;
    const int ne = hp.n_embd;
    EmbedParams ep{m->tok_embd, tokpos_b, xb, ne, m->pos_embd, 1, nullptr};
    launch_embed_multi(ep, nt, stream);
    // a row set quantised for the matrix `type` reads
    auto quant = [&](const QuantAct& q, int type) {
        const ActQ8 act = ub_act(q.x_stride, nt, type);
        launch_quant_act(q, act, stream);
        return act;
    };
    for (int l = 0; l < hp.n_layer; ++l) {
        const Layer& L = m->layers[l];
        {
            const ActQ8 act = quant(qa_layernorm(xb, ne, L.attn_norm, L.attn_norm_b), L.qkv[0].type);
            const int row0[3] = {0, ne, 2 * ne}, nrows[3] = {ne, ne, ne};
            const int epi[3] = {EPI_STORE, EPI_ROPE_K, EPI_V};   // (n_rot 0: K rows unrotated)
            launch_mmq32_rows(bqkv_gpt2_params(l, nt), row0, nrows, epi, 3, act, ub_rope, stream);
        }
        if (attn_mfma) launch_attn_mfma(battn_params(l), nt, attnb, stream);
        else launch_attn_multi(battn_params(l), nt, attnb, stream);
        launch_mmq32(bwo_params(l, nt, false, nullptr), quant(qa_rows(attnb, ne), L.wo.type), ub_rope, stream);
        launch_mmq32(bup_gelu_params(l, nt), quant(qa_layernorm(xb, ne, L.ffn_norm, L.ffn_norm_b), L.up.type), ub_rope, stream);
        launch_mmq32(bdown_params(l, nt, false, nullptr), quant(qa_rows(hb, hp.n_ff), L.down.type), ub_rope, stream);
    }
    if (embeddings) {
        embd_tail(xb, nt, c0);
    } else if (all) {   // final LayerNorm + the tied head over every token of the batch
        const ActQ8 a_out = quant(qa_layernorm(xb, ne, m->output_norm, m->output_norm_b), m->output.type);
        launch_mmq32(mmq32_params(m->output, nullptr, nt, tokpos_b, logits_all + (size_t)c0 * hp.n_vocab, hp.n_vocab), a_out,
                     ub_rope, stream);
        finish_logits_all(c0, nt, last);
    } else if (last) {
        enqueue_output(ACT_PRO, xb + (size_t)(nt - 1) * ne, nullptr);
    }
}

// ================================================== unquantised F16 models ===
void Ctx::f16_gemm(const QMat* const* mats, float* const* outs, int n, const float* x, int nt, int out_stride,
                   const float* resid) {
    EncGemm g;
    std::memset(&g, 0, sizeof(g));
    for (int i = 0; i < n; ++i) {
        g.m[i].w = reinterpret_cast<const __half*>(mats[i]->p[0]);
        g.m[i].rows = mats[i]->rows;
        g.m[i].out = outs[i];
    }
    g.nmat = n;
    g.epi = resid ? ENC_ADD : ENC_NONE;
    g.K = mats[0]->K;
    g.ntok = nt;
    g.x = x;
    g.x_stride = g.K;
    g.out_stride = out_stride;
    g.resid = resid;
    launch_enc_gemm(g, stream);
}

// Prompt ingestion / batched verification of an F16 model in physical batches of up to kBatchRows
// tokens on the F16 MFMA GEMM (enc.hip): the layer of llm_build_llama with every matrix streamed
// once per batch.  Per layer: norm rows, Q | K | V raw rows in one launch, RoPE + KV append
// (qkv_finish, one part), causal attention, WO + residual, norm rows, gate | up raw rows, SwiGLU,
// down + residual (the control vector's row by a pass of its own).  `all`: the head over every
// token (rows of logits_all), else over the last one.
void Ctx::decode_f16_batch(const int32_t* tokens, int n, bool all) {
    const HParams& hp = m->hp;
    const int ne = hp.n_embd, nff = hp.n_ff;
    for (int c0 = 0; c0 < n; c0 += kBatchRows) {
        const int nt = std::min((int)kBatchRows, n - c0);
        upload_batch(tokens + c0, nt);
        EmbedParams ep{m->tok_embd, tokpos_b, xb, ne};
        launch_embed_multi(ep, nt, stream);
        launch_rope_table(tokpos_b, nt, hp.n_rot, theta_scale(), hp.freq_scale, m->rope_freqs, ub_rope, stream);
        for (int l = 0; l < hp.n_layer; ++l) {
            const Layer& L = m->layers[l];
            f16_norm(xb, nt, L.attn_norm, fb_xn);
            {
                const QMat* ms[3] = {&L.wq, &L.wk, &L.wv};
                float* os[3] = {fb_t, fb_t + ne, fb_t + ne + kv_dim};
                f16_gemm(ms, os, 3, fb_xn, nt, fb_t_stride, nullptr);
            }
            QkvFinish F{fb_t, fb_t_stride, 1, nt, L.wq.rows, L.wk.rows, L.wv.rows, qb, ne, k_layer(l), v_layer(l), kv_dim,
                        cell_pos, tokpos_b, ub_rope, hp.n_rot, hp.head_dim};
            launch_qkv_finish(F, stream);
            if (attn_mfma) launch_attn_mfma(battn_params(l), nt, attnb, stream);
            else launch_attn_multi(battn_params(l), nt, attnb, stream);
            {
                const QMat* ms[1] = {&L.wo};
                float* os[1] = {xb};
                f16_gemm(ms, os, 1, attnb, nt, ne, xb);
            }
            f16_norm(xb, nt, L.ffn_norm, fb_xn);
            {
                const QMat* ms[2] = {&L.gate, &L.up};
                float* os[2] = {fb_t, fb_t + nff};
                f16_gemm(ms, os, 2, fb_xn, nt, fb_t_stride, nullptr);
            }
            {   // silu(gate) * up
                PartSum ps = part_sum(fb_t, 1, nt, nff, fb_t_stride, hb, nff);
                ps.swiglu = nff;
                launch_part_sum(ps, stream);
            }
            {
                const QMat* ms[1] = {&L.down};
                float* os[1] = {xb};
                f16_gemm(ms, os, 1, hb, nt, ne, xb);
            }
            if (const float* cv = cvec_for(l)) {   // build_cvec: after the FFN residual add (the row as the "residual")
                PartSum ps = part_sum(xb, 1, nt, ne, ne, xb, ne);
                ps.resid = cv;
                ps.rstride = 0;
                launch_part_sum(ps, stream);
            }
        }
        const bool last = c0 + nt == n;
        if (embeddings) {
            embd_tail(xb, nt, c0);
        } else if (all) {   // final norm + output head over every token of the batch
            f16_norm(xb, nt, m->output_norm, fb_xn);
            const QMat* ms[1] = {&m->output};
            float* os[1] = {logits_all + (size_t)c0 * hp.n_vocab};
            f16_gemm(ms, os, 1, fb_xn, nt, hp.n_vocab, nullptr);
            finish_logits_all(c0, nt, last);
        } else if (last) {   // the last token's row through the decode step's head
            f16_norm(xb + (size_t)(nt - 1) * ne, 1, m->output_norm, f_xn);
            launch_fgemv(fhead_params(), stream);
            run_topk(logits);
        }
    }
    logits_valid = !embeddings;
}

// One short physical batch (tokens uploaded to tokpos_b): embedding, the rope table, the layers on
// mmqs, then the output -- every token's logits rows (`all`, rows c0.. of logits_all; the last
// chunk's last row also feeds `logits` and the top-k) or the last token's through the decode head;
// in embeddings mode the embedding tail over xb once the pending parts are in.
void Ctx::enqueue_ubatch_short(int nt, bool all, int c0, bool last) {
    const HParams& hp = m->hp;
    EmbedParams ep{m->tok_embd, tokpos_b, xb, hp.n_embd};
    launch_embed_multi(ep, nt, stream);
    launch_rope_table(tokpos_b, nt, hp.n_rot, theta_scale(), hp.freq_scale, m->rope_freqs, ub_rope, stream);
    const int pend_k = ubatch_layers_short(nt);
    // (the parts pending are the last layer's FFN down's -- dense models; its control-vector row
    // goes in with them)
    PendParts pend{};
    if (pend_k) pend = {ub_spart, pend_k, cvec_for(hp.n_layer - 1)};
    if (all && !embeddings) {   // final norm + output head on mmqs, its parts summed into the logits rows
        const ActQ8 a_out = ub_act(hp.n_embd, nt, m->output.type);
        launch_quant_act(qa_norm(xb, hp.n_embd, m->output_norm, pend), a_out, stream);
        const int kp = mmqs_one(m->output, false, 0, a_out, hp.n_vocab);
        launch_part_sum(part_sum(ub_spart, kp, nt, hp.n_vocab, hp.n_vocab, logits_all + (size_t)c0 * hp.n_vocab, hp.n_vocab),
                        stream);
        finish_logits_all(c0, nt, last);
    } else {
        // the last residual parts into xb (the next chunk, or the output, reads it)
        if (pend_k) {
            PartSum ps = part_sum(ub_spart, pend_k, nt, hp.n_embd, hp.n_embd, xb, hp.n_embd);
            ps.resid = xb;
            ps.rstride = hp.n_embd;
            ps.addend = pend.addend;
            launch_part_sum(ps, stream);
        }
        if (embeddings) embd_tail(xb, nt, c0);   // embeddings mode: the rows of the now whole xb, no head
        else if (last) enqueue_output(ACT_PRO, xb + (size_t)(nt - 1) * hp.n_embd, nullptr);
    }
}

// One short physical batch (<= mmqs_max tokens) through the layers on the split-K streaming GEMM
// (mmqs.hip): every launch writes K-part sums to ub_spart, and the next kernel adds them --
// quant_act (the residual, or SwiGLU of the gate/up parts), qkv_finish (RoPE, KV append).
// Returns the count of the last FFN down's parts, still to be added into xb.
int Ctx::ubatch_layers_short(int nt) {
    const HParams& hp = m->hp;
    const int qkv_rows = hp.n_embd + 2 * kv_dim;
    int pend_k = 0;   // residual parts of ub_spart not yet added into xb
    for (int l = 0; l < hp.n_layer; ++l) {
        const Layer& L = m->layers[l];
        // Q / K / V: one quantisation of rms_norm(x) * attn_norm per activation format (the first
        // also adds the residual parts), the matrices of one type in one launch, rows [Q | K | V]
        const QMat* mats[3] = {&L.wq, &L.wk, &L.wv};
        const QkvGroups G = qkv_type_groups(L);
        for (int f = 0; f < 2; ++f)
            if (G.fmt >> f & 1) {
                // (parts pending here are the previous layer's FFN down's: its control-vector row with them)
                PendParts pend{};
                if (pend_k) pend = {ub_spart, pend_k, l > 0 ? cvec_for(l - 1) : nullptr};
                launch_quant_act(qa_norm(xb, hp.n_embd, L.attn_norm, pend), ub_act(hp.n_embd, nt, f ? T_Q8_0 : T_Q4_K), stream);
                pend_k = 0;
            }
        int kp = 0;
        for (int g = 0; g < G.n; ++g) {
            const QMat* ms[3];
            int pr[3];
            for (int k = 0; k < G.cnt[g]; ++k) {
                ms[k] = mats[G.idx[g][k]];
                pr[k] = lora_pre_row(l, 0, G.idx[g][k]);   // the parts' rows share the [Q | K | V] layout
            }
            kp = launch_mmqs(ms, pr, G.cnt[g], false, 0, ub_act(hp.n_embd, nt, ms[0]->type), ub_spart, qkv_rows, stream);
        }
        QkvFinish F{ub_spart, qkv_rows, kp, nt, L.wq.rows, L.wk.rows, L.wv.rows, qb, hp.n_embd, k_layer(l), v_layer(l), kv_dim,
                    cell_pos, tokpos_b, ub_rope, hp.n_rot, hp.head_dim};
        launch_qkv_finish(F, stream);
        AttnParams a = battn_params(l);
        // within ATTN_SHORT cells the decode step's kernel (attn_plan's ATTN_BATCH_QUANT /
        // ATTN_BATCH_FUSED), one grid row per token
        // (20-token verify 3.52 -> 3.30 ms against the MFMA kernel's 32-token tiles; 64 tokens
        // equal, same box)
        const ActQ8 act_wo = ub_act(hp.n_embd, nt, L.wo.type);
        const bool qattn = attn_quant_supported(hp.n_head, hp.n_head_kv, hp.head_dim);
        if (attn_mfma && n_cells > ATTN_SHORT) {
            launch_attn_mfma(a, nt, attnb, stream);
            launch_quant_act(qa_rows(attnb, hp.n_embd), act_wo, stream);
        } else if (qattn) {   // the launch also quantises each token's output for W_o
            a.act_q8 = act_wo;
            launch_attn_multi(a, nt, attnb, stream);
        } else {
            launch_attn_multi(a, nt, attnb, stream);
            launch_quant_act(qa_rows(attnb, hp.n_embd), act_wo, stream);
        }
        // output projection: parts of W_o attn, added to x by the FFN's quant_act
        pend_k = mmqs_one(L.wo, false, 0, act_wo, hp.n_embd);
        if (hp.n_expert > 0) {   // routed experts: x += W_o parts first (the router reads x)
            PartSum ps = part_sum(ub_spart, pend_k, nt, hp.n_embd, hp.n_embd, xb, hp.n_embd);
            ps.resid = xb;
            ps.rstride = hp.n_embd;
            launch_part_sum(ps, stream);
            pend_k = 0;
            moe_ffn_short(l, nt);
            continue;
        }
        // FFN gate/up: parts of both, SwiGLU'd by the down input's quant_act
        const ActQ8 act = ub_act(hp.n_embd, nt, L.gate.type);
        launch_quant_act(qa_norm(xb, hp.n_embd, L.ffn_norm, {ub_spart, pend_k}), act, stream);   // (W_o's parts)
        const int kg = mmqs_one(L.gate, true, hp.n_ff, act, 2 * hp.n_ff);
        const ActQ8 a2 = ub_act(hp.n_ff, nt, L.down.type);
        launch_quant_act(qa_swiglu(ub_spart, kg, hp.n_ff), a2, stream);
        pend_k = mmqs_one(L.down, false, 0, a2, hp.n_embd);
    }
    return pend_k;
}

}  // namespace mi
