// Engine internals: GGUF parsing and the device-resident model (model.cpp), the decode context
// (engine.cpp: buffers, the decode step, graphs, sampling reads, KV cache, state; batch.cpp: the
// prompt-batch paths; lora.cpp: adapters).  The public surface is the C ABI in include/mi_engine.h:
// capi.cpp implements the product's entry points, ops.cpp the op-level ones (mi_op_*) the tests
// reach single kernels through.
#pragma once
#include <mutex>
#include <cmath>
#include <cstdlib>
#include "common.h"
#include "kernels.h"
#include "mi_engine.h"

#include <map>
#include <memory>
#include <string>
#include <vector>

namespace mi {

// ---------------------------------------------------------------- GGUF ----
struct GgufValue {
    int type = -1;                // gguf_type
    long long i = 0;
    double f = 0.0;
    std::string s;
    int arr_type = -1;
    long long arr_n = 0;
    std::vector<std::string> arr_s;
    std::vector<double> arr_num;
};

struct GgufTensor {
    std::string name;
    int type = 0;
    int n_dims = 0;
    long long ne[4] = {1, 1, 1, 1};
    unsigned long long offset = 0;   // within the data section
    size_t nbytes = 0;
};

struct Gguf {
    std::map<std::string, GgufValue> kv;
    std::vector<GgufTensor> tensors;
    size_t data_offset = 0;          // start of the data section in the file
    // parse the header (metadata + tensor infos) from a memory image
    void parse(const uint8_t* data, size_t size);
    const GgufValue* get(const std::string& k) const {
        auto it = kv.find(k);
        return it == kv.end() ? nullptr : &it->second;
    }
    long long get_int(const std::string& k, long long def) const;
    double get_float(const std::string& k, double def) const;
    std::string get_str(const std::string& k, const std::string& def) const;
    const GgufTensor* tensor(const std::string& name) const;
};

// --------------------------------------------------------------- model ----
std::vector<unsigned short> gelu_table_host();   // ggml_table_gelu_f16, built on the host (model.cpp)

struct HParams {
    int n_vocab = 0, n_embd = 0, n_layer = 0, n_head = 0, n_head_kv = 0, n_ff = 0, n_ctx_train = 0;
    int n_rot = 0, head_dim = 0, n_expert = 0, n_expert_used = 0;
    float eps = 1e-5f, rope_base = 10000.0f, freq_scale = 1.0f;
    int arch = 0;                       // ARCH_LLAMA (llm_build_llama), ARCH_GPT2 (llm_build_gpt2) or ARCH_BERT (llm_build_bert)
    int pooling_type = -1;              // {arch}.pooling_type (llama_pooling_type), -1: the GGUF has none
};
enum { ARCH_LLAMA = 0, ARCH_GPT2 = 1, ARCH_BERT = 2 };

struct Layer {
    float* attn_norm = nullptr;
    float* ffn_norm = nullptr;
    QMat wq{}, wk{}, wv{}, wo{};
    QMat gate{}, up{}, down{};          // dense FFN, or the *_exps tensors for MoE
    float* router = nullptr;            // ffn_gate_inp (F32) for MoE
    // Q, K, V as 1-3 groups of adjacent same-type rows (the arena stores the planes of a group's
    // tensors back to back, so a group is one matrix to the decode GEMV): group g holds nq[g] Q
    // rows, then nk[g] K rows, then V rows
    int n_qkv = 0;
    QMat qkv[3]{};
    int qkv_nq[3] = {0, 0, 0}, qkv_nk[3] = {0, 0, 0};
    // GPT-2: LayerNorm biases and the projection biases (attn_qkv is the one fused QKV group)
    float *attn_norm_b = nullptr, *ffn_norm_b = nullptr;
    float *bqkv = nullptr, *bo = nullptr, *bup = nullptr, *bdown = nullptr;
};

// A layer of an encoder model (llm_build_bert): F16 matrices [rows][K], F32 biases and LayerNorms
struct EncLayer {
    const __half *wq = nullptr, *wk = nullptr, *wv = nullptr, *wo = nullptr, *up = nullptr, *down = nullptr;
    const float *bq = nullptr, *bk = nullptr, *bv = nullptr, *bo = nullptr, *bup = nullptr, *bdown = nullptr;
    const float *attn_out_norm = nullptr, *attn_out_norm_b = nullptr;     // attn_output_norm
    const float *layer_out_norm = nullptr, *layer_out_norm_b = nullptr;   // layer_output_norm
};

struct Model {
    HParams hp;
    Gguf gguf;
    std::vector<std::string> tokens;
    std::vector<int> token_type;
    std::vector<float> token_score;     // SPM merge scores (tokenizer.ggml.scores)
    std::string tok_model;              // tokenizer.ggml.model ("llama" = SPM, "gpt2" = BPE)
    std::vector<std::string> merges;    // tokenizer.ggml.merges (BPE: "left right", rank = index)
    int bos = -1, eos = -1, eot = -1;
    bool add_bos = true;
    int device = 0;
    bool vocab_only = false;
    // An unquantised model: a dense LLaMA graph (n_expert == 0) whose matrices -- token_embd, output
    // (absent: the head is token_embd, a tied model) and the seven per layer -- are all F16; norm
    // weights and rope_freqs F32.  The matrices stay plain [rows][K] f16 rows in the arena (QMat::p[0],
    // type T_F16): no planes, no MFMA-order copy (ensure_mmq_copies has nothing to do).
    // Shape rules (check_f16, refused with a message otherwise): n_embd = n_head x head_dim, n_head a
    // multiple of n_head_kv; n_embd and n_ff multiples of 32, at most 16384 (fgemv.hip: K);
    // n_head_kv x head_dim and n_vocab multiples of 32 (the batch GEMM's 32-row tiles); n_rot even.
    // Refused: BF16 or F32 matrices, F16 mixed with quantised matrices, F16 MoE, F16 GPT-2.  LoRA
    // adapters on an F16 model are out of scope: Lora::load refuses it.
    bool f16 = false;
    bool check_f16() const;
    // Q4_0 / Q5_0 matrices (32-weight blocks, f16 scale, Q8_0 activations as Q8_0's): served in a
    // dense LLaMA graph, alone (llama-quantize's Q4_0 / Q5_0 files, head Q6_K) or inside a k-quant
    // file.  check_types reads the header only: true when a matrix has one of the two types; refuses,
    // with the tensor and the type's name, such a matrix in a MoE, GPT-2 or BERT model and a matrix of
    // a quantised type no kernel here reads (Q4_1, Q5_1 -- Q8_1 activations --, Q2_K, Q3_K, IQ*, TQ*).
    bool legacy = false;
    bool check_types() const;
    void account(const GgufTensor& t, int experts);   // weight_bytes, type_bytes

    uint8_t* arena = nullptr;
    size_t arena_bytes = 0;
    // MFMA-order copies of the layer matrices and the output head for prompt batches (mmq32),
    // built from the arena on the device the first time a context needs them (replicas build
    // their own after the arena broadcast): one more weight-sized allocation, HBM for speed
    uint8_t* mmq_arena = nullptr;
    size_t mmq_bytes = 0;
    std::mutex mmq_mu;
    // false when the copy does not fit (the batch path then uses the v_dot4 GEMM).  The copies are
    // taken from the arena once: writes to the arena (mi_model_arena, mi_model_replicate) must
    // come before the first context (mi_model_replicate checks this).
    bool ensure_mmq_copies();
    long long weight_bytes = 0;         // GGUF bytes streamed per token (all but tok_embd)
    long long type_bytes[32] = {0};

    QMat tok_embd{};
    QMat pos_embd{};                    // GPT-2 learned positions (position_embd.weight)
    QMat output{};
    float* output_norm = nullptr;
    float* output_norm_b = nullptr;     // GPT-2
    unsigned short* gelu_tab = nullptr; // GPT-2: ggml_table_gelu_f16 on the device
    float* rope_freqs = nullptr;
    std::vector<Layer> layers;
    // BERT: the token-type table (row 0 is added to every token), the embedding LayerNorm, the layers
    QMat tok_types{};
    const float *embd_norm = nullptr, *embd_norm_b = nullptr;
    std::vector<EncLayer> enc_layers;

    ~Model();
    // data: the GGUF image (header at least; tensor data unless no_upload/vocab_only)
    void load(const uint8_t* data, size_t size, const mi_model_params& p);
    const QMat* find_qmat(const std::string& name) const;
};

// m's planes hold n_exp matrices of equal rows, stacked (a MoE *_exps tensor; dense: 1): rows,
// n_exp and expert_stride[] become one expert's
void split_experts(QMat& m, int n_exp);
// Expert e of a MoE tensor as a matrix of its own (planes and MFMA-order copy offset).
QMat expert_view(const QMat& q, int e);
// One MFMA-order copy per expert of A (B set: gate and up in one) into dst, expert e's
// mmq32_copy_bytes at dst + e * A.sw_expert_stride; enqueued, not synchronised
void build_mmq_copies(QMat& A, const QMat* B, uint8_t* dst);

// ---------------------------------------------------------------- LoRA ----
// A LoRA adapter file (llama_adapter_lora_init, src/llama-adapter.cpp b5187), parsed and validated
// against its base model (lora.cpp).  It keeps the pairs as they stand in the file; a context that
// is given the adapter builds its device stacks from them (Ctx::lora_rebuild) and shares ownership,
// so the handle may be freed while a context still uses it.
enum LoraTarget { LT_Q = 0, LT_K, LT_V, LT_O, LT_GATE, LT_UP, LT_DOWN, LT_N };
struct LoraPair {
    int layer = 0, target = 0;
    int r = 0, K = 0, rows = 0;          // A [r][K], B [rows][r] (row-major, as in the file)
    int a_type = T_F32, b_type = T_F32;  // T_F16 or T_F32
    std::vector<uint8_t> a, b;           // empty for a vocab_only model (validation only)
};
struct Lora {
    const Model* m = nullptr;
    float alpha = 0.0f;
    std::vector<LoraPair> pairs;
    // throws Error naming the tensor or the reason
    static std::shared_ptr<Lora> load(const Model* m, const uint8_t* data, size_t size);
};

// ------------------------------------------------------------- context ----
int dev_chain_contexts(int device);   // live contexts on the device

// A decode launch's segment of one matrix (dense: no experts, no bias, no residual yet)
GemvSeg seg_of(const QMat& A, int pair, int epi, float* out);
// The routed experts' two decode launches on gemv_kernel, over plain arguments (the caller sets
// the activation).  Gate/up: experts sel[0] and sel[1] of the pair + SwiGLU into h and h2.  Down:
// x = (down[sel[0]] h * selw[0] + down[sel[1]] h2 * selw[1]) + x [+ addend], in place.
void moe_gate_up_segs(GemvParams& p, const QMat& gate, const QMat& up, const int* sel, const float* selw, float* h,
                      float* h2);
void moe_down_seg(GemvParams& p, const QMat& down, const int* sel, const float* selw, const float* h2, float* x,
                  const float* addend);
// mmq32's launch of A (B set: the gate/up pair + SwiGLU, else a store) over ntok activation rows
// into out [ntok][out_stride] (batch.cpp).  grp set: launch_moe_group's table, the rows grouped by
// A's experts, at most grp_max rows each.
GemmParams mmq32_params(const QMat& A, const QMat* B, int ntok, const int* tokpos, float* out, int out_stride,
                        const int* grp = nullptr, int grp_max = 0);
// activation formats a set of matrices reads: bit 0 Q8_K (k-quants), bit 1 Q8_0
int act_fmt(std::initializer_list<int> types);
void ensure_kernel_attributes(int device);   // init_kernel_attributes, once per device
int mmqs_token_limit();                      // short batches: MMQS_MAX tokens, or MI_MMQS_MAX below it (0: off)

// Owner of a context's device buffers, pinned host buffers, stream and events: one hipMalloc /
// hipHostMalloc per buffer, every one recorded and released by the destructor -- which, as Ctx's
// first member, also runs when Ctx's constructor throws part-way.
struct CtxMem {
    std::vector<void*> dev_ptrs, host_ptrs;
    std::vector<hipEvent_t> events;
    hipStream_t stream_ = nullptr;
    CtxMem() = default;
    CtxMem(const CtxMem&) = delete;
    CtxMem& operator=(const CtxMem&) = delete;
    ~CtxMem();
    void* dev_bytes(size_t bytes, bool zero);
    void* host_bytes(size_t bytes, unsigned flags);
    template <class T> T* dev(size_t n, bool zero = false) { return static_cast<T*>(dev_bytes(n * sizeof(T), zero)); }
    // pinned host memory (flags: hipHostMallocMapped | hipHostMallocCoherent for kernel-written buffers)
    template <class T> T* host(size_t n, unsigned flags = hipHostMallocDefault) {
        return static_cast<T*>(host_bytes(n * sizeof(T), flags));
    }
    // frees one buffer of either kind now and nulls p (null: nothing); for buffers that grow
    template <class T> void release(T*& p) {
        free_one(p);
        p = nullptr;
    }
    void free_one(void* p);
    hipStream_t stream();    // the context's stream, created on the first call
    hipEvent_t event();
};

struct Ctx {
    CtxMem mem;                         // first: released last, and on a throwing constructor
    Model* m = nullptr;
    int device = 0;
    uint32_t n_ctx = 0, n_batch = 0, n_ubatch = 0;
    int kv_dim = 0;
    hipStream_t stream = nullptr;       // mem's

    // device buffers
    __half* kcache = nullptr;           // [n_layer][n_ctx][kv_dim]
    __half* vcache = nullptr;
    __half* kv_scratch = nullptr;       // compaction scratch (allocated lazily)
    int* cell_pos = nullptr;            // [n_ctx]
    int* tokpos = nullptr;              // {token, pos, cell, 0}
    float *x = nullptr, *q = nullptr, *attn = nullptr, *h = nullptr, *h2 = nullptr, *logits = nullptr;
    unsigned long long* cand = nullptr;
    int* topk_ids = nullptr;
    float* topk_vals = nullptr;
    int* sel = nullptr;
    float* selw = nullptr;
    int* gather_ids = nullptr;
    float* gather_out = nullptr;
    int* cell_delta = nullptr;
    int* move_src = nullptr;
    float* part_o = nullptr;            // split-K attention partials [ATTN_SMAX][n_head][hd]
    float* attn_smax = nullptr;         // [ATTN_SMAX][n_head] split maxima
    float* attn_scores = nullptr;       // [n_head][n_ctx] scaled KQ
    // the single-launch long-context attention's exchange (attn_long_kernel) and the step counter
    unsigned* attn_xflags = nullptr;    // [n_head][ATTN_SMAX][32]
    float* attn_xmax = nullptr;
    double* attn_xsum = nullptr;
    unsigned* step_ctr = nullptr;       // decode steps so far (incremented by the embedding launch)
    unsigned* h_attn_xerr = nullptr;    // host-mapped: an exchange timed out
    unsigned* d_attn_xerr = nullptr;
    // batched prompt ingestion (LLaMA, GPT-2): kBatchRows rows of residual / q / attention / FFN
    bool batch_ok = false;
    float *xb = nullptr, *qb = nullptr, *attnb = nullptr, *hb = nullptr;
    int* tokpos_b = nullptr;            // [GEMM_NT][4]
    int* h_tokpos_b = nullptr;          // pinned ring [kTokbRing][GEMM_NT][4]
    long long tokb_slot = 0;
    static constexpr int kTokbRing = 256;
    static constexpr int kBatchRows = UB_MAX;
    bool mmq_ok = false;                // int8-MFMA GEMM for prompt chunks (all layers Q4_K / Q6_K)
    // physical batches of up to UB_MAX tokens on mmq32 (mmq.hip): activations, rope table
    int8_t* ub_q = nullptr;             // Q8_K rows [UB_MAX][kmax]
    float* ub_dT = nullptr;             // [kmax/256][UB_MAX]
    int8_t* ub_bsb = nullptr;           // [UB_MAX][kmax/256][16]
    float2* ub_rope = nullptr;          // [UB_MAX][n_rot/2]
    float* ub_part = nullptr;           // [2][UB_MAX][n_embd] split-K partials (dense models)
    // short batches (<= mmqs_max tokens, dense models): the split-K streaming GEMM's partial sums
    // [kp][ntok][rows] of every launch (mmq.hip mmqs; MI_MMQS_MAX=0: off)
    float* ub_spart = nullptr;
    int mmqs_max = 0;
    bool out_mmq = false;               // the output head is mmq32-capable (batched logits of every token)
    bool ub_q80 = false;                // the layer matrices are Q8_0: Q8_0 batch activations
    bool attn_mfma = false;             // batch attention on f16 MFMA (attn_mfma.hip)
    // MI_OUT_ALL: logits of every token of the last decode call, [out_rows][n_vocab]
    float* logits_all = nullptr;
    int logits_all_cap = 0;
    int out_rows = 0;                   // rows of logits_all valid (0: the last decode was MI_OUT_LAST)
    int topk_row = -1;                  // output row the mapped top-k buffers hold (-1: the last token)
    // Embeddings mode (llama_context_params.embeddings + pooling_type, b5187): every pass ends in
    // the embedding tail -- the final norm to f32 rows (embd.hip), pooled over the tokens of the
    // decode call -- in place of the output head; no logits then.  A property of the context, not
    // of its state.  embd: [n_batch] token rows, the pooled row, the decode step's row (the
    // captured step graph writes there); allocated by the first embeddings decode.
    bool embeddings = false;
    int pooling = MI_POOLING_NONE;      // resolved (never unspecified)
    float* embd = nullptr;
    float* h_embd = nullptr;            // pinned [n_embd]: the row mi_embeddings returns
    bool embd_valid = false;            // a decode has written embd since the mode was set
    int embd_rows = 0;                  // token rows valid (pooling NONE after MI_OUT_ALL), else 0
    int embd_n = 0;                     // the decode call being enqueued: its tokens, and whether
    bool embd_all = false;              // every token's row is wanted (MI_OUT_ALL, pooling NONE)
    float* embd_pooled() const { return embd + (size_t)n_batch * m->hp.n_embd; }
    float* embd_step() const { return embd + ((size_t)n_batch + 1) * m->hp.n_embd; }
    void set_embeddings(bool on, int pooling_type);   // synchronises, drops the graphs
    void enqueue_embd_norm(const float* xrows, int nt, float* out);
    // the tail of one physical batch: residual rows xrows [nt][n_embd] are tokens c0.. of the call
    void embd_tail(const float* xrows, int nt, int c0);
    // token rows r0 .. r0 + nt - 1 of embd into the pooled row (MEAN: accumulated; CLS: row 0; LAST: row n - 1)
    void embd_pool_rows(int r0, int nt);
    const float* embeddings_host(int row);
    // Encoder models (ARCH_BERT): no KV cache; every decode call is one stateless pass over its n
    // tokens at positions 0 .. n - 1 (enc.cpp), ending in the embedding rows.  Always in embeddings mode.
    // Invariant: with enc set the constructor returned before any decoder buffer was allocated (kcache,
    // cell_pos, logits, topk / gather buffers, h_logits ... are null) and `embeddings` stays true
    // (set_embeddings refuses to turn it off), so every entry point that touches a decoder buffer
    // must either check `embeddings` (the logits reads do) or check `enc` first.
    bool enc = false;
    int enc_max = 0;                    // tokens a call may hold: min(n_batch, ENC_MAX_TOK, n_ctx_train)
    int* enc_tok = nullptr;             // [enc_max] token ids
    int* h_enc_tok = nullptr;           // pinned ring [kEncRing][enc_max]
    long long enc_slot = 0;
    static constexpr int kEncRing = 16;
    float *enc_x = nullptr, *enc_a = nullptr, *enc_x1 = nullptr, *enc_q = nullptr, *enc_o = nullptr, *enc_h = nullptr;
    __half *enc_k = nullptr, *enc_v = nullptr;   // [enc_max][n_embd] f16 K / V of the layer
    void enc_init();
    int decode_enc(const int32_t* tokens, int n, bool all);
    // control vector (llama_adapter_cvec, b5187): row l is layer l's direction, added to the
    // residual stream after the layer's FFN residual add (build_cvec) in every path.  A property
    // of the context, not of its state (mi_state_get / mi_state_set leave it alone).
    float* cvec = nullptr;              // [n_layer][n_embd], allocated by the first apply_cvec
    std::vector<char> cvec_on;          // [n_layer]: the layer carries its row (empty: no vector)
    const float* cvec_for(int l) const {
        return !cvec_on.empty() && cvec_on[l] ? cvec + (size_t)l * m->hp.n_embd : nullptr;
    }
    // llama_adapter_cvec::apply: data == null clears; layer il in [max(1, il_start), min(il_end,
    // n_layer - 1)] with il * n_embd <= len carries data[(il - 1) * n_embd ..).  Synchronises the
    // stream and drops the captured decode graphs (their launches hold the old arguments).
    void apply_cvec(const float* data, size_t len, int n_embd, int il_start, int il_end);
    // LoRA adapters (llama_set_adapter_lora / llama_rm_adapter_lora / llama_clear_adapter_lora): a
    // property of the context like the control vector.  The adapters set are stacked into one
    // adapter of concatenated rank per base tensor; the tensors that read one activation -- group
    // 0: Q, K, V; 1: attn_output; 2: gate, up; 3: ffn_down -- share one A stack and one shrink launch.
    struct LoraSet {
        std::shared_ptr<Lora> a;
        float scale;
    };
    struct LoraGroup {
        void* A = nullptr;              // [R][K]
        int a_f16 = 0, R = 0;
        unsigned char* rnd = nullptr;   // [R]
        void* B[3] = {nullptr, nullptr, nullptr};   // the group's tensors: [rows][Rt[i]]
        int Rt[3] = {0, 0, 0}, off[3] = {0, 0, 0}, b_f16[3] = {0, 0, 0};
        int* tab[3] = {nullptr, nullptr, nullptr};  // LoraFold::tab of each tensor
    };
    std::vector<LoraSet> loras;
    std::vector<LoraGroup> lora_g;      // [n_layer][4]; empty: no adapter
    char* lora_mem = nullptr;           // the stacks
    float* lora_t = nullptr;            // [kBatchRows][3 * LORA_MAX_RANK]: the shrink's output
    float* lora_pre = nullptr;          // batches: [kBatchRows][max(Q|K|V rows, 2 n_ff)] (GemmParams::pre)
    int lora_pre_stride = 0;
    bool lora_on() const { return !lora_g.empty(); }
    const LoraGroup* lora_group(int l, int g) const {
        return !lora_g.empty() && lora_g[(size_t)l * 4 + g].R ? &lora_g[(size_t)l * 4 + g] : nullptr;
    }
    void set_lora(const std::shared_ptr<Lora>& a, float scale);
    int rm_lora(const Lora* a);          // 0, or -1 when not set
    void clear_lora();
    void lora_rebuild();                // synchronises, drops the graphs, rebuilds the stacks of `loras`
    LoraFold* lora_folds = nullptr;     // [n_layer][4] on the device: the groups' LoraFold (GemvSeg::lora)
    const LoraFold* lora_fold(int l, int g) const { return lora_group(l, g) ? lora_folds + (size_t)l * 4 + g : nullptr; }
    void lora_shrink(const LoraGroup& G, const float* xin, int x_stride, int K, int ntok, const float* norm_w);
    // tensor i of the group: out[tok][row] = its terms (zeros when it has no adapter)
    void lora_expand(const LoraGroup& G, int i, float* out, int out_stride, int rows, int ntok);
    // The terms of group g of layer l for the launches that take them precomputed (GemvSeg::pre,
    // GemmParams::pre): the shrink over act [ntok][K] (rms_norm'd with norm_w when set) and every
    // tensor's expand into lora_pre, row layout lora_pre_row.  Returns lora_pre, or null when the
    // group has no adapter (nothing launched).
    const float* lora_pre_terms(int l, int g, const float* act, int K, int ntok, const float* norm_w);
    // first row of tensor i of group g in a lora_pre row: [Q | K | V], [W_o], [gate | up], [down]
    int lora_pre_row(int l, int g, int i) const;
    // the terms at `pre` (null: none) into a GEMM launch: tensor i of group g (a gate/up pair: i = 0)
    void set_pre(GemmParams& p, const float* pre, int l, int g, int i) const {
        if (!pre) return;
        p.pre = pre;
        p.pre_stride = lora_pre_stride;
        p.pre_off = lora_pre_row(l, g, i);
        p.pre_up = p.pair == PAIR_AB ? lora_pre_row(l, g, 1) : 0;
    }
    // diagnostics (MI_STAMPS builds only): s_memrealtime stamps of every
    // workgroup of every launch of the last enqueued step [launch][wg][8]
    static constexpr int kStampLaunches = 320, kStampWgs = 512;
    unsigned long long* stamps = nullptr;

    // pinned host buffers
    int* h_tokpos = nullptr;            // ring of kTokRing x 4 ints
    int* h_topk_ids = nullptr;
    float* h_topk_vals = nullptr;
    float* h_logits = nullptr;
    float* h_gather = nullptr;
    int* d_h_topk_ids = nullptr;        // device views of h_topk_ids / h_topk_vals
    float* d_h_topk_vals = nullptr;
    long long tok_slot = 0;

    // host mirror of the cache cells
    std::vector<int> h_cell_pos;
    int n_cells = 0;
    int pos_max = -1;
    bool logits_valid = false;

    // decode graphs (with / without the output head).  With profiling on, the
    // full step is split in three graphs around one layer's FFN gate/up GEMV so
    // that plain HIP events on the stream bracket exactly that launch.
    // MI_NO_GRAPH=1: launch every kernel eagerly (profilers that cannot trace
    // graph-launched kernels); the default replays one hipGraph per step
    bool use_graphs = getenv("MI_NO_GRAPH") == nullptr;
    // [attention mode]: 1 = the context fits the fused short-attention launch (ATTN_SHORT
    // cells), 0 = split attention; the host knows the cell count of every step.
    hipGraphExec_t g_full[2] = {nullptr, nullptr}, g_nolog[2] = {nullptr, nullptr};
    hipGraphExec_t g_embd[2] = {nullptr, nullptr};   // embeddings mode: the step ending in the embedding row
    hipGraphExec_t g_seg[2][3] = {{nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr}};
    int attn_fused = 0;                 // mode of the step being enqueued
    bool attn_long_off = false;         // an exchange of attn_long_kernel timed out: split kernels only
    bool unsynced = false;              // decodes enqueued since the last sync()
    int undo_cells = 0, undo_pos = -1;  // n_cells / pos_max at the last sync (xerr rollback)
    int prof_layer = -1;
    hipEvent_t prof_ev[2] = {nullptr, nullptr};
    bool prof_pending = false;
    long long prof_bytes = 0;            // algorithmic bytes of the timed launch (mi_prof_bytes)
    int seg_filter = -1;                // -1: enqueue everything; else only ops of this segment

    static constexpr int kTokRing = 8192;

    // streaming decode step (dgemv.hip) for LLaMA contexts of any length whose every launch has a
    // compiled variant (MoE: the attention half; the experts keep gemv_kernel): a GEMV reads its
    // activation quantised from sp_act[role] -- WO's written by the attention kernel (past
    // ATTN_SHORT cells by attn_combine_quant), the others' by a dv_quant launch (rms_norm'd x, or
    // h) -- or quantises the fp32 row itself (SpLayer::hq, sp_nq_in)
    enum { HQ_LAUNCH = 0, HQ_WG8 = 1, HQ_WG16 = 2 };   // who quantises h for the FFN down launch
    struct SpLayer {
        int fA, fB, fC, fD;             // activation formats of QKV, WO, gate/up, down: bit 0 Q8_K, bit 1 Q8_0
        int hq;                         // HQ_LAUNCH: a dv_quant launch; HQ_WG8 / HQ_WG16: every down workgroup of 8 / 16 waves
    };
    bool sp_ok = false;                 // false: the r04 step on gemv_kernel (GPT-2, geometries sp_setup rejects)
    std::vector<SpLayer> sp;
    int sp_fH = 0;                      // the output head's activation formats
    bool sp_nq_in = false;              // Q/K/V and gate/up norm and quantise x in-launch
    char* sp_mem = nullptr;
    char* sp_act[5] = {};               // QKV, WO, gate/up, down, head inputs
    bool sp_setup();
    void set_down_quant(int form);      // diagnostics: every layer's SpLayer::hq (the parity tests' A/B of the forms)
    void enqueue_step_sp(bool with_logits);

    // ---- unquantised F16 models (Model::f16): the decode step on fgemv.hip (engine.cpp), prompt
    // batches of up to kBatchRows rows on enc.hip's F16 MFMA GEMM (batch.cpp).  Every matrix launch
    // reads an f32 activation row and rounds it to f16 itself; the normed rows come from a small
    // launch of their own (embd.hip's norm kernel).  Per layer: norm, Q/K/V (+ RoPE, KV append),
    // attention (+ the splits' combine past ATTN_SHORT cells), WO + residual, norm, gate/up + SwiGLU,
    // down + residual (+ the control vector's row).
    float* f_xn = nullptr;              // [n_embd]: the normed row of the step
    float* fb_xn = nullptr;             // batches: [kBatchRows][n_embd] normed rows
    float* fb_t = nullptr;              // batches: [kBatchRows][max(n_embd + 2 kv_dim, 2 n_ff)], a GEMM's raw rows
    int fb_t_stride = 0;
    void f16_init();
    void f16_norm(const float* xrows, int nt, const float* w, float* out);
    FgemvParams fqkv_params(int l) const;
    FgemvParams fwo_params(int l) const;
    FgemvParams fgate_up_params(int l) const;
    FgemvParams fdown_params(int l) const;
    FgemvParams fhead_params() const;
    void run_fgemv(const FgemvParams& p, int l = -1, bool gate_up = false);
    void enqueue_step_f16(bool with_logits);
    // one F16 GEMM of a physical batch: 1-3 matrices over x [nt][K] into out [nt][out_stride] (+ resid)
    void f16_gemm(const QMat* const* mats, float* const* outs, int n, const float* x, int nt, int out_stride,
                  const float* resid);
    void decode_f16_batch(const int32_t* tokens, int n, bool all);

    // ---- the parameter block of each decode launch, built in one place (engine.cpp) ----
    // How a GEMV's activation arrives:
    enum ActSrc {
        ACT_PRO,                        // fp32 row through gemv_kernel's prologue (the r04 step)
        ACT_QUANT,                      // quantised at sp_act[role] (dgemv)
        ACT_RAW,                        // fp32 row, normed and quantised inside the dgemv launch
    };
    GemvParams gemv_base() const;
    int qkv_params(int l, ActSrc src, GemvParams out[3]) const;   // 1-3 launches of the layer's row groups
    GemvParams wo_params(int l, ActSrc src) const;
    GemvParams gate_up_params(int l, ActSrc src) const;
    GemvParams down_params(int l, ActSrc src) const;
    GemvParams down_params_sp(int l) const;   // the streaming step's, by sp[l].hq
    GemvParams head_params(ActSrc src, const float* xrow) const;
    AttnParams attn_params(int l, bool quant_out) const;
    ActOut act_out(int role, int fmt, int K, const float* norm_w) const;
    void set_act(GemvParams& p, ActSrc src, int role, int fmt, const float* xin, const float* norm_w,
                 const float* norm_b) const;
    // values every path's launches share
    __half* k_layer(int l) const { return kcache + (size_t)l * n_ctx * kv_dim; }
    __half* v_layer(int l) const { return vcache + (size_t)l * n_ctx * kv_dim; }
    float theta_scale() const { return std::pow(m->hp.rope_base, -2.0f / (float)m->hp.n_rot); }
    float kq_scale() const { return 1.0f / std::sqrt((float)m->hp.head_dim); }
    void run_topk(const float* src);    // top-k of a logits row into the device and the mapped buffers
    // ---- the parameter block of each batch launch, built in one place (batch.cpp) for the three
    // batch paths: decode_batch (v_dot4 GEMM), decode_ubatch (tiled mmq32), ubatch_layers_short (mmqs)
    // the next nt tokens into a ring slot and tokpos_b, the cell mirror advanced
    void upload_batch(const int32_t* tokens, int nt);
    // the dense layer's GEMMs over nt rows.  vdot4: the launch's own RoPE scalars and eps (the caller
    // adds its input row, prologue and units); else mmq32's form, which reads the rope table.  pre:
    // lora_pre_terms' result for the launch's group.  The caller sets ksplit / part.
    GemmParams gemm_base(int l, int nt, bool vdot4) const;
    GemmParams bqkv_params(int l, int nt, bool vdot4, int i, const float* pre) const;   // i: Q, K, V
    GemmParams bwo_params(int l, int nt, bool vdot4, const float* pre) const;
    GemmParams bgate_up_params(int l, int nt, bool vdot4, const float* pre) const;
    GemmParams bdown_params(int l, int nt, bool vdot4, const float* pre) const;   // addend: the control vector's row
    AttnParams battn_params(int l) const;
    GemmParams bqkv_gpt2_params(int l, int nt) const;   // GPT-2: the fused attn_qkv + bias
    GemmParams bup_gelu_params(int l, int nt) const;    // GPT-2: ffn_up + bias + GELU
    // Q / K / V by type: the activation formats they read (bit 0 Q8_K, bit 1 Q8_0) and the launches,
    // each the matrices of one type (idx: 0 Q, 1 K, 2 V, ascending; launches ordered by their first)
    struct QkvGroups {
        int fmt, n, cnt[3], idx[3][3];
    };
    static QkvGroups qkv_type_groups(const Layer& L);
    // What launch_quant_act quantises for the next GEMM (rows of K elements; the caller adds `rows`
    // for the MoE rows of a batch, each reading the row rows[t] names):
    struct PendParts {         // split-K parts not yet added into x: nks of them, then the addend row (may be null)
        const float* part;
        int nks;
        const float* addend;
    };
    QuantAct qa_rows(const float* x, int K) const;                                  // the rows as they are
    // rms_norm(x) * norm_w -- norm_b set (GPT-2): layer_norm(x) * norm_w + norm_b -- of x, or of x plus
    // the pending parts (pend.part set), x written back
    QuantAct qa_norm(const float* x, int K, const float* norm_w, PendParts pend = {}) const;
    QuantAct qa_layernorm(const float* x, int K, const float* norm_w, const float* norm_b) const;
    QuantAct qa_swiglu(const float* part, int nks, int K) const;                    // silu(gate) * up of a pair launch's parts
    // one matrix (or gate/up pair) on mmqs, its rows from 0 of the parts; returns the part count
    int mmqs_one(const QMat& A, bool pair, int nff, const ActQ8& act, int pstride);
    // MoE: router and grouping of nt tokens (pend: W_o's split-K parts, added first); returns the
    // row capacity.  moe_act: the grouped rows' activation buffers.
    int moe_route(int l, int nt, const float* pend);
    ActQ8 moe_act(int K, int cap, bool q80) const;
    // MI_OUT_ALL: after rows c0.. of logits_all are written, the last chunk's last row also feeds
    // `logits` and the mapped top-k
    void finish_logits_all(int c0, int nt, bool last);
    // ---- the profiling gate of the step being enqueued: with seg_filter >= 0 only the launches of
    // that segment go out (0: up to layer prof_layer's FFN gate/up, 1: that launch, 2: the rest)
    int enq_seg = 0, enq_launch = 0;
    bool seg_on() const { return seg_filter < 0 || seg_filter == enq_seg; }
    unsigned long long* next_stamp();   // MI_STAMPS builds: one slab per gemv_kernel / attention launch
    void run_gemv(GemvParams p, int l = -1, bool gate_up = false);
    void run_attn(AttnParams a);
    void enqueue_moe_ffn(int l);

    Ctx(Model* model, uint32_t n_ctx, uint32_t n_batch, uint32_t n_ubatch);
    ~Ctx();
    void enqueue_step(bool with_logits);
    void enqueue_output(ActSrc src, const float* xrow, unsigned long long* stamps_slab);
    void decode_batch(const int32_t* tokens, int n);
    void decode_ubatch(const int32_t* tokens, int n, bool all);
    // the layers of one short physical batch on mmqs; returns the residual parts still to add
    // into xb (pend_k parts of ub_spart)
    int ubatch_layers_short(int nt);
    void enqueue_ubatch_short(int nt, bool all, int c0, bool last);
    // one physical batch of a GPT-2 model on the tiled GEMM (batch.cpp)
    void enqueue_ubatch_gpt2(int nt, bool all, int c0, bool last);
    // mi_batch_path: the form the most recent decode call took (its first physical batch's; -1: no call yet)
    int batch_path = -1;
    ActQ8 ub_act(int K, int ntok, int type) const;   // the activation format `type`'s matrices read
    bool hp_dense() const { return m->hp.n_expert == 0; }
    // a second activation set (Q8_0) for a model mixing Q8_0 and k-quant matrices
    int8_t* ub_q0 = nullptr;
    float* ub_dT0 = nullptr;
    // MoE prompt batches: router picks and weights [token][n_used], the tokens grouped by expert on
    // the device (moe_rows: source token of each (expert, token) row, -1 for padding; moe_pos: the
    // row of each (token, slot)), the experts' down outputs [row][n_embd]
    float* yb = nullptr;
    int* sel_b = nullptr;
    float* selw_b = nullptr;
    int* moe_rows = nullptr;
    int* moe_pos = nullptr;
    int* moe_rowsel = nullptr;          // row r or -1 (padding): the down projection's input rows
    int* moe_grp = nullptr;             // launch_moe_group's {offsets, counts}
    int8_t* moe_q = nullptr;            // the rows' Q8_K / Q8_0 activations (moe_rows_cap rows)
    float* moe_dT = nullptr;
    int8_t* moe_bsb = nullptr;
    void moe_ffn_batch(int l, int nt, const float* pend = nullptr);
    // a short MoE batch's routed experts on the grouped mmqs (every expert matrix a k-quant)
    void moe_ffn_short(int l, int nt);
    bool moe_short = false;
    bool short_ok() const { return hp_dense() || moe_short; }
    const float* out_row(int row) const;   // device logits of output row `row` (-1: the last)
    hipGraphExec_t build_graph(bool with_logits, int seg);
    void invalidate_graphs();
    int decode(const int32_t* tokens, int n, bool all = false);
    void sync();
    int topk(int row, int k, int32_t* ids, float* vals);
    int gather(int row, const int32_t* ids, int n, float* out);
    int gather_rows(int row0, int nrows, const int32_t* ids, int k, float* out);
    int* grows_ids = nullptr;           // gather_rows buffers (grown on demand)
    float* grows_out = nullptr;
    float* h_grows = nullptr;
    size_t grows_cap = 0;
    const float* logits_host(int row);
    void kv_clear();
    int kv_seq_rm(int p0, int p1);
    int kv_seq_shift(int p0, int p1, int delta, int div);
    size_t state_size() const;
    size_t state_get(uint8_t* dst, size_t size);
    size_t state_set(const uint8_t* src, size_t size);
    int prof_read(float* us, int n);
    long long ffn_bytes() const;
};

}  // namespace mi
