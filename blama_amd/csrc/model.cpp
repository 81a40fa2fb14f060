// Model host code: GGUF parsing and weight residency (the arena, the MFMA-order copies for prompt
// batches, the GPT-2 GELU table).
//
// Reference anchor (the llama.h function this replaces):
//   llama_model_load_from_file  /root/reference/inference/code/llama/Model.cpp:52
#include "engine.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>

namespace mi {

static thread_local std::string g_last_error;
void set_last_error(const std::string& s) { g_last_error = s; }
const char* last_error() { return g_last_error.c_str(); }

// ================================================================== GGUF ===
namespace {
struct Reader {
    const uint8_t* p;
    size_t n, pos = 0;
    void need(size_t k) {
        if (pos + k > n) throw Error("GGUF: truncated header");
    }
    template <class T> T rd() {
        need(sizeof(T));
        T v;
        std::memcpy(&v, p + pos, sizeof(T));
        pos += sizeof(T);
        return v;
    }
    std::string str() {
        const uint64_t len = rd<uint64_t>();
        need(len);
        std::string s(reinterpret_cast<const char*>(p + pos), len);
        pos += len;
        return s;
    }
};

enum { G_U8 = 0, G_I8, G_U16, G_I16, G_U32, G_I32, G_F32, G_BOOL, G_STR, G_ARR, G_U64, G_I64, G_F64 };

double read_num(Reader& r, int t, bool* is_float) {
    *is_float = false;
    switch (t) {
    case G_U8: return r.rd<uint8_t>();
    case G_I8: return r.rd<int8_t>();
    case G_U16: return r.rd<uint16_t>();
    case G_I16: return r.rd<int16_t>();
    case G_U32: return r.rd<uint32_t>();
    case G_I32: return r.rd<int32_t>();
    case G_F32: *is_float = true; return r.rd<float>();
    case G_BOOL: return r.rd<uint8_t>();
    case G_U64: return (double)r.rd<uint64_t>();
    case G_I64: return (double)r.rd<int64_t>();
    case G_F64: *is_float = true; return r.rd<double>();
    default: throw Error("GGUF: bad value type");
    }
}
}  // namespace

void Gguf::parse(const uint8_t* data, size_t size) {
    Reader r{data, size};
    if (size < 24 || std::memcmp(data, "GGUF", 4) != 0) throw Error("not a GGUF file");
    r.pos = 4;
    const uint32_t ver = r.rd<uint32_t>();
    if (ver != 2 && ver != 3) throw Error("unsupported GGUF version " + std::to_string(ver));
    const uint64_t nt = r.rd<uint64_t>(), nkv = r.rd<uint64_t>();
    for (uint64_t i = 0; i < nkv; ++i) {
        std::string key = r.str();
        GgufValue v;
        v.type = (int)r.rd<uint32_t>();
        if (v.type == G_STR) {
            v.s = r.str();
        } else if (v.type == G_ARR) {
            v.arr_type = (int)r.rd<uint32_t>();
            v.arr_n = (long long)r.rd<uint64_t>();
            if (v.arr_type == G_STR) {
                v.arr_s.reserve(v.arr_n);
                for (long long k = 0; k < v.arr_n; ++k) v.arr_s.push_back(r.str());
            } else {
                v.arr_num.reserve(v.arr_n);
                bool fl;
                for (long long k = 0; k < v.arr_n; ++k) v.arr_num.push_back(read_num(r, v.arr_type, &fl));
            }
        } else {
            bool fl;
            const double d = read_num(r, v.type, &fl);
            v.f = d;
            v.i = (long long)d;
        }
        kv.emplace(std::move(key), std::move(v));
    }
    for (uint64_t i = 0; i < nt; ++i) {
        GgufTensor t;
        t.name = r.str();
        t.n_dims = (int)r.rd<uint32_t>();
        if (t.n_dims < 1 || t.n_dims > 4) throw Error("GGUF: bad n_dims for " + t.name);
        long long n = 1;
        for (int d = 0; d < t.n_dims; ++d) { t.ne[d] = (long long)r.rd<uint64_t>(); n *= t.ne[d]; }
        t.type = (int)r.rd<uint32_t>();
        t.offset = r.rd<uint64_t>();
        const int be = block_elems(t.type), bb = block_bytes(t.type);
        if (bb == 0) {
            t.nbytes = 0;   // unsupported type: only an error if the tensor is used
        } else {
            if (n % be) throw Error("GGUF: tensor " + t.name + " not a whole number of blocks");
            t.nbytes = (size_t)(n / be) * bb;
        }
        tensors.push_back(t);
    }
    const long long align = get_int("general.alignment", 32);
    data_offset = (r.pos + align - 1) / align * align;
}

long long Gguf::get_int(const std::string& k, long long def) const {
    const GgufValue* v = get(k);
    return (v && v->type != G_STR && v->type != G_ARR) ? v->i : def;
}
double Gguf::get_float(const std::string& k, double def) const {
    const GgufValue* v = get(k);
    return (v && v->type != G_STR && v->type != G_ARR) ? v->f : def;
}
std::string Gguf::get_str(const std::string& k, const std::string& def) const {
    const GgufValue* v = get(k);
    return (v && v->type == G_STR) ? v->s : def;
}
const GgufTensor* Gguf::tensor(const std::string& name) const {
    for (const auto& t : tensors)
        if (t.name == name) return &t;
    return nullptr;
}

// ================================================================= model ===
// One tensor into the model's byte counts: the bytes a decode step streams (not the embedding
// tables; an expert tensor contributes the n_expert_used experts the router picks -- build_moe_ffn
// reads only those -- not all n_expert of them; a BERT model counts its matrices itself) and the
// type histogram.
void Model::account(const GgufTensor& t, int experts) {
    if (hp.arch != ARCH_BERT && t.name != "token_embd.weight" && t.name != "position_embd.weight")
        weight_bytes += experts > 1 ? (long long)t.nbytes / experts * hp.n_expert_used : (long long)t.nbytes;
    if (t.type >= 0 && t.type < 32) type_bytes[t.type] += (long long)t.nbytes;
}

// Whether the file is an all-F16 dense LLaMA model (engine.h, Model::f16): false for a file whose
// layer matrices and output head are all quantised (its token_embd may be of any served type, as
// before); otherwise every matrix must be F16 and the shape rules must hold, or the load is
// refused with the tensor and the reason.  Reads the header only.
bool Model::check_f16() const {
    std::vector<std::string> names = {"output.weight"};
    const char* dense[] = {"attn_q", "attn_k", "attn_v", "attn_output", "ffn_gate", "ffn_up", "ffn_down",
                           "ffn_gate_exps", "ffn_up_exps", "ffn_down_exps", "attn_qkv"};
    for (int l = 0; l < hp.n_layer; ++l)
        for (const char* d : dense) names.push_back("blk." + std::to_string(l) + "." + d + ".weight");
    std::vector<const GgufTensor*> mats;
    bool plain = false;   // a layer matrix or the head is not quantised
    for (const std::string& n : names)
        if (const GgufTensor* t = gguf.tensor(n)) {
            mats.push_back(t);
            plain = plain || !is_quant(t->type);
        }
    if (!plain) return false;
    if (const GgufTensor* t = gguf.tensor("token_embd.weight")) mats.push_back(t);
    const GgufTensor* first_f16 = nullptr;
    for (const GgufTensor* t : mats)
        if (t->type == T_F16 && !first_f16) first_f16 = t;
    for (const GgufTensor* t : mats) {
        if (t->type == T_BF16)
            throw Error("tensor " + t->name + ": BF16 matrices are not served (convert the model to F16, or quantise it)");
        if (t->type == T_F32)
            throw Error("tensor " + t->name + ": F32 matrices are not served (convert the model to F16, or quantise it)");
        if (is_quant(t->type) && first_f16)
            throw Error("tensor " + t->name + ": the file mixes F16 (" + first_f16->name +
                        ") and quantised matrices; an unquantised model must be F16 throughout");
        if (t->type != T_F16) throw Error("tensor " + t->name + ": unsupported ggml type " + std::to_string(t->type) + " for a matrix");
    }
    if (hp.arch == ARCH_GPT2)
        throw Error("tensor " + mats[0]->name + ": F16 GPT-2 models are not served (the gpt2 graph takes quantised matrices only)");
    if (hp.n_expert > 0)
        throw Error("tensor " + mats[0]->name + ": F16 MoE models are not served (the expert kernels take quantised matrices only)");
    // shape rules of the F16 kernels (engine.h)
    const int kv = hp.n_head_kv * hp.head_dim;
    auto rule = [](bool ok, const std::string& what) {
        if (!ok) throw Error("F16 model: " + what);
    };
    rule(hp.n_head * hp.head_dim == hp.n_embd && hp.n_head_kv > 0 && hp.n_head % hp.n_head_kv == 0,
         "embedding_length must be head_count x head_dim, head_count a multiple of head_count_kv");
    rule(hp.n_embd % 32 == 0 && hp.n_embd <= FGEMV_MAX_K, "embedding_length " + std::to_string(hp.n_embd) + " must be a multiple of 32, at most 16384");
    rule(hp.n_ff > 0 && hp.n_ff % 32 == 0 && hp.n_ff <= FGEMV_MAX_K, "feed_forward_length " + std::to_string(hp.n_ff) + " must be a multiple of 32, at most 16384");
    rule(kv % 32 == 0, "head_count_kv x head_dim = " + std::to_string(kv) + " must be a multiple of 32");
    rule(hp.n_vocab > 0 && hp.n_vocab % 32 == 0, "vocabulary size " + std::to_string(hp.n_vocab) + " must be a multiple of 32");
    rule(hp.n_rot % 2 == 0 && hp.n_rot <= hp.head_dim, "rope.dimension_count must be even and at most head_dim");
    auto shape = [&](const std::string& n, long long rows, long long K) {
        const GgufTensor* t = gguf.tensor(n);
        if (!t) throw Error("GGUF: missing tensor " + n);
        if (t->n_dims != 2 || t->ne[0] != K || t->ne[1] != rows)
            throw Error("tensor " + n + ": expected " + std::to_string(rows) + " x " + std::to_string(K) + " (rows x K)");
    };
    shape("token_embd.weight", hp.n_vocab, hp.n_embd);
    if (gguf.tensor("output.weight")) shape("output.weight", hp.n_vocab, hp.n_embd);
    for (int l = 0; l < hp.n_layer; ++l) {
        const std::string b = "blk." + std::to_string(l) + ".";
        shape(b + "attn_q.weight", hp.n_embd, hp.n_embd);
        shape(b + "attn_k.weight", kv, hp.n_embd);
        shape(b + "attn_v.weight", kv, hp.n_embd);
        shape(b + "attn_output.weight", hp.n_embd, hp.n_embd);
        shape(b + "ffn_gate.weight", hp.n_ff, hp.n_embd);
        shape(b + "ffn_up.weight", hp.n_ff, hp.n_embd);
        shape(b + "ffn_down.weight", hp.n_embd, hp.n_ff);
    }
    return true;
}

bool Model::check_types() const {
    bool any = false;
    // (a MoE model: its expert tensors first, so that the message names one of them)
    std::vector<const GgufTensor*> order;
    for (const GgufTensor& t : gguf.tensors)
        if (t.name.find("_exps.") != std::string::npos) order.push_back(&t);
    for (const GgufTensor& t : gguf.tensors)
        if (t.name.find("_exps.") == std::string::npos) order.push_back(&t);
    for (const GgufTensor* tp : order) {
        const GgufTensor& t = *tp;
        if (t.n_dims < 2) continue;   // matrices: the tables, the head, the layers' projections
        const int ty = t.type;
        if (is_legacy_quant(ty)) {
            any = true;
            const char* why = hp.arch == ARCH_GPT2 ? "a GPT-2 model" : hp.arch == ARCH_BERT ? "a BERT model"
                            : hp.n_expert > 0 ? "a MoE model" : nullptr;
            if (why)
                throw Error("tensor " + t.name + ": " + type_name(ty) + " matrices are not served in " + why +
                            " (Q4_0 / Q5_0 are read by the dense LLaMA kernels only)");
            if (t.ne[0] % 256)
                throw Error("tensor " + t.name + ": a " + type_name(ty) + " matrix needs a row length that is a multiple of 256");
        } else if (ty != T_F32 && ty != T_F16 && ty != T_BF16 && !is_quant(ty) && block_bytes(ty) == 0) {
            const bool q81 = ty == 3 || ty == 7;   // Q4_1, Q5_1
            throw Error("tensor " + t.name + ": " + type_name(ty) + " matrices are not served" +
                        (q81 ? " (they take Q8_1 activations; requantise to Q4_0, Q5_0, Q8_0 or a k-quant)"
                             : " (served: Q4_0, Q5_0, Q8_0, Q4_K, Q5_K, Q6_K, or F16 throughout)"));
        }
    }
    return any;
}

Model::~Model() {
    if (arena || mmq_arena || gelu_tab) hipSetDevice(device);
    if (arena) hipFree(arena);
    if (mmq_arena) hipFree(mmq_arena);
    if (gelu_tab) hipFree(gelu_tab);
}

// ggml_table_gelu_f16 (ggml-cpu.c init with GGML_GELU_FP16): fp16(ggml_gelu_f32(fp32(h))) for
// every f16 bit pattern h, ggml_gelu_f32(x) = 0.5f*x*(1.0f + tanhf(SQRT_2_OVER_PI*x*(1.0f +
// GELU_COEF_A*x*x))), evaluated on the host with the C library's tanhf (no FMA contraction:
// -ffp-contract=off), as the reference's CPU build evaluates it.
std::vector<unsigned short> gelu_table_host() {
    std::vector<unsigned short> t(65536);
    const float A = 0.044715f, K = 0.79788456080286535587989211986876f;
    for (int i = 0; i < 65536; ++i) {
        const unsigned short h = (unsigned short)i;
        _Float16 hf;
        std::memcpy(&hf, &h, 2);
        const float x = (float)hf;
        const float g = 0.5f * x * (1.0f + tanhf(K * x * (1.0f + A * x * x)));
        const _Float16 r = (_Float16)g;
        std::memcpy(&t[i], &r, 2);
    }
    return t;
}

void split_experts(QMat& m, int n_exp) {
    m.rows /= n_exp;
    m.n_exp = n_exp;
    for (int k = 0; k < plane_count(m.type); ++k) m.expert_stride[k] = (long long)m.rows * m.nb * plane_sb_bytes(m.type, k);
}

QMat expert_view(const QMat& q, int e) {
    QMat v = q;
    for (int k = 0; k < 4; ++k)
        if (v.p[k]) v.p[k] += e * q.expert_stride[k];
    if (v.sw) v.sw += e * q.sw_expert_stride;
    return v;
}

void build_mmq_copies(QMat& A, const QMat* B, uint8_t* dst) {
    const size_t one = mmq32_copy_bytes(A, B != nullptr);
    for (int e = 0; e < std::max(1, A.n_exp); ++e) {   // expert e's planes -> its own copy
        const QMat a = expert_view(A, e), b = B ? expert_view(*B, e) : QMat{};
        launch_mmq32_swizzle(a, B ? &b : nullptr, dst + one * e, nullptr);
    }
    A.sw = dst;
    A.sw_expert_stride = (long long)one;
}

bool Model::ensure_mmq_copies() {
    std::lock_guard<std::mutex> lk(mmq_mu);
    if (mmq_arena) return true;
    MI_HIP(hipSetDevice(device));
    // every mmq32-capable projection (gate and up as one pair copy; MoE: one copy per expert,
    // expert e at sw + e * sw_expert_stride) and the output head
    std::vector<std::pair<QMat*, QMat*>> todo;
    for (Layer& L : layers) {
        if (hp.arch == ARCH_GPT2) {   // the fused attn_qkv as one copy (its Q, K and V rows are row segments of it), ffn_up alone
            for (QMat* q : {&L.qkv[0], &L.wo, &L.up, &L.down})
                if (mmq32_supported(q->type)) todo.push_back({q, nullptr});
            continue;
        }
        for (QMat* q : {&L.wq, &L.wk, &L.wv, &L.wo, &L.down})
            if (mmq32_supported(q->type)) todo.push_back({q, nullptr});
        if (mmq32_supported(L.gate.type) && L.up.type == L.gate.type) todo.push_back({&L.gate, &L.up});
    }
    if (mmq32_supported(output.type)) todo.push_back({&output, nullptr});
    auto experts = [](const QMat& q) { return std::max(1, q.n_exp); };
    size_t total = 0;
    std::vector<size_t> offs;
    for (auto& t : todo) {
        offs.push_back(total);
        const size_t one = mmq32_copy_bytes(*t.first, t.second != nullptr);
        total = (total + one * experts(*t.first) + 255) & ~size_t(255);
    }
    if (!total) return true;
    if (hipMalloc(&mmq_arena, total) != hipSuccess) {
        (void)hipGetLastError();   // clear the sticky error; the caller falls back
        mmq_arena = nullptr;
        return false;
    }
    mmq_bytes = total;
    for (size_t i = 0; i < todo.size(); ++i) build_mmq_copies(*todo[i].first, todo[i].second, mmq_arena + offs[i]);
    MI_HIP(hipDeviceSynchronize());
    return true;
}

const QMat* Model::find_qmat(const std::string&) const { return nullptr; }

namespace {
size_t align256(size_t x) { return (x + 255) & ~size_t(255); }

struct Planned {
    const GgufTensor* t;
    size_t off[4];     // arena offsets of the planes (quant) or of the raw copy (p0)
    long long rows;    // rows across all experts
    int K;
    int experts;
};
}  // namespace

void Model::load(const uint8_t* data, size_t size, const mi_model_params& p) {
    device = p.device_ordinal;
    vocab_only = p.vocab_only != 0;
    gguf.parse(data, size);
    const std::string arch = gguf.get_str("general.architecture", "");
    if (arch != "llama" && arch != "gpt2" && arch != "bert")
        throw Error("unsupported architecture '" + arch + "' (this backend serves the llama, gpt2 and bert graphs)");
    hp.arch = arch == "gpt2" ? ARCH_GPT2 : arch == "bert" ? ARCH_BERT : ARCH_LLAMA;
    const bool bert = hp.arch == ARCH_BERT;
    auto key = [&](const char* k) { return arch + "." + k; };
    hp.n_embd = (int)gguf.get_int(key("embedding_length"), 0);
    hp.n_layer = (int)gguf.get_int(key("block_count"), 0);
    hp.n_ff = (int)gguf.get_int(key("feed_forward_length"), 0);
    hp.n_head = (int)gguf.get_int(key("attention.head_count"), 0);
    hp.n_head_kv = (int)gguf.get_int(key("attention.head_count_kv"), hp.n_head);
    hp.n_ctx_train = (int)gguf.get_int(key("context_length"), 2048);
    hp.eps = (float)gguf.get_float(key(hp.arch != ARCH_LLAMA ? "attention.layer_norm_epsilon"
                                                             : "attention.layer_norm_rms_epsilon"), 1e-5);
    hp.rope_base = (float)gguf.get_float(key("rope.freq_base"), 10000.0);
    // llama.cpp b5187 (llama-model.cpp load_hparams): the factor is rope.scaling.factor, else the
    // older rope.scale_linear; rope.scaling.type (default linear) picks the mode.  The kernels
    // implement ggml_rope_ext with ext_factor 0 and mscale 1 only: linear scaling or none.
    const double fs = gguf.get_float(key("rope.scaling.factor"), gguf.get_float(key("rope.scale_linear"), 0.0));
    const std::string rope_type = gguf.get_str(key("rope.scaling.type"), "linear");
    if (rope_type != "linear" && rope_type != "none")
        throw Error("unsupported " + key("rope.scaling.type") + " '" + rope_type +
                    "' (this backend implements linear RoPE scaling only)");
    hp.freq_scale = (rope_type == "linear" && fs > 0.0) ? (float)(1.0 / fs) : 1.0f;
    hp.n_expert = (int)gguf.get_int(key("expert_count"), 0);
    hp.n_expert_used = (int)gguf.get_int(key("expert_used_count"), 0);
    // llama_pooling_type of the model ({arch}.pooling_type, u32), read for every architecture; absent: unspecified
    hp.pooling_type = (int)gguf.get_int(key("pooling_type"), -1);
    if (hp.n_embd <= 0 || hp.n_layer <= 0 || hp.n_head <= 0) throw Error("GGUF: missing llama hparams");
    hp.head_dim = hp.n_embd / hp.n_head;
    hp.n_rot = hp.arch == ARCH_GPT2 ? 0 : (int)gguf.get_int(key("rope.dimension_count"), hp.head_dim);
    if (hp.arch == ARCH_GPT2 && hp.n_expert) throw Error("gpt2: no MoE");
    if (bert) {   // llm_build_bert: no RoPE, every head its own K / V, no experts, no output head
        hp.n_rot = 0;
        hp.n_head_kv = hp.n_head;
        hp.n_expert = hp.n_expert_used = 0;
        if (gguf.get_int(key("attention.causal"), 0) != 0)
            throw Error("bert: " + key("attention.causal") + " = true is not served (the encoder pass is bidirectional)");
        if (hp.n_ff <= 0) throw Error("GGUF: missing bert hparams");
        if (hp.n_embd % 32) throw Error("bert: embedding_length " + std::to_string(hp.n_embd) + " is not a multiple of 32");
        if (hp.n_ff % 32) throw Error("bert: feed_forward_length " + std::to_string(hp.n_ff) + " is not a multiple of 32");
        if (hp.n_embd % hp.n_head || !enc_attn_supported(hp.head_dim))
            throw Error("bert: head_dim " + std::to_string(hp.head_dim) + " is not served (32 or 64)");
    }

    if (const GgufValue* tv = gguf.get("tokenizer.ggml.tokens")) tokens = tv->arr_s;
    if (const GgufValue* tt = gguf.get("tokenizer.ggml.token_type"))
        for (double d : tt->arr_num) token_type.push_back((int)d);
    if (const GgufValue* ts = gguf.get("tokenizer.ggml.scores"))
        for (double d : ts->arr_num) token_score.push_back((float)d);
    tok_model = gguf.get_str("tokenizer.ggml.model", "llama");
    if (const GgufValue* mv = gguf.get("tokenizer.ggml.merges")) merges = mv->arr_s;
    hp.n_vocab = (int)tokens.size();
    if (const GgufTensor* te = gguf.tensor("token_embd.weight")) hp.n_vocab = (int)te->ne[1];
    bos = (int)gguf.get_int("tokenizer.ggml.bos_token_id", 1);
    eos = (int)gguf.get_int("tokenizer.ggml.eos_token_id", 2);
    eot = (int)gguf.get_int("tokenizer.ggml.eot_token_id", -1);
    add_bos = gguf.get_int("tokenizer.ggml.add_bos_token", 1) != 0;
    legacy = check_types();
    if (!bert) f16 = check_f16();
    if (vocab_only) {
        // an F16 model's weight bytes and type histogram are known from the header alone, and so
        // are those of a file with Q4_0 / Q5_0 matrices (dense: every tensor streams whole)
        if (f16 || legacy) {
            for (const GgufTensor& t : gguf.tensors) account(t, 1);
            if (!gguf.tensor("output.weight")) weight_bytes += (long long)gguf.tensor("token_embd.weight")->nbytes;   // tied head
        }
        return;
    }
    if (p.cpu_only) throw Error("cpu_only models are served by the CPU reference path, not this engine");

    // ---- plan the arena ----
    std::vector<Planned> plan;
    size_t off = 0;
    auto add = [&](const std::string& name, bool required, int experts) -> int {
        const GgufTensor* t = gguf.tensor(name);
        if (!t) {
            if (required) throw Error("GGUF: missing tensor " + name);
            return -1;
        }
        Planned pl{};
        pl.t = t;
        pl.K = (int)t->ne[0];
        pl.experts = experts;
        pl.rows = t->ne[1] * (t->n_dims > 2 ? t->ne[2] : 1);
        if (is_quant(t->type)) {
            if (pl.K % 256) throw Error("tensor " + name + ": K not a multiple of 256");
            const long long nsb = pl.rows * (pl.K / 256);
            for (int k = 0; k < plane_count(t->type); ++k) {
                pl.off[k] = off;   // + 8 superblocks of tail padding read by idle GEMV lanes
                off = align256(off + (size_t)(nsb + kPlanePadSb) * plane_sb_bytes(t->type, k));
            }
        } else if (t->type == T_F32 || t->type == T_F16) {
            pl.off[0] = off;
            off = align256(off + t->nbytes);
        } else {
            throw Error("tensor " + name + ": unsupported ggml type " + std::to_string(t->type) + " (" + type_name(t->type) + ")");
        }
        plan.push_back(pl);
        return (int)plan.size() - 1;
    };
    // Q/K/V of one layer as groups of adjacent same-type tensors whose planes are stored back to
    // back (plane k of the group = plane k of each tensor in order): one decode-GEMV matrix each
    auto add_group = [&](const std::vector<std::string>& names, std::vector<int>& idx) {
        std::vector<const GgufTensor*> ts;
        for (const auto& n : names) {
            const GgufTensor* t = gguf.tensor(n);
            if (!t) throw Error("GGUF: missing tensor " + n);
            ts.push_back(t);
        }
        const int type = ts[0]->type;
        const int K = (int)ts[0]->ne[0];
        if (f16) {   // plain [rows][K] rows, one raw copy each
            for (const auto& n : names) idx.push_back(add(n, true, 1));
            return;
        }
        if (!is_quant(type) || K % 256) throw Error("tensor " + names[0] + ": not a quantised matrix with K % 256 == 0");
        const size_t first = plan.size();
        for (const GgufTensor* t : ts) {
            if (t->type != type || (int)t->ne[0] != K) throw Error("add_group: mixed tensors");
            Planned pl{};
            pl.t = t;
            pl.K = K;
            pl.experts = 1;
            pl.rows = t->ne[1];
            plan.push_back(pl);
            idx.push_back((int)plan.size() - 1);
        }
        for (int k = 0; k < plane_count(type); ++k) {
            for (size_t i = first; i < plan.size(); ++i) {
                plan[i].off[k] = off;
                off += (size_t)plan[i].rows * (K / 256) * plane_sb_bytes(type, k);
            }
            off = align256(off + (size_t)kPlanePadSb * plane_sb_bytes(type, k));
        }
    };
    struct LayerIdx {
        int an, fn, q, k, v, o, g, u, d, r;
        std::vector<std::vector<int>> qkv_groups;
        int anb = -1, fnb = -1, bqkv = -1, bo = -1, bu = -1, bd = -1;   // GPT-2 biases
    };
    const bool gpt2 = hp.arch == ARCH_GPT2;
    const int i_te = add("token_embd.weight", true, 1);
    const int i_pe = gpt2 || bert ? add("position_embd.weight", true, 1) : -1;
    const int i_on = bert ? -1 : add("output_norm.weight", true, 1);
    const int i_onb = gpt2 ? add("output_norm.bias", true, 1) : -1;
    int i_out = bert ? -1 : add("output.weight", false, 1);
    const int i_rf = bert ? -1 : add("rope_freqs.weight", false, 1);
    std::vector<LayerIdx> li(hp.n_layer);
    const int E = hp.n_expert > 0 ? hp.n_expert : 1;
    // llm_build_bert's tensors (LLM_ARCH_BERT): F16 matrices [rows][K] -- K = 384 of bge-small is no
    // multiple of a k-quant's 256 -- and tables, F32 biases and LayerNorms
    struct BertIdx {
        int w[6], b[6], an, anb, on, onb;   // q, k, v, o, up, down
    };
    std::vector<BertIdx> bi(bert ? hp.n_layer : 0);
    int i_tt = -1, i_en = -1, i_enb = -1;
    auto bert_mat = [&](const std::string& name, int rows, int K) {
        const int i = add(name, true, 1);
        const GgufTensor* t = plan[i].t;
        if (t->type != T_F16)
            throw Error("tensor " + name + ": a BERT matrix must be F16 (ggml type " + std::to_string(t->type) + " is not served)");
        if (t->n_dims != 2 || t->ne[0] != K || t->ne[1] != rows) throw Error("tensor " + name + ": unexpected shape");
        return i;
    };
    auto bert_vec = [&](const std::string& name, int n) {
        const int i = add(name, true, 1);
        const GgufTensor* t = plan[i].t;
        if (t->type != T_F32) throw Error("tensor " + name + " must be F32");
        if (t->ne[0] != n || plan[i].rows != 1) throw Error("tensor " + name + ": unexpected shape");
        return i;
    };
    if (bert) {
        auto table = [&](int i, long long rows_min) {
            const GgufTensor* t = plan[i].t;
            if (t->type != T_F16 && t->type != T_F32) throw Error("tensor " + t->name + ": a BERT embedding table must be F16 or F32");
            if (t->ne[0] != hp.n_embd || t->ne[1] < rows_min) throw Error("tensor " + t->name + ": unexpected shape");
        };
        table(i_te, 1);
        table(i_pe, 1);
        hp.n_ctx_train = (int)std::min<long long>(hp.n_ctx_train, plan[i_pe].t->ne[1]);   // the position table ends here
        i_tt = add("token_types.weight", true, 1);
        table(i_tt, 1);
        i_en = bert_vec("token_embd_norm.weight", hp.n_embd);
        i_enb = bert_vec("token_embd_norm.bias", hp.n_embd);
        const int E_ = hp.n_embd, F = hp.n_ff;
        const char* mats[6] = {"attn_q", "attn_k", "attn_v", "attn_output", "ffn_up", "ffn_down"};
        const int mrows[6] = {E_, E_, E_, E_, F, E_}, mK[6] = {E_, E_, E_, E_, E_, F};
        for (int l = 0; l < hp.n_layer; ++l) {
            const std::string b = "blk." + std::to_string(l) + ".";
            BertIdx& x = bi[l];
            for (int k = 0; k < 6; ++k) {
                x.w[k] = bert_mat(b + mats[k] + ".weight", mrows[k], mK[k]);
                x.b[k] = bert_vec(b + mats[k] + ".bias", mrows[k]);
                weight_bytes += (long long)plan[x.w[k]].t->nbytes;
            }
            x.an = bert_vec(b + "attn_output_norm.weight", E_);
            x.anb = bert_vec(b + "attn_output_norm.bias", E_);
            x.on = bert_vec(b + "layer_output_norm.weight", E_);
            x.onb = bert_vec(b + "layer_output_norm.bias", E_);
        }
    }
    for (int l = 0; l < hp.n_layer && gpt2; ++l) {   // llm_build_gpt2's tensors (LLM_ARCH_GPT2)
        const std::string b = "blk." + std::to_string(l) + ".";
        LayerIdx& x = li[l];
        x.an = add(b + "attn_norm.weight", true, 1);
        x.anb = add(b + "attn_norm.bias", true, 1);
        x.fn = add(b + "ffn_norm.weight", true, 1);
        x.fnb = add(b + "ffn_norm.bias", true, 1);
        std::vector<int> idx;
        add_group({b + "attn_qkv.weight"}, idx);   // one fused [3 n_embd] x n_embd matrix
        x.qkv_groups.push_back(idx);
        x.q = x.k = x.v = idx[0];
        x.bqkv = add(b + "attn_qkv.bias", true, 1);
        x.o = add(b + "attn_output.weight", true, 1);
        x.bo = add(b + "attn_output.bias", true, 1);
        x.r = -1;
        x.g = x.u = add(b + "ffn_up.weight", true, 1);
        x.bu = add(b + "ffn_up.bias", true, 1);
        x.d = add(b + "ffn_down.weight", true, 1);
        x.bd = add(b + "ffn_down.bias", true, 1);
    }
    for (int l = 0; l < hp.n_layer && !gpt2 && !bert; ++l) {
        const std::string b = "blk." + std::to_string(l) + ".";
        LayerIdx& x = li[l];
        x.an = add(b + "attn_norm.weight", true, 1);
        x.fn = add(b + "ffn_norm.weight", true, 1);
        {
            const std::string nq = b + "attn_q.weight", nk = b + "attn_k.weight", nv = b + "attn_v.weight";
            const GgufTensor *tq = gguf.tensor(nq), *tk = gguf.tensor(nk), *tv = gguf.tensor(nv);
            if (!tq || !tk || !tv) throw Error("GGUF: missing attention tensors in " + b);
            std::vector<std::vector<std::string>> groups;
            if (tq->type == tk->type && tk->type == tv->type) groups = {{nq, nk, nv}};
            else if (tq->type == tk->type) groups = {{nq, nk}, {nv}};
            else if (tk->type == tv->type) groups = {{nq}, {nk, nv}};
            else groups = {{nq}, {nk}, {nv}};
            std::vector<int> all;
            for (const auto& g : groups) {
                std::vector<int> idx;
                add_group(g, idx);
                x.qkv_groups.push_back(idx);
                all.insert(all.end(), idx.begin(), idx.end());
            }
            x.q = all[0];
            x.k = all[1];
            x.v = all[2];
        }
        x.o = add(b + "attn_output.weight", true, 1);
        if (hp.n_expert > 0) {
            x.r = add(b + "ffn_gate_inp.weight", true, 1);
            x.g = add(b + "ffn_gate_exps.weight", true, E);
            x.u = add(b + "ffn_up_exps.weight", true, E);
            x.d = add(b + "ffn_down_exps.weight", true, E);
        } else {
            x.r = -1;
            x.g = add(b + "ffn_gate.weight", true, 1);
            x.u = add(b + "ffn_up.weight", true, 1);
            x.d = add(b + "ffn_down.weight", true, 1);
        }
    }
    if (hp.n_expert > 0 && hp.n_expert_used != 2)
        throw Error("MoE: this build serves top-2 routing (expert_used_count=2)");
    arena_bytes = off;
    for (const auto& pl : plan) account(*pl.t, pl.experts);
    if (i_out < 0 && !bert) weight_bytes += (long long)plan[i_te].t->nbytes;   // tied output head

    MI_HIP(hipSetDevice(device));
    MI_HIP(hipMalloc(&arena, arena_bytes));

    // ---- upload + repack ----
    if (!p.no_upload) {
        size_t max_raw = 0;
        for (const auto& pl : plan)
            if (is_quant(pl.t->type)) max_raw = std::max(max_raw, pl.t->nbytes);
        uint8_t* staging = nullptr;
        if (max_raw) MI_HIP(hipMalloc(&staging, max_raw));
        for (const auto& pl : plan) {
            const size_t src = gguf.data_offset + pl.t->offset;
            if (src + pl.t->nbytes > size) {
                if (staging) hipFree(staging);
                throw Error("GGUF: tensor data of " + pl.t->name + " beyond the end of the image");
            }
            if (is_quant(pl.t->type)) {
                MI_HIP(hipMemcpy(staging, data + src, pl.t->nbytes, hipMemcpyHostToDevice));
                uint8_t* planes[4] = {arena + pl.off[0], arena + pl.off[1], arena + pl.off[2], arena + pl.off[3]};
                launch_repack(staging, pl.t->type, pl.rows, pl.K, planes, nullptr);
            } else {
                MI_HIP(hipMemcpy(arena + pl.off[0], data + src, pl.t->nbytes, hipMemcpyHostToDevice));
            }
        }
        MI_HIP(hipDeviceSynchronize());
        if (staging) hipFree(staging);
    }

    // ---- device views ----
    auto qm = [&](int idx) -> QMat {
        QMat m{};
        const Planned& pl = plan[idx];
        m.type = pl.t->type;
        m.K = pl.K;
        m.nb = pl.K / 256;
        m.rows = (int)pl.rows;
        for (int k = 0; k < std::max(1, plane_count(m.type)); ++k) m.p[k] = arena + pl.off[k];   // (not quantised: the raw copy)
        split_experts(m, pl.experts);
        return m;
    };
    auto f32p = [&](int idx) -> float* {
        if (idx < 0) return nullptr;
        if (plan[idx].t->type != T_F32) throw Error("tensor " + plan[idx].t->name + " must be F32");
        return reinterpret_cast<float*>(arena + plan[idx].off[0]);
    };
    tok_embd = qm(i_te);
    if (i_pe >= 0) pos_embd = qm(i_pe);
    if (bert) {
        auto f16p = [&](int idx) { return reinterpret_cast<const __half*>(arena + plan[idx].off[0]); };
        tok_types = qm(i_tt);
        embd_norm = f32p(i_en);
        embd_norm_b = f32p(i_enb);
        enc_layers.resize(hp.n_layer);
        for (int l = 0; l < hp.n_layer; ++l) {
            EncLayer& L = enc_layers[l];
            const BertIdx& x = bi[l];
            L.wq = f16p(x.w[0]); L.wk = f16p(x.w[1]); L.wv = f16p(x.w[2]);
            L.wo = f16p(x.w[3]); L.up = f16p(x.w[4]); L.down = f16p(x.w[5]);
            L.bq = f32p(x.b[0]); L.bk = f32p(x.b[1]); L.bv = f32p(x.b[2]);
            L.bo = f32p(x.b[3]); L.bup = f32p(x.b[4]); L.bdown = f32p(x.b[5]);
            L.attn_out_norm = f32p(x.an); L.attn_out_norm_b = f32p(x.anb);
            L.layer_out_norm = f32p(x.on); L.layer_out_norm_b = f32p(x.onb);
        }
    }
    output_norm_b = f32p(i_onb);
    if (!bert) {
        output = i_out >= 0 ? qm(i_out) : qm(i_te);
        if (!f16 && !is_quant(output.type)) throw Error("output head must be a quantised tensor in this build");
    }
    output_norm = f32p(i_on);
    rope_freqs = f32p(i_rf);
    layers.resize(bert ? 0 : hp.n_layer);
    for (int l = 0; l < hp.n_layer && !bert; ++l) {
        Layer& L = layers[l];
        const LayerIdx& x = li[l];
        L.attn_norm = f32p(x.an);
        L.ffn_norm = f32p(x.fn);
        L.wq = qm(x.q); L.wk = qm(x.k); L.wv = qm(x.v); L.wo = qm(x.o);
        L.gate = qm(x.g); L.up = qm(x.u); L.down = qm(x.d);
        L.router = f32p(x.r);
        L.attn_norm_b = f32p(x.anb);
        L.ffn_norm_b = f32p(x.fnb);
        L.bqkv = f32p(x.bqkv);
        L.bo = f32p(x.bo);
        L.bup = f32p(x.bu);
        L.bdown = f32p(x.bd);
        for (const QMat* m : {&L.wq, &L.wk, &L.wv, &L.wo, &L.gate, &L.up, &L.down})
            if (!f16 && !is_quant(m->type)) throw Error("layer weights must be quantised (Q4_K/Q5_K/Q6_K/Q8_0)");
        if (f16) continue;   // Q, K and V stay three matrices (wq, wk, wv): no row groups
        if (gpt2) {   // the fused QKV rows: n_embd Q rows, n_embd K rows, n_embd V rows
            L.n_qkv = 1;
            L.qkv[0] = qm(x.qkv_groups[0][0]);
            L.qkv_nq[0] = hp.n_embd;
            L.qkv_nk[0] = hp.n_head_kv * hp.head_dim;
            if (L.qkv[0].rows != L.qkv_nq[0] + 2 * L.qkv_nk[0]) throw Error("gpt2: attn_qkv must have 3 n_embd rows");
            continue;
        }
        L.n_qkv = (int)x.qkv_groups.size();
        int seen = 0;   // Q rows, then K rows, then V rows across the groups
        for (int g = 0; g < L.n_qkv; ++g) {
            QMat m = qm(x.qkv_groups[g][0]);
            int nq = 0, nk = 0, rows = 0;
            for (int i : x.qkv_groups[g]) {
                const int r = (int)plan[i].rows;
                if (seen == 0) nq += r;
                else if (seen == 1) nk += r;
                rows += r;
                ++seen;
            }
            m.rows = rows;
            L.qkv[g] = m;
            L.qkv_nq[g] = nq;
            L.qkv_nk[g] = nk;
        }
    }
    if (gpt2 || bert) {
        const std::vector<unsigned short> t = gelu_table_host();
        MI_HIP(hipMalloc(&gelu_tab, t.size() * sizeof(unsigned short)));
        MI_HIP(hipMemcpy(gelu_tab, t.data(), t.size() * sizeof(unsigned short), hipMemcpyHostToDevice));
    }
}

}  // namespace mi
