// LoRA adapters, host side: the adapter-file loader and a context's adapter state.
//
// Reference anchors:
//   llama_adapter_lora_init    /root/reference/inference/code/llama/LoraAdapter.cpp:12-19
//   llama_set_adapter_lora     /root/reference/inference/code/llama/Instance.cpp:52-57
//   llama_clear_adapter_lora   /root/reference/inference/code/llama/Instance.cpp:59-61
// Semantics: llama.cpp b5187 src/llama-adapter.cpp (llama_adapter_lora_init_impl) and
// src/llama-graph.cpp (build_lora_mm).
#include "engine.h"

#include <algorithm>
#include <cstring>

namespace mi {

namespace {
const char* const kTargetNames[LT_N] = {"attn_q", "attn_k", "attn_v", "attn_output", "ffn_gate", "ffn_up", "ffn_down"};

bool ends_with(const std::string& s, const char* suf) {
    const size_t n = std::strlen(suf);
    return s.size() >= n && s.compare(s.size() - n, n, suf) == 0;
}

// "blk.<l>.<target>.weight" -> (l, target); false for any other base tensor
bool parse_base(const std::string& name, int n_layer, int& layer, int& target) {
    if (name.compare(0, 4, "blk.") != 0) return false;
    size_t p = 4;
    long long l = 0;
    if (p >= name.size() || name[p] < '0' || name[p] > '9') return false;
    while (p < name.size() && name[p] >= '0' && name[p] <= '9' && l < 100000) l = l * 10 + (name[p++] - '0');
    if (p >= name.size() || name[p] != '.' || l >= n_layer) return false;
    const std::string rest = name.substr(p + 1);
    for (int t = 0; t < LT_N; ++t)
        if (rest == std::string(kTargetNames[t]) + ".weight") {
            layer = (int)l;
            target = t;
            return true;
        }
    return false;
}
}  // namespace

std::shared_ptr<Lora> Lora::load(const Model* m, const uint8_t* data, size_t size) {
    if (!m) throw Error("lora: null model");
    if (!data) throw Error("lora: null image");
    if (m->f16) throw Error("lora: adapters on an unquantised F16 base model are not supported");
    Gguf g;
    g.parse(data, size);
    if (g.get_str("general.type", "") != "adapter") throw Error("lora: general.type is not 'adapter'");
    if (g.get_str("adapter.type", "") != "lora") throw Error("lora: adapter.type is not 'lora'");
    const std::string arch = g.get_str("general.architecture", ""), march = m->gguf.get_str("general.architecture", "");
    if (arch != march) throw Error("lora: the adapter's architecture '" + arch + "' differs from the base model's '" + march + "'");
    if (m->hp.arch != ARCH_LLAMA) {   // worded for any other architecture ("GPT-2" as that family is written)
        throw Error("lora: " + (march == "gpt2" ? std::string("GPT-2") : march) +
                    " base models are not supported: adapters are served on LLaMA-architecture base models only");
    }
    if (m->hp.n_expert > 0) throw Error("lora: MoE base models are not supported");
    auto out = std::make_shared<Lora>();
    out->m = m;
    out->alpha = (float)g.get_float("adapter.lora.alpha", 0.0);
    struct Half {
        const GgufTensor *a = nullptr, *b = nullptr;
    };
    std::map<std::string, Half> ab;
    std::vector<std::string> order;
    for (const GgufTensor& t : g.tensors) {
        const bool is_a = ends_with(t.name, ".lora_a"), is_b = ends_with(t.name, ".lora_b");
        if (!is_a && !is_b) throw Error("lora: tensor '" + t.name + "' has an unexpected suffix (neither .lora_a nor .lora_b)");
        const std::string base = t.name.substr(0, t.name.size() - 7);
        if (!ab.count(base)) order.push_back(base);
        (is_a ? ab[base].a : ab[base].b) = &t;
    }
    for (const std::string& base : order) {
        const Half& h = ab[base];
        if (!h.a || !h.b) throw Error("lora: '" + base + "' is missing its " + (h.a ? "lora_b" : "lora_a") + " half");
        const GgufTensor* w = m->gguf.tensor(base);
        if (!w) throw Error("lora: base tensor '" + base + "' does not exist in the model");
        LoraPair p;
        if (!parse_base(base, m->hp.n_layer, p.layer, p.target))
            throw Error("lora: base tensor '" + base + "' is not supported (attn_q/k/v/output, ffn_gate/up/down of a layer only)");
        for (const GgufTensor* t : {h.a, h.b}) {
            if (t->type != T_F16 && t->type != T_F32) throw Error("lora: tensor '" + t->name + "' is neither F16 nor F32");
            if (t->n_dims > 2) throw Error("lora: tensor '" + t->name + "' has an invalid shape (more than 2 dimensions)");
        }
        if (h.a->ne[0] != w->ne[0] || h.b->ne[1] != w->ne[1])
            throw Error("lora: tensor '" + base + "' has an invalid shape for this base model");
        if (h.a->ne[1] != h.b->ne[0]) throw Error("lora: '" + base + "': the lora_a tensor is not transposed (rank mismatch)");
        if (h.a->ne[1] < 1 || h.a->ne[1] > LORA_MAX_RANK)
            throw Error("lora: '" + base + "' has rank " + std::to_string(h.a->ne[1]) + " (1.." + std::to_string(LORA_MAX_RANK) + " supported)");
        if (h.a->ne[0] % 4) throw Error("lora: '" + base + "': the input width must be a multiple of 4");
        p.r = (int)h.a->ne[1];
        p.K = (int)h.a->ne[0];
        p.rows = (int)h.b->ne[1];
        p.a_type = h.a->type;
        p.b_type = h.b->type;
        for (const GgufTensor* t : {h.a, h.b}) {
            const size_t src = g.data_offset + t->offset;
            if (src > size || t->nbytes > size - src) throw Error("lora: tensor data of '" + t->name + "' beyond the end of the file (truncated)");
            if (!m->vocab_only) (t == h.a ? p.a : p.b).assign(data + src, data + src + t->nbytes);
        }
        out->pairs.push_back(std::move(p));
    }
    return out;
}

// ------------------------------------------------------------ the context ----
namespace {
constexpr int kMaxLoras = 4;
int group_of(int target) { return target <= LT_V ? 0 : target == LT_O ? 1 : target <= LT_UP ? 2 : 3; }
int slot_of(int target) { return target <= LT_V ? target : target == LT_UP ? 1 : 0; }

// the adapters' summed rank per base tensor must fit the kernels
void check_ranks(const std::vector<Ctx::LoraSet>& set, int n_layer) {
    static_assert(kMaxLoras == LORA_MAX_STACK, "LoraFold::tab holds LORA_MAX_STACK adapters");
    if ((int)set.size() > kMaxLoras) throw Error("set_lora: at most 4 adapters on a context");
    std::vector<int> sum((size_t)n_layer * LT_N, 0);
    for (const Ctx::LoraSet& s : set)
        for (const LoraPair& p : s.a->pairs)
            if ((sum[(size_t)p.layer * LT_N + p.target] += p.r) > LORA_MAX_RANK)
                throw Error("set_lora: the adapters' summed rank on blk." + std::to_string(p.layer) + "." + kTargetNames[p.target] +
                            " exceeds " + std::to_string(LORA_MAX_RANK));
}

float half_to_float(uint16_t h) {
    const uint32_t sign = (uint32_t)(h & 0x8000) << 16, exp = (h >> 10) & 0x1F, man = h & 0x3FF;
    uint32_t bits;
    if (exp == 0) {
        if (man == 0) {
            bits = sign;
        } else {   // subnormal
            int e = -1;
            uint32_t mm = man;
            do {
                ++e;
                mm <<= 1;
            } while (!(mm & 0x400));
            bits = sign | ((uint32_t)(127 - 15 - e) << 23) | ((mm & 0x3FF) << 13);
        }
    } else if (exp == 31) {
        bits = sign | 0x7F800000u | (man << 13);
    } else {
        bits = sign | ((exp + 112) << 23) | (man << 13);
    }
    float f;
    std::memcpy(&f, &bits, 4);
    return f;
}

// n elements of `type` at src -> dst as F16 (to_f16: the source is F16 too) or F32
void put_elems(uint8_t* dst, bool to_f16, const uint8_t* src, int type, size_t n) {
    if (to_f16) {
        std::memcpy(dst, src, n * 2);
    } else if (type == T_F32) {
        std::memcpy(dst, src, n * 4);
    } else {
        for (size_t i = 0; i < n; ++i) {
            uint16_t h;
            std::memcpy(&h, src + 2 * i, 2);
            const float f = half_to_float(h);
            std::memcpy(dst + 4 * i, &f, 4);
        }
    }
}
}  // namespace

void Ctx::set_lora(const std::shared_ptr<Lora>& a, float scale) {
    if (!a) throw Error("set_lora: null adapter");
    if (a->m != m) throw Error("set_lora: the adapter belongs to another model");
    if (m->f16) throw Error("set_lora: adapters on an unquantised F16 base model are not supported");
    std::vector<LoraSet> next = loras;
    auto it = std::find_if(next.begin(), next.end(), [&](const LoraSet& s) { return s.a == a; });
    if (it != next.end()) it->scale = scale;
    else next.push_back(LoraSet{a, scale});
    check_ranks(next, m->hp.n_layer);
    std::swap(loras, next);
    try {
        lora_rebuild();
    } catch (...) {   // (an allocation failed: back to the adapters that were set)
        std::swap(loras, next);
        lora_g.clear();
        try {
            lora_rebuild();
        } catch (...) {
            loras.clear();
        }
        throw;
    }
}

int Ctx::rm_lora(const Lora* a) {
    auto it = std::find_if(loras.begin(), loras.end(), [&](const LoraSet& s) { return s.a.get() == a; });
    if (it == loras.end()) return -1;
    loras.erase(it);
    lora_rebuild();
    return 0;
}

void Ctx::clear_lora() {
    if (loras.empty() && lora_g.empty()) return;
    loras.clear();
    lora_rebuild();
}

// The stacks of the adapters in `loras`, in one device allocation: per layer and group the A rows
// of the group's tensors (tensor order, then adapter order) with each rank row's s and rounding
// rules, per tensor its B columns in the same order.  A stack is F16 when every member is, else F32
// (an F16 member widened exactly); every tensor's table lists its adapters' rank-row ends and s.
void Ctx::lora_rebuild() {
    const HParams& hp = m->hp;
    MI_HIP(hipSetDevice(device));
    sync();                 // steps in flight still read the old stacks
    invalidate_graphs();    // the next step re-captures with the new arguments
    lora_g.clear();
    mem.release(lora_mem);
    if (loras.empty()) return;
    struct Member {
        const LoraPair* p;
        float s;
    };
    std::vector<std::vector<Member>> mem_of((size_t)hp.n_layer * LT_N);
    for (const LoraSet& ls : loras)
        for (const LoraPair& p : ls.a->pairs)
            // llama_adapter_lora_weight::get_scale
            mem_of[(size_t)p.layer * LT_N + p.target].push_back(Member{&p, ls.a->alpha != 0.0f ? ls.scale * ls.a->alpha / (float)p.r : ls.scale});
    std::vector<uint8_t> img;
    auto reserve = [&](size_t n) {
        const size_t off = (img.size() + 255) / 256 * 256;
        img.resize(off + n, 0);
        return off;
    };
    struct Offs {
        size_t A = 0, rnd = 0, B[3] = {0, 0, 0}, tab[3] = {0, 0, 0};
    };
    std::vector<LoraGroup> gs((size_t)hp.n_layer * 4);
    std::vector<Offs> offs(gs.size());
    bool any = false;
    for (int l = 0; l < hp.n_layer; ++l)
        for (int g = 0; g < 4; ++g) {
            std::vector<int> targets;
            for (int t = 0; t < LT_N; ++t)
                if (group_of(t) == g) targets.push_back(t);
            LoraGroup& G = gs[(size_t)l * 4 + g];
            Offs& O = offs[(size_t)l * 4 + g];
            int K = 0;
            bool a16 = true;
            for (int t : targets)
                for (const Member& mb : mem_of[(size_t)l * LT_N + t]) {
                    G.R += mb.p->r;
                    K = mb.p->K;
                    a16 = a16 && mb.p->a_type == T_F16;
                }
            if (!G.R) continue;
            any = true;
            G.a_f16 = a16 ? 1 : 0;
            const size_t ae = a16 ? 2 : 4;
            O.A = reserve((size_t)G.R * K * ae);
            O.rnd = reserve((size_t)G.R);
            int j = 0;
            for (int t : targets) {
                const std::vector<Member>& ms = mem_of[(size_t)l * LT_N + t];
                const int i = slot_of(t);
                G.off[i] = j;
                bool b16 = true;
                int rows = 0;
                for (const Member& mb : ms) {
                    G.Rt[i] += mb.p->r;
                    rows = mb.p->rows;
                    b16 = b16 && mb.p->b_type == T_F16;
                }
                if (!G.Rt[i]) continue;
                G.b_f16[i] = b16 ? 1 : 0;
                const size_t be = b16 ? 2 : 4;
                O.B[i] = reserve((size_t)rows * G.Rt[i] * be);
                O.tab[i] = reserve((1 + 2 * LORA_MAX_STACK) * sizeof(int));
                const int na = (int)ms.size();
                std::memcpy(img.data() + O.tab[i], &na, sizeof(int));
                int c0 = 0, ai = 0;
                for (const Member& mb : ms) {
                    const LoraPair& p = *mb.p;
                    put_elems(img.data() + O.A + (size_t)j * K * ae, a16, p.a.data(), p.a_type, (size_t)p.r * K);
                    for (int k = 0; k < p.r; ++k)
                        img[O.rnd + j + k] = (uint8_t)((p.a_type == T_F16 ? 1 : 0) | (p.b_type == T_F16 ? 2 : 0));
                    const int end = c0 + p.r;
                    std::memcpy(img.data() + O.tab[i] + (size_t)(1 + ai) * sizeof(int), &end, sizeof(int));
                    std::memcpy(img.data() + O.tab[i] + (size_t)(1 + LORA_MAX_STACK + ai) * sizeof(int), &mb.s, sizeof(float));
                    ++ai;
                    const size_t se = p.b_type == T_F16 ? 2 : 4;
                    for (int r = 0; r < rows; ++r)
                        put_elems(img.data() + O.B[i] + ((size_t)r * G.Rt[i] + c0) * be, b16, p.b.data() + (size_t)r * p.r * se, p.b_type,
                                  (size_t)p.r);
                    j += p.r;
                    c0 += p.r;
                }
            }
        }
    if (!any) return;   // (adapters without a pair)
    lora_mem = mem.dev<char>(img.size());
    MI_HIP(hipMemcpy(lora_mem, img.data(), img.size(), hipMemcpyHostToDevice));
    for (size_t k = 0; k < gs.size(); ++k) {
        LoraGroup& G = gs[k];
        if (!G.R) continue;
        G.A = lora_mem + offs[k].A;
        G.rnd = reinterpret_cast<unsigned char*>(lora_mem + offs[k].rnd);
        for (int i = 0; i < 3; ++i)
            if (G.Rt[i]) {
                G.B[i] = lora_mem + offs[k].B[i];
                G.tab[i] = reinterpret_cast<int*>(lora_mem + offs[k].tab[i]);
            }
    }
    if (!lora_t) lora_t = mem.dev<float>((size_t)kBatchRows * 3 * LORA_MAX_RANK);
    if (!lora_pre) {   // (a context without batch paths: the decode step's one row)
        lora_pre_stride = std::max(hp.n_embd + 2 * kv_dim, 2 * hp.n_ff);
        lora_pre = mem.dev<float>((size_t)(batch_ok ? kBatchRows : 1) * lora_pre_stride);
    }
    // the groups' fold descriptors, read by the decode launches through one pointer
    std::vector<LoraFold> folds(gs.size());
    std::memset(folds.data(), 0, folds.size() * sizeof(LoraFold));
    for (size_t k = 0; k < gs.size(); ++k) {
        const LoraGroup& G = gs[k];
        if (!G.R) continue;
        LoraFold& f = folds[k];
        f.t = lora_t;
        f.t_stride = G.R;
        for (int i = 0; i < 3; ++i) {
            f.B[i] = G.B[i];
            f.R[i] = G.Rt[i];
            f.off[i] = G.off[i];
            f.f16[i] = G.b_f16[i];
            f.tab[i] = G.tab[i];
        }
    }
    if (!lora_folds) lora_folds = mem.dev<LoraFold>(folds.size());
    MI_HIP(hipMemcpy(lora_folds, folds.data(), folds.size() * sizeof(LoraFold), hipMemcpyHostToDevice));
    lora_g = std::move(gs);
}

void Ctx::lora_shrink(const LoraGroup& G, const float* xin, int x_stride, int K, int ntok, const float* norm_w) {
    if (!seg_on()) return;
    LoraShrink p{xin, x_stride, K, ntok, norm_w, m->hp.eps, G.A, G.a_f16, G.R, G.rnd, lora_t};
    launch_lora_shrink(p, stream);
}

void Ctx::lora_expand(const LoraGroup& G, int i, float* out, int out_stride, int rows, int ntok) {
    if (!seg_on()) return;
    LoraExpand p;
    std::memset(&p, 0, sizeof(p));
    p.F.t = lora_t;
    p.F.t_stride = G.R;
    p.F.B[0] = G.B[i];
    p.F.R[0] = G.Rt[i];
    p.F.off[0] = G.off[i];
    p.F.f16[0] = G.b_f16[i];
    p.F.tab[0] = G.tab[i];
    p.ntok = ntok;
    p.rows = rows;
    p.out = out;
    p.out_stride = out_stride;
    launch_lora_expand(p, stream);
}

// rows of tensor i of group g (0: the group has no such tensor); a lora_pre row holds them in order
static int lora_rows(const Model& m, int l, int g, int i) {
    const Layer& L = m.layers[l];
    const int rows[4][3] = {{L.wq.rows, L.wk.rows, L.wv.rows}, {m.hp.n_embd, 0, 0}, {m.hp.n_ff, m.hp.n_ff, 0}, {m.hp.n_embd, 0, 0}};
    return i < 3 ? rows[g][i] : 0;
}

int Ctx::lora_pre_row(int l, int g, int i) const {
    int row = 0;
    for (int j = 0; j < i; ++j) row += lora_rows(*m, l, g, j);
    return row;
}

const float* Ctx::lora_pre_terms(int l, int g, const float* act, int K, int ntok, const float* norm_w) {
    const LoraGroup* G = lora_group(l, g);
    if (!G) return nullptr;
    lora_shrink(*G, act, K, K, ntok, norm_w);
    for (int i = 0; lora_rows(*m, l, g, i); ++i)
        lora_expand(*G, i, lora_pre + lora_pre_row(l, g, i), lora_pre_stride, lora_rows(*m, l, g, i), ntok);
    return lora_pre;
}

}  // namespace mi
