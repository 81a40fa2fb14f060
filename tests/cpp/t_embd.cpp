// bl::llama::InstanceEmbedding (reference InstanceEmbedding.hpp:22-49, InstanceEmbedding.cpp) on a
// synthetic model.  tests/test_host_embd.py writes the inputs, runs this and compares what it
// writes with numpy and with the Python binding's embeddings through the C ABI.
//
//   t_embd --norm-only --in=FILE --out=FILE
//       FILE in: n f32.  out: for each normalisation -1, 0, 1, 2, 3 the normalised vector, then the
//       same five for the all-zero vector of that length (f32, back to back).  No GPU.
//   t_embd --model=M --prompt=1,2,3 --out=FILE
//       out: getEmbeddingVector(prompt, 2), then getEmbeddingVector(prompt, -1) (f32).
#include "llama.hpp"
#include "mi_engine.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

using namespace bl::llama;

static int g_fail = 0;
#define CHECK(expr)                                                       \
    do {                                                                  \
        if (!(expr)) {                                                    \
            ++g_fail;                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #expr); \
        }                                                                 \
    } while (0)

static bool write_all(const std::string& path, const std::vector<float>& v) {
    std::FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    const bool ok = std::fwrite(v.data(), sizeof(float), v.size(), f) == v.size();
    std::fclose(f);
    return ok;
}

template <class F>
static bool throws(F&& f) {
    try {
        f();
    } catch (const std::exception&) {
        return true;
    }
    return false;
}

int main(int argc, char** argv) {
    std::string model_path, in, out, prompt_s;
    bool norm_only = false;
    for (int i = 1; i < argc; ++i) {
        const std::string s = argv[i];
        if (s == "--norm-only") norm_only = true;
        else if (s.rfind("--model=", 0) == 0) model_path = s.substr(8);
        else if (s.rfind("--in=", 0) == 0) in = s.substr(5);
        else if (s.rfind("--out=", 0) == 0) out = s.substr(6);
        else if (s.rfind("--prompt=", 0) == 0) prompt_s = s.substr(9);
    }
    if (out.empty() || (norm_only ? in.empty() : model_path.empty() || prompt_s.empty())) {
        std::printf("usage: t_embd --norm-only --in=FILE --out=FILE | t_embd --model=M --prompt=1,2,3 --out=FILE\n");
        return 2;
    }
    try {
        std::vector<float> res;
        if (norm_only) {
            std::vector<float> x;
            std::FILE* f = std::fopen(in.c_str(), "rb");
            if (!f) {
                std::printf("cannot read %s\n", in.c_str());
                return 2;
            }
            float v;
            while (std::fread(&v, sizeof(v), 1, f) == 1) x.push_back(v);
            std::fclose(f);
            const std::vector<float> zero(x.size(), 0.0f);
            const std::vector<float>* srcs[2] = {&x, &zero};
            for (const std::vector<float>* src : srcs)
                for (int norm : {-1, 0, 1, 2, 3}) {
                    std::vector<float> y(src->size(), -7.0f);
                    InstanceEmbedding::normalize(*src, y, norm);
                    res.insert(res.end(), y.begin(), y.end());
                }
            std::vector<float> small(1);
            CHECK(throws([&] { InstanceEmbedding::normalize(x, small, 2); }) || x.size() <= 1);
        } else {
            std::vector<Token> prompt;
            for (size_t p = 0; p < prompt_s.size();) {
                size_t q = prompt_s.find(',', p);
                if (q == std::string::npos) q = prompt_s.size();
                prompt.push_back((Token)std::atoi(prompt_s.substr(p, q - p).c_str()));
                p = q + 1;
            }
            Model model(model_path, Model::Params{});
            InstanceEmbedding inst(model, InstanceEmbedding::InitParams{.ctxSize = 64});
            CHECK(inst.embeddingDim() == (uint32_t)mi_model_n_embd(model.mmodel()));
            CHECK(&inst.model() == &model);
            CHECK(mi_ctx_pooling(inst.mctx()) == (mi_model_pooling_type(model.mmodel()) < 0 ? MI_POOLING_NONE
                                                                                           : mi_model_pooling_type(model.mmodel())));
            const std::vector<float> e2 = inst.getEmbeddingVector(prompt);   // Euclidean by default
            CHECK(e2.size() == inst.embeddingDim());
            double s = 0.0;
            for (float v : e2) s += (double)v * (double)v;
            CHECK(std::fabs(std::sqrt(s) - 1.0) <= 1e-6);
            const std::vector<float> raw = inst.getEmbeddingVector(prompt, -1);
            // a second call clears the cache first: the same embedding, bit for bit
            CHECK(inst.getEmbeddingVector(prompt) == e2);
            CHECK(mi_logits(inst.mctx(), -1) == nullptr);   // embeddings mode: no head
            CHECK(throws([&] { inst.getEmbeddingVector({}); }));
            const std::vector<Token> longp(65, 5);          // past the 64-cell context (and its batch)
            CHECK(throws([&] { inst.getEmbeddingVector(longp); }));
            CHECK(inst.getEmbeddingVector(prompt) == e2);   // the failed calls left the instance usable
            res = e2;
            res.insert(res.end(), raw.begin(), raw.end());
        }
        if (!write_all(out, res)) {
            std::printf("cannot write %s\n", out.c_str());
            return 2;
        }
    } catch (const std::exception& e) {
        std::printf("FAILED: exception: %s\n", e.what());
        return 1;
    }
    std::printf("%s (%d failed)\n", g_fail ? "FAILED" : "ok", g_fail);
    return g_fail ? 1 : 0;
}
