// bl::llama::ControlVector and Instance::addControlVector / clearControlVector on a synthetic model
// (reference ControlVector.cpp:101-133, Instance.cpp:73-84).  tests/test_host_cvec.py writes the
// model and the control-vector files, runs this and compares the top-10 it prints with what the
// Python binding obtains through the C ABI.
//
//   t_cvec --model=M --a=A.gguf --b=B.gguf --other=C.gguf --out=FILE
// A and B: vectors of the model's n_embd (loaded with strengths 0.5 and -2); C: another n_embd.
#include "llama.hpp"
#include "mi_engine.h"

#include <cstdio>
#include <cstring>
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

static const Token kPrompt[] = {1, 300, 301, 302, 303, 400, 77, 5};

struct Top {
    int32_t ids[10];
    float vals[10];
    bool operator==(const Top& o) const { return !std::memcmp(ids, o.ids, sizeof(ids)) && !std::memcmp(vals, o.vals, sizeof(vals)); }
};

// the distribution after the prompt on an empty cache
static Top top10(Instance& inst) {
    Top t{};
    mi_kv_clear(inst.mctx());
    CHECK(mi_decode(inst.mctx(), kPrompt, (int32_t)(sizeof(kPrompt) / sizeof(kPrompt[0])), MI_OUT_LAST) == 0);
    CHECK(mi_topk(inst.mctx(), -1, 10, t.ids, t.vals) == 10);
    return t;
}

static void print(std::FILE* f, const char* tag, const Top& t) {
    std::fprintf(f, "%s", tag);
    for (int i = 0; i < 10; ++i) std::fprintf(f, " %d:%.9g", t.ids[i], t.vals[i]);
    std::fprintf(f, "\n");
}

int main(int argc, char** argv) {
    std::string model_path, a, b, other, out;
    for (int i = 1; i < argc; ++i) {
        const std::string s = argv[i];
        if (s.rfind("--model=", 0) == 0) model_path = s.substr(8);
        else if (s.rfind("--a=", 0) == 0) a = s.substr(4);
        else if (s.rfind("--b=", 0) == 0) b = s.substr(4);
        else if (s.rfind("--other=", 0) == 0) other = s.substr(8);
        else if (s.rfind("--out=", 0) == 0) out = s.substr(6);
    }
    if (model_path.empty() || a.empty() || b.empty() || other.empty() || out.empty()) {
        std::printf("usage: t_cvec --model=M --a=A --b=B --other=C --out=FILE\n");
        return 2;
    }
    try {
        Model model(model_path, Model::Params{});
        Instance inst(model, Instance::InitParams{.ctxSize = 64});
        const int n_layer = mi_model_n_layer(model.mmodel()), n_embd = mi_model_n_embd(model.mmodel());

        const Top base = top10(inst);
        ControlVector cv(model, {{a, 0.5f}, {b, -2.0f}});
        CHECK(cv.nEmbd == n_embd);
        CHECK(cv.controlVectorLayerStart == 1);
        CHECK(cv.controlVectorLayerEnd == n_layer);
        CHECK(!cv.data.empty() && cv.data.size() % (size_t)n_embd == 0);
        ControlVector ranged(model, {{a, 1.0f}}, 2, 3);
        CHECK(ranged.controlVectorLayerStart == 2 && ranged.controlVectorLayerEnd == 3);

        inst.addControlVector(cv);
        const Top steered = top10(inst);
        CHECK(!(steered == base));
        inst.clearControlVector();
        const Top cleared = top10(inst);
        CHECK(cleared == base);

        // another n_embd: the loader accepts the file, the engine refuses the vector
        ControlVector wrong(model, {{other, 1.0f}});
        CHECK(wrong.nEmbd > 0 && wrong.nEmbd != n_embd);
        bool thrown = false;
        try {
            inst.addControlVector(wrong);
        } catch (const std::exception& e) {
            thrown = std::string(e.what()) == "Failed to apply control vectors!";
        }
        CHECK(thrown);
        CHECK(top10(inst) == base);   // and the context stays unsteered
        // files of differing widths, or an unreadable one: nEmbd -1, no data
        ControlVector mixed(model, {{a, 1.0f}, {other, 1.0f}});
        CHECK(mixed.nEmbd == -1 && mixed.data.empty());
        ControlVector missing(model, {{a + ".missing", 1.0f}});
        CHECK(missing.nEmbd == -1 && missing.data.empty());

        std::FILE* f = std::fopen(out.c_str(), "w");
        if (!f) {
            std::printf("cannot write %s\n", out.c_str());
            return 2;
        }
        print(f, "base", base);
        print(f, "steered", steered);
        print(f, "cleared", cleared);
        std::fclose(f);
    } catch (const std::exception& e) {
        std::printf("FAILED: exception: %s\n", e.what());
        return 1;
    }
    std::printf("%s (%d failed)\n", g_fail ? "FAILED" : "ok", g_fail);
    return g_fail ? 1 : 0;
}
