// bl::llama::LoraAdapter and Instance::addLora / clearLoraState on a synthetic model (reference
// LoraAdapter.cpp:12-19, Instance.cpp:52-61).  tests/test_host_lora.py writes the model and the
// adapter files, runs this and compares the top-10 it prints with what the Python binding obtains
// through the C ABI.
//
//   t_lora --model=M --lora=A.gguf --bad=B.gguf --out=FILE
// A: an adapter of the model (set with scale 0.75, then 0.25); B: a file the loader refuses.
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

// the same through a Session: the top-1 logit of the first predicted token
static Top session_top(Instance& inst) {
    Top t{};
    Session& s = inst.startSession({});
    s.setInitialPrompt(std::vector<Token>(kPrompt, kPrompt + sizeof(kPrompt) / sizeof(kPrompt[0])));
    CHECK(mi_topk(inst.mctx(), -1, 10, t.ids, t.vals) == 10);
    inst.stopSession();
    return t;
}

static void print(std::FILE* f, const char* tag, const Top& t) {
    std::fprintf(f, "%s", tag);
    for (int i = 0; i < 10; ++i) std::fprintf(f, " %d:%.9g", t.ids[i], t.vals[i]);
    std::fprintf(f, "\n");
}

int main(int argc, char** argv) {
    std::string model_path, lora, bad, out;
    for (int i = 1; i < argc; ++i) {
        const std::string s = argv[i];
        if (s.rfind("--model=", 0) == 0) model_path = s.substr(8);
        else if (s.rfind("--lora=", 0) == 0) lora = s.substr(7);
        else if (s.rfind("--bad=", 0) == 0) bad = s.substr(6);
        else if (s.rfind("--out=", 0) == 0) out = s.substr(6);
    }
    if (model_path.empty() || lora.empty() || bad.empty() || out.empty()) {
        std::printf("usage: t_lora --model=M --lora=A --bad=B --out=FILE\n");
        return 2;
    }
    try {
        Model model(model_path, Model::Params{});
        Model other(model_path, Model::Params{});
        Instance inst(model, Instance::InitParams{.ctxSize = 64});

        const Top base = top10(inst);
        LoraAdapter adapter(model, lora);
        CHECK(adapter.madapter() != nullptr && adapter.path() == lora && &adapter.model() == &model);
        CHECK(mi_lora_n_pairs(adapter.madapter()) > 0);

        // the loader's refusal throws, with the engine's reason
        bool thrown = false;
        try {
            LoraAdapter refused(model, bad);
        } catch (const std::exception& e) {
            thrown = std::string(e.what()).find("Failed to load LoRA adapter") != std::string::npos &&
                     std::string(e.what()).find("general.type") != std::string::npos;
        }
        CHECK(thrown);

        inst.addLora(adapter, 0.75f);
        const Top adapted = top10(inst);
        CHECK(!(adapted == base));
        CHECK(session_top(inst) == adapted);   // a Session's prompt sees the adapter
        inst.addLora(adapter, 0.25f);          // the same adapter again: its scale is updated
        const Top rescaled = top10(inst);
        CHECK(!(rescaled == adapted) && !(rescaled == base));
        inst.clearLoraState();
        const Top cleared = top10(inst);
        CHECK(cleared == base);
        CHECK(session_top(inst) == base);

        // an adapter of another Model object (Instance.cpp:53-55)
        LoraAdapter foreign(other, lora);
        thrown = false;
        try {
            inst.addLora(foreign, 1.0f);
        } catch (const std::exception& e) {
            thrown = std::string(e.what()) == "LoraAdapter model does not match the instance model";
        }
        CHECK(thrown);
        CHECK(top10(inst) == base);   // and the context stays without an adapter

        std::FILE* f = std::fopen(out.c_str(), "w");
        if (!f) {
            std::printf("cannot write %s\n", out.c_str());
            return 2;
        }
        print(f, "base", base);
        print(f, "adapted", adapted);
        print(f, "rescaled", rescaled);
        print(f, "cleared", cleared);
        std::fclose(f);
    } catch (const std::exception& e) {
        std::printf("FAILED: exception: %s\n", e.what());
        return 1;
    }
    std::printf("%s (%d failed)\n", g_fail ? "FAILED" : "ok", g_fail);
    return g_fail ? 1 : 0;
}
