// The host mirror on a GPT-2 model: Instance + Session complete 20 tokens greedily, and two more
// Instances' Sessions verify them with fillCtx -- the serial loop (one decode per claimed token, what
// BLAMA_SERIAL_VERIFY=1 makes the server run) and batchedVerify (one mi_decode MI_OUT_ALL, on the
// GPT-2 batch path: mi_batch_path 2).  The batched result must pass the reference's LogitComparer
// gate against the serial one (identical top-1, score >= 0.95).  tests/test_host_gpt2_batch.py
// writes the model and runs this.
//
//   t_gpt2_batch --model=M --prompt=1,2,3 --out=FILE
//       out: {u32 n, n x i32} the generated tokens.
#include "llama.hpp"
#include "mi_engine.h"

#include <cstdint>
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

int main(int argc, char** argv) {
    std::string model_path, out, prompt_s;
    for (int i = 1; i < argc; ++i) {
        const std::string s = argv[i];
        if (s.rfind("--model=", 0) == 0) model_path = s.substr(8);
        else if (s.rfind("--out=", 0) == 0) out = s.substr(6);
        else if (s.rfind("--prompt=", 0) == 0) prompt_s = s.substr(9);
    }
    if (model_path.empty() || out.empty() || prompt_s.empty()) {
        std::printf("usage: t_gpt2_batch --model=M --prompt=1,2,3 --out=FILE\n");
        return 2;
    }
    try {
        std::vector<Token> prompt;
        for (size_t p = 0; p < prompt_s.size();) {
            size_t q = prompt_s.find(',', p);
            if (q == std::string::npos) q = prompt_s.size();
            prompt.push_back((Token)std::atoi(prompt_s.substr(p, q - p).c_str()));
            p = q + 1;
        }
        Model model(model_path, Model::Params{});
        Instance gen(model, {.ctxSize = 128}), ver(model, {.ctxSize = 128}), verb(model, {.ctxSize = 128});
        CHECK(mi_decode_path(gen.mctx()) == 0);   // GPT-2: the gemv_kernel step
        gen.warmup();
        auto& s = gen.startSession({.temperature = 0.0f});
        s.setInitialPrompt(prompt);
        CHECK(mi_batch_path(gen.mctx()) == 2);     // the prompt went through the batch path
        std::vector<TokenPrediction> p = s.complete({.maxTokens = 20});
        CHECK(p.size() == 20);
        auto& s1 = ver.startSession({.temperature = 0.0f});
        s1.setInitialPrompt(prompt);
        std::vector<TokenPrediction> p1 = s1.fillCtx(p);
        CHECK(mi_batch_path(ver.mctx()) == 0);     // one decode step per claimed token
        auto& s2 = verb.startSession({.temperature = 0.0f, .batchedVerify = true});
        s2.setInitialPrompt(prompt);
        std::vector<TokenPrediction> p2 = s2.fillCtx(p);
        CHECK(mi_batch_path(verb.mctx()) == 2);    // the 20 claimed tokens as one tiled batch
        CHECK(p1.size() == p.size() && p2.size() == p.size());
        MetricsAggregator agg;
        float score = 0;
        for (size_t i = 0; i < p.size() && i < p1.size() && i < p2.size(); ++i) {
            const ComparisonMetrics m = LogitComparer::compare(p1[i].logits, p2[i].logits);
            CHECK(m.top1Match == 1.0f);
            score = agg.pushAndVerify({&m, 1});
        }
        CHECK(score >= 0.95f);
        std::printf("verification: batched against serial, score %.4f\n", score);
        gen.stopSession();
        ver.stopSession();
        verb.stopSession();

        std::FILE* f = std::fopen(out.c_str(), "wb");
        const uint32_t n = (uint32_t)p.size();
        bool ok = f && std::fwrite(&n, 4, 1, f) == 1;
        for (const TokenPrediction& tp : p) {
            const int32_t t = tp.token;
            ok = ok && std::fwrite(&t, 4, 1, f) == 1;
        }
        if (f) std::fclose(f);
        if (!ok) {
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
