// InstanceEmbedding::getEmbeddingVectors on a BERT model.  tests/test_gpu_enc_seqs.py writes the
// prompts, runs this and compares.
//
//   t_enc_seqs --model=M --in=FILE --out=FILE --batch=N
//       in: per prompt {u32 n, n x i32 token ids}.  out, P = prompts, f32 rows of n_embd:
//       P rows getEmbeddingVectors(all, -1), P rows getEmbeddingVectors(all) (Euclidean),
//       P rows getEmbeddingVector(prompt, -1).  Checked here: one getEmbeddingVectors call per
//       prompt gives the bits of the call over all of them.
#include "llama.hpp"
#include "mi_engine.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace bl::llama;

int main(int argc, char** argv) {
    std::string model_path, in, out;
    uint32_t batch = 0;
    for (int i = 1; i < argc; ++i) {
        const std::string s = argv[i];
        if (s.rfind("--model=", 0) == 0) model_path = s.substr(8);
        else if (s.rfind("--in=", 0) == 0) in = s.substr(5);
        else if (s.rfind("--out=", 0) == 0) out = s.substr(6);
        else if (s.rfind("--batch=", 0) == 0) batch = (uint32_t)std::atoi(s.c_str() + 8);
    }
    if (model_path.empty() || in.empty() || out.empty() || batch == 0) {
        std::printf("usage: t_enc_seqs --model=M --in=FILE --out=FILE --batch=N\n");
        return 2;
    }
    int fail = 0;
    try {
        std::vector<std::vector<Token>> prompts;
        std::FILE* f = std::fopen(in.c_str(), "rb");
        uint32_t n;
        while (f && std::fread(&n, 4, 1, f) == 1) {
            prompts.emplace_back(n);
            if (std::fread(prompts.back().data(), 4, n, f) != n) return 2;
        }
        if (f) std::fclose(f);
        Model model(model_path, Model::Params{});
        InstanceEmbedding inst(model, InstanceEmbedding::InitParams{.ctxSize = batch, .batchSize = batch});
        const auto raw = inst.getEmbeddingVectors(prompts, -1);
        if (mi_batch_path(inst.mctx()) != 6) ++fail, std::printf("FAILED: batch path %d\n", mi_batch_path(inst.mctx()));
        const auto e2 = inst.getEmbeddingVectors(prompts);
        std::vector<std::vector<float>> single;
        for (size_t i = 0; i < prompts.size(); ++i) {
            const auto one = inst.getEmbeddingVectors(std::span<const std::vector<Token>>(&prompts[i], 1), -1);
            if (one.size() != 1 || std::memcmp(one[0].data(), raw[i].data(), raw[i].size() * sizeof(float)) != 0)
                ++fail, std::printf("FAILED: prompt %zu alone differs from the batch\n", i);
            single.push_back(inst.getEmbeddingVector(prompts[i], -1));
        }
        f = std::fopen(out.c_str(), "wb");
        for (const std::vector<std::vector<float>>* set : {&raw, &e2, &std::as_const(single)})
            for (const std::vector<float>& v : *set)
                if (!f || std::fwrite(v.data(), sizeof(float), v.size(), f) != v.size()) return 2;
        std::fclose(f);
    } catch (const std::exception& e) {
        std::printf("FAILED: exception: %s\n", e.what());
        return 1;
    }
    std::printf("%s (%d failed)\n", fail ? "FAILED" : "ok", fail);
    return fail ? 1 : 0;
}
