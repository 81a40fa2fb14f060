// The WordPiece tokenizer of bl::llama::Vocab (llm_tokenizer_wpm) and InstanceEmbedding on a BERT
// model.  tests/test_host_bert.py and tests/test_gpu_bert.py write the inputs, run this and compare.
//
//   t_bert --tok --model=M --in=FILE --out=FILE
//       M is loaded vocab-only (no GPU).  FILE in: records {u8 addSpecial, u8 parseSpecial, u32 len,
//       len bytes of UTF-8}.  out: per record {u32 n, n x i32 token ids}.
//   t_bert --embd --model=M --text=TEXT --out=FILE
//       out: {u32 n, n x i32} the tokens of TEXT (addSpecial), then getEmbeddingVector(tokens, 2) and
//       getEmbeddingVector(tokens, -1) (f32).
#include "llama.hpp"
#include "mi_engine.h"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
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

static bool read_file(const std::string& path, std::vector<unsigned char>& v) {
    std::FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) return false;
    unsigned char buf[4096];
    size_t n;
    while ((n = std::fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + n);
    std::fclose(f);
    return true;
}

static void put_tokens(std::vector<unsigned char>& o, const std::vector<Token>& t) {
    const uint32_t n = (uint32_t)t.size();
    const unsigned char* p = reinterpret_cast<const unsigned char*>(&n);
    o.insert(o.end(), p, p + 4);
    for (Token x : t) {
        const int32_t v = x;
        p = reinterpret_cast<const unsigned char*>(&v);
        o.insert(o.end(), p, p + 4);
    }
}

int main(int argc, char** argv) {
    std::string model_path, in, out, text;
    bool tok = false, embd = false;
    for (int i = 1; i < argc; ++i) {
        const std::string s = argv[i];
        if (s == "--tok") tok = true;
        else if (s == "--embd") embd = true;
        else if (s.rfind("--model=", 0) == 0) model_path = s.substr(8);
        else if (s.rfind("--in=", 0) == 0) in = s.substr(5);
        else if (s.rfind("--out=", 0) == 0) out = s.substr(6);
        else if (s.rfind("--text=", 0) == 0) text = s.substr(7);
    }
    if (tok == embd || model_path.empty() || out.empty() || (tok && in.empty())) {
        std::printf("usage: t_bert --tok --model=M --in=FILE --out=FILE | t_bert --embd --model=M --text=TEXT --out=FILE\n");
        return 2;
    }
    try {
        std::vector<unsigned char> res;
        if (tok) {
            Model model(model_path, Model::Params{.vocabOnly = true});
            const Vocab& v = model.vocab();
            CHECK(!model.hasEncoder());   // llama.cpp keeps that for encoder-decoder models
            CHECK(v.cls() >= 0 && v.sep() >= 0 && v.unk() >= 0 && v.pad() >= 0);
            CHECK(v.tokenToString(v.cls(), true) == "[CLS]" && v.tokenToString(v.cls(), false).empty());
            std::vector<unsigned char> data;
            if (!read_file(in, data)) {
                std::printf("cannot read %s\n", in.c_str());
                return 2;
            }
            for (size_t p = 0; p + 6 <= data.size();) {
                const bool add = data[p] != 0, parse = data[p + 1] != 0;
                uint32_t len;
                std::memcpy(&len, &data[p + 2], 4);
                p += 6;
                if (p + len > data.size()) {
                    std::printf("truncated input\n");
                    return 2;
                }
                const std::string s(reinterpret_cast<const char*>(data.data() + p), len);
                p += len;
                const std::vector<Token> t = v.tokenize(s, add, parse);
                // pieces: a word start reads back with a leading space, a continuation without
                for (Token x : t) {
                    const std::string piece = v.tokenToString(x, true);
                    CHECK(!piece.empty() && piece.rfind("\xe2\x96\x81", 0) != 0);
                }
                put_tokens(res, t);
            }
        } else {
            Model model(model_path, Model::Params{});
            const std::vector<Token> t = model.vocab().tokenize(text, true, true);
            InstanceEmbedding inst(model, InstanceEmbedding::InitParams{});
            CHECK(inst.embeddingDim() == (uint32_t)mi_model_n_embd(model.mmodel()));
            CHECK(mi_ctx_pooling(inst.mctx()) == (mi_model_pooling_type(model.mmodel()) < 0 ? MI_POOLING_NONE
                                                                                           : mi_model_pooling_type(model.mmodel())));
            CHECK(mi_decode_path(inst.mctx()) == 2 && mi_model_causal_attn(model.mmodel()) == 0);
            const std::vector<float> e2 = inst.getEmbeddingVector(t);   // Euclidean by default
            CHECK(e2.size() == inst.embeddingDim());
            double s = 0.0;
            for (float x : e2) s += (double)x * (double)x;
            CHECK(std::fabs(std::sqrt(s) - 1.0) <= 1e-6);
            const std::vector<float> raw = inst.getEmbeddingVector(t, -1);
            CHECK(inst.getEmbeddingVector(t) == e2);   // stateless: the same bits again
            CHECK(mi_logits(inst.mctx(), -1) == nullptr);
            put_tokens(res, t);
            for (const std::vector<float>* f : {&e2, &raw}) {
                const unsigned char* p = reinterpret_cast<const unsigned char*>(f->data());
                res.insert(res.end(), p, p + f->size() * sizeof(float));
            }
        }
        std::FILE* f = std::fopen(out.c_str(), "wb");
        if (!f || std::fwrite(res.data(), 1, res.size(), f) != res.size()) {
            std::printf("cannot write %s\n", out.c_str());
            return 2;
        }
        std::fclose(f);
    } catch (const std::exception& e) {
        std::printf("FAILED: exception: %s\n", e.what());
        return 1;
    }
    std::printf("%s (%d failed)\n", g_fail ? "FAILED" : "ok", g_fail);
    return g_fail ? 1 : 0;
}
