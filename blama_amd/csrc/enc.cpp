// Encoder models (ARCH_BERT): the context's buffers and the one pass of a decode call --
// llm_build_bert of llama.cpp b5187 with flash_attn off -- on the kernels of enc.hip.
//
// A call's n tokens take positions 0 .. n - 1 and attend to each other only: there is no KV cache
// and nothing survives the call but the embedding rows.  The launches, in stream order:
//   enc_embed, embd_norm (token_embd_norm), then per layer
//   Q|K|V GEMM (one launch, three matrices; K and V written as f16), attention,
//   W_o GEMM (+ bias + residual), embd_norm (attn_output_norm),
//   up GEMM (+ bias, GELU), down GEMM (+ bias + residual), embd_norm (layer_output_norm)
// -- 7 n_layer + 2 launches, and the pooling launch of a pooled context.  They are not captured
// in a hipGraph: a graph per distinct n would be replayed once by most callers.
#include "engine.h"

#include <algorithm>
#include <cmath>

namespace mi {

void Ctx::enc_init() {
    const HParams& hp = m->hp;
    enc = true;
    enc_max = (int)std::min<uint32_t>({n_batch, (uint32_t)ENC_MAX_TOK, (uint32_t)hp.n_ctx_train});
    if (enc_max < 1) throw Error("encoder context: no room for a token");
    init_enc_attributes();
    const size_t rows = (size_t)enc_max, ne = (size_t)hp.n_embd;
    enc_tok = mem.dev<int>(rows);
    h_enc_tok = mem.host<int>((size_t)kEncRing * rows);
    enc_x = mem.dev<float>(rows * ne);
    enc_a = mem.dev<float>(rows * ne);
    enc_x1 = mem.dev<float>(rows * ne);
    enc_q = mem.dev<float>(rows * ne);
    enc_o = mem.dev<float>(rows * ne);
    enc_h = mem.dev<float>(rows * (size_t)hp.n_ff);
    enc_k = mem.dev<__half>(rows * ne);
    enc_v = mem.dev<__half>(rows * ne);
    // always in embeddings mode: [n_batch] token rows, the pooled row, the last token's row
    embeddings = true;
    embd = mem.dev<float>(((size_t)n_batch + 2) * ne);
    h_embd = mem.host<float>(ne);
}

int Ctx::decode_enc(const int32_t* tokens, int n, bool all) {
    const HParams& hp = m->hp;
    if (n > enc_max)
        throw Error("decode: an encoder call takes at most " + std::to_string(enc_max) +
                    " tokens (min of n_batch, 512 and n_ctx_train), got " + std::to_string(n));
    const int ne = hp.n_embd, nff = hp.n_ff;
    const bool pooled = pooling != MI_POOLING_NONE;
    embd_n = n;
    embd_all = all && !pooled;
    embd_rows = 0;
    embd_valid = false;
    out_rows = 0;

    const long long slot = enc_slot++ % kEncRing;
    if (slot == 0 && enc_slot > 1) MI_HIP(hipStreamSynchronize(stream));   // the ring's copies are done
    int* ht = h_enc_tok + slot * enc_max;
    std::copy(tokens, tokens + n, ht);
    MI_HIP(hipMemcpyAsync(enc_tok, ht, (size_t)n * sizeof(int), hipMemcpyHostToDevice, stream));

    auto norm = [&](const float* in, const float* w, const float* b, float* out) {
        launch_embd_norm(EmbdNorm{in, ne, n, ne, w, b, hp.eps, out, ne}, stream);
    };
    auto gemm = [&](int epi, const float* xin, int K, int rows, const __half* w, const float* bias, const float* resid,
                    float* out) {
        EncGemm g{};
        g.m[0] = EncMat{w, bias, rows, out, nullptr};
        g.nmat = 1;
        g.epi = epi;
        g.K = K;
        g.ntok = n;
        g.x = xin;
        g.x_stride = K;
        g.out_stride = rows;
        g.resid = resid;
        g.gelu_tab = m->gelu_tab;
        launch_enc_gemm(g, stream);
    };

    EncEmbed e{};
    e.tokens = enc_tok;
    e.ntok = n;
    e.n_embd = ne;
    e.tok = m->tok_embd.p[0];
    e.typ = m->tok_types.p[0];
    e.pos = m->pos_embd.p[0];
    e.tok_f16 = m->tok_embd.type == T_F16;
    e.typ_f16 = m->tok_types.type == T_F16;
    e.pos_f16 = m->pos_embd.type == T_F16;
    e.out = enc_a;
    launch_enc_embed(e, stream);
    norm(enc_a, m->embd_norm, m->embd_norm_b, enc_x);

    for (int l = 0; l < hp.n_layer; ++l) {
        const EncLayer& L = m->enc_layers[l];
        EncGemm g{};
        g.m[0] = EncMat{L.wq, L.bq, ne, enc_q, nullptr};
        g.m[1] = EncMat{L.wk, L.bk, ne, nullptr, enc_k};
        g.m[2] = EncMat{L.wv, L.bv, ne, nullptr, enc_v};
        g.nmat = 3;
        g.epi = ENC_BIAS;
        g.K = ne;
        g.ntok = n;
        g.x = enc_x;
        g.x_stride = ne;
        g.out_stride = ne;
        launch_enc_gemm(g, stream);
        launch_enc_attn(EncAttn{enc_q, enc_k, enc_v, ne, ne, ne, hp.n_head, hp.head_dim, n, kq_scale(), enc_o}, stream);
        gemm(ENC_RESID, enc_o, ne, ne, L.wo, L.bo, enc_x, enc_a);
        norm(enc_a, L.attn_out_norm, L.attn_out_norm_b, enc_x1);
        gemm(ENC_GELU, enc_x1, ne, nff, L.up, L.bup, nullptr, enc_h);
        gemm(ENC_RESID, enc_h, nff, ne, L.down, L.bdown, enc_x1, enc_a);
        // the last layer's rows are the embeddings (no final norm): token t -> row t of embd
        norm(enc_a, L.layer_out_norm, L.layer_out_norm_b, l == hp.n_layer - 1 ? embd : enc_x);
    }
    if (pooled) {
        embd_pool_rows(0, n);
    } else if (embd_all) {
        embd_rows = n;
    } else {
        MI_HIP(hipMemcpyAsync(embd_step(), embd + (size_t)(n - 1) * ne, (size_t)ne * sizeof(float), hipMemcpyDeviceToDevice,
                              stream));
    }
    embd_valid = true;
    return 0;
}

}  // namespace mi
