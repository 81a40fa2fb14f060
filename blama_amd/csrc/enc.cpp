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
//
// encode_seqs (mi_encode_seqs) runs the same chain once over several sequences laid end to end:
// the embedding takes each row's position inside its sequence, the norm and GEMM launches take all
// rows, the attention is enc_seq.hip's segmented kernel, and one launch pools every sequence.
//
// nomic-bert (hp.nomic) runs the same chain on the kernels of enc_nomic.hip: no
// position add, the call's rope table once, the fused Q|K|V launch with the NEOX rotation in its
// epilogue, no biases (ENC_ADD), the gate/up pair launch for the FFN.  A sequence of more than
// ENC_MAX_TOK tokens, of any architecture, runs its attention on enc_attn_long_kernel.
//
// jina-bert-v2 (hp.jina) is BERT's chain with three differences: no position add,
// the attention launches take the context's ALiBi slopes, and the FFN's first launch is the GELU-gated
// pair launch of enc_jina.hip (no bias).  A sequence of more than ENC_MAX_LONG tokens, of any
// architecture, runs its attention on enc_attn_xlong_kernel.
#include "engine.h"

#include <algorithm>
#include <cmath>

namespace mi {

EncGemmRope enc_rope_gemm_of(const __half* wqkv, const float* x, int ntok, int K, int n_head, int head_dim, int n_rot,
                             const float2* rope, float* q, __half* k, __half* v) {
    EncGemmRope g{};
    g.w = wqkv;
    g.x = x;
    g.x_stride = K;
    g.K = K;
    g.ntok = ntok;
    g.n_head = n_head;
    g.head_dim = head_dim;
    g.n_rot = n_rot;
    g.rope = rope;
    g.q = q;
    g.k = k;
    g.v = v;
    g.out_stride = n_head * head_dim;
    return g;
}

EncGemmPair enc_swiglu_gemm_of(const __half* gate, const __half* up, int rows, int K, const float* x, int ntok, float* out) {
    return EncGemmPair{gate, up, rows, K, ntok, x, K, out, rows};
}

EncGemmPair enc_geglu_gemm_of(const __half* gate, const __half* up, int rows, int K, const float* x, int ntok, float* out,
                              const unsigned short* gelu_tab) {
    EncGemmPair g = enc_swiglu_gemm_of(gate, up, rows, K, x, ntok, out);
    g.gelu_tab = gelu_tab;
    return g;
}

void Ctx::enc_init() {
    const HParams& hp = m->hp;
    enc = true;
    enc_max = (int)std::min<uint32_t>({n_batch, (uint32_t)ENC_MAX_SEQ, (uint32_t)hp.n_ctx_train});
    if (enc_max < 1) throw Error("encoder context: no room for a token");
    init_enc_attributes();
    // the row buffers hold a multi-sequence call: up to n_batch rows, ENC_MAX_ROWS at the most
    enc_rows = (int)std::min<uint32_t>(n_batch, (uint32_t)ENC_MAX_ROWS);
    const size_t rows = (size_t)enc_rows, ne = (size_t)hp.n_embd;
    // one upload per call: token ids, positions, the sequence list, the tile list (int4 entries)
    enc_tok = mem.dev<int>(kEncInts * (rows + 1));
    h_enc_tok = mem.host<int>((size_t)kEncRing * kEncInts * (rows + 1));
    enc_x = mem.dev<float>(rows * ne);
    enc_a = mem.dev<float>(rows * ne);
    enc_x1 = mem.dev<float>(rows * ne);
    enc_q = mem.dev<float>(rows * ne);
    enc_o = mem.dev<float>(rows * ne);
    enc_h = mem.dev<float>(rows * (size_t)hp.n_ff);
    enc_k = mem.dev<__half>(rows * ne);
    enc_v = mem.dev<__half>(rows * ne);
    enc_pool = mem.dev<float>(rows * ne);
    if (hp.nomic) enc_rope = mem.dev<float2>(rows * (size_t)(hp.n_rot / 2));
    if (hp.jina) {
        std::vector<float> sl((size_t)hp.n_head);
        alibi_slopes(hp.n_head, kJinaMaxAlibiBias, sl.data());
        enc_slopes = mem.dev<float>(sl.size());
        MI_HIP(hipMemcpy(enc_slopes, sl.data(), sl.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    // always in embeddings mode: [n_batch] token rows, the pooled row, the last token's row
    embeddings = true;
    embd = mem.dev<float>(((size_t)n_batch + 2) * ne);
    h_embd = mem.host<float>(ne);
}

int* Ctx::enc_upload_slot() {
    const long long slot = enc_slot++ % kEncRing;
    if (slot == 0 && enc_slot > 1) MI_HIP(hipStreamSynchronize(stream));   // the ring's copies are done
    return h_enc_tok + slot * kEncInts * (enc_rows + 1);
}

// The launch chain over n token rows whose ids are in enc_tok.  seq_len == nullptr: one sequence,
// position = row, enc_attn_kernel.  Otherwise the rows are n_seq sequences end to end, with their
// positions at d_pos and the tile list at d_tiles (device).
void Ctx::enc_pass(int n, const int* d_pos, const int* d_tiles, const int* seq_len, int n_seq) {
    const HParams& hp = m->hp;
    const int ne = hp.n_embd, nff = hp.n_ff;
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
    e.positions = d_pos;
    e.ntok = n;
    e.n_embd = ne;
    e.tok = m->tok_embd.p[0];
    e.typ = m->tok_types.p[0];
    e.pos = hp.nomic || hp.jina ? nullptr : m->pos_embd.p[0];   // nomic-bert: no table, Q and K are rotated instead; jina: ALiBi
    e.tok_f16 = m->tok_embd.type == T_F16;
    e.typ_f16 = m->tok_types.type == T_F16;
    e.pos_f16 = m->pos_embd.type == T_F16;
    e.out = enc_a;
    launch_enc_embed(e, stream);
    norm(enc_a, m->embd_norm, m->embd_norm_b, enc_x);
    // the call's rope table, once: each row at its position inside its sequence
    if (hp.nomic) launch_enc_rope_table(d_pos, n, hp.n_rot, theta_scale(), hp.freq_scale, enc_rope, stream);

    for (int l = 0; l < hp.n_layer; ++l) {
        const EncLayer& L = m->enc_layers[l];
        if (hp.nomic) {
            launch_enc_gemm_rope(enc_rope_gemm_of(L.wqkv, enc_x, n, ne, hp.n_head, hp.head_dim, hp.n_rot, enc_rope, enc_q, enc_k, enc_v),
                                 stream);
        } else {
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
        }
        if (seq_len)
            launch_enc_attn_seq(EncAttnSeq{enc_q, enc_k, enc_v, ne, ne, ne, hp.n_head, hp.head_dim, n, kq_scale(), enc_o,
                                           d_tiles, seq_len, n_seq, enc_slopes},
                                stream);
        else
            launch_enc_attn(EncAttn{enc_q, enc_k, enc_v, ne, ne, ne, hp.n_head, hp.head_dim, n, kq_scale(), enc_o, enc_slopes}, stream);
        // nomic-bert: no biases (ENC_ADD: the residual alone), h = silu(gate x) * (up x) in one launch
        gemm(hp.nomic ? ENC_ADD : ENC_RESID, enc_o, ne, ne, L.wo, L.bo, enc_x, enc_a);
        norm(enc_a, L.attn_out_norm, L.attn_out_norm_b, enc_x1);
        if (hp.nomic) launch_enc_gemm_swiglu(enc_swiglu_gemm_of(L.gate, L.up, nff, ne, enc_x1, n, enc_h), stream);
        else if (hp.jina) launch_enc_gemm_geglu(enc_geglu_gemm_of(L.gate, L.up, nff, ne, enc_x1, n, enc_h, m->gelu_tab), stream);
        else gemm(ENC_GELU, enc_x1, ne, nff, L.up, L.bup, nullptr, enc_h);
        gemm(hp.nomic ? ENC_ADD : ENC_RESID, enc_h, nff, ne, L.down, L.bdown, enc_x1, enc_a);
        // the last layer's rows are the embeddings (no final norm): token t -> row t of embd
        norm(enc_a, L.layer_out_norm, L.layer_out_norm_b, l == hp.n_layer - 1 ? embd : enc_x);
    }
}

int Ctx::decode_enc(const int32_t* tokens, int n, bool all) {
    if (n > enc_max)
        throw Error("decode: an encoder call takes at most " + std::to_string(enc_max) +
                    " tokens (min of n_batch, 8192 and n_ctx_train), got " + std::to_string(n));
    const int ne = m->hp.n_embd;
    const bool pooled = pooling != MI_POOLING_NONE;
    embd_n = n;
    embd_all = all && !pooled;
    embd_rows = 0;
    embd_valid = false;
    enc_nseq = 0;
    out_rows = 0;

    int* ht = enc_upload_slot();
    std::copy(tokens, tokens + n, ht);
    MI_HIP(hipMemcpyAsync(enc_tok, ht, (size_t)n * sizeof(int), hipMemcpyHostToDevice, stream));
    enc_pass(n, nullptr, nullptr, nullptr, 0);
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

int Ctx::encode_seqs(const int32_t* tokens, const int32_t* seq_len, int n_seq) {
    MI_HIP(hipSetDevice(device));
    if (!enc) throw Error("encode_seqs: the model is not an encoder (general.architecture bert)");
    if (n_seq < 1) throw Error("encode_seqs: n_seq must be at least 1, got " + std::to_string(n_seq));
    const HParams& hp = m->hp;
    long long total = 0;
    for (int s = 0; s < n_seq; ++s) {
        if (seq_len[s] < 1 || seq_len[s] > enc_max)
            throw Error("encode_seqs: sequence " + std::to_string(s) + " has " + std::to_string(seq_len[s]) +
                        " tokens; a sequence takes 1 to " + std::to_string(enc_max) + " (min of n_batch, 8192 and n_ctx_train)");
        total += seq_len[s];
        if (total > enc_rows)
            throw Error("encode_seqs: the call holds more than " + std::to_string(enc_rows) +
                        " tokens (min of n_batch and 8192) with sequence " + std::to_string(s));
    }
    const int n = (int)total;
    for (int s = 0, i = 0; s < n_seq; ++s)
        for (int t = 0; t < seq_len[s]; ++t, ++i)
            if (tokens[i] < 0 || tokens[i] >= hp.n_vocab)
                throw Error("encode_seqs: token id out of range in sequence " + std::to_string(s) + " (token " + std::to_string(t) + ")");
    const bool pooled = pooling != MI_POOLING_NONE;
    unsynced = true;
    batch_path = 6;
    embd_n = n;
    embd_all = !pooled;
    embd_rows = 0;
    embd_valid = false;
    enc_nseq = 0;
    out_rows = 0;

    // ids | positions | sequence list | tile list, the lists 16-byte aligned, in one copy
    int* ht = enc_upload_slot();
    const size_t o_pos = ((size_t)n + 3) & ~(size_t)3, o_seq = 2 * o_pos, o_tile = o_seq + 4 * (size_t)n_seq;
    std::copy(tokens, tokens + n, ht);
    for (int s = 0, i = 0; s < n_seq; ++s)
        for (int t = 0; t < seq_len[s]; ++t) ht[o_pos + i++] = t;
    const int n_tiles = enc_seq_lists(seq_len, n_seq, ht + o_seq, ht + o_tile);
    MI_HIP(hipMemcpyAsync(enc_tok, ht, (o_tile + 4 * (size_t)n_tiles) * sizeof(int), hipMemcpyHostToDevice, stream));
    enc_pass(n, enc_tok + o_pos, enc_tok + o_tile, seq_len, n_seq);
    if (pooled) launch_enc_pool_seq(EncPoolSeq{embd, hp.n_embd, hp.n_embd, n_seq, pooling, enc_tok + o_seq, enc_pool}, stream);
    else embd_rows = n;
    enc_nseq = n_seq;
    embd_valid = true;
    return 0;
}

const float* Ctx::embeddings_seq_host(int seq) {
    if (!embeddings) throw Error("embeddings: the context is not in embeddings mode (mi_ctx_set_embeddings)");
    if (!embd_valid) throw Error("no embeddings: decode since the mode was set first");
    if (pooling == MI_POOLING_NONE)
        throw Error("embeddings_seq: the context pools nothing (pooling NONE): read token rows with mi_embeddings");
    if (enc_nseq == 0) {   // after mi_decode: the call is sequence 0
        if (seq != 0) throw Error("embeddings_seq: sequence out of range (the last call held one sequence)");
        return embeddings_host(0);
    }
    if (seq < 0 || seq >= enc_nseq)
        throw Error("embeddings_seq: sequence " + std::to_string(seq) + " out of range (the last call held " + std::to_string(enc_nseq) + ")");
    const int ne = m->hp.n_embd;
    MI_HIP(hipSetDevice(device));
    MI_HIP(hipMemcpyAsync(h_embd, enc_pool + (size_t)seq * ne, (size_t)ne * sizeof(float), hipMemcpyDeviceToHost, stream));
    sync();
    return h_embd;
}

}  // namespace mi
