// The kernels the nomic-bert graph adds to the encoder pass (gfx950, wave64): llm_build_bert's nomic
// branch (llama.cpp b5187) rotates Q and K NEOX-style, gates its FFN and is trained on 2048 tokens.
//
//  * enc_rope_table_kernel: ggml_rope_cache_init (ext_factor 0, mscale 1, no frequency factors) per
//    token row: theta = pos * theta_scale^i iterated in f32, (cosf, sinf) of freq_scale * theta.
//  * gemm_tiles<NA>: the K loop of enc_gemm_f16_kernel (enc.hip; the operand and D layouts are stated
//    there) for NA 32-row tiles per wave over ONE read of the activation tile: the two LDS reads of
//    a 32-column step feed 2 NA MFMAs.  Each accumulator adds its products in enc_gemm_f16_kernel's
//    order, so a row has the bits that kernel gives it.
//  * enc_gemm_rope_kernel<HD>: the fused attn_qkv matrix ([3 n_embd][K]: Q rows, K rows, V rows)
//    with ggml_rope_ext (mode NEOX) in the epilogue.  A wave owns one HEAD of Q, K or V -- HD rows,
//    HD / 32 accumulator sets -- so both partners of a pair (i, i + n_rot / 2) of a token are in the
//    token's lane: D register r of set a is row 32 a + 8 (r >> 2) + 4 h + (r & 3) of the head, i.e.
//    flat register f = 16 a + r holds row 8 (f >> 2) + 4 h + (f & 3), and with n_rot a multiple of 16
//    the partner of flat register f is flat register f + n_rot / 4 of the same lane.  No LDS exchange,
//    no second launch.  (cos, sin) of 4 consecutive pairs are two 16-byte loads of the table row.
//    Q is stored as f32, K (rotated) and V as f16; a head's rows at or past n_rot are copied.
//  * enc_gemm_swiglu_kernel: a wave accumulates the same 32 rows of ffn_gate and of ffn_up and stores
//    silu(g) * u as f32 (silu as the LLaMA paths form it: x / (1 + expf(-x))).
//  * enc_attn_long_kernel<HD>: bidirectional attention of a sequence of 513 .. 2048 tokens, one
//    workgroup of 4 waves per (head, 32-query tile of ONE sequence), both products on
//    v_mfma_f32_32x32x16_f16.  No [32][len] score matrix: QK^T is recomputed in each of three passes
//    over the sequence's 32-key blocks, block kb always by wave kb & 3.
//      pass 1  the exact row maximum: per lane over its 16 keys of each block, then the other
//              half-wave (one shuffle), then the 4 waves through LDS.  max is order-free.
//      pass 2  sum of expf(s - max) in double: per lane in ascending block and register order, plus
//              the other half-wave, then ((w0 + w1) + w2) + w3 through LDS.
//      pass 3  p = f16(expf(s - max) * (float)(1 / sum)) of the wave's block goes to the wave's own
//              [32 queries][32 keys] LDS block and is the B operand of PV; A = V transposed, staged
//              as enc_attn_seq_kernel stages it, 128 keys (one block per wave) per chunk.  Each wave
//              accumulates its blocks' PV in registers (HD / 32 D tiles); at the end the 4 partial
//              tiles are added in wave order ((p0 + p1) + p2) + p3.
//    So the scores, the maximum and every p are enc_attn_seq_kernel's values; only the order of the
//    f32 additions of PV (and of the double additions of the sum) differs.
//    LDS, whatever the length: 1024 (sums) + 512 (maxima) + 64 (HD + 8) (q) + the larger of
//    {V chunk 272 HD + p blocks 10240} and {partial tiles 512 (HD + 4)}: 40960 bytes at HD 64, 23040
//    at HD 32.  Every loop bound and LDS offset is a function of (len, tile offset, HD) alone: a
//    sequence's rows have the same bits alone and in any batch.
#include "enc_common.h"
#include "kernels.h"

namespace mi {
namespace enc {

__global__ void enc_rope_table_kernel(const int* pos, int ntok, int n_rot, float theta_scale, float freq_scale, float2* out) {
    const int t = blockIdx.x;
    const int p = pos ? pos[t] : t;
    for (int i = threadIdx.x; i < n_rot / 2; i += blockDim.x) {
        float theta = (float)p;
        for (int k = 0; k < i; ++k) theta = theta * theta_scale;
        const float th = freq_scale * theta;
        out[(long long)t * (n_rot / 2) + i] = make_float2(cosf(th), sinf(th));
    }
}

// ----------------------------------------------------------------------- GEMMs ---
// (gemm_tiles<NA>, NW, NKC, NXS: enc_common.h, shared with enc_jina.hip)
template <int HD>
__global__ __launch_bounds__(64 * NW) void enc_gemm_rope_kernel(const EncGemmRope P) {
    constexpr int NA = HD / 32;    // accumulator sets: the head's 32-row tiles
    constexpr int NF = 16 * NA;    // flat registers: row 8 (f >> 2) + 4 h + (f & 3) of the head
    __shared__ __attribute__((aligned(16))) _Float16 xs[32 * NXS];
    const int lane = threadIdx.x & 63, col = lane & 31, h = lane >> 5;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int t0 = blockIdx.y * 32;
    const int u = blockIdx.x * NW + w;           // the head: Q heads, then K heads, then V heads
    const bool act = u < 3 * P.n_head;
    const __half* wrow[NA];
#pragma unroll
    for (int a = 0; a < NA; ++a) wrow[a] = act ? P.w + (long long)(u * HD + 32 * a + col) * P.K + 16 * h : nullptr;
    f32x16 acc[NA];
    gemm_tiles<NA>(wrow, act, P.x, P.x_stride, P.K, P.ntok, t0, xs, acc);
    const int tok = t0 + col;
    if (!act || tok >= P.ntok) return;
    float y[NF];
#pragma unroll
    for (int f = 0; f < NF; ++f) y[f] = acc[f >> 4][f & 15];
    const int seg = u / P.n_head, head = u - seg * P.n_head;
    if (seg < 2) {   // ggml_rope_ext, NEOX: pair ic = (row ic, row ic + n_rot / 2), ic = 8 (f >> 2) + 4 h + (f & 3)
        const int nq = P.n_rot >> 4;   // quads of flat registers below n_rot / 2
        const float2* cs = P.rope + (long long)tok * (P.n_rot >> 1) + 4 * h;
#pragma unroll
        for (int NQ = 1; NQ <= HD / 16; ++NQ) {
            if (nq != NQ) continue;
#pragma unroll
            for (int qi = 0; qi < NQ; ++qi) {
                const float4 c01 = *reinterpret_cast<const float4*>(cs + 8 * qi);       // cos, sin of pairs ic, ic + 1
                const float4 c23 = *reinterpret_cast<const float4*>(cs + 8 * qi + 2);   // of pairs ic + 2, ic + 3
                const float c[4] = {c01.x, c01.z, c23.x, c23.z}, sn[4] = {c01.y, c01.w, c23.y, c23.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float x0 = y[4 * qi + e], x1 = y[4 * (qi + NQ) + e];
                    y[4 * qi + e] = x0 * c[e] - x1 * sn[e];
                    y[4 * (qi + NQ) + e] = x0 * sn[e] + x1 * c[e];
                }
            }
        }
    }
    const long long o = (long long)tok * P.out_stride + head * HD + 4 * h;
#pragma unroll
    for (int qi = 0; qi < NF / 4; ++qi) {
        const float* v = y + 4 * qi;
        if (seg == 0)
            *reinterpret_cast<float4*>(P.q + o + 8 * qi) = float4{v[0], v[1], v[2], v[3]};
        else
            *reinterpret_cast<u32x2*>((seg == 1 ? P.k : P.v) + o + 8 * qi) = u32x2{pack2(v[0], v[1]), pack2(v[2], v[3])};
    }
}

__device__ __forceinline__ float silu_f(float x) { return x / (1.0f + expf(-x)); }   // qdot.h's, mmq_common.h's

__global__ __launch_bounds__(64 * NW) void enc_gemm_swiglu_kernel(const EncGemmPair P) {
    __shared__ __attribute__((aligned(16))) _Float16 xs[32 * NXS];
    const int lane = threadIdx.x & 63, col = lane & 31, h = lane >> 5;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int t0 = blockIdx.y * 32;
    const int r0 = (blockIdx.x * NW + w) * 32;
    const bool act = r0 < P.rows;
    const long long wo = (long long)(r0 + col) * P.K + 16 * h;
    const __half* wrow[2] = {act ? P.gate + wo : nullptr, act ? P.up + wo : nullptr};
    f32x16 acc[2];
    gemm_tiles<2>(wrow, act, P.x, P.x_stride, P.K, P.ntok, t0, xs, acc);
    const int tok = t0 + col;
    if (!act || tok >= P.ntok) return;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        float y[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) y[e] = silu_f(acc[0][4 * q + e]) * acc[1][4 * q + e];
        *reinterpret_cast<float4*>(P.out + (long long)tok * P.out_stride + r0 + 8 * q + 4 * h) = float4{y[0], y[1], y[2], y[3]};
    }
}

// ------------------------------------------------------------ long attention ---
constexpr int LW = 4;          // waves per workgroup
constexpr int LVC = 32 * LW;   // keys per staged V chunk: one 32-key block per wave
constexpr int LVS = LVC + 8;   // halves per row of the transposed chunk
constexpr int LPS = 40;        // halves per row of a wave's p block

template <int HD>
struct LongLds {
    static constexpr int QS = HD + 8;                                  // halves per staged q row
    static constexpr int RS = HD + 4;                                  // floats per row of a partial output tile
    static constexpr int o_sum = 0;                                    // double [LW][32]
    static constexpr int o_max = o_sum + LW * 32 * 8;                  // float [LW][32]
    static constexpr int o_q = o_max + LW * 32 * 4;                    // f16 [32][QS]
    static constexpr int o_vt = o_q + 32 * QS * 2;                     // f16 [HD][LVS], or after the passes
    static constexpr int o_red = o_vt;                                 //   float [LW][32][RS]
    static constexpr int o_p = o_vt + HD * LVS * 2;                    // f16 [LW][32][LPS]
    static constexpr int pv_end = o_p + LW * 32 * LPS * 2, red_end = o_red + LW * 32 * RS * 4;
    static constexpr int bytes = pv_end > red_end ? pv_end : red_end;
};

// ALIBI (jina-bert-v2; enc_jina.hip states the arithmetic): every recomputed score takes slopes[head] *
// -(float)|query - key| after the scale, from the D layout's indices.
template <int HD, bool ALIBI>
__global__ __launch_bounds__(64 * LW) void enc_attn_long_kernel(const EncAttnSeq P) {
    using L = LongLds<HD>;
    constexpr int QS = L::QS, RS = L::RS, NJ = HD / 16, NH = HD / 32;
    __shared__ __attribute__((aligned(16))) char smem[L::bytes];
    double* smw = reinterpret_cast<double*>(smem + L::o_sum);
    float* mxw = reinterpret_cast<float*>(smem + L::o_max);
    _Float16* qs = reinterpret_cast<_Float16*>(smem + L::o_q);
    _Float16* vt = reinterpret_cast<_Float16*>(smem + L::o_vt);
    float* red = reinterpret_cast<float*>(smem + L::o_red);
    // a tile of the list, or (no list) of the call's one sequence
    const int4 tile = P.tiles ? reinterpret_cast<const int4*>(P.tiles)[blockIdx.y] : int4{0, P.ntok, 32 * (int)blockIdx.y, 0};
    const int start = tile.x, len = tile.y, off = tile.z;
    const int live = min(32, len - off);
    const int nblk = (len + 31) >> 5, npad = nblk * 32;
    const int head = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int col = lane & 31, h = lane >> 5;
    _Float16* pw = reinterpret_cast<_Float16*>(smem + L::o_p) + w * 32 * LPS;

    for (int i = tid; i < 32 * (HD / 4); i += 64 * LW) {
        const int t = i / (HD / 4), c = i - t * (HD / 4);
        float4 v = float4{0.0f, 0.0f, 0.0f, 0.0f};               // queries past the end: zero rows, never stored
        if (t < live) v = *reinterpret_cast<const float4*>(P.q + (long long)(start + off + t) * P.q_stride + head * HD + 4 * c);
        *reinterpret_cast<u32x2*>(qs + t * QS + 4 * c) = u32x2{pack2(v.x, v.y), pack2(v.z, v.w)};
    }
    __syncthreads();
    u32x4 bq[NJ];   // this lane's q operand: the same in every block of every pass
#pragma unroll
    for (int j = 0; j < NJ; ++j) bq[j] = *reinterpret_cast<const u32x4*>(qs + col * QS + 16 * j + 8 * h);

    // the scaled scores of key block kb: lane = query, register r = key 32 kb + (r & 3) + 8 (r >> 2) + 4 h
    const __half* kbase = P.k + (long long)start * P.kv_stride + head * HD + 8 * h;
    auto scores = [&](int kb) {
        const int key = kb * 32 + col;
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            u32x4 a = u32x4{0u, 0u, 0u, 0u};                     // keys past the end: zero registers, never loaded
            if (key < len) a = *reinterpret_cast<const u32x4*>(kbase + (long long)key * P.kv_stride + 16 * j);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(as_h8(a), as_h8(bq[j]), acc, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = acc[r] * P.scale;
        if (ALIBI) {
            const float m = P.slopes[head];
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = acc[r] + m * alibi_dist(off + col, kb * 32 + (r & 3) + 8 * (r >> 2) + 4 * h);
        }
        return acc;
    };
    auto key_of = [&](int kb, int r) { return kb * 32 + (r & 3) + 8 * (r >> 2) + 4 * h; };

    // ---- pass 1: the row maximum ----
    float mx = -INFINITY;
    for (int kb = w; kb < nblk; kb += LW) {
        const f32x16 s = scores(kb);
#pragma unroll
        for (int r = 0; r < 16; ++r)
            if (key_of(kb, r) < len) mx = fmaxf(mx, s[r]);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    if (h == 0) mxw[w * 32 + col] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(mxw[col], mxw[32 + col]), fmaxf(mxw[64 + col], mxw[96 + col]));

    // ---- pass 2: the sum of expf(s - max), in double ----
    double sum = 0.0;
    for (int kb = w; kb < nblk; kb += LW) {
        const f32x16 s = scores(kb);
#pragma unroll
        for (int r = 0; r < 16; ++r)
            if (key_of(kb, r) < len) sum += (double)expf(s[r] - mx);
    }
    sum += __shfl_xor(sum, 32, 64);
    if (h == 0) smw[w * 32 + col] = sum;
    __syncthreads();
    sum = ((smw[col] + smw[32 + col]) + smw[64 + col]) + smw[96 + col];
    const float inv = (float)(1.0 / sum);

    // ---- pass 3: p of the wave's block, then PV; D lane = query, registers = head dimensions ----
    f32x16 o[NH];
#pragma unroll
    for (int a = 0; a < NH; ++a)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[a][r] = 0.0f;
    const __half* vbase = P.v + (long long)start * P.kv_stride + head * HD;
    for (int c0 = 0; c0 < npad; c0 += LVC) {
        if (c0) __syncthreads();   // the previous chunk and the previous p blocks are read
        for (int i = tid; i < (LVC / 2) * (HD / 8); i += 64 * LW) {
            const int kp = i & (LVC / 2 - 1), ch = i / (LVC / 2);
            const int key = c0 + 2 * kp;
            if (key >= npad) continue;   // blocks past npad are never read
            u32x4 a = u32x4{0u, 0u, 0u, 0u}, b = a;   // keys past the end: zero columns
            if (key < len) a = *reinterpret_cast<const u32x4*>(vbase + (long long)key * P.kv_stride + 8 * ch);
            if (key + 1 < len) b = *reinterpret_cast<const u32x4*>(vbase + (long long)(key + 1) * P.kv_stride + 8 * ch);
            unsigned* dst = reinterpret_cast<unsigned*>(vt + (8 * ch) * LVS + 2 * kp);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                dst[(2 * e) * (LVS / 2)] = (a[e] & 0xffffu) | (b[e] << 16);
                dst[(2 * e + 1) * (LVS / 2)] = (a[e] >> 16) | (b[e] & 0xffff0000u);
            }
        }
        const int kb = (c0 >> 5) + w;
        if (kb < nblk) {
            const f32x16 s = scores(kb);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                float p[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) p[e] = key_of(kb, 4 * q + e) < len ? expf(s[4 * q + e] - mx) * inv : 0.0f;
                *reinterpret_cast<u32x2*>(pw + col * LPS + 8 * q + 4 * h) = u32x2{pack2(p[0], p[1]), pack2(p[2], p[3])};
            }
        }
        __syncthreads();
        if (kb < nblk) {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const u32x4 b = *reinterpret_cast<const u32x4*>(pw + col * LPS + 16 * j + 8 * h);
#pragma unroll
                for (int a = 0; a < NH; ++a) {
                    const u32x4 va = *reinterpret_cast<const u32x4*>(vt + (32 * a + col) * LVS + 32 * w + 16 * j + 8 * h);
                    o[a] = __builtin_amdgcn_mfma_f32_32x32x16_f16(as_h8(va), as_h8(b), o[a], 0, 0, 0);
                }
            }
        }
    }
    __syncthreads();   // the last chunk is read: the partial tiles go over it
#pragma unroll
    for (int a = 0; a < NH; ++a)
#pragma unroll
        for (int q = 0; q < 4; ++q)
            *reinterpret_cast<float4*>(red + (w * 32 + col) * RS + 32 * a + 8 * q + 4 * h) =
                float4{o[a][4 * q], o[a][4 * q + 1], o[a][4 * q + 2], o[a][4 * q + 3]};
    __syncthreads();
    for (int i = tid; i < 32 * (HD / 4); i += 64 * LW) {
        const int t = i / (HD / 4), d = 4 * (i - t * (HD / 4));
        if (t >= live) continue;
        const float* src = red + t * RS + d;
        float4 r = *reinterpret_cast<const float4*>(src);
#pragma unroll
        for (int k = 1; k < LW; ++k) {
            const float4 p = *reinterpret_cast<const float4*>(src + k * 32 * RS);
            r.x = r.x + p.x;
            r.y = r.y + p.y;
            r.z = r.z + p.z;
            r.w = r.w + p.w;
        }
        *reinterpret_cast<float4*>(P.out + (long long)(start + off + t) * P.out_stride + head * HD + d) = r;
    }
}

}  // namespace enc

void launch_enc_rope_table(const int* pos, int ntok, int n_rot, float theta_scale, float freq_scale, float2* out, hipStream_t s) {
    if (ntok < 1 || n_rot < 2 || n_rot % 2 || !out) throw Error("enc rope table: unsupported shape");
    hipLaunchKernelGGL(enc::enc_rope_table_kernel, dim3(ntok), dim3(64), 0, s, pos, ntok, n_rot, theta_scale, freq_scale, out);
    MI_HIP(hipGetLastError());
}

bool enc_rope_supported(int head_dim, int n_rot) { return enc_attn_supported(head_dim) && n_rot >= 16 && n_rot % 16 == 0 && n_rot <= head_dim; }

void launch_enc_gemm_rope(const EncGemmRope& p, hipStream_t s) {
    if (p.ntok < 1 || p.ntok > ENC_MAX_ROWS) throw Error("enc rope gemm: 1 to 8192 token rows");
    if (p.K < 32 || p.K % 32 || p.x_stride % 4 || p.out_stride % 8 || !p.x || !p.w) throw Error("enc rope gemm: K must be a multiple of 32");
    if (p.n_head < 1 || !enc_rope_supported(p.head_dim, p.n_rot))
        throw Error("enc rope gemm: head_dim 32 or 64, n_rot a multiple of 16 and at most head_dim");
    if (p.n_head * p.head_dim > p.out_stride || !p.q || !p.k || !p.v || !p.rope) throw Error("enc rope gemm: unsupported shape");
    const dim3 grid((3 * p.n_head + enc::NW - 1) / enc::NW, (p.ntok + 31) / 32), block(64 * enc::NW);
    if (p.head_dim == 32) hipLaunchKernelGGL(enc::enc_gemm_rope_kernel<32>, grid, block, 0, s, p);
    else hipLaunchKernelGGL(enc::enc_gemm_rope_kernel<64>, grid, block, 0, s, p);
    MI_HIP(hipGetLastError());
}

void launch_enc_gemm_swiglu(const EncGemmPair& p, hipStream_t s) {
    if (p.ntok < 1 || p.ntok > ENC_MAX_ROWS) throw Error("enc swiglu gemm: 1 to 8192 token rows");
    if (p.K < 32 || p.K % 32 || p.x_stride % 4 || p.out_stride % 4 || !p.x) throw Error("enc swiglu gemm: K must be a multiple of 32");
    if (p.rows < 32 || p.rows % 32 || p.rows > p.out_stride || !p.gate || !p.up || !p.out)
        throw Error("enc swiglu gemm: rows must be a multiple of 32");
    const dim3 grid((p.rows / 32 + enc::NW - 1) / enc::NW, (p.ntok + 31) / 32), block(64 * enc::NW);
    hipLaunchKernelGGL(enc::enc_gemm_swiglu_kernel, grid, block, 0, s, p);
    MI_HIP(hipGetLastError());
}

void launch_enc_attn_long(const EncAttnSeq& p, int n_tiles, hipStream_t s) {
    if (!enc_attn_supported(p.head_dim)) throw Error("enc attention: head_dim 32 or 64");
    if (p.n_head < 1 || n_tiles < 1 || !p.q || !p.k || !p.v || !p.out) throw Error("enc attention: unsupported shape");
    if (p.kv_stride % 8 || p.q_stride % 4 || p.out_stride % 4) throw Error("enc attention: kv_stride % 8, q_stride % 4, out_stride % 4");
    if (!p.tiles && (p.ntok < 1 || p.ntok > ENC_MAX_LONG || n_tiles != (p.ntok + 31) / 32)) throw Error("enc attention: 1 to 2048 tokens");
    const dim3 grid(p.n_head, n_tiles), block(64 * enc::LW);
    if (p.slopes) {
        if (p.head_dim == 32) hipLaunchKernelGGL((enc::enc_attn_long_kernel<32, true>), grid, block, 0, s, p);
        else hipLaunchKernelGGL((enc::enc_attn_long_kernel<64, true>), grid, block, 0, s, p);
    } else {
        if (p.head_dim == 32) hipLaunchKernelGGL((enc::enc_attn_long_kernel<32, false>), grid, block, 0, s, p);
        else hipLaunchKernelGGL((enc::enc_attn_long_kernel<64, false>), grid, block, 0, s, p);
    }
    MI_HIP(hipGetLastError());
}

}  // namespace mi
