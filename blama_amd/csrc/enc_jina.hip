// The kernels the jina-bert-v2 graph adds to the encoder pass (gfx950, wave64): llm_build_bert's
// LLM_ARCH_JINA_BERT_V2 branch (llama.cpp b5187) has no position input -- its attention scores carry
// ALiBi --, gates its FFN with GELU and is trained on 8192 tokens.
//
//  * ALiBi.  ggml_soft_max_ext forms the score of (query i, key j) as s * scale, rounded to f32, then
//    adds slope_h * mask with mask = -(float)|i - j| (i, j the positions inside the sequence) and
//    slope_h from alibi_slopes() below, computed on the host in f32 and uploaded, one float per head.
//    Every attention kernel of the encoder has a compile-time ALIBI variant that forms the bias in
//    registers from its own (query, key) indices -- no mask tensor, no LDS change -- chosen by a
//    non-null slope pointer; the variants without it are the code they were.  The two short kernels'
//    variants also keep the residual of p's f16 rounding (enc_seq.hip says why).  This library is built
//    with -ffp-contract=off, so the device does NOT contract the two steps into an fma: the product
//    s * scale, the product slope * mask and the add are three f32 roundings, ggml's own when its
//    compiler does not contract either.
//  * enc_gemm_geglu_kernel: enc_gemm_swiglu_kernel's pair launch (gemm_tiles<2>: a wave accumulates the
//    same 32 rows of ffn_gate and of ffn_up over one activation read) with the epilogue gelu(g) * u,
//    gelu by ggml's f16 table exactly as epilogue ENC_GELU of enc_gemm_f16_kernel reads it.
//  * enc_attn_xlong_kernel<HD, ALIBI>: bidirectional attention of a sequence of 2049 .. 8192 tokens.
//    enc_attn_long_kernel gives a workgroup ONE 32-query tile and deals the key blocks to its 4 waves,
//    so every tile streams all of K three times and V once from global memory / L2: per query the
//    traffic grows with the length and nothing is reused inside the workgroup.  Here a workgroup of 4
//    waves owns FOUR consecutive 32-query tiles (ENC_XL_Q = 128 queries) of one (head, sequence), each
//    wave one tile for the whole kernel, and the workgroup walks the sequence's keys in chunks of 128:
//    a chunk of K is staged into LDS once per pass and is the MFMA A operand of all four waves, so K
//    and V are read a quarter as often per query and every wave's reductions stay in its registers.
//      pass 1  the exact row maximum: per lane over its 16 keys of every block, then the other
//              half-wave (one shuffle).
//      pass 2  the sum of expf(s - max) in double: per lane in ascending chunk, block and register
//              order, then plus the other half-wave (one shuffle).
//      pass 3  K again and V, transposed as enc_attn_long_kernel stages it; per 32-key block the wave
//              writes p = f16(expf(s - max) * (float)(1 / sum)) to its own [32][40] LDS slice, reads it
//              back as the B operand and accumulates PV in its HD / 32 D tiles (f32).  The slice is
//              written and read by one wave only: LDS operations of a wave complete in order, and a
//              wave-level fence keeps the compiler from moving them.
//    There is no cross-wave reduction and no partial-tile sum: the D tiles are stored straight to the
//    output rows.  The scores are v_mfma_f32_32x32x16_f16 of f16 q (rounded once, held in registers for
//    the whole kernel) and f16 k, scaled (and biased) as above: enc_attn_long_kernel's values.
//    LDS, whatever the length: K chunk 256 (HD + 8) + V chunk 272 HD + p slices 10240 bytes: 46080 at
//    HD 64 (three workgroups per CU), 29184 at HD 32.  Every loop bound and LDS offset is a function of
//    (len, group offset, HD) alone, so a sequence's rows have the same bits alone and in any batch;
//    a wave whose tile lies past the sequence's end stages its share and reaches every barrier, and
//    computes nothing.
#include "enc_common.h"
#include "kernels.h"

#include <cmath>

namespace mi {
namespace enc {

__global__ __launch_bounds__(64 * NW) void enc_gemm_geglu_kernel(const EncGemmPair P) {
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
        for (int e = 0; e < 4; ++e) {   // ggml_vec_gelu_f32 (GGML_GELU_FP16 table), then ggml_mul
            const float g = acc[0][4 * q + e];
            const unsigned short hb = __half_as_ushort(__float2half_rn(g));
            const float t = __half2float(__ushort_as_half(P.gelu_tab[hb]));
            y[e] = (g <= -10.0f ? 0.0f : (g >= 10.0f ? g : t)) * acc[1][4 * q + e];
        }
        *reinterpret_cast<float4*>(P.out + (long long)tok * P.out_stride + r0 + 8 * q + 4 * h) = float4{y[0], y[1], y[2], y[3]};
    }
}

// ----------------------------------------------------- attention past ENC_MAX_LONG ---
constexpr int XW = 4;            // waves per workgroup: one 32-query tile each
constexpr int XC = 128;          // keys per staged chunk of K and of V
constexpr int XVS = XC + 8;      // halves per row of the transposed V chunk
constexpr int XPS = 40;          // halves per row of a wave's p slice
static_assert(32 * XW == ENC_XL_Q, "a workgroup's queries");

template <int HD>
struct XlongLds {
    static constexpr int KS = HD + 8;                        // halves per staged K row
    static constexpr int o_k = 0;                            // f16 [XC][KS]
    static constexpr int o_vt = o_k + XC * KS * 2;           // f16 [HD][XVS]
    static constexpr int o_p = o_vt + HD * XVS * 2;          // f16 [XW][32][XPS]
    static constexpr int bytes = o_p + XW * 32 * XPS * 2;
};

template <int HD, bool ALIBI>
__global__ __launch_bounds__(64 * XW) void enc_attn_xlong_kernel(const EncAttnSeq P) {
    using L = XlongLds<HD>;
    constexpr int KS = L::KS, NJ = HD / 16, NH = HD / 32;
    __shared__ __attribute__((aligned(16))) char smem[L::bytes];
    _Float16* ks = reinterpret_cast<_Float16*>(smem + L::o_k);
    _Float16* vt = reinterpret_cast<_Float16*>(smem + L::o_vt);
    // a group of the list, or (no list) of the call's one sequence
    const int4 grp = P.tiles ? reinterpret_cast<const int4*>(P.tiles)[blockIdx.y] : int4{0, P.ntok, ENC_XL_Q * (int)blockIdx.y, 0};
    const int start = grp.x, len = grp.y;
    const int nblk = (len + 31) >> 5, npad = nblk * 32;
    const int head = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int col = lane & 31, h = lane >> 5;
    const int off = grp.z + 32 * w;                            // this wave's tile
    const int live = min(32, len - off);                       // its queries; <= 0: an idle wave
    const bool busy = live > 0;
    const int qi = off + col;                                  // the lane's query (position inside the sequence)
    _Float16* pw = reinterpret_cast<_Float16*>(smem + L::o_p) + w * 32 * XPS;
    const float slope = ALIBI ? P.slopes[head] : 0.0f;

    // the lane's q operand, rounded to f16 once: 8 head dimensions per MFMA, straight from global memory
    u32x4 bq[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        float4 a = float4{0.0f, 0.0f, 0.0f, 0.0f}, b = a;      // queries past the end: zero columns, never stored
        if (col < live) {
            const float* src = P.q + (long long)(start + qi) * P.q_stride + head * HD + 16 * j + 8 * h;
            a = *reinterpret_cast<const float4*>(src);
            b = *reinterpret_cast<const float4*>(src + 4);
        }
        bq[j] = u32x4{pack2(a.x, a.y), pack2(a.z, a.w), pack2(b.x, b.y), pack2(b.z, b.w)};
    }

    const __half* kbase = P.k + (long long)start * P.kv_stride + head * HD;
    const __half* vbase = P.v + (long long)start * P.kv_stride + head * HD;
    // keys c0 .. c0 + XC - 1 of K into ks, row = key; keys past the end are zero rows, blocks past npad are never read
    auto stage_k = [&](int c0) {
        for (int i = tid; i < XC * (HD / 8); i += 64 * XW) {
            const int r = i / (HD / 8), ch = i - r * (HD / 8);
            const int key = c0 + r;
            if (key >= npad) continue;
            u32x4 v = u32x4{0u, 0u, 0u, 0u};
            if (key < len) v = *reinterpret_cast<const u32x4*>(kbase + (long long)key * P.kv_stride + 8 * ch);
            *reinterpret_cast<u32x4*>(ks + r * KS + 8 * ch) = v;
        }
    };
    // the scores of block b of the staged chunk: lane = query, register r = key c0 + 32 b + (r & 3) + 8 (r >> 2) + 4 h
    auto scores = [&](int c0, int b) {
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const u32x4 a = *reinterpret_cast<const u32x4*>(ks + (32 * b + col) * KS + 16 * j + 8 * h);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(as_h8(a), as_h8(bq[j]), acc, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = acc[r] * P.scale;
        if (ALIBI) {
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = acc[r] + slope * alibi_dist(qi, c0 + 32 * b + (r & 3) + 8 * (r >> 2) + 4 * h);
        }
        return acc;
    };
    auto key_of = [&](int c0, int b, int r) { return c0 + 32 * b + (r & 3) + 8 * (r >> 2) + 4 * h; };

    // ---- pass 1: the row maximum ----
    float mx = -INFINITY;
    for (int c0 = 0; c0 < npad; c0 += XC) {
        if (c0) __syncthreads();   // the previous chunk is read
        stage_k(c0);
        __syncthreads();
        if (!busy) continue;
        for (int b = 0; b < XC / 32 && c0 + 32 * b < npad; ++b) {
            const f32x16 s = scores(c0, b);
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if (key_of(c0, b, r) < len) mx = fmaxf(mx, s[r]);
        }
    }
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));

    // ---- pass 2: the sum of expf(s - max), in double ----
    double sum = 0.0;
    for (int c0 = 0; c0 < npad; c0 += XC) {
        __syncthreads();           // the previous chunk (pass 1's last) is read
        stage_k(c0);
        __syncthreads();
        if (!busy) continue;
        for (int b = 0; b < XC / 32 && c0 + 32 * b < npad; ++b) {
            const f32x16 s = scores(c0, b);
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if (key_of(c0, b, r) < len) sum += (double)expf(s[r] - mx);
        }
    }
    sum += __shfl_xor(sum, 32, 64);
    const float inv = (float)(1.0 / sum);

    // ---- pass 3: p of each block through the wave's slice, then PV; D lane = query, registers = head dimensions ----
    f32x16 o[NH];
#pragma unroll
    for (int a = 0; a < NH; ++a)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[a][r] = 0.0f;
    for (int c0 = 0; c0 < npad; c0 += XC) {
        __syncthreads();           // the previous chunk of K and of V is read
        stage_k(c0);
        for (int i = tid; i < (XC / 2) * (HD / 8); i += 64 * XW) {
            const int kp = i & (XC / 2 - 1), ch = i / (XC / 2);
            const int key = c0 + 2 * kp;
            if (key >= npad) continue;   // blocks past npad are never read
            u32x4 a = u32x4{0u, 0u, 0u, 0u}, b = a;   // keys past the end: zero columns
            if (key < len) a = *reinterpret_cast<const u32x4*>(vbase + (long long)key * P.kv_stride + 8 * ch);
            if (key + 1 < len) b = *reinterpret_cast<const u32x4*>(vbase + (long long)(key + 1) * P.kv_stride + 8 * ch);
            unsigned* dst = reinterpret_cast<unsigned*>(vt + (8 * ch) * XVS + 2 * kp);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                dst[(2 * e) * (XVS / 2)] = (a[e] & 0xffffu) | (b[e] << 16);
                dst[(2 * e + 1) * (XVS / 2)] = (a[e] >> 16) | (b[e] & 0xffff0000u);
            }
        }
        __syncthreads();
        if (!busy) continue;
        for (int b = 0; b < XC / 32 && c0 + 32 * b < npad; ++b) {
            const f32x16 s = scores(c0, b);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   // the slice's previous block is read
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                float p[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) p[e] = key_of(c0, b, 4 * q + e) < len ? expf(s[4 * q + e] - mx) * inv : 0.0f;
                *reinterpret_cast<u32x2*>(pw + col * XPS + 8 * q + 4 * h) = u32x2{pack2(p[0], p[1]), pack2(p[2], p[3])};
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   // the block is written: the other lanes read it
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const u32x4 pb = *reinterpret_cast<const u32x4*>(pw + col * XPS + 16 * j + 8 * h);
#pragma unroll
                for (int a = 0; a < NH; ++a) {
                    const u32x4 va = *reinterpret_cast<const u32x4*>(vt + (32 * a + col) * XVS + 32 * b + 16 * j + 8 * h);
                    o[a] = __builtin_amdgcn_mfma_f32_32x32x16_f16(as_h8(va), as_h8(pb), o[a], 0, 0, 0);
                }
            }
        }
    }
    // D: lane = query off + col, register r of tile a = head dimension 32 a + (r & 3) + 8 (r >> 2) + 4 h
    if (col >= live) return;
    float* orow = P.out + (long long)(start + qi) * P.out_stride + head * HD + 4 * h;
#pragma unroll
    for (int a = 0; a < NH; ++a)
#pragma unroll
        for (int q = 0; q < 4; ++q)
            *reinterpret_cast<float4*>(orow + 32 * a + 8 * q) = float4{o[a][4 * q], o[a][4 * q + 1], o[a][4 * q + 2], o[a][4 * q + 3]};
}

}  // namespace enc

void alibi_slopes(int n_head, float max_bias, float* out) {
    int n2 = 1;
    while (2 * n2 <= n_head) n2 *= 2;   // 2^floor(log2(n_head))
    const float m0 = powf(2.0f, -max_bias / (float)n2), m1 = powf(2.0f, -(max_bias / 2.0f) / (float)n2);
    for (int h = 0; h < n_head; ++h) out[h] = h < n2 ? powf(m0, (float)(h + 1)) : powf(m1, (float)(2 * (h - n2) + 1));
}

void launch_enc_gemm_geglu(const EncGemmPair& p, hipStream_t s) {
    if (p.ntok < 1 || p.ntok > ENC_MAX_ROWS) throw Error("enc geglu gemm: 1 to 8192 token rows");
    if (p.K < 32 || p.K % 32 || p.x_stride % 4 || p.out_stride % 4 || !p.x) throw Error("enc geglu gemm: K must be a multiple of 32");
    if (p.rows < 32 || p.rows % 32 || p.rows > p.out_stride || !p.gate || !p.up || !p.out)
        throw Error("enc geglu gemm: rows must be a multiple of 32");
    if (!p.gelu_tab) throw Error("enc geglu gemm: the GELU epilogue needs the table");
    const dim3 grid((p.rows / 32 + enc::NW - 1) / enc::NW, (p.ntok + 31) / 32), block(64 * enc::NW);
    hipLaunchKernelGGL(enc::enc_gemm_geglu_kernel, grid, block, 0, s, p);
    MI_HIP(hipGetLastError());
}

void launch_enc_attn_xlong(const EncAttnSeq& p, int n_groups, hipStream_t s) {
    if (!enc_attn_supported(p.head_dim)) throw Error("enc attention: head_dim 32 or 64");
    if (p.n_head < 1 || n_groups < 1 || !p.q || !p.k || !p.v || !p.out) throw Error("enc attention: unsupported shape");
    if (p.kv_stride % 8 || p.q_stride % 4 || p.out_stride % 4) throw Error("enc attention: kv_stride % 8, q_stride % 4, out_stride % 4");
    if (p.n_head * p.head_dim > p.q_stride || p.n_head * p.head_dim > p.kv_stride || p.n_head * p.head_dim > p.out_stride)
        throw Error("enc attention: the heads do not fit the row strides");
    if (!p.tiles && (p.ntok < 1 || p.ntok > ENC_MAX_SEQ || n_groups != (p.ntok + ENC_XL_Q - 1) / ENC_XL_Q))
        throw Error("enc attention: 1 to 8192 tokens");
    const dim3 grid(p.n_head, n_groups), block(64 * enc::XW);
    if (p.slopes) {
        if (p.head_dim == 32) hipLaunchKernelGGL((enc::enc_attn_xlong_kernel<32, true>), grid, block, 0, s, p);
        else hipLaunchKernelGGL((enc::enc_attn_xlong_kernel<64, true>), grid, block, 0, s, p);
    } else {
        if (p.head_dim == 32) hipLaunchKernelGGL((enc::enc_attn_xlong_kernel<32, false>), grid, block, 0, s, p);
        else hipLaunchKernelGGL((enc::enc_attn_xlong_kernel<64, false>), grid, block, 0, s, p);
    }
    MI_HIP(hipGetLastError());
}

}  // namespace mi
