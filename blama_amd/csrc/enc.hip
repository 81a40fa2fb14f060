// Encoder models on the device (gfx950, wave64): the launches of llm_build_bert (llama.cpp b5187,
// flash_attn off) for the n <= ENC_MAX_TOK tokens of one call -- the first workload of this engine
// with no quantised matrix in it.
//
//  * enc_embed_kernel: x[t] = pos_embd[t] + (tok_embd[token t] + token_types[0]): two f32 adds in
//    that order, F16 table rows widened first (ggml_get_rows, ggml_add, ggml_add).
//  * enc_gemm_f16_kernel<EPI>: y[t][r] = sum_k f16(x[t][k]) * W[r][k] on v_mfma_f32_32x32x16_f16
//    for one to three F16 matrices over one activation.  ggml_mul_mat of an F16 matrix rounds its
//    f32 operand to f16 (the f16 vec_dot_type) and accumulates the exact products in f32; only the
//    f32 order differs here.  The weight rows are the A operand (M), straight from global memory:
//    lane (row r, half h) reads the 32 contiguous bytes W[r][32j + 16h .. + 15] and feeds them to
//    two MFMAs (the k index of an MFMA is free as long as both operands agree on it).  The tokens
//    are the B operand (N): the workgroup's 32-token activation tile is rounded to f16 once on its
//    way into LDS, KC columns at a time, and read back 16 B per lane.  D then has the token on the
//    lane and 4 x 4 consecutive weight rows in its registers: the bias, the GELU table, the
//    residual and the store are 16-byte accesses.  A workgroup is 4 waves = 128 weight rows x 32
//    tokens; tokens past ntok are zero columns that are never stored, row tiles past the last
//    matrix are idle waves, the last K chunk is as short as K leaves it (K % 32 == 0): no padding
//    of the caller's buffers.  One accumulator per output, one fixed order: the same input gives
//    the same bits.
//  * enc_attn_kernel<HD>: attention of every token over all n tokens (no mask, no cache), one
//    workgroup per (head, 32-query tile), plain per-wave FMAs: at n <= 512 and head_dim 32 / 64 a
//    call is bound by its launches, not by the 2 x 32 x n x HD FLOPs of a workgroup.  The
//    arithmetic is attn_mfma.hip's: q rounded to f16, KQ summed in f32, scaled; the two-pass exact
//    softmax (max, expf, the sum in double, p = e * (float)(1 / sum)); p rounded to f16; PV in f32.
//    K and V of the head stream through LDS in 64-key chunks; the tile's scores stay in LDS
//    ([32][n] f32) between the passes.
#include "kernels.h"
#include <hip/hip_runtime.h>

namespace mi {
namespace enc {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ unsigned pack2(float a, float b) {
    const unsigned lo = __half_as_ushort(__float2half_rn(a)), hi = __half_as_ushort(__float2half_rn(b));
    return lo | (hi << 16);
}
__device__ __forceinline__ half8 as_h8(u32x4 v) { return __builtin_bit_cast(half8, v); }
// elements i .. i + 7 of an F16 or F32 table row as f32 (i % 8 == 0: one or two 16-byte loads)
__device__ __forceinline__ void widen8(const void* tab, int f16, long long i, float (&v)[8]) {
    if (f16) {
        const half8 h = *reinterpret_cast<const half8*>(static_cast<const _Float16*>(tab) + i);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = (float)h[e];
    } else {
        const float4 a = *reinterpret_cast<const float4*>(static_cast<const float*>(tab) + i);
        const float4 b = *reinterpret_cast<const float4*>(static_cast<const float*>(tab) + i + 4);
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
        v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    }
}

// ------------------------------------------------------------------ embedding ---
__global__ __launch_bounds__(256) void enc_embed_kernel(const EncEmbed P) {
    const int t = blockIdx.x;
    const long long tok = P.tokens[t];
    float* out = P.out + (long long)t * P.n_embd;
    for (int d = 8 * threadIdx.x; d < P.n_embd; d += 8 * 256) {   // 8 columns per thread: 16-byte accesses
        float a[8], b[8], c[8];
        widen8(P.tok, P.tok_f16, tok * P.n_embd + d, a);
        widen8(P.typ, P.typ_f16, d, b);
        widen8(P.pos, P.pos_f16, (long long)t * P.n_embd + d, c);
#pragma unroll
        for (int e = 0; e < 8; ++e) a[e] = c[e] + (a[e] + b[e]);
        *reinterpret_cast<float4*>(out + d) = float4{a[0], a[1], a[2], a[3]};
        *reinterpret_cast<float4*>(out + d + 4) = float4{a[4], a[5], a[6], a[7]};
    }
}

// ----------------------------------------------------------------------- GEMM ---
constexpr int GW = 4;          // waves per workgroup: 32-row tiles of the weight matrices
constexpr int KC = 512;        // activation columns per LDS chunk
constexpr int XS = KC + 8;     // halves per LDS row (the 16-B pad spreads the rows over the banks)

template <int EPI>
__global__ __launch_bounds__(64 * GW) void enc_gemm_f16_kernel(const EncGemm P) {
    __shared__ __attribute__((aligned(16))) _Float16 xs[32 * XS];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int col = lane & 31, h = lane >> 5;
    const int t0 = blockIdx.y * 32;
    // this wave's 32-row tile: tile wt of the matrices' tiles laid end to end
    int wt = blockIdx.x * GW + w;
    const __half* W = nullptr;
    const float* bias = nullptr;
    float* out = nullptr;
    __half* out16 = nullptr;
    int r0 = 0;
    bool act = false;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        if (i < P.nmat && !act) {
            const int nt = P.m[i].rows >> 5;
            if (wt < nt) {
                act = true;
                r0 = wt * 32;
                W = P.m[i].w;
                bias = P.m[i].bias;
                out = P.m[i].out;
                out16 = P.m[i].out16;
            } else {
                wt -= nt;
            }
        }
    }
    const int K = P.K;
    const __half* wrow = W + (long long)(r0 + col) * K + 16 * h;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    for (int k0 = 0; k0 < K; k0 += KC) {
        const int kc = min(KC, K - k0);
        const int n4 = kc >> 2;
        if (k0) __syncthreads();   // the previous chunk is read
        for (int i = tid; i < 32 * n4; i += 64 * GW) {
            const int t = i / n4, c = i - t * n4;
            float4 v = float4{0.0f, 0.0f, 0.0f, 0.0f};
            if (t0 + t < P.ntok) v = *reinterpret_cast<const float4*>(P.x + (long long)(t0 + t) * P.x_stride + k0 + 4 * c);
            *reinterpret_cast<u32x2*>(xs + t * XS + 4 * c) = u32x2{pack2(v.x, v.y), pack2(v.z, v.w)};
        }
        __syncthreads();
        if (act) {
            const _Float16* xrow = xs + col * XS + 16 * h;
            for (int kk = 0; kk < kc; kk += 32) {
                const u32x4 a0 = *reinterpret_cast<const u32x4*>(wrow + k0 + kk);
                const u32x4 a1 = *reinterpret_cast<const u32x4*>(wrow + k0 + kk + 8);
                const u32x4 b0 = *reinterpret_cast<const u32x4*>(xrow + kk);
                const u32x4 b1 = *reinterpret_cast<const u32x4*>(xrow + kk + 8);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(as_h8(a0), as_h8(b0), acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(as_h8(a1), as_h8(b1), acc, 0, 0, 0);
            }
        }
    }
    // D: lane = token t0 + col, register r = weight row r0 + (r & 3) + 8 (r >> 2) + 4 h
    const int tok = t0 + col;
    if (!act || tok >= P.ntok) return;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int row = r0 + 8 * q + 4 * h;
        float y[4] = {acc[4 * q], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]};
        if (EPI != ENC_NONE && EPI != ENC_ADD) {   // ggml_add of the bias, a separate f32 operation
            const float4 b = *reinterpret_cast<const float4*>(bias + row);
            y[0] = y[0] + b.x;
            y[1] = y[1] + b.y;
            y[2] = y[2] + b.z;
            y[3] = y[3] + b.w;
        }
        if (EPI == ENC_GELU) {   // ggml_vec_gelu_f32 (GGML_GELU_FP16 table)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float v = y[e];
                const unsigned short hb = __half_as_ushort(__float2half_rn(v));
                const float t = __half2float(__ushort_as_half(P.gelu_tab[hb]));
                y[e] = v <= -10.0f ? 0.0f : (v >= 10.0f ? v : t);
            }
        }
        if (EPI == ENC_RESID || EPI == ENC_ADD) {  // the residual, after the bias
            const float4 r = *reinterpret_cast<const float4*>(P.resid + (long long)tok * P.out_stride + row);
            y[0] = y[0] + r.x;
            y[1] = y[1] + r.y;
            y[2] = y[2] + r.z;
            y[3] = y[3] + r.w;
        }
        if (out16)
            *reinterpret_cast<u32x2*>(out16 + (long long)tok * P.out_stride + row) = u32x2{pack2(y[0], y[1]), pack2(y[2], y[3])};
        else
            *reinterpret_cast<float4*>(out + (long long)tok * P.out_stride + row) = float4{y[0], y[1], y[2], y[3]};
    }
}

// ------------------------------------------------------------------ attention ---
constexpr int AW = 4;          // waves per workgroup: 8 of the tile's 32 queries each
constexpr int CK = 64;         // keys per LDS chunk

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

template <int HD>
__global__ __launch_bounds__(64 * AW) void enc_attn_kernel(const EncAttn P) {
    constexpr int KS = HD + 8;           // halves per staged K / V row
    constexpr int NCH = HD / 8;          // 16-B pieces per row
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int n = P.ntok, npad = (n + CK - 1) & ~(CK - 1);
    float* sc = reinterpret_cast<float*>(smem);                  // [32][npad] scores, then probabilities
    float* qs = sc + 32 * npad;                                  // [32][HD] f16-rounded q
    _Float16* kv = reinterpret_cast<_Float16*>(qs + 32 * HD);    // [CK][KS] the K or V chunk
    const int head = blockIdx.x, t0 = blockIdx.y * 32;
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (int i = tid; i < 32 * HD; i += 64 * AW) {
        const int t = i / HD, d = i - t * HD;
        const float v = t0 + t < n ? P.q[(long long)(t0 + t) * P.q_stride + head * HD + d] : 0.0f;
        qs[i] = __half2float(__float2half_rn(v));
    }
    auto stage = [&](const __half* src, int c0) {
        for (int i = tid; i < CK * NCH; i += 64 * AW) {
            const int r = i / NCH, ch = i - r * NCH;
            u32x4 v = u32x4{0u, 0u, 0u, 0u};   // keys past n: zero rows
            if (c0 + r < n) v = *reinterpret_cast<const u32x4*>(src + (long long)(c0 + r) * P.kv_stride + head * HD + 8 * ch);
            *reinterpret_cast<u32x4*>(kv + r * KS + 8 * ch) = v;
        }
    };
    // ---- pass 1: scaled KQ of the tile, key = lane of the chunk, 8 queries per wave ----
    for (int c0 = 0; c0 < n; c0 += CK) {
        __syncthreads();
        stage(P.k, c0);
        __syncthreads();
        float s[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) s[j] = 0.0f;
        const _Float16* krow = kv + lane * KS;
        const float* qw = qs + 8 * w * HD;
#pragma unroll
        for (int d = 0; d < HD; d += 8) {
            const half8 kk = *reinterpret_cast<const half8*>(krow + d);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float kf = (float)kk[e];
#pragma unroll
                for (int j = 0; j < 8; ++j) s[j] = s[j] + qw[j * HD + d + e] * kf;
            }
        }
        if (c0 + lane < n) {
#pragma unroll
            for (int j = 0; j < 8; ++j) sc[(8 * w + j) * npad + c0 + lane] = s[j] * P.scale;
        }
    }
    __syncthreads();
    // ---- pass 2: the exact softmax of each query row (a wave per row), p rounded to f16 ----
    for (int j = 0; j < 8; ++j) {
        float* row = sc + (8 * w + j) * npad;
        float mx = -INFINITY;
        for (int c = lane; c < n; c += 64) mx = fmaxf(mx, row[c]);
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
        double sum = 0.0;
        for (int c = lane; c < n; c += 64) {
            const float e = expf(row[c] - mx);
            row[c] = e;
            sum += (double)e;
        }
        sum = wave_sum_d(sum);
        const float inv = (float)(1.0 / sum);
        for (int c = lane; c < npad; c += 64) row[c] = c < n ? __half2float(__float2half_rn(row[c] * inv)) : 0.0f;
    }
    // ---- pass 3: PV, head dimension on the lane (HD 32: the two half-waves take alternate key quads) ----
    constexpr int HV = 64 / HD;          // half-waves sharing a head dimension
    const int d = lane & (HD - 1), hh = lane / HD;
    float o[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = 0.0f;
    for (int c0 = 0; c0 < n; c0 += CK) {
        __syncthreads();
        stage(P.v, c0);
        __syncthreads();
        for (int c = 4 * hh; c < CK; c += 4 * HV) {
            float vf[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) vf[e] = (float)kv[(c + e) * KS + d];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float4 p = *reinterpret_cast<const float4*>(sc + (8 * w + j) * npad + c0 + c);
                o[j] = o[j] + p.x * vf[0];
                o[j] = o[j] + p.y * vf[1];
                o[j] = o[j] + p.z * vf[2];
                o[j] = o[j] + p.w * vf[3];
            }
        }
    }
    if (HV == 2) {
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = o[j] + __shfl_xor(o[j], 32, 64);
    }
    if (hh != 0) return;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int tok = t0 + 8 * w + j;
        if (tok < n) P.out[(long long)tok * P.out_stride + head * HD + d] = o[j];
    }
}

size_t attn_lds(int ntok, int hd) {
    const size_t npad = (size_t)((ntok + CK - 1) & ~(CK - 1));
    return 32 * npad * 4 + 32 * (size_t)hd * 4 + (size_t)CK * (hd + 8) * 2;
}

}  // namespace enc

void launch_enc_embed(const EncEmbed& p, hipStream_t s) {
    if (p.ntok < 1 || p.n_embd < 8 || p.n_embd % 8 || !p.tokens || !p.tok || !p.typ || !p.pos || !p.out) throw Error("enc embed: unsupported shape");
    hipLaunchKernelGGL(enc::enc_embed_kernel, dim3(p.ntok), dim3(256), 0, s, p);
    MI_HIP(hipGetLastError());
}

void launch_enc_gemm(const EncGemm& p, hipStream_t s) {
    if (p.ntok < 1 || p.ntok > ENC_MAX_TOK) throw Error("enc gemm: 1 to 512 tokens");
    if (p.K < 32 || p.K % 32 || p.x_stride % 4 || p.out_stride % 4 || !p.x) throw Error("enc gemm: K must be a multiple of 32");
    if (p.nmat < 1 || p.nmat > 3) throw Error("enc gemm: one to three matrices");
    int tiles = 0;
    for (int i = 0; i < p.nmat; ++i) {
        const EncMat& m = p.m[i];
        if (m.rows < 32 || m.rows % 32 || !m.w || (!m.out && !m.out16)) throw Error("enc gemm: rows must be a multiple of 32");
        if (m.rows > p.out_stride) throw Error("enc gemm: rows past the output stride");
        if (p.epi != ENC_NONE && p.epi != ENC_ADD && !m.bias) throw Error("enc gemm: this epilogue needs a bias");
        tiles += m.rows / 32;
    }
    if (p.epi == ENC_GELU && !p.gelu_tab) throw Error("enc gemm: the GELU epilogue needs the table");
    if ((p.epi == ENC_RESID || p.epi == ENC_ADD) && !p.resid) throw Error("enc gemm: residual epilogue without resid");
    const dim3 grid((tiles + enc::GW - 1) / enc::GW, (p.ntok + 31) / 32), block(64 * enc::GW);
    switch (p.epi) {
    case ENC_NONE: hipLaunchKernelGGL(enc::enc_gemm_f16_kernel<ENC_NONE>, grid, block, 0, s, p); break;
    case ENC_BIAS: hipLaunchKernelGGL(enc::enc_gemm_f16_kernel<ENC_BIAS>, grid, block, 0, s, p); break;
    case ENC_GELU: hipLaunchKernelGGL(enc::enc_gemm_f16_kernel<ENC_GELU>, grid, block, 0, s, p); break;
    case ENC_RESID: hipLaunchKernelGGL(enc::enc_gemm_f16_kernel<ENC_RESID>, grid, block, 0, s, p); break;
    case ENC_ADD: hipLaunchKernelGGL(enc::enc_gemm_f16_kernel<ENC_ADD>, grid, block, 0, s, p); break;
    default: throw Error("enc gemm: epilogue 0 .. 4");
    }
    MI_HIP(hipGetLastError());
}

bool enc_attn_supported(int head_dim) { return head_dim == 32 || head_dim == 64; }

// the scores of a 512-token call need more dynamic LDS (81 KiB of the CU's 160) than the default limit
void init_enc_attributes() {
    const int lds = (int)enc::attn_lds(ENC_MAX_TOK, 64);
    MI_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(enc::enc_attn_kernel<32>), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    MI_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(enc::enc_attn_kernel<64>), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
}

void launch_enc_attn(const EncAttn& p, hipStream_t s) {
    if (p.ntok < 1 || p.ntok > ENC_MAX_TOK) throw Error("enc attention: 1 to 512 tokens");
    if (!enc_attn_supported(p.head_dim)) throw Error("enc attention: head_dim 32 or 64");
    if (p.n_head < 1 || p.kv_stride % 8 || !p.q || !p.k || !p.v || !p.out) throw Error("enc attention: unsupported shape");
    const dim3 grid(p.n_head, (p.ntok + 31) / 32), block(64 * enc::AW);
    const size_t lds = enc::attn_lds(p.ntok, p.head_dim);
    if (p.head_dim == 32) hipLaunchKernelGGL(enc::enc_attn_kernel<32>, grid, block, lds, s, p);
    else hipLaunchKernelGGL(enc::enc_attn_kernel<64>, grid, block, lds, s, p);
    MI_HIP(hipGetLastError());
}

}  // namespace mi
