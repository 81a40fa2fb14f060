// Shared by the encoder kernels (enc.hip, enc_seq.hip): the MFMA operand types and the small
// conversions both files use.
#pragma once
#include <hip/hip_fp16.h>
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

// the ALiBi mask value of (query i, key j) of one sequence: -(float)|i - j|, exact in f32
__device__ __forceinline__ float alibi_dist(int i, int j) { return -(float)(i > j ? i - j : j - i); }

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// The K loop of the multi-tile GEMMs (enc_nomic.hip, enc_jina.hip; described above enc_nomic.hip)
constexpr int NW = 4;          // waves per workgroup
constexpr int NKC = 512;       // activation columns per LDS chunk
constexpr int NXS = NKC + 8;   // halves per LDS row

// wrow[a]: row (tile a's first row + lane & 31) of the weights, at column 16 (lane >> 5)
template <int NA>
__device__ __forceinline__ void gemm_tiles(const __half* const (&wrow)[NA], bool act, const float* x, int x_stride, int K,
                                           int ntok, int t0, _Float16* xs, f32x16 (&acc)[NA]) {
    const int tid = threadIdx.x, lane = tid & 63, col = lane & 31, h = lane >> 5;
#pragma unroll
    for (int a = 0; a < NA; ++a)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[a][r] = 0.0f;
    for (int k0 = 0; k0 < K; k0 += NKC) {
        const int kc = min(NKC, K - k0);
        const int n4 = kc >> 2;
        if (k0) __syncthreads();   // the previous chunk is read
        for (int i = tid; i < 32 * n4; i += 64 * NW) {
            const int t = i / n4, c = i - t * n4;
            float4 v = float4{0.0f, 0.0f, 0.0f, 0.0f};   // tokens past ntok: zero columns, never stored
            if (t0 + t < ntok) v = *reinterpret_cast<const float4*>(x + (long long)(t0 + t) * x_stride + k0 + 4 * c);
            *reinterpret_cast<u32x2*>(xs + t * NXS + 4 * c) = u32x2{pack2(v.x, v.y), pack2(v.z, v.w)};
        }
        __syncthreads();
        if (act) {
            const _Float16* xrow = xs + col * NXS + 16 * h;
            for (int kk = 0; kk < kc; kk += 32) {
                const u32x4 b0 = *reinterpret_cast<const u32x4*>(xrow + kk);
                const u32x4 b1 = *reinterpret_cast<const u32x4*>(xrow + kk + 8);
#pragma unroll
                for (int a = 0; a < NA; ++a) {
                    const u32x4 a0 = *reinterpret_cast<const u32x4*>(wrow[a] + k0 + kk);
                    const u32x4 a1 = *reinterpret_cast<const u32x4*>(wrow[a] + k0 + kk + 8);
                    acc[a] = __builtin_amdgcn_mfma_f32_32x32x16_f16(as_h8(a0), as_h8(b0), acc[a], 0, 0, 0);
                    acc[a] = __builtin_amdgcn_mfma_f32_32x32x16_f16(as_h8(a1), as_h8(b1), acc[a], 0, 0, 0);
                }
            }
        }
    }
}

void init_attn_seq_attributes();   // enc_seq.hip: the dynamic-LDS limit of its attention kernels

}  // namespace enc
}  // namespace mi
