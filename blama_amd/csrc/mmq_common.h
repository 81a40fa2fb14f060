// Device helpers shared by the int8-MFMA batch kernels: quant_act.hip (the kernels that run between
// GEMMs), mmq.hip (the tiled GEMM, mmq2_t) and mmqs.hip (the short streaming GEMMs).
//
// The arithmetic contract of all of them is ggml b5187's CPU mul_mat for these types: the
// activation rows are quantised to Q8_K exactly as quantize_row_q8_K_ref (one row per token, as the
// CPU graph does for src1; Q8_0 weights: quantize_row_q8_0), and every weight row x activation row
// product is
//   Q4_K / Q5_K  sum_sb [ d_x d_y * sum_j sc_j * dot_j  -  dmin_x d_y * sum_j m_j * bsum_j ]
//   Q6_K         sum_sb [ d_x d_y * sum_g sc_g * dot_g ]               (vec_dot_q*_K_q8_K)
//   Q8_0         sum_b  [ d_x d_y * dot_b ]                            (vec_dot_q8_0_q8_0)
// with the sub-block dots dot_j (32 elements; Q6_K: 16-element groups g) and the min terms computed
// EXACTLY in int32 by v_mfma_i32_32x32x32_i8, and one fused float update (fmaf) per superblock
// (Q8_0: per 32-block).  Only the fp32 sum across superblocks runs in another order than the
// CPU's.  "The contract" in the kernel files means this paragraph.
//
// MFMA geometry.  A wave computes a 32x32 D tile per MFMA, D[token][weight row]:
//   A operand = activations: lane l holds token l&31, k-half l>>5 (16 int8)
//   B operand = weights:     lane l holds weight row l&31, the same k-half
//   D: lane l, register r  = token (r&3) + 8(r>>2) + 4(l>>5), weight row l&31
// (the k order inside an MFMA does not matter: A and B share it; scripts/exp_mfma_layout.cpp
// checks the D map).  So every lane owns ONE weight row: its scales and mins are per-lane scalars.
#pragma once
#include "kernels.h"
#include <hip/hip_runtime.h>

namespace mi {
namespace mmq {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

template <typename T>
__device__ __forceinline__ const __attribute__((address_space(1))) T* gp(const T* p) {
    return (const __attribute__((address_space(1))) T*)(p);
}
__device__ __forceinline__ float h2f(uint32_t bits) {
    return __half2float(__ushort_as_half(static_cast<unsigned short>(bits & 0xFFFFu)));
}
template <int CTRL, int RMASK>
__device__ __forceinline__ int dpp_i(int v) {
    return __builtin_amdgcn_update_dpp(0, v, CTRL, RMASK, 0xf, false);
}
template <int CTRL, int RMASK>
__device__ __forceinline__ double dpp_d(double v) {
    const long long b = __double_as_longlong(v);
    const int lo = dpp_i<CTRL, RMASK>((int)b), hi = dpp_i<CTRL, RMASK>((int)(b >> 32));
    return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}
// full-wave double sum (fixed order), total in lane 63
__device__ __forceinline__ double wave_sum63_d(double v) {
    v += dpp_d<0x111, 0xf>(v);
    v += dpp_d<0x112, 0xf>(v);
    v += dpp_d<0x114, 0xf>(v);
    v += dpp_d<0x118, 0xf>(v);
    v += dpp_d<0x142, 0xa>(v);
    v += dpp_d<0x143, 0xc>(v);
    return v;
}
__device__ __forceinline__ float wave_max_pos(float v) {
#define MX(ctrl, rm) v = fmaxf(v, __int_as_float(dpp_i<ctrl, rm>(__float_as_int(v))))
    MX(0x111, 0xf); MX(0x112, 0xf); MX(0x114, 0xf); MX(0x118, 0xf); MX(0x142, 0xa); MX(0x143, 0xc);
#undef MX
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}

__device__ __forceinline__ float silu(float x) { return x / (1.0f + expf(-x)); }

// ((p[0] + p[s]) + p[2s]) + ... over n parts, in part order, the loads of up to 8 parts issued
// together (a runtime-length loop of load-then-add pays one memory round trip per part)
template <typename V>
__device__ __forceinline__ V sum_parts(const V* p, long long stride, int n) {
    V v[7];
#pragma unroll
    for (int k = 1; k < 8; ++k)
        if (k < n) v[k - 1] = p[k * stride];
    V acc = p[0];
#pragma unroll
    for (int k = 1; k < 8; ++k)
        if (k < n) acc = acc + v[k - 1];
    for (int k = 8; k < n; k += 4) {   // (past 8 parts: 4 at a time)
        V w[4];
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (k + q < n) w[q] = p[(k + q) * stride];
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (k + q < n) acc = acc + w[q];
    }
    return acc;
}

__device__ __forceinline__ v16i mfma(v4i a, v4i b) {
    const v16i z = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    return __builtin_amdgcn_mfma_i32_32x32x32_i8(a, b, z, 0, 0, 0);
}

// MFMA-order weight copy: one 32-row x superblock tile (lane = h*32 + c holds row c's bytes of
// k-half h; rows of a gate/up pair tile: c < 16 gate row 16*rt + c, c >= 16 up row 16*rt + c - 16)
//   Q4_K  [p 4][lane 64][16] qs bytes 32p + 16h.. | [c 32][16] header                       4608 B
//   Q6_K  the scaled weights w = (q - 32) * scale (|w| <= 4096, exact in int16) as two int8 MFMA
//         operands w = 64*hi + lo (hi -64..64, lo 0..63): [s 8][lane 64][16] hi of span s (superblock
//         elements 32s + 16h..) | the same for lo | [c 32][2] d                              16448 B
//         (a 32-element span holds two 16-element scale groups, one per k-half: with the scale
//         folded into the operand, one MFMA per span and operand carries the exact integer sum)
//   Q8_0  [j 8][lane 64][16] qs bytes 32j + 16h.. | [c 32][8 f16] d                            8704 B
//   Q5_K  as Q4_K, plus [lane 64][16] qh bytes 16h..: [p 4][lane][16] qs | qh | [c 32][16] header 5632 B
//   Q4_0 / Q5_0  the Q8_0 tile of the same blocks: every block is the Q8_0 block with the same d and
//         qs[i] = the signed weight (q - 8, q - 16), expanded to int8 once when the copy is built, so
//         the GEMMs run their Q8_0 form on it (mmq_op_type) with the same exact int32 sums          8704 B
__host__ __device__ constexpr int mmq32_tile_bytes_d(int type) {
    return type == T_Q4_K ? 4608 : type == T_Q5_K ? 5632 : type == T_Q6_K ? 16448
         : (type == T_Q8_0 || type == T_Q4_0 || type == T_Q5_0) ? 8704 : 0;
}
// the operand format of a type's MFMA-order copy: the kernels' template type
__host__ __device__ constexpr int mmq_op_type(int type) { return (type == T_Q4_0 || type == T_Q5_0) ? (int)T_Q8_0 : type; }

constexpr int MMQ_SEGS = 3;    // matrices (row segments) one launch carries
typedef __attribute__((address_space(3))) char lchar;
// register pins: the value is materialised at this point of the (volatile) instruction stream,
// so LDS reads issued before it stay in flight together instead of being sunk to their uses
__device__ __forceinline__ void pin(v4i& x) { asm volatile("" : "+v"(x)); }
__device__ __forceinline__ void pin_all() { asm volatile("" ::: "memory"); }
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
// the two 16-bit halves of x times s (v_pk_mul_lo_u16), each product < 65536
__device__ __forceinline__ unsigned wmul16(unsigned x, unsigned s) {
    u16x2 a;
    __builtin_memcpy(&a, &x, 4);
    const u16x2 r = a * u16x2{(unsigned short)s, (unsigned short)s};
    unsigned o;
    __builtin_memcpy(&o, &r, 4);
    return o;
}
// the bytes of x times s, every byte product < 256 (no carry between bytes): v_pk_mul_lo_u16
__device__ __forceinline__ unsigned bmul(unsigned x, unsigned s) {
    u16x2 a;
    __builtin_memcpy(&a, &x, 4);
    const u16x2 r = a * u16x2{(unsigned short)s, (unsigned short)s};
    unsigned o;
    __builtin_memcpy(&o, &r, 4);
    return o;
}
template <typename V>
__device__ __forceinline__ V lds_ld(const lchar* p) { return *reinterpret_cast<const __attribute__((address_space(3))) V*>(p); }

}  // namespace mmq
}  // namespace mi
