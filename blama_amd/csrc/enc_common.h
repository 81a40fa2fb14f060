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

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

void init_attn_seq_attributes();   // enc_seq.hip: the dynamic-LDS limit of its attention kernels

}  // namespace enc
}  // namespace mi
