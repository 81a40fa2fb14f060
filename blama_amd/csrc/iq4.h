// The codebook of the IQ4_NL / IQ4_XS kernels and its lookup (qdot.h: the decode dots;
// mmq_common.h: the MFMA operand decode; kernels.hip / mmq.hip: dequantisation and the IQ4_NL copy).
#pragma once
#include <hip/hip_runtime.h>

namespace mi {

// kvalues_iq4nl (ggml-common.h): the 16-entry int8 codebook a nibble of IQ4_NL / IQ4_XS indexes.
// The one copy: iq4_lut's table dwords are packed from it.
__host__ __device__ constexpr int iq4_kv(int i) {
    constexpr signed char kv[16] = {-127, -104, -83, -65, -49, -35, -22, -10, 1, 13, 25, 38, 53, 69, 89, 113};
    return kv[i];
}
// entries 4 k .. 4 k + 3, each + off, as the bytes of one dword (entry 4 k lowest)
constexpr unsigned iq4_kv4(int k, int off) {
    unsigned d = 0;
    for (int b = 0; b < 4; ++b) d |= (unsigned)((iq4_kv(4 * k + b) + off) & 0xFF) << (8 * b);
    return d;
}

// iq4_lut turns a dword of four indices (one per byte, 0..15) into the four codebook entries, the
// table held as four literal dwords: v_perm_b32 over the table halves with the low three index bits
// as byte selectors (selector 0-3: a byte of the second operand, 4-7: of the first), then a third
// v_perm_b32 that takes every byte from the upper or the lower half by index bit 3.  No branch, no
// LDS table.  OFF 128: the table of kv + 128 (1..241, unsigned bytes) the MFMA decode multiplies
// (mmq_common.h iq4xs_span).
template <int OFF = 0>
__device__ __forceinline__ unsigned iq4_lut(unsigned idx) {
    constexpr unsigned T0 = iq4_kv4(0, OFF), T1 = iq4_kv4(1, OFF), T2 = iq4_kv4(2, OFF), T3 = iq4_kv4(3, OFF);
    static_assert(OFF != 0 || (T0 == 0xBFAD9881u && T3 == 0x71594535u), "iq4_kv4 packs entry 4 k into the low byte");
    const unsigned s = idx & 0x07070707u;
    const unsigned lo = __builtin_amdgcn_perm(T1, T0, s), hi = __builtin_amdgcn_perm(T3, T2, s);
    return __builtin_amdgcn_perm(hi, lo, ((idx >> 1) & 0x04040404u) | 0x03020100u);
}

}  // namespace mi
