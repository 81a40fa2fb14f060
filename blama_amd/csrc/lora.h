// The LoRA terms of one output row (kernels.h LoraFold), shared by the decode GEMV that folds them
// into its own launch (no expand launch, no delta buffer) and by lora.hip's expand kernel.
#pragma once
#include "qdot.h"

namespace mi {

// y plus range i's terms for `row` of token `tok`, adapter by adapter: y = y + f32(sum_j B[row][j]
// t[j]) * s.  The sum is taken by the whole wave in double (lane l takes j = l, l + 64, ...; DPP
// tree), so the result stands in lane 63, as wave_sum63's; i and row are wave-uniform.
__device__ __forceinline__ float lora_fold_wave(const LoraFold& F, int i, long long row, int tok, int lane, float y) {
    const void* B = F.B[i];
    if (!B) return y;
    const int R = F.R[i], off = F.off[i], f16 = F.f16[i];
    const int* tab = F.tab[i];
    const float* t = F.t + (long long)tok * F.t_stride + off;
    const int n = tab[0];
    int beg = 0;
    for (int a = 0; a < n; ++a) {
        const int end = tab[1 + a];
        const float s = __int_as_float(tab[1 + LORA_MAX_STACK + a]);
        double d = 0.0;
        for (int j = beg + lane; j < end; j += 64) {
            const float b = f16 ? __half2float(reinterpret_cast<const __half*>(B)[row * R + j])
                                : reinterpret_cast<const float*>(B)[row * R + j];
            d = fma((double)b, (double)t[j], d);
        }
        d = wave_sum63_d(d);
        y = y + (float)d * s;
        beg = end;
    }
    return y;
}

// the same by one thread (ts: the token's t of this range, e.g. in LDS)
__device__ __forceinline__ float lora_fold_row(const LoraFold& F, long long row, const float* ts) {
    const void* B = F.B[0];
    const int R = F.R[0], n = F.tab[0][0];
    float y = 0.0f;
    int beg = 0;
    for (int a = 0; a < n; ++a) {
        const int end = F.tab[0][1 + a];
        const float s = __int_as_float(F.tab[0][1 + LORA_MAX_STACK + a]);
        double d = 0.0;
        for (int j = beg; j < end; ++j) {
            const float b = F.f16[0] ? __half2float(reinterpret_cast<const __half*>(B)[row * R + j])
                                     : reinterpret_cast<const float*>(B)[row * R + j];
            d = fma((double)b, (double)ts[j], d);
        }
        y = a == 0 ? (float)d * s : y + (float)d * s;
        beg = end;
    }
    return y;
}

}  // namespace mi
