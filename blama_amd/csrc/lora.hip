// LoRA adapters on the device (gfx950, wave64): the two small products of llama-graph.cpp's
// build_lora_mm (b5187), y = W cur + s * (B (A cur)), around the engine's own W cur.
//
//  * lora_shrink_kernel: t = A cur, a rank-row GEMV over K per token -- a wave per rank row,
//    four rows per workgroup, a grid row per token (the decode step: one token; a batch: the same
//    kernel over its tokens, A served from L2).  cur is the f32 activation the base mul_mat reads;
//    for Q/K/V and gate/up the streaming step keeps rms_norm(x) * norm_w only quantised, so the
//    workgroup rebuilds it from x (dv_quant_kernel's arithmetic: the sum of squares in double).
//  * lora_expand_kernel: out = s * (B t), a thread per output row: the terms of the launches that
//    take them precomputed (the batch GEMMs, gemv_kernel).  The streaming decode step folds this
//    product into dgemv_kernel instead (lora_fold_wave, lora.h).
//
// ggml's arithmetic: an F16 matrix has its f32 operand rounded to f16 (ggml_vec_dot_f16), an F32
// matrix is a plain dot.  The products are summed in double here and rounded to f32 once.
#include "lora.h"

namespace mi {

namespace {

constexpr int LS_NW = 4;   // waves (rank rows) per workgroup


__global__ __launch_bounds__(64 * LS_NW) void lora_shrink_kernel(const LoraShrink P) {
    __shared__ double red[LS_NW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tok = blockIdx.y;
    const float* x = P.x + (long long)tok * P.x_stride;
    const int n4 = P.K >> 2;
    float scale = 1.0f;
    if (P.norm_w) {   // ggml_compute_forward_rms_norm_f32: mean of squares in double, 1 / sqrtf(mean + eps)
        double sq = 0.0;
        for (int i = tid; i < n4; i += 64 * LS_NW) {
            const f32x4 v = reinterpret_cast<const f32x4*>(x)[i];
            sq += (double)(v.x * v.x);
            sq += (double)(v.y * v.y);
            sq += (double)(v.z * v.z);
            sq += (double)(v.w * v.w);
        }
        sq = wave_sum63_d(sq);
        if (lane == 63) red[wave] = sq;
        __syncthreads();
        double tot = 0.0;
#pragma unroll
        for (int k = 0; k < LS_NW; ++k) tot += red[k];
        scale = 1.0f / sqrtf((float)(tot / (double)P.K) + P.eps);
    }
    const int j = blockIdx.x * LS_NW + wave;   // this wave's rank row
    if (j >= P.R) return;
    const int rnd = P.rnd[j];
    double acc = 0.0;
    for (int i = lane; i < n4; i += 64) {
        f32x4 c = reinterpret_cast<const f32x4*>(x)[i];
        if (P.norm_w) {   // ggml_vec_scale_f32 then ggml_mul
            const f32x4 w = reinterpret_cast<const f32x4*>(P.norm_w)[i];
            c.x = (c.x * scale) * w.x;
            c.y = (c.y * scale) * w.y;
            c.z = (c.z * scale) * w.z;
            c.w = (c.w * scale) * w.w;
        }
        if (rnd & 1) {
            c.x = __half2float(__float2half_rn(c.x));
            c.y = __half2float(__float2half_rn(c.y));
            c.z = __half2float(__float2half_rn(c.z));
            c.w = __half2float(__float2half_rn(c.w));
        }
        f32x4 a;
        if (P.a_f16) {
            const __half* ap = reinterpret_cast<const __half*>(P.A) + (long long)j * P.K + 4 * i;
            const __half2 a01 = reinterpret_cast<const __half2*>(ap)[0], a23 = reinterpret_cast<const __half2*>(ap)[1];
            a.x = __low2float(a01);
            a.y = __high2float(a01);
            a.z = __low2float(a23);
            a.w = __high2float(a23);
        } else {
            a = reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(P.A) + (long long)j * P.K)[i];
        }
        acc = fma((double)a.x, (double)c.x, acc);
        acc = fma((double)a.y, (double)c.y, acc);
        acc = fma((double)a.z, (double)c.z, acc);
        acc = fma((double)a.w, (double)c.w, acc);
    }
    acc = wave_sum63_d(acc);
    if (lane == 63) {
        float v = (float)acc;
        if (rnd & 2) v = __half2float(__float2half_rn(v));
        P.t[(long long)tok * P.R + j] = v;
    }
}

__global__ __launch_bounds__(256) void lora_expand_kernel(const LoraExpand P) {
    __shared__ float ts[LORA_MAX_RANK];
    const int tok = blockIdx.y;
    const int R = P.F.B[0] ? P.F.R[0] : 0;
    for (int j = threadIdx.x; j < R; j += 256) ts[j] = P.F.t[(long long)tok * P.F.t_stride + P.F.off[0] + j];
    __syncthreads();
    const int row = blockIdx.x * 256 + threadIdx.x;
    if (row >= P.rows) return;
    P.out[(long long)tok * P.out_stride + row] = R ? lora_fold_row(P.F, row, ts) : 0.0f;
}

}  // namespace

void launch_lora_shrink(const LoraShrink& p, hipStream_t s) {
    if (p.R < 1 || p.R > 3 * LORA_MAX_RANK || p.ntok < 1 || p.K < 4 || p.K % 4 || p.x_stride % 4 || !p.x || !p.A || !p.t ||
        !p.rnd)
        throw Error("lora shrink: unsupported shape");
    hipLaunchKernelGGL(lora_shrink_kernel, dim3((p.R + LS_NW - 1) / LS_NW, p.ntok), dim3(64 * LS_NW), 0, s, p);
    MI_HIP(hipGetLastError());
}

void launch_lora_expand(const LoraExpand& p, hipStream_t s) {
    if (p.ntok < 1 || p.rows < 1 || !p.out || (p.F.B[0] && (!p.F.t || !p.F.tab[0] || p.F.R[0] < 1 || p.F.R[0] > LORA_MAX_RANK)))
        throw Error("lora expand: unsupported shape");
    hipLaunchKernelGGL(lora_expand_kernel, dim3((p.rows + 255) / 256, p.ntok), dim3(256), 0, s, p);
    MI_HIP(hipGetLastError());
}

}  // namespace mi
