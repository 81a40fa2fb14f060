// Embeddings on the device (gfx950, wave64): the tail of a forward pass in embeddings mode, in
// place of "final norm + quantisation + output head" (llama.cpp b5187: result_norm is what
// llama_get_embeddings_ith returns; build_pooling reduces it over a sequence).
//
//  * embd_norm_kernel: the final norm of nt residual rows to f32 rows, one workgroup per row --
//    rms_norm(x, eps) * w (LLaMA, MoE) or layer_norm(x, eps) * w + b (GPT-2).  The arithmetic is the
//    quantising kernels' (dv_quant_kernel, gemv_kernel's PRO_LAYERNORM): f32 squares summed in
//    double -- each thread its 16-byte pieces tid, tid + 256, ... in that order, the wave by the
//    DPP scan, the four waves' totals from LDS in wave order -- scale = 1 / sqrtf((float)(sum / n) +
//    eps), then the weight multiplied and the bias added as separate f32 operations.
//  * embd_pool_kernel: MEAN over token rows (the mean matrix of build_pooling: every term
//    row_t[j] * (1.0f / n), summed in f32 in ascending token order onto the pooled row, which
//    carries the sum from one physical batch of a call to the next) or the copy of one row (CLS,
//    LAST).  A lane per column, consecutive lanes consecutive columns; no atomics, one fixed order.
#include "qdot.h"

namespace mi {

namespace {

constexpr int EN_NW = 4;   // waves per workgroup (row)

// the workgroup's sum of every thread's double, in a fixed order; all threads get it
__device__ __forceinline__ double embd_block_sum(double v, double* red, int lane, int wave) {
    v = wave_sum63_d(v);
    if (lane == 63) red[wave] = v;
    __syncthreads();
    double tot = 0.0;
#pragma unroll
    for (int k = 0; k < EN_NW; ++k) tot += red[k];
    return tot;
}

__global__ __launch_bounds__(64 * EN_NW) void embd_norm_kernel(const EmbdNorm P) {
    __shared__ double red[2][EN_NW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const f32x4* x = reinterpret_cast<const f32x4*>(P.x + (long long)blockIdx.x * P.x_stride);
    f32x4* out = reinterpret_cast<f32x4*>(P.out + (long long)blockIdx.x * P.out_stride);
    const f32x4* w = reinterpret_cast<const f32x4*>(P.w);
    const int n4 = P.K >> 2;
    float mean = 0.0f;
    if (P.b) {   // ggml_compute_forward_norm_f32: the mean from a double sum of the elements
        double s = 0.0;
        for (int i = tid; i < n4; i += 64 * EN_NW) {
            const f32x4 v = x[i];
            s += (double)v.x;
            s += (double)v.y;
            s += (double)v.z;
            s += (double)v.w;
        }
        mean = (float)(embd_block_sum(s, red[0], lane, wave) / (double)P.K);
    }
    // the double sum of the f32 squares of (x - mean): the variance, or (mean 0) rms_norm's mean square
    double sq = 0.0;
    for (int i = tid; i < n4; i += 64 * EN_NW) {
        f32x4 v = x[i];
        if (P.b) v = f32x4{v.x - mean, v.y - mean, v.z - mean, v.w - mean};
        sq += (double)(v.x * v.x);
        sq += (double)(v.y * v.y);
        sq += (double)(v.z * v.z);
        sq += (double)(v.w * v.w);
    }
    const float scale = 1.0f / sqrtf((float)(embd_block_sum(sq, red[1], lane, wave) / (double)P.K) + P.eps);
    for (int i = tid; i < n4; i += 64 * EN_NW) {
        const f32x4 v = x[i], g = w[i];
        f32x4 y;
        if (P.b) {   // (x - mean) * scale, then ggml_mul, ggml_add
            const f32x4 b = reinterpret_cast<const f32x4*>(P.b)[i];
            y.x = ((v.x - mean) * scale) * g.x + b.x;
            y.y = ((v.y - mean) * scale) * g.y + b.y;
            y.z = ((v.z - mean) * scale) * g.z + b.z;
            y.w = ((v.w - mean) * scale) * g.w + b.w;
        } else {     // ggml_vec_scale_f32 then ggml_mul
            y.x = (v.x * scale) * g.x;
            y.y = (v.y * scale) * g.y;
            y.z = (v.z * scale) * g.z;
            y.w = (v.w * scale) * g.w;
        }
        out[i] = y;
    }
}

// (a wave per workgroup: the column count is all the parallelism a token-ordered sum has, so the
// columns are spread over as many CUs as they give waves, and EP_LD rows are requested together --
// one load per row and lane in flight at a time made a 512-token call wait out 512 round trips)
constexpr int EP_LD = 16;
__global__ __launch_bounds__(64) void embd_pool_kernel(const EmbdPool P) {
    const int j = blockIdx.x * 64 + threadIdx.x;
    if (j >= P.K) return;
    if (P.nt == 0) {   // CLS / LAST: the one row
        P.out[j] = P.rows[j];
        return;
    }
    float acc = P.accumulate ? P.out[j] : 0.0f;
    for (int t0 = 0; t0 < P.nt; t0 += EP_LD) {
        float v[EP_LD];
#pragma unroll
        for (int k = 0; k < EP_LD; ++k) v[k] = t0 + k < P.nt ? P.rows[(long long)(t0 + k) * P.stride + j] : 0.0f;
#pragma unroll
        for (int k = 0; k < EP_LD; ++k)
            if (t0 + k < P.nt) acc = __fadd_rn(acc, __fmul_rn(v[k], P.inv_n));
    }
    P.out[j] = acc;
}

}  // namespace

void launch_embd_norm(const EmbdNorm& p, hipStream_t s) {
    if (p.nt < 1 || p.K < 4 || p.K % 4 || p.x_stride % 4 || p.out_stride % 4 || !p.x || !p.w || !p.out)
        throw Error("embd norm: unsupported shape");
    hipLaunchKernelGGL(embd_norm_kernel, dim3(p.nt), dim3(64 * EN_NW), 0, s, p);
    MI_HIP(hipGetLastError());
}

void launch_embd_pool(const EmbdPool& p, hipStream_t s) {
    if (p.nt < 0 || p.K < 1 || !p.rows || !p.out) throw Error("embd pool: unsupported shape");
    hipLaunchKernelGGL(embd_pool_kernel, dim3((p.K + 63) / 64), dim3(64), 0, s, p);
    MI_HIP(hipGetLastError());
}

}  // namespace mi
