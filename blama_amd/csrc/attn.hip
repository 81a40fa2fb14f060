// Attention of decode steps and short batches over the f16 cache (gfx950, wave64): the five
// cache-attention kernels, the combine kernels, and attn_plan, the one place where a launch's kernel,
// template arguments, grid, block, LDS size and qsplit are chosen.  (attn_mfma.hip: a batch's
// attention on MFMA; enc.hip: the encoder's.)  Compiled with -ffp-contract=off, as kernels.hip.
#include "kernels.h"
#include "qdot.h"
#include <hip/hip_runtime.h>
#include <algorithm>

namespace mi {

// ---------------------------------------------------------------------------
// Attention of one query token over the f16 cache, split over cells, in two
// launches so that the softmax weights can be rounded exactly as the CPU graph
// rounds them (non-flash path, Instance.hpp:25 flash_attn=false):
//   KQ  = ggml_mul_mat(k, q):  q is converted to the f16 vec_dot_type, s = k.q
//   ggml_soft_max_ext(KQ, mask, 1/sqrt(hd)): w = s*scale, e = expf(w - max),
//        sum in double, p = e * (float)(1/sum)
//   KQV = ggml_mul_mat(v, kq): p is converted to f16, o = sum_c f16(p_c) v_c
// Rounding p to f16 needs the head's global max and sum before any weight is
// formed, so:
//   attn_scores_kernel  grid (n_head_kv, ATTN_SMAX): split s writes w_c of its
//                       cells for the R = n_head/n_head_kv query heads of kv
//                       head g, and the split's max per head.
//   attn_pv_kernel      same grid: global max from the split maxes, the sum of
//                       expf(w - max) over ALL cells (every split recomputes it
//                       in the same fixed order -> identical in every split),
//                       then sum_c f16(p_c) v_c over its own cells -> part_o.
// The WO GEMV's PRO_ATTN prologue adds the splits' partials in split order.
// Only the order of the fp32 sums differs from the CPU's.
// Lane layout: LPC = head_dim/8 lanes hold one cache row (8 halves = one
// 16-byte load each); a wave covers CPW = 64/LPC cells per step.
// ---------------------------------------------------------------------------
// U: cell steps whose cache loads are in flight together.  The first step's loads are issued at
// entry, ahead of the loads the arithmetic waits on first (q; the split maxima and scores), so
// the cache round trip overlaps them.
template <int R, int LPC, int U>
__global__ __launch_bounds__(256) void attn_scores_kernel(const AttnParams P) {
    constexpr int CPW = 64 / LPC;
    constexpr int HD = LPC * 8;
    __shared__ float red[4][R];
    // kv head, and the first of the R q heads this workgroup serves (qsplit: one q head each)
    const int g = P.qsplit ? (int)blockIdx.x / P.qsplit : (int)blockIdx.x, s = blockIdx.y;
    const int gq = P.qsplit ? (int)blockIdx.x : (int)blockIdx.x * R;
#ifdef MI_STAMPS
    unsigned long long* const stp = P.stamps ? P.stamps + (blockIdx.y * gridDim.x + blockIdx.x) * 8 : nullptr;
    if (stp && threadIdx.x == 0) stp[0] = __builtin_amdgcn_s_memrealtime();
#endif
    const int ncell = P.tokpos[2] + 1, qpos = P.tokpos[1];
    int chunk, nsplit;
    attn_split(ncell, chunk, nsplit);
    if (s >= nsplit) return;
    const int c0 = s * chunk, c1 = min(ncell, c0 + chunk);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int L = lane % LPC, G = lane / LPC;
    const long long row_off = (long long)g * HD + L * 8;
    u32x4 kk[U];
    int cpos[U];
    auto fetch = [&](int cb) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            int c = cb + u * 4 * CPW + G;
            c = c < c1 ? c : c1 - 1;
            kk[u] = *reinterpret_cast<const u32x4*>(P.kcache + (long long)c * P.kv_dim + row_off);
            cpos[u] = P.cell_pos[c];
        }
    };
    fetch(c0 + wave * CPW);
    float q[R][8];
#pragma unroll
    for (int t = 0; t < R; ++t) {
        const float4* qp = reinterpret_cast<const float4*>(P.q + (long long)(gq + t) * HD + L * 8);
        const float4 a = qp[0], b = qp[1];
        const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
        for (int e = 0; e < 8; ++e) q[t][e] = __half2float(__float2half_rn(v[e]));
    }
    float mx[R];
#pragma unroll
    for (int t = 0; t < R; ++t) mx[t] = -INFINITY;
    for (int cb = c0 + wave * CPW; cb < c1; cb += 4 * CPW * U) {
        if (cb != c0 + wave * CPW) fetch(cb);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int c = cb + u * 4 * CPW + G;
            const bool valid = c < c1 && cpos[u] <= qpos;
            const unsigned kw[4] = {kk[u].x, kk[u].y, kk[u].z, kk[u].w};
            float kf[8];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                kf[2 * e] = h2f(kw[e]);
                kf[2 * e + 1] = h2f(kw[e] >> 16);
            }
#pragma unroll
            for (int t = 0; t < R; ++t) {
                float d = 0.0f;
#pragma unroll
                for (int e = 0; e < 8; ++e) d = fmaf(q[t][e], kf[e], d);
#pragma unroll
                for (int off = LPC / 2; off > 0; off >>= 1) d += __shfl_xor(d, off, 64);
                const float w = valid ? d * P.scale : -INFINITY;
                mx[t] = fmaxf(mx[t], w);
                if (L == 0 && c < c1) P.scores[(long long)(gq + t) * P.n_ctx + c] = w;
            }
        }
    }
#pragma unroll
    for (int t = 0; t < R; ++t) {
        const float m = wave_max(mx[t]);
        if (lane == 0) red[wave][t] = m;
    }
    __syncthreads();
    if (threadIdx.x < R) {
        const int t = threadIdx.x;
        const float m = fmaxf(fmaxf(red[0][t], red[1][t]), fmaxf(red[2][t], red[3][t]));
        P.smax[s * P.n_head + gq + t] = m;
    }
#ifdef MI_STAMPS
    if (stp && threadIdx.x == 0) stp[4] = __builtin_amdgcn_s_memrealtime();
#endif
}

template <int R, int LPC, int U>
__global__ __launch_bounds__(256) void attn_pv_kernel(const AttnParams P) {
    constexpr int CPW = 64 / LPC;
    constexpr int HD = LPC * 8;
    __shared__ double dred[4][R];
    __shared__ float gm[R], ginv[R];
    __shared__ float red_o[4][R][HD];
    // kv head, and the first of the R q heads this workgroup serves (qsplit: one q head each)
    const int g = P.qsplit ? (int)blockIdx.x / P.qsplit : (int)blockIdx.x, s = blockIdx.y;
    const int gq = P.qsplit ? (int)blockIdx.x : (int)blockIdx.x * R;
#ifdef MI_STAMPS
    unsigned long long* const stp = P.stamps2 ? P.stamps2 + (blockIdx.y * gridDim.x + blockIdx.x) * 8 : nullptr;
    if (stp && threadIdx.x == 0) stp[0] = __builtin_amdgcn_s_memrealtime();
#endif
    const int ncell = P.tokpos[2] + 1;
    int chunk, nsplit;
    attn_split(ncell, chunk, nsplit);
    if (s >= nsplit) return;
    const int c0 = s * chunk, c1 = min(ncell, c0 + chunk);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int L = lane % LPC, G = lane / LPC;
    const long long row_off = (long long)g * HD + L * 8;
    u32x4 vv[U];
    auto fetch = [&](int cb) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            int c = cb + u * 4 * CPW + G;
            c = c < c1 ? c : c1 - 1;
            vv[u] = *reinterpret_cast<const u32x4*>(P.vcache + (long long)c * P.kv_dim + row_off);
        }
    };
    fetch(c0 + wave * CPW);   // in flight while the softmax statistics are formed
    // global max of every head of the group
    float M[R];
#pragma unroll
    for (int t = 0; t < R; ++t) {
        float m = -INFINITY;
        for (int k = 0; k < nsplit; ++k) m = fmaxf(m, P.smax[k * P.n_head + gq + t]);
        M[t] = m;
    }
    // sum over all cells of expf(w - max), in double, fixed order
#pragma unroll
    for (int t = 0; t < R; ++t) {
        const float* w = P.scores + (long long)(gq + t) * P.n_ctx;
        double acc = 0.0;
        for (int c = tid; c < ncell; c += 256) acc += (double)expf(w[c] - M[t]);
        acc = wave_sum_d(acc);
        if (lane == 0) dred[wave][t] = acc;
    }
    __syncthreads();
    if (tid < R) {
        const double tot = ((dred[0][tid] + dred[1][tid]) + dred[2][tid]) + dred[3][tid];
        ginv[tid] = (float)(1.0 / tot);
        gm[tid] = M[tid];
    }
    __syncthreads();
    float o[R][8];
#pragma unroll
    for (int t = 0; t < R; ++t)
#pragma unroll
        for (int e = 0; e < 8; ++e) o[t][e] = 0.0f;
    for (int cb = c0 + wave * CPW; cb < c1; cb += 4 * CPW * U) {
        if (cb != c0 + wave * CPW) fetch(cb);
        float pw[U][R];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            int c = cb + u * 4 * CPW + G;
            const bool in = c < c1;
            c = in ? c : c1 - 1;
#pragma unroll
            for (int t = 0; t < R; ++t) {
                const float w = P.scores[(long long)(gq + t) * P.n_ctx + c];
                // ggml_vec_soft_max_f32 then the f16 vec_dot_type conversion of KQV's src1
                const float p = expf(w - gm[t]) * ginv[t];
                pw[u][t] = in ? __half2float(__float2half_rn(p)) : 0.0f;
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const unsigned vw[4] = {vv[u].x, vv[u].y, vv[u].z, vv[u].w};
            float vf[8];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                vf[2 * e] = h2f(vw[e]);
                vf[2 * e + 1] = h2f(vw[e] >> 16);
            }
#pragma unroll
            for (int t = 0; t < R; ++t)
#pragma unroll
                for (int e = 0; e < 8; ++e) o[t][e] = fmaf(pw[u][t], vf[e], o[t][e]);
        }
    }
    // sum the CPW cell groups of the wave, then the 4 waves in fixed order
#pragma unroll
    for (int t = 0; t < R; ++t)
#pragma unroll
        for (int off = LPC; off < 64; off <<= 1)
#pragma unroll
            for (int e = 0; e < 8; ++e) o[t][e] += __shfl_xor(o[t][e], off, 64);
    if (G == 0) {
#pragma unroll
        for (int t = 0; t < R; ++t)
#pragma unroll
            for (int e = 0; e < 8; ++e) red_o[wave][t][L * 8 + e] = o[t][e];
    }
    __syncthreads();
    for (int i = tid; i < R * HD; i += 256) {
        const int t = i / HD, d = i % HD;
        const float acc = ((red_o[0][t][d] + red_o[1][t][d]) + red_o[2][t][d]) + red_o[3][t][d];
        P.part_o[((long long)s * P.n_head + gq + t) * HD + d] = acc;
    }
#ifdef MI_STAMPS
    if (stp && threadIdx.x == 0) stp[4] = __builtin_amdgcn_s_memrealtime();
#endif
}

// Contexts past ATTN_SHORT cells in ONE launch: grid (n_head, ATTN_SMAX), one q head per
// workgroup row, split s of the head's cells per column (attn_split's chunks).  The split keeps its
// scaled scores in LDS; the splits of a head exchange their maxima, then their partial sums of
// expf(w - M) in double, through flag lines (agent-scope stores, bounded polls), so every split
// rounds p = f16(expf(w - M) * (1/S)) with the head's global M and S -- the CPU graph's softmax --
// without the scores' round trip through global memory and the second launch of
// attn_scores_kernel / attn_pv_kernel.  The V chunk's loads are issued before the exchange.
// The splits of one head are co-resident (n_head * 16 workgroups of 4 waves fit the chip many
// times over); a poll gives up after 2 s and flags the step invalid (xerr) instead of hanging.
__device__ __forceinline__ unsigned ld_ag(const unsigned* p) {
    return __hip_atomic_load(const_cast<unsigned*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <int LPC>
__global__ __launch_bounds__(256) void attn_long_kernel(const AttnParams P) {
    constexpr int CPW = 64 / LPC;
    constexpr int HD = LPC * 8;
    constexpr int U = 4;
    extern __shared__ __attribute__((aligned(16))) float sw[];   // [chunk] scaled scores
    __shared__ float redm[4];
    __shared__ double dred[4];
    __shared__ float stat[2];                                     // M, inv
    __shared__ float red_o[4][HD];
    const int h = blockIdx.x, s = blockIdx.y;
    const int g = h / (P.n_head / P.n_head_kv);
    const int ncell = P.tokpos[2] + 1, qpos = P.tokpos[1];
    int chunk, nsplit;
    attn_split(ncell, chunk, nsplit);
    if (s >= nsplit) return;
    const int c0 = s * chunk, c1 = min(ncell, c0 + chunk);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int L = lane % LPC, G = lane / LPC;
    const long long row_off = (long long)g * HD + L * 8;
    // strictly increasing over (step, layer, phase) for any depth
    const unsigned epoch = *P.step * (2u * (unsigned)max(P.n_layer, 1) + 2u) + 2u * (unsigned)P.layer;
    unsigned* const fl = P.xflags + (long long)h * ATTN_SMAX * 32;
    u32x4 kk[U];
    int cpos[U];
    auto fetch_k = [&](int cb) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            int c = cb + u * 4 * CPW + G;
            c = c < c1 ? c : c1 - 1;
            kk[u] = *reinterpret_cast<const u32x4*>(P.kcache + (long long)c * P.kv_dim + row_off);
            cpos[u] = P.cell_pos[c];
        }
    };
    fetch_k(c0 + wave * CPW);
    float q[8];
    {
        const float4* qp = reinterpret_cast<const float4*>(P.q + (long long)h * HD + L * 8);
        const float4 a = qp[0], b = qp[1];
        const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
        for (int e = 0; e < 8; ++e) q[e] = __half2float(__float2half_rn(v[e]));
    }
    // 1. scaled KQ of the split's cells into LDS, the split's max
    float mx = -INFINITY;
    for (int cb = c0 + wave * CPW; cb < c1; cb += 4 * CPW * U) {
        if (cb != c0 + wave * CPW) fetch_k(cb);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int c = cb + u * 4 * CPW + G;
            const bool valid = c < c1 && cpos[u] <= qpos;
            const unsigned kw[4] = {kk[u].x, kk[u].y, kk[u].z, kk[u].w};
            float d = 0.0f;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                d = fmaf(q[2 * e], h2f(kw[e]), d);
                d = fmaf(q[2 * e + 1], h2f(kw[e] >> 16), d);
            }
#pragma unroll
            for (int off = LPC / 2; off > 0; off >>= 1) d += __shfl_xor(d, off, 64);
            const float w = valid ? d * P.scale : -INFINITY;
            mx = fmaxf(mx, w);
            if (L == 0 && c < c1) sw[c - c0] = w;
        }
    }
    // the V chunk a wave reads first: waves 1-3 issue it before the exchange; wave 0, which polls,
    // after it (vmcnt retires in issue order: a flag load would wait behind it)
    u32x4 vv[U];
    auto fetch_v = [&](int cb) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            int c = cb + u * 4 * CPW + G;
            c = c < c1 ? c : c1 - 1;
            vv[u] = *reinterpret_cast<const u32x4*>(P.vcache + (long long)c * P.kv_dim + row_off);
        }
    };
    mx = wave_max(mx);
    if (lane == 0) redm[wave] = mx;
    __syncthreads();
    // publish this split's value of phase ph (stored by thread 0 before), then wait for every
    // split's (wave 0); false after a timeout
    auto exchange = [&](int ph) -> bool {
        bool ok = true;
        if (wave == 0) {
            const unsigned tgt = epoch + 1u + (unsigned)ph;
            if (lane == 0) {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the value's store completed
                __hip_atomic_store(fl + s * 32, tgt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
            for (;;) {
                const unsigned f = lane < nsplit ? ld_ag(fl + lane * 32) : tgt;
                if (__all((int)(f - tgt) >= 0)) break;
                if (__builtin_amdgcn_s_memrealtime() - t0 > 200000000ull) {
                    ok = false;
                    if (lane == 0 && P.xerr) __hip_atomic_store(P.xerr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    break;
                }
            }
            asm volatile("" ::: "memory");
        }
        return ok;
    };
    if (tid == 0) {
        const float m = fmaxf(fmaxf(redm[0], redm[1]), fmaxf(redm[2], redm[3]));
        __hip_atomic_store(P.xmax + h * ATTN_SMAX + s, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (wave != 0) fetch_v(c0 + wave * CPW);
    exchange(0);
    if (wave == 0) {
        float m = lane < nsplit ? __hip_atomic_load(P.xmax + h * ATTN_SMAX + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                                : -INFINITY;
        m = wave_max(m);
        if (lane == 0) stat[0] = m;
    }
    __syncthreads();
    const float M = stat[0];
    // 2. the split's sum of expf(w - M) in double; the head's sum in split order
    double acc = 0.0;
    for (int c = c0 + tid; c < c1; c += 256) acc += (double)expf(sw[c - c0] - M);
    acc = wave_sum_d(acc);
    if (lane == 0) dred[wave] = acc;
    __syncthreads();
    if (tid == 0) {
        const double ss = ((dred[0] + dred[1]) + dred[2]) + dred[3];
        __hip_atomic_store(P.xsum + h * ATTN_SMAX + s, ss, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    exchange(1);
    if (tid == 0) {
        double v[ATTN_SMAX];
#pragma unroll
        for (int k = 0; k < ATTN_SMAX; ++k)
            v[k] = k < nsplit ? __hip_atomic_load(P.xsum + h * ATTN_SMAX + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
        double tot = 0.0;
        for (int k = 0; k < nsplit; ++k) tot += v[k];
        stat[1] = (float)(1.0 / tot);
    }
    if (wave == 0) fetch_v(c0 + wave * CPW);
    __syncthreads();
    const float inv = stat[1];
    // 3. sum over the split's cells of f16(p_c) v_c
    float o[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = 0.0f;
    for (int cb = c0 + wave * CPW; cb < c1; cb += 4 * CPW * U) {
        if (cb != c0 + wave * CPW) fetch_v(cb);
        float pw[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int c = cb + u * 4 * CPW + G;
            const bool in = c < c1;
            const float p = expf(sw[(in ? c : c1 - 1) - c0] - M) * inv;   // ggml_vec_soft_max_f32, f16 vec_dot_type
            pw[u] = in ? __half2float(__float2half_rn(p)) : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const unsigned vw[4] = {vv[u].x, vv[u].y, vv[u].z, vv[u].w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                o[2 * e] = fmaf(pw[u], h2f(vw[e]), o[2 * e]);
                o[2 * e + 1] = fmaf(pw[u], h2f(vw[e] >> 16), o[2 * e + 1]);
            }
        }
    }
#pragma unroll
    for (int off = LPC; off < 64; off <<= 1)
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] += __shfl_xor(o[e], off, 64);
    if (G == 0) {
#pragma unroll
        for (int e = 0; e < 8; ++e) red_o[wave][L * 8 + e] = o[e];
    }
    __syncthreads();
    for (int d = tid; d < HD; d += 256)
        P.part_o[((long long)s * P.n_head + h) * HD + d] = ((red_o[0][d] + red_o[1][d]) + red_o[2][d]) + red_o[3][d];
}

// Short contexts (<= ATTN_SHORT cells): the same arithmetic as the two kernels above with a
// single split, in one launch.  One workgroup per kv head keeps its scores in LDS, so no
// other workgroup's result is needed between the softmax statistics and the PV sum.
// Where the workgroup's R q heads cover whole 256-blocks of the output, it also quantises them into
// P.act_out (the WO launch's activation) or P.act_q8 (a short batch's).
// HG: groups of 4 waves per workgroup, one kv head (or, qsplit, one q head) each.  Only HG = 1 is
// instantiated (attn_fns): the geometries that needed HG > 1 to fill a 256-block, one q head per
// group of head_dim 64 / 128, are attn_dec_kernel's.  The parameter stays because without it the
// compiler knows the unit to be wave-uniform and emits other code for every instantiation.
template <int R, int LPC, int HG>
__global__ __launch_bounds__(256 * HG) void attn_fused_kernel(const AttnParams P) {
    constexpr int CPW = 64 / LPC;
    constexpr int HD = LPC * 8;
    __shared__ float sw[HG][R][ATTN_SHORT];
    __shared__ float redm[HG][4][R];
    __shared__ double dred[HG][4][R];
    __shared__ float gm[HG][R], ginv[HG][R];
    __shared__ float red_o[HG][4][R][HD];
    const int grp = (int)threadIdx.x >> 8;
    const int unit = (int)blockIdx.x * HG + grp;   // this group's kv head (qsplit: q head)
    // kv head, and the first of the R q heads this group serves (qsplit: one q head each)
    const int g = P.qsplit ? unit / P.qsplit : unit;
    const int gq = P.qsplit ? unit : unit * R;
    const int tok = blockIdx.y;   // query token (launch_attn_multi); 0 for a decode step
#ifdef MI_STAMPS
    unsigned long long* const stp = P.stamps && tok == 0 ? P.stamps + blockIdx.x * 8 : nullptr;
    if (stp && threadIdx.x == 0) stp[0] = __builtin_amdgcn_s_memrealtime();
#endif
    const int* tp = P.tokpos + 4 * tok;
    const int tp2 = tp[2], qpos = tp[1];
    const float* qrow = P.q + (long long)tok * P.n_head * HD;
    float* orow = P.part_o + (long long)tok * P.n_head * HD;
    const int tid = threadIdx.x & 255, lane = tid & 63, wave = tid >> 6;
    const int L = lane % LPC, G = lane / LPC;
    const long long row_off = (long long)g * HD + L * 8;
    constexpr int U = 4;
    // The first chunk of K, V and cell positions is fetched at entry, before the cell count
    // arrives, so the token-position, K and V round trips overlap instead of chaining.  Cells
    // past the count are clamped to the cache and masked by select below, never by arithmetic.
    // (the first TWO chunks of a wave: a decode step within 128 cells makes no dependent cache
    // round trip after entry)
    constexpr int STRIDE = 4 * CPW * U;   // cells between a wave's chunks
    u32x4 k0[U], v0[U], k1[U], v1[U];
    int cp0[U], cp1[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int c = min(wave * CPW + u * 4 * CPW + G, P.n_ctx - 1);
        const int c1 = min(wave * CPW + STRIDE + u * 4 * CPW + G, P.n_ctx - 1);
        k0[u] = *reinterpret_cast<const u32x4*>(P.kcache + (long long)c * P.kv_dim + row_off);
        v0[u] = *reinterpret_cast<const u32x4*>(P.vcache + (long long)c * P.kv_dim + row_off);
        cp0[u] = P.cell_pos[c];
        k1[u] = *reinterpret_cast<const u32x4*>(P.kcache + (long long)c1 * P.kv_dim + row_off);
        v1[u] = *reinterpret_cast<const u32x4*>(P.vcache + (long long)c1 * P.kv_dim + row_off);
        cp1[u] = P.cell_pos[c1];
    }
    const int ncell = min(tp2 + 1, ATTN_SHORT);
    float q[R][8];
#pragma unroll
    for (int t = 0; t < R; ++t) {
        const float4* qp = reinterpret_cast<const float4*>(qrow + (long long)(gq + t) * HD + L * 8);
        const float4 a = qp[0], b = qp[1];
        const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
        for (int e = 0; e < 8; ++e) q[t][e] = __half2float(__float2half_rn(v[e]));
    }
    // 1. scaled KQ of every cell into LDS, and the per-head max
    float mx[R];
#pragma unroll
    for (int t = 0; t < R; ++t) mx[t] = -INFINITY;
    for (int cb = wave * CPW; cb < ncell; cb += 4 * CPW * U) {
        u32x4 kk[U];
        int cpos[U];
        if (cb == wave * CPW) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                kk[u] = k0[u];
                cpos[u] = cp0[u];
            }
        } else if (cb == wave * CPW + STRIDE) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                kk[u] = k1[u];
                cpos[u] = cp1[u];
            }
        } else {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                int c = cb + u * 4 * CPW + G;
                c = c < ncell ? c : ncell - 1;
                kk[u] = *reinterpret_cast<const u32x4*>(P.kcache + (long long)c * P.kv_dim + row_off);
                cpos[u] = P.cell_pos[c];
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int c = cb + u * 4 * CPW + G;
            const bool valid = c < ncell && cpos[u] <= qpos;
            const unsigned kw[4] = {kk[u].x, kk[u].y, kk[u].z, kk[u].w};
            float kf[8];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                kf[2 * e] = h2f(kw[e]);
                kf[2 * e + 1] = h2f(kw[e] >> 16);
            }
#pragma unroll
            for (int t = 0; t < R; ++t) {
                float d = 0.0f;
#pragma unroll
                for (int e = 0; e < 8; ++e) d = fmaf(q[t][e], kf[e], d);
#pragma unroll
                for (int off = LPC / 2; off > 0; off >>= 1) d += __shfl_xor(d, off, 64);
                const float w = valid ? d * P.scale : -INFINITY;
                mx[t] = fmaxf(mx[t], w);
                if (L == 0 && c < ncell) sw[grp][t][c] = w;
            }
        }
    }
#pragma unroll
    for (int t = 0; t < R; ++t) {
        const float m = wave_max(mx[t]);
        if (lane == 0) redm[grp][wave][t] = m;
    }
    __syncthreads();
    // 2. sum over all cells of expf(w - max), in double, fixed order (as attn_pv_kernel)
#pragma unroll
    for (int t = 0; t < R; ++t) {
        const float M = fmaxf(fmaxf(redm[grp][0][t], redm[grp][1][t]), fmaxf(redm[grp][2][t], redm[grp][3][t]));
        double acc = 0.0;
        for (int c = tid; c < ncell; c += 256) acc += (double)expf(sw[grp][t][c] - M);
        acc = wave_sum_d(acc);
        if (lane == 0) dred[grp][wave][t] = acc;
        if (tid == 0) gm[grp][t] = M;
    }
    __syncthreads();
    if (tid < R) ginv[grp][tid] = (float)(1.0 / (((dred[grp][0][tid] + dred[grp][1][tid]) + dred[grp][2][tid]) + dred[grp][3][tid]));
    __syncthreads();
    // 3. sum_c f16(p_c) v_c
    float o[R][8];
#pragma unroll
    for (int t = 0; t < R; ++t)
#pragma unroll
        for (int e = 0; e < 8; ++e) o[t][e] = 0.0f;
    for (int cb = wave * CPW; cb < ncell; cb += 4 * CPW * U) {
        u32x4 vv[U];
        float pw[U][R];
        const bool first = cb == wave * CPW, second = cb == wave * CPW + STRIDE;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            int c = cb + u * 4 * CPW + G;
            const bool in = c < ncell;
            c = in ? c : ncell - 1;
            if (first || second) {   // prefetched at entry; a cell past the count may hold non-finite bits
                const u32x4 z = {0u, 0u, 0u, 0u};
                vv[u] = in ? (first ? v0[u] : v1[u]) : z;
            } else {
                vv[u] = *reinterpret_cast<const u32x4*>(P.vcache + (long long)c * P.kv_dim + row_off);
            }
#pragma unroll
            for (int t = 0; t < R; ++t) {
                const float p = expf(sw[grp][t][c] - gm[grp][t]) * ginv[grp][t];
                pw[u][t] = in ? __half2float(__float2half_rn(p)) : 0.0f;
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const unsigned vw[4] = {vv[u].x, vv[u].y, vv[u].z, vv[u].w};
            float vf[8];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                vf[2 * e] = h2f(vw[e]);
                vf[2 * e + 1] = h2f(vw[e] >> 16);
            }
#pragma unroll
            for (int t = 0; t < R; ++t)
#pragma unroll
                for (int e = 0; e < 8; ++e) o[t][e] = fmaf(pw[u][t], vf[e], o[t][e]);
        }
    }
#pragma unroll
    for (int t = 0; t < R; ++t)
#pragma unroll
        for (int off = LPC; off < 64; off <<= 1)
#pragma unroll
            for (int e = 0; e < 8; ++e) o[t][e] += __shfl_xor(o[t][e], off, 64);
    if (G == 0) {
#pragma unroll
        for (int t = 0; t < R; ++t)
#pragma unroll
            for (int e = 0; e < 8; ++e) red_o[grp][wave][t][L * 8 + e] = o[t][e];
    }
    __syncthreads();
    for (int i = tid; i < R * HD; i += 256) {
        const int t = i / HD, d = i % HD;
        orow[(long long)(gq + t) * HD + d] = ((red_o[grp][0][t][d] + red_o[grp][1][t][d]) + red_o[grp][2][t][d]) + red_o[grp][3][t][d];
    }
    if ((P.act_out.act && gridDim.y == 1) || P.act_q8.q) {
        // the WO launch's quantised activation: this workgroup's R * HG heads are whole 256-blocks
        // (launch_attn / launch_attn_multi check), one wave per block; element e of the workgroup's
        // span lies in group e / (R * HD), head (e / HD) % R.  A decode step writes act_layout
        // (act_out); a short batch, token blockIdx.y's row of the batch GEMMs' format (act_q8)
        constexpr int NE = HG * R * HD;
        const int e0 = (int)blockIdx.x * HG * (P.qsplit ? 1 : R) * HD;
        const int gw = (int)threadIdx.x >> 6;
        for (int b = gw; b < NE / 256; b += 4 * HG) {
            float v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int e = b * 256 + lane * 4 + k, gg = e / (R * HD), t = (e / HD) % R, d = e % HD;
                v[k] = ((red_o[gg][0][t][d] + red_o[gg][1][t][d]) + red_o[gg][2][t][d]) + red_o[gg][3][t][d];
            }
            if (P.act_q8.q) quant_actq8_block(P.act_q8, tok, e0 / 256 + b, v, lane);
            else dv_quant_block(P.act_out, e0 / 256 + b, v, lane);
        }
    }
#ifdef MI_STAMPS
    if (stp && threadIdx.x == 0) stp[4] = __builtin_amdgcn_s_memrealtime();
#endif
}

// The streaming decode step's attention (one token, contexts within ATTN_SHORT cells, the output
// quantised into P.act_out): attn_fused_kernel's arithmetic for one q head per group (R = 1: a kv
// head per group, or a q head of a GQA kv head with qsplit), with NWV waves per group -- twice the
// fused kernel's 4, so each wave walks half the cells -- and the score reductions on DPP (the
// fused kernel's ds_bpermute shuffles were one LDS round trip each).  f16(q) . k over the f16
// cache, scale, causal mask by cell position, the exact softmax (global max; the double sum of
// expf(w - max); p = f16(e * (1/sum))), sum_c f16(p_c) v_c; then whole 256-blocks of the output
// (HG groups) quantised as the WO launch's activation.
template <int CTRL, int RMASK>
__device__ __forceinline__ float dppf(float v, float old) {
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(old), __float_as_int(v), CTRL, RMASK, 0xf, false));
}
// max over the wave of any floats (-inf identity), every lane
__device__ __forceinline__ float wave_max_any(float v) {
    const float ni = -INFINITY;
    v = fmaxf(v, dppf<0x111, 0xf>(v, ni));
    v = fmaxf(v, dppf<0x112, 0xf>(v, ni));
    v = fmaxf(v, dppf<0x114, 0xf>(v, ni));
    v = fmaxf(v, dppf<0x118, 0xf>(v, ni));
    v = fmaxf(v, dppf<0x142, 0xa>(v, ni));
    v = fmaxf(v, dppf<0x143, 0xc>(v, ni));
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}
template <int LPC, int HG, int NWV>
__global__ __launch_bounds__(64 * NWV * HG) void attn_dec_kernel(const AttnParams P) {
    static_assert(LPC == 8 || LPC == 16, "head_dim 64 or 128");
    constexpr int HD = LPC * 8, CPW = 64 / LPC, NT = 64 * NWV, STEP = NWV * CPW;
    // the steps of the first 128 cells: q, then the cache rows and positions, requested at entry
    // (buffer loads parked past the descriptor for steps at or past ncell: zeros, no memory
    // access; K before V, which is needed last); past that, a loop.  The depth barely matters:
    // 1, 2, 3 and 4 steps (32-128 cells at 8 waves) measured within 0.8 % of each other, the
    // first 256 cells at entry 1-2 % slower (profiles/r06_fuse_ab.txt)
    constexpr int UM = (128 + STEP - 1) / STEP;
    __shared__ float sw[HG][ATTN_SHORT];
    __shared__ float redm[HG][NWV];
    __shared__ double dred[HG][NWV];
    __shared__ float red_o[HG][NWV][HD];
    const int grp = (int)threadIdx.x / NT;
    const int tid = (int)threadIdx.x % NT, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int unit = (int)blockIdx.x * HG + grp;   // this group's q head
    const int g = P.qsplit ? unit / P.qsplit : unit;   // its kv head
    const int L = lane % LPC, G = lane / LPC;
    const int tok = blockIdx.y;   // query token of a short batch (launch_attn_multi); 0 for a decode step
    const int tp2 = P.tokpos[4 * tok + 2], qpos = P.tokpos[4 * tok + 1];
    const int ncell = min(tp2 + 1, ATTN_SHORT);
    float q[8];
    const float* qrow = P.q + (long long)tok * P.n_head * HD;
    const f32x4 qa = gptr(reinterpret_cast<const f32x4*>(qrow + (long long)unit * HD + L * 8))[0];
    const f32x4 qb = gptr(reinterpret_cast<const f32x4*>(qrow + (long long)unit * HD + L * 8))[1];
    const __amdgpu_buffer_rsrc_t rk = __builtin_amdgcn_make_buffer_rsrc(const_cast<__half*>(rfl_ptr(P.kcache + (long long)g * HD)), 0, 0x7FFFFFFF, 0x00020000);
    const __amdgpu_buffer_rsrc_t rv = __builtin_amdgcn_make_buffer_rsrc(const_cast<__half*>(rfl_ptr(P.vcache + (long long)g * HD)), 0, 0x7FFFFFFF, 0x00020000);
    const __amdgpu_buffer_rsrc_t rc = __builtin_amdgcn_make_buffer_rsrc(const_cast<int*>(P.cell_pos), 0, 0x7FFFFFFF, 0x00020000);
    u32x4 k0[UM], v0[UM];
    int cp0[UM];
    unsigned ko[UM];
#pragma unroll
    for (int u = 0; u < UM; ++u) {
        const bool park = wave * CPW + u * STEP >= ncell;
        const unsigned c = (unsigned)min(wave * CPW + u * STEP + G, ncell - 1);
        ko[u] = oob((c * (unsigned)P.kv_dim + (unsigned)L * 8u) * 2u, park);
        k0[u] = __builtin_amdgcn_raw_buffer_load_b128(rk, ko[u], 0, 0);
        cp0[u] = (int)__builtin_amdgcn_raw_buffer_load_b32(rc, oob(c * 4u, park), 0, 0);
    }
#pragma unroll
    for (int u = 0; u < UM; ++u) v0[u] = __builtin_amdgcn_raw_buffer_load_b128(rv, ko[u], 0, 0);
    {
        const float t[8] = {qa.x, qa.y, qa.z, qa.w, qb.x, qb.y, qb.z, qb.w};
#pragma unroll
        for (int e = 0; e < 8; ++e) q[e] = __half2float(__float2half_rn(t[e]));
    }
    auto cvt8 = [](const u32x4& w, float (&f)[8]) {
        const unsigned ww[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            f[2 * e] = h2f(ww[e]);
            f[2 * e + 1] = h2f(ww[e] >> 16);
        }
    };
    // 1. scaled KQ of every cell into LDS (lane L == 0 of each cell's group), the wave's maximum
    float mx = -INFINITY;
    auto score = [&](int c, const u32x4& kk, int cp) {
        float kf[8];
        cvt8(kk, kf);
        float d = 0.0f;
#pragma unroll
        for (int e = 0; e < 8; ++e) d = fmaf(q[e], kf[e], d);
        d += dppf<0xB1, 0xf>(d, 0.0f);    // quad_perm [1,0,3,2]
        d += dppf<0x4E, 0xf>(d, 0.0f);    // quad_perm [2,3,0,1]: every lane its quad's sum
        d += dppf<0x141, 0xf>(d, 0.0f);   // row_half_mirror: the 8-lane group's sum
        if (LPC == 16) d += dppf<0x140, 0xf>(d, 0.0f);   // row_mirror: the 16-lane row's
        const bool valid = c < ncell && cp <= qpos;
        const float w = valid ? d * P.scale : -INFINITY;
        mx = fmaxf(mx, w);
        if (L == 0 && c < ncell) sw[grp][c] = w;
    };
#pragma unroll
    for (int u = 0; u < UM; ++u) {
        const int c = wave * CPW + u * STEP + G;
        if (wave * CPW + u * STEP < ncell) score(c, k0[u], cp0[u]);
    }
    for (int cb = wave * CPW + UM * STEP; cb < ncell; cb += STEP) {
        const int c = min(cb + G, ncell - 1);
        const u32x4 kk = *gptr(reinterpret_cast<const u32x4*>(P.kcache + (long long)c * P.kv_dim + (long long)g * HD + L * 8));
        const int cp = gptr(P.cell_pos)[c];
        score(cb + G, kk, cp);
    }
    const float wm = wave_max_any(mx);
    if (lane == 0) redm[grp][wave] = wm;
    __syncthreads();
    float M = redm[grp][0];
#pragma unroll
    for (int w = 1; w < NWV; ++w) M = fmaxf(M, redm[grp][w]);
    // 2. sum over every cell of expf(w - M) in double, fixed order (a cell per thread, waves in order)
    {
        double acc = 0.0;
        for (int c = tid; c < ncell; c += NT) acc += (double)expf(sw[grp][c] - M);
        acc = wave_sum63_d(acc);
        if (lane == 63) dred[grp][wave] = acc;
    }
    __syncthreads();
    double tot = 0.0;
#pragma unroll
    for (int w = 0; w < NWV; ++w) tot += dred[grp][w];
    const float inv = (float)(1.0 / tot);
    // 3. sum_c f16(p_c) v_c over the wave's cells, then the wave's cell groups, then the waves in order
    float o[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = 0.0f;
    auto pv = [&](int c, const u32x4& vv) {
        float vf[8];
        cvt8(vv, vf);
        const bool in = c < ncell;
        const float p = expf(sw[grp][in ? c : 0] - M) * inv;   // ggml_vec_soft_max_f32, f16 vec_dot_type
        const float pw = in ? __half2float(__float2half_rn(p)) : 0.0f;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = fmaf(pw, vf[e], o[e]);
    };
#pragma unroll
    for (int u = 0; u < UM; ++u) {
        const int c = wave * CPW + u * STEP + G;
        if (wave * CPW + u * STEP < ncell) pv(c, v0[u]);
    }
    for (int cb = wave * CPW + UM * STEP; cb < ncell; cb += STEP) {
        const int c = min(cb + G, ncell - 1);
        const u32x4 vv = *gptr(reinterpret_cast<const u32x4*>(P.vcache + (long long)c * P.kv_dim + (long long)g * HD + L * 8));
        pv(cb + G, vv);
    }
#pragma unroll
    for (int off = LPC; off < 64; off <<= 1)
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] += __shfl_xor(o[e], off, 64);
    if (G == 0) {
#pragma unroll
        for (int e = 0; e < 8; ++e) red_o[grp][wave][L * 8 + e] = o[e];
    }
    __syncthreads();
    // (the fp32 output is stored only on request, out_f32 below: the streaming WO launch reads the
    // quantised one)
    // the WO launch's quantised activation: the workgroup's HG heads are whole 256-blocks, one
    // wave per block; element e of the workgroup's span is head e / HD, dim e % HD
    constexpr int NE = HG * HD;
    const int gw = (int)threadIdx.x >> 6;
    const int e0 = (int)blockIdx.x * NE;
    for (int b = gw; b < NE / 256; b += HG * NWV) {
        float v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int e = b * 256 + lane * 4 + k, gg = e / HD, d = e % HD;
            float s = red_o[gg][0][d];
#pragma unroll
            for (int w = 1; w < NWV; ++w) s += red_o[gg][w][d];
            v[k] = s;
        }
        if (P.out_f32) {   // (uniform) a LoRA adapter on attn_output reads the fp32 row
            float* of = P.out_f32 + (long long)tok * P.n_head * HD + e0 + b * 256 + lane * 4;
#pragma unroll
            for (int k = 0; k < 4; ++k) of[k] = v[k];
        }
        if (P.act_q8.q) quant_actq8_block(P.act_q8, tok, e0 / 256 + b, v, lane);   // a short batch's WO input
        else dv_quant_block(P.act_out, e0 / 256 + b, v, lane);
    }
}

// ---------------------------------------------------------------------------
// Where an attention launch is chosen.  attn_plan is a pure function of the mode and the head
// geometry (no device, no pointers; mi_op_attn_plan shows it to the tests); attn_fns is the one
// table from a plan to the instantiated kernels; the launchers derive the mode from AttnParams,
// ask for the plan and launch it.
// ---------------------------------------------------------------------------
AttnPlan attn_plan(AttnMode mode, int n_head, int n_head_kv, int head_dim, int n_ctx, int ntok, bool long_ok) {
    const AttnPlan none{AK_NONE, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (n_head_kv <= 0 || n_head % n_head_kv) return none;
    const int r = n_head / n_head_kv;
    if (r != 1 && r != 2 && r != 4 && r != 8) return none;
    if (head_dim != 32 && head_dim != 64 && head_dim != 128 && head_dim != 256) return none;
    const bool batch = mode == ATTN_BATCH_QUANT || mode == ATTN_BATCH_FUSED;
    // few kv heads: a workgroup (the decode kernel: a group) per q head, on the R = 1 kernels.
    // A short batch's non-quantising launch never does this: it is the v_dot4 / tiled fallback's
    // form, kept as it is.
    const bool qs = r > 1 && n_head_kv < 16 && mode != ATTN_BATCH_FUSED;
    AttnPlan k{AK_FUSED, qs ? 1 : r, head_dim / 8, 1, 4, qs ? n_head : n_head_kv, batch ? ntok : 1, 256, 0, qs ? r : 0};
    if (mode == ATTN_DECODE_QUANT || mode == ATTN_BATCH_QUANT) {
        // the output also quantised: a workgroup serves whole 256-blocks of it, HG groups of R q
        // heads (R * head_dim is a power of two)
        const int per = k.R * head_dim;
        k.HG = per >= 256 ? 1 : 256 / per;
        if (k.grid_x % k.HG) return none;
        // one q head per group of head_dim 64 / 128: the decode kernel, 4-8 waves per group; also a
        // short batch's, one grid row per token (20 / 64 claimed tokens 3.38 / 5.15 -> 3.36 / 5.09 ms
        // against the fused kernel, profiles/r06_short_attn_ab.txt)
        if (k.R == 1 && (head_dim == 64 || head_dim == 128)) {
            k.kernel = AK_DEC;
            k.NWV = head_dim == 128 ? 8 : 4;
        } else if (k.HG > 1 || qs) {
            return none;   // the fused kernel's workgroup is one group, the R q heads of one kv head
        }
        k.grid_x /= k.HG;
        k.block = 64 * k.NWV * k.HG;
    } else if (mode == ATTN_DECODE_SPLIT) {
        k.grid_y = ATTN_SMAX;
        k.kernel = AK_SCORES_PV;
        if (long_ok && (head_dim == 64 || head_dim == 128)) {
            // one launch, a workgroup per q head and split, the splits exchanging their softmax
            // statistics; the split's scores in LDS
            k = AttnPlan{AK_LONG, 1, head_dim / 8, 1, 4, n_head, ATTN_SMAX, 256, 0, 0};
            k.lds = (size_t)std::max(64, ((n_ctx + ATTN_SMAX - 1) / ATTN_SMAX + 63) / 64 * 64) * sizeof(float);
        }
    }
    return k;
}

typedef void (*AttnFn)(const AttnParams);
struct AttnFns {
    AttnFn a, b;   // b: the pv launch that follows the scores launch (AK_SCORES_PV)
};
template <int R, int LPC>
static AttnFns attn_fns_rl(AttnKernel k) {
    if (k == AK_FUSED) return {attn_fused_kernel<R, LPC, 1>, nullptr};
    // the split kernels issue the cache loads of 4 cell steps per wave together (8: no faster, r03)
    return {attn_scores_kernel<R, LPC, 4>, attn_pv_kernel<R, LPC, 4>};
}
template <int R>
static AttnFns attn_fns_r(const AttnPlan& k) {
    switch (k.LPC) {
    case 4: return attn_fns_rl<R, 4>(k.kernel);
    case 8: return attn_fns_rl<R, 8>(k.kernel);
    case 16: return attn_fns_rl<R, 16>(k.kernel);
    case 32: return attn_fns_rl<R, 32>(k.kernel);
    default: return {nullptr, nullptr};
    }
}
// the only place a kernel of the family is instantiated
static AttnFns attn_fns(const AttnPlan& k) {
    switch (k.kernel) {
    case AK_DEC: return {k.LPC == 16 ? attn_dec_kernel<16, 2, 8> : attn_dec_kernel<8, 4, 4>, nullptr};
    case AK_LONG: return {k.LPC == 16 ? attn_long_kernel<16> : attn_long_kernel<8>, nullptr};
    case AK_FUSED:
    case AK_SCORES_PV:
        switch (k.R) {
        case 1: return attn_fns_r<1>(k);
        case 2: return attn_fns_r<2>(k);
        case 4: return attn_fns_r<4>(k);
        case 8: return attn_fns_r<8>(k);
        default: return {nullptr, nullptr};
        }
    default: return {nullptr, nullptr};
    }
}

// Can `need` workgroups of attn_long_kernel (256 threads, `lds` dynamic LDS) be resident on the
// current device at once?  The splits of a head spin on each other, so they all must be.
static bool attn_long_resident(const void* fn, size_t lds, long long need) {
    int dev = 0, cus = 0, per_cu = 0;
    if (hipGetDevice(&dev) != hipSuccess) return false;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return false;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, 256, lds) != hipSuccess) return false;
    return (long long)per_cu * cus >= need;
}

static void attn_launch(const AttnPlan& k, AttnParams p, hipStream_t s) {
    const AttnFns f = attn_fns(k);
    p.qsplit = k.qsplit;
    hipLaunchKernelGGL(f.a, dim3(k.grid_x, k.grid_y), dim3(k.block), k.lds, s, p);
    MI_HIP(hipGetLastError());
    if (!f.b) return;
    hipLaunchKernelGGL(f.b, dim3(k.grid_x, k.grid_y), dim3(k.block), k.lds, s, p);
    MI_HIP(hipGetLastError());
}

bool attn_quant_supported(int n_head, int n_head_kv, int head_dim) {
    return attn_plan(ATTN_DECODE_QUANT, n_head, n_head_kv, head_dim, 0, 1, false).kernel != AK_NONE;
}

void launch_attn(const AttnParams& p, hipStream_t s) {
    if (p.n_head % p.n_head_kv) throw Error("attn: n_head must be a multiple of n_head_kv");
    // fused: the caller guarantees <= ATTN_SHORT cells (the kernels clamp anyway); with act_out the
    // streaming decode step, the output also quantised
    const AttnMode mode = !p.fused ? ATTN_DECODE_SPLIT : p.act_out.act ? ATTN_DECODE_QUANT : ATTN_DECODE_FUSED;
    auto plan = [&](AttnMode m, bool long_ok) {
        return attn_plan(m, p.n_head, p.n_head_kv, p.head_dim, p.n_ctx, 1, long_ok);
    };
    AttnPlan k = plan(mode, p.xflags && p.step && !p.long_off);
    if (k.kernel == AK_NONE && (mode != ATTN_DECODE_QUANT || plan(ATTN_DECODE_FUSED, false).kernel == AK_NONE))
        throw Error("attn: unsupported head_dim / GQA ratio (head_dim 32..256, ratio 1/2/4/8)");
    if (mode == ATTN_DECODE_QUANT && (k.kernel == AK_NONE || p.act_out.K != p.n_head * p.head_dim))
        throw Error("attn: no quantising decode kernel for this head geometry");
    if (k.kernel == AK_LONG &&
        !(k.lds <= 64 * 1024 && attn_long_resident(reinterpret_cast<const void*>(attn_fns(k).a), k.lds,
                                                   (long long)p.n_head * ATTN_SMAX * std::max(1, p.long_share))))
        k = plan(mode, false);   // the two launches
    attn_launch(k, p, s);
}

void launch_attn_multi(const AttnParams& p_in, int ntok, float* out, hipStream_t s) {
    AttnParams p = p_in;
    p.part_o = out;
    p.fused = 1;
    if (ntok < 1) return;
    // act_q8: each token's output also quantised (a short batch's WO input): the decode step's
    // quantising geometry, one grid row per token
    const AttnMode mode = p.act_q8.q ? ATTN_BATCH_QUANT : ATTN_BATCH_FUSED;
    const AttnPlan k = attn_plan(mode, p.n_head, p.n_head_kv, p.head_dim, p.n_ctx, ntok, false);
    if (mode == ATTN_BATCH_QUANT && (k.kernel == AK_NONE || p.act_q8.K != p.n_head * p.head_dim || p.act_q8.ntok != ntok))
        throw Error("attn: no quantising batch kernel for this head geometry");
    if (k.kernel == AK_NONE) throw Error("attn: unsupported head_dim / GQA ratio");
    attn_launch(k, p, s);
}

// Stand-alone combine (same arithmetic as the PRO_ATTN prologue).
__global__ void attn_combine_kernel(const AttnPartials A, const int* tokpos, float* out) {
    int chunk, nsplit;
    attn_split(tokpos[2] + 1, chunk, nsplit);
    const int h = blockIdx.x;
    for (int d = threadIdx.x; d < A.head_dim; d += blockDim.x) {
        float acc = 0.0f;
        for (int s = 0; s < nsplit; ++s) acc += A.o[((long long)s * A.n_head + h) * A.head_dim + d];
        out[h * A.head_dim + d] = acc;
    }
}

// one wave per 256-block of the output: its 4 elements per lane summed over the splits in split
// order (split 0 first, then += 1, 2, ..), then dv_quant_block
__global__ __launch_bounds__(64) void attn_combine_quant_kernel(const AttnPartials A, const int* tokpos, const ActOut t) {
    int chunk, nsplit;
    attn_split(tokpos[2] + 1, chunk, nsplit);
    const int b = blockIdx.x, lane = threadIdx.x;
    const long long stride = (long long)A.n_head * A.head_dim;
    const f32x4* o = reinterpret_cast<const f32x4*>(A.o);
    f32x4 v = o[b * 64 + lane];
    for (int s0 = 1; s0 < nsplit; s0 += 4) {   // four splits' loads in flight, added in order
        f32x4 t4[4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (s0 + j < nsplit) t4[j] = o[(s0 + j) * stride / 4 + b * 64 + lane];
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (s0 + j < nsplit) {
                v.x += t4[j].x;
                v.y += t4[j].y;
                v.z += t4[j].z;
                v.w += t4[j].w;
            }
    }
    const float q[4] = {v.x, v.y, v.z, v.w};
    dv_quant_block(t, b, q, lane);
}

void launch_attn_combine_quant(const AttnPartials& a, const int* tokpos, const ActOut& t, hipStream_t s) {
    if (t.K != a.n_head * a.head_dim || t.K % 256 || !t.act || t.norm_w) throw Error("attn combine: bad activation");
    hipLaunchKernelGGL(attn_combine_quant_kernel, dim3(t.K / 256), dim3(64), 0, s, a, tokpos, t);
    MI_HIP(hipGetLastError());
}

void launch_attn_combine(const AttnPartials& a, const int* tokpos, float* out, hipStream_t s) {
    hipLaunchKernelGGL(attn_combine_kernel, dim3(a.n_head), dim3(128), 0, s, a, tokpos, out);
    MI_HIP(hipGetLastError());
}

}  // namespace mi
