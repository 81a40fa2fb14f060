// The kernels that run BETWEEN the batch GEMMs of a prompt batch or a verification batch:
//   quant_act_kernel   f32 rows -> Q8_K / Q8_0 activations in MFMA-fragment order (optionally after
//                      RMSNorm / LayerNorm, after adding a split-K GEMM's parts into the residual, or
//                      as silu(gate) * up of a pair launch's parts): the A operand of mmq.hip / mmqs.hip
//   rope_table_kernel  the batch's (cos, sin) table the GEMM epilogues and qkv_finish_kernel read
//   qkv_finish_kernel  Q / K / V from the parts of a short batch's GEMMs: RoPE, the KV append
//   part_sum_kernel    the sum of a short batch's parts (the output head, the last residual, SwiGLU)
// Every sum of parts is taken in part order ((p0 + p1) + ...), so a consumer's value does not depend
// on how the producer's grid was scheduled.  The arithmetic contract is mmq_common.h's.
#include "mmq_common.h"

namespace mi {
namespace mmq {

// ---------------------------------------------------------------------------
// Activation rows -> Q8_K (quantize_row_q8_K_ref), one workgroup per token row.
// Writes q in MFMA-fragment order (below), d transposed [nb][npad] (4 consecutive tokens = one
// 16-B load in the GEMM), and per superblock the 8 sub-block bsums split as 64*hi + lo (hi = floor(b/64),
// lo in 0..63): bytes 0-7 hi_j, 8-15 lo_j -- the int8 A operand of the MFMA that forms
// sum_j m_j*bsum_j = 64*sum m_j hi_j + sum m_j lo_j exactly.  Rows ntok..npad-1 are zero.
// ---------------------------------------------------------------------------
// QA_W waves per token row (16: one 256-element block each at K = 4096); XR blocks per wave at
// most (the host picks the smallest that covers K: fewer predicated copies, fewer registers)
// LN: the LayerNorm instantiation (GPT-2; norm_w and norm_b set): layer_norm(x) * norm_w + norm_b as
// gemv.hip's PRO_LAYERNORM prologue forms it (ggml_compute_forward_norm_f32: the sum and the sum of
// the f32 squares of (x - mean) in double, mean and variance in float), so a row's quantised
// activation is the decode step's.  The RMSNorm instantiations carry no trace of it.
template <int QA_W, int XR, bool LN>
__global__ __launch_bounds__(64 * QA_W) void quant_act_kernel(const float* x, int x_stride, const float* norm_w,
                                                        float eps, ActQ8 a, const int* rows, const float* part, int nks,
                                                        int swiglu, const float* addend, const float* norm_b) {
    const int t = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nb = a.K >> 8;
    // this wave's blocks: w0, w0 + bst, ... (gridDim.y > 1, rows without a norm: the row's blocks
    // spread over gridDim.y workgroups)
    const int w0 = (int)blockIdx.y * QA_W + wave, bst = QA_W * (int)gridDim.y;
    __shared__ double red[LN ? 2 * QA_W : QA_W];
    // MFMA-fragment order (one wave load = 1 KiB contiguous): q [tile][sb][j][h*32 + t%32][16 B],
    // element 32j + 16h + e of superblock sb of token t at byte e; bsb [tile][sb][t%32][16 B]
    const int tile = t >> 5, tr = t & 31;
    const int fj = lane >> 3, fh = (lane >> 2) & 1, fw = lane & 3;   // this lane's 4 elements
    int8_t* q = a.q + (long long)tile * nb * 8192 + fj * 1024 + (fh * 32 + tr) * 16 + 4 * fw;
    int8_t* bsb = a.q80 ? nullptr : a.bsb + ((long long)tile * nb * 32 + tr) * 16;
    if (t >= a.ntok || (rows && rows[t] < 0)) {   // padding rows (and MoE group padding) are zero
        for (int blk = w0; blk < nb; blk += bst) {
            *reinterpret_cast<int*>(q + blk * 8192) = 0;
            if (!a.q80 && lane < 4) reinterpret_cast<int*>(bsb + blk * 512)[lane] = 0;
            if (a.q80 && lane < 8) a.dT[(long long)(blk * 8 + lane) * a.npad + t] = 0.0f;
            if (!a.q80 && lane == 0) a.dT[(long long)blk * a.npad + t] = 0.0f;
        }
        return;
    }
    const f32x4* x4 = x ? reinterpret_cast<const f32x4*>(x + (long long)(rows ? rows[t] : t) * x_stride) : nullptr;
    // this wave's blocks read once, kept for the quantisation
    f32x4 xr[XR];
    if (swiglu) {   // silu(g) * u of the pair launch's parts: g = ((g0 + g1) + ...), u likewise
        const f32x4* p4 = reinterpret_cast<const f32x4*>(part + (long long)t * 2 * a.K);
        const long long kst = (long long)a.ntok * 2 * a.K / 4;   // one part, in f32x4
#pragma unroll
        for (int i = 0; i < XR; ++i) {
            const int blk = w0 + bst * i;
            if (blk < nb) {
                const f32x4 g = sum_parts(p4 + blk * 64 + lane, kst, nks);
                const f32x4 u = sum_parts(p4 + a.K / 4 + blk * 64 + lane, kst, nks);
                xr[i] = f32x4{silu(g.x) * u.x, silu(g.y) * u.y, silu(g.z) * u.z, silu(g.w) * u.w};
            }
            asm volatile("" ::: "memory");   // one block's part loads in flight at a time (registers)
        }
    } else {
#pragma unroll
        for (int i = 0; i < XR; ++i)
            if (w0 + bst * i < nb) xr[i] = x4[(w0 + bst * i) * 64 + lane];
    }
    if (part && !swiglu) {   // the split-K GEMM's nks partials: x = (((p0 + p1) + p2) + ...) + x (EPI_ADD's o + resid), written back
        f32x4* xw = reinterpret_cast<f32x4*>(const_cast<float*>(x) + (long long)t * x_stride);
#pragma unroll
        for (int i = 0; i < XR; ++i) {
            const int blk = w0 + bst * i;
            if (blk < nb) {
                const f32x4 acc = sum_parts(reinterpret_cast<const f32x4*>(part + (long long)t * a.K) + blk * 64 + lane,
                                            (long long)a.ntok * a.K / 4, nks);
                xr[i] = f32x4{acc.x + xr[i].x, acc.y + xr[i].y, acc.z + xr[i].z, acc.w + xr[i].w};
                if (addend) {   // the parts closed a layer's FFN: its control-vector direction, after the residual
                    const f32x4 v = reinterpret_cast<const f32x4*>(addend)[blk * 64 + lane];
                    xr[i] = f32x4{xr[i].x + v.x, xr[i].y + v.y, xr[i].z + v.z, xr[i].w + v.w};
                }
                xw[blk * 64 + lane] = xr[i];
            }
            asm volatile("" ::: "memory");   // one block's part loads in flight at a time (registers)
        }
    }
    float scale = 1.0f, mean = 0.0f;
    if constexpr (LN) {
        double sacc = 0.0;
#pragma unroll
        for (int i = 0; i < XR; ++i) {
            if (w0 + bst * i < nb) {
                const f32x4 v = xr[i];
                sacc += (double)v.x;
                sacc += (double)v.y;
                sacc += (double)v.z;
                sacc += (double)v.w;
            }
        }
        sacc = wave_sum63_d(sacc);
        if (lane == 63) red[wave] = sacc;
        __syncthreads();
        double tot = 0.0;
#pragma unroll
        for (int k = 0; k < QA_W; ++k) tot += red[k];
        mean = (float)(tot / (double)a.K);
        double s2 = 0.0;
#pragma unroll
        for (int i = 0; i < XR; ++i) {
            if (w0 + bst * i < nb) {
                const f32x4 v = xr[i];
                const float v0 = v.x - mean, v1 = v.y - mean, v2 = v.z - mean, v3 = v.w - mean;
                s2 += (double)(v0 * v0);
                s2 += (double)(v1 * v1);
                s2 += (double)(v2 * v2);
                s2 += (double)(v3 * v3);
            }
        }
        s2 = wave_sum63_d(s2);
        if (lane == 63) red[QA_W + wave] = s2;
        __syncthreads();
        double tot2 = 0.0;
#pragma unroll
        for (int k = 0; k < QA_W; ++k) tot2 += red[QA_W + k];
        scale = 1.0f / sqrtf((float)(tot2 / (double)a.K) + eps);
    } else if (norm_w) {   // ggml_compute_forward_rms_norm_f32: sum of squares in double
        double sacc = 0.0;
#pragma unroll
        for (int i = 0; i < XR; ++i) {
            if (w0 + bst * i < nb) {
                const f32x4 v = xr[i];
                sacc += (double)(v.x * v.x);
                sacc += (double)(v.y * v.y);
                sacc += (double)(v.z * v.z);
                sacc += (double)(v.w * v.w);
            }
        }
        sacc = wave_sum63_d(sacc);
        if (lane == 63) red[wave] = sacc;
        __syncthreads();
        double tot = 0.0;
#pragma unroll
        for (int k = 0; k < QA_W; ++k) tot += red[k];
        scale = 1.0f / sqrtf((float)(tot / (double)a.K) + eps);
    }
    const f32x4* w4 = reinterpret_cast<const f32x4*>(norm_w);
#pragma unroll
    for (int i = 0; i < XR; ++i) {
        const int blk = w0 + bst * i;
        if (blk >= nb) break;
        const f32x4 xv = xr[i];
        float v[4] = {xv.x, xv.y, xv.z, xv.w};
        if constexpr (LN) {   // (x - mean) * scale, then ggml_mul, ggml_add
            const f32x4 w = w4[blk * 64 + lane];
            const f32x4 b = reinterpret_cast<const f32x4*>(norm_b)[blk * 64 + lane];
            v[0] = ((v[0] - mean) * scale) * w.x + b.x;
            v[1] = ((v[1] - mean) * scale) * w.y + b.y;
            v[2] = ((v[2] - mean) * scale) * w.z + b.z;
            v[3] = ((v[3] - mean) * scale) * w.w + b.w;
        } else if (norm_w) {
            const f32x4 w = w4[blk * 64 + lane];
            v[0] = (v[0] * scale) * w.x;   // ggml_vec_scale_f32, then ggml_mul
            v[1] = (v[1] * scale) * w.y;
            v[2] = (v[2] * scale) * w.z;
            v[3] = (v[3] * scale) * w.w;
        }
        if (a.q80) {   // quantize_row_q8_0 (x86 SIMD form): per 32 elements = 8 lanes
            float am = fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fmaxf(fabsf(v[2]), fabsf(v[3])));
            am = fmaxf(am, __int_as_float(dpp_i<0xB1, 0xf>(__float_as_int(am))));
            am = fmaxf(am, __int_as_float(dpp_i<0x4E, 0xf>(__float_as_int(am))));
            am = fmaxf(am, __int_as_float(dpp_i<0x141, 0xf>(__float_as_int(am))));   // row_half_mirror
            const float d0 = am / 127.0f;
            const float id = am != 0.0f ? 127.0f / am : 0.0f;
            int qz[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) qz[k] = (int)rintf(v[k] * id);
            *reinterpret_cast<int*>(q + blk * 8192) =
                (qz[0] & 0xFF) | ((qz[1] & 0xFF) << 8) | ((qz[2] & 0xFF) << 16) | ((qz[3] & 0xFF) << 24);
            if ((lane & 7) == 0) a.dT[(long long)(blk * 8 + (lane >> 3)) * a.npad + t] = __half2float(__float2half_rn(d0));
            continue;
        }
        const float a0 = fabsf(v[0]), a1 = fabsf(v[1]), a2 = fabsf(v[2]), a3 = fabsf(v[3]);
        const float amax = wave_max_pos(fmaxf(fmaxf(a0, a1), fmaxf(a2, a3)));
        int qv[4];
        float d;
        if (amax == 0.0f) {
            qv[0] = qv[1] = qv[2] = qv[3] = 0;
            d = 0.0f;
        } else {   // max = the signed value at the FIRST index whose |x| is the maximum
            const int e = a0 == amax ? 0 : a1 == amax ? 1 : a2 == amax ? 2 : a3 == amax ? 3 : 4;
            const float mine = e == 0 ? v[0] : e == 1 ? v[1] : e == 2 ? v[2] : v[3];
            const unsigned long long m = __ballot(e < 4);
            const int src = __builtin_ctzll(m);
            const float mx = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(mine), src));
            const float iscale = -127.0f / mx;
#pragma unroll
            for (int k = 0; k < 4; ++k) qv[k] = min(127, (int)rintf(iscale * v[k]));
            d = 1.0f / iscale;
        }
        *reinterpret_cast<int*>(q + blk * 8192) =
            (qv[0] & 0xFF) | ((qv[1] & 0xFF) << 8) | ((qv[2] & 0xFF) << 16) | ((qv[3] & 0xFF) << 24);
        // the 32-element sub-block sums: lanes 8j..8j+7
        int sm = (qv[0] + qv[1]) + (qv[2] + qv[3]);
        sm += dpp_i<0xB1, 0xf>(sm);    // quad_perm [1,0,3,2]
        sm += dpp_i<0x4E, 0xf>(sm);    // quad_perm [2,3,0,1]
        sm += __shfl_xor(sm, 4, 64);   // the two quads of a sub-block
        if ((lane & 7) == 0) {
            const int j = lane >> 3;
            bsb[blk * 512 + j] = (int8_t)(sm >> 6);          // floor(b/64), -64..63
            bsb[blk * 512 + 8 + j] = (int8_t)(sm & 63);      // b - 64*floor(b/64), 0..63
        }
        if (lane == 0) a.dT[(long long)blk * a.npad + t] = d;
    }
}

// ggml_rope_cache_init (rope NORM) for every token of the batch: theta iterated from the
// position as the CPU does, table [ntok][n_rot/2] of (cos, sin).
__global__ void rope_table_kernel(const int* tokpos, int ntok, int n_rot, float theta_scale, float freq_scale,
                                  const float* freq_factors, float2* out) {
    const int t = blockIdx.x;
    if (t >= ntok) return;
    const int pos = tokpos[t * 4 + 1];
    for (int i = threadIdx.x; i < n_rot / 2; i += blockDim.x) {
        float theta = (float)pos;
        for (int k = 0; k < i; ++k) theta = theta * theta_scale;
        const float ff = freq_factors ? freq_factors[i] : 1.0f;
        const float th = freq_scale * (theta / ff);
        out[(long long)t * (n_rot / 2) + i] = make_float2(cosf(th), sinf(th));
    }
}

// the sum of the K-parts in part order, with the consumer's epilogue: Q / K RoPE (ggml NORM, the
// rope table of the batch), Q to q, K / V to the f16 caches (and the cell positions)
__global__ __launch_bounds__(256) void qkv_finish_kernel(const QkvFinish F) {
    const int t = blockIdx.y;
    const int pr = blockIdx.x * 256 + threadIdx.x;   // row pair
    const int r = 2 * pr;
    if (r >= F.nq + F.nk + F.nv) return;
    const float2* p = reinterpret_cast<const float2*>(F.part + (long long)t * F.pstride + r);
    const float2 v = sum_parts(p, (long long)F.ntok * F.pstride / 2, F.kp);   // (pstride even: nq, nk, nv are)
    const float v0 = v.x, v1 = v.y;
    const int seg = r < F.nq ? 0 : r < F.nq + F.nk ? 1 : 2;
    const int row = seg == 0 ? r : seg == 1 ? r - F.nq : r - F.nq - F.nk;
    float o0 = v0, o1 = v1;
    if (seg < 2) {
        const int i0 = row % F.head_dim;
        if (i0 < F.n_rot) {   // mmq_epilogue's expressions: even v cos - pv sin, odd pv sin + v cos
            const float2 cs = F.rope[(long long)t * (F.n_rot / 2) + i0 / 2];
            o0 = v0 * cs.x - v1 * cs.y;
            o1 = v0 * cs.y + v1 * cs.x;
        }
    }
    const int* tp = F.tokpos + t * 4;
    if (seg == 0) {
        F.q[(long long)t * F.q_stride + row] = o0;
        F.q[(long long)t * F.q_stride + row + 1] = o1;
    } else {
        __half* c = (seg == 1 ? F.kcache : F.vcache) + (long long)tp[2] * F.kv_dim + row;
        c[0] = __float2half_rn(o0);
        c[1] = __float2half_rn(o1);
        if (seg == 1 && row == 0) F.cell_pos[tp[2]] = tp[1];
    }
}

// out[t][r] = ((p0 + p1) + ...) [+ resid[t][r]]; swiglu > 0: silu(sum of row r) * (sum of row
// swiglu + r) (a pair launch's gate and up rows)
__global__ __launch_bounds__(256) void part_sum_kernel(const float* part, int kp, int ntok, int rows, int pstride,
                                                       const float* resid, int rstride, float* out, int ostride,
                                                       int swiglu, const float* addend) {
    const int t = blockIdx.y;
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    float acc = sum_parts(part + (long long)t * pstride + r, (long long)ntok * pstride, kp);
    if (swiglu) acc = silu(acc) * sum_parts(part + (long long)t * pstride + swiglu + r, (long long)ntok * pstride, kp);
    if (resid) acc = acc + resid[(long long)t * rstride + r];
    if (addend) acc = acc + addend[r];
    out[(long long)t * ostride + r] = acc;
}

}  // namespace mmq

void launch_quant_act(const QuantAct& q, const ActQ8& a, hipStream_t s) {
    const float *x = q.x, *norm_w = q.norm_w, *norm_b = q.norm_b, *part = q.part, *addend = q.addend;
    const int x_stride = q.x_stride, swiglu = q.swiglu;
    const int* rows = q.rows;
    const int nks = part ? q.nks : 0;   // (the kernels read it only with part)
    const float eps = q.eps;
    if (addend && (!part || swiglu)) throw Error("quant_act: an addend goes with the residual's split-K partials");
    if (norm_b && !norm_w) throw Error("quant_act: a LayerNorm bias goes with the norm weight");
    if (part && (nks < 1 || nks > 64)) throw Error("quant_act: 1..64 split-K partials");
    // (swiglu with rows: the MoE rows of a grouped pair launch, rows[t] < 0 marking padding rows)
    if (swiglu && (!part || norm_w)) throw Error("quant_act: swiglu takes a pair launch's parts, no norm");
    if (!swiglu && !x) throw Error("quant_act: no input rows");
    if (a.K % 256) throw Error("quant_act: K must be a multiple of 256");
    if (part && !swiglu && (rows || x_stride != a.K)) throw Error("quant_act: split-K partials take a dense [ntok][K] x");
    // (more than UB_MAX rows only for the MoE rows of a batch: one per (token, slot), padded)
    if (a.npad % 32 || a.ntok > a.npad || a.npad > 4 * UB_MAX) throw Error("quant_act: bad token count");
    if (a.K > 65536) throw Error("quant_act: K past 65536");
    // a row without a norm needs no row-wide sum: its blocks go to ceil(nb / 16) workgroups, one
    // block per wave (the FFN down input: 3 at n_ff = 11008)
    const int nb = a.K / 256;
    const int ny = norm_w ? 1 : (nb + 15) / 16;
    const int xr = (nb + 16 * ny - 1) / (16 * ny);
    auto f = xr <= 1 ? mmq::quant_act_kernel<16, 1, false> : xr <= 2 ? mmq::quant_act_kernel<16, 2, false>
           : xr <= 4 ? mmq::quant_act_kernel<16, 4, false> : mmq::quant_act_kernel<16, 16, false>;
    if (norm_b)   // LayerNorm (ny == 1: the row's blocks in one workgroup)
        f = xr <= 1 ? mmq::quant_act_kernel<16, 1, true> : xr <= 2 ? mmq::quant_act_kernel<16, 2, true>
          : xr <= 4 ? mmq::quant_act_kernel<16, 4, true> : mmq::quant_act_kernel<16, 16, true>;
    hipLaunchKernelGGL(f, dim3(a.npad, ny), dim3(1024), 0, s, x, x_stride, norm_w, eps, a, rows, part, nks, swiglu, addend,
                       norm_b);
    MI_HIP(hipGetLastError());
}

void launch_rope_table(const int* tokpos, int ntok, int n_rot, float theta_scale, float freq_scale,
                       const float* freq_factors, float2* out, hipStream_t s) {
    if (ntok <= 0 || n_rot <= 0) return;
    hipLaunchKernelGGL(mmq::rope_table_kernel, dim3(ntok), dim3(64), 0, s, tokpos, ntok, n_rot, theta_scale,
                       freq_scale, freq_factors, out);
    MI_HIP(hipGetLastError());
}

void launch_qkv_finish(const QkvFinish& F, hipStream_t s) {
    if (F.ntok < 1 || F.kp < 1 || F.nq % 2 || F.nk % 2 || F.nv % 2 || F.head_dim % 2 || F.n_rot > F.head_dim || !F.rope)
        throw Error("qkv_finish: bad shape");
    const int npair = (F.nq + F.nk + F.nv) / 2;
    hipLaunchKernelGGL(mmq::qkv_finish_kernel, dim3((npair + 255) / 256, F.ntok), dim3(256), 0, s, F);
    MI_HIP(hipGetLastError());
}

void launch_part_sum(const PartSum& p, hipStream_t s) {
    if (p.addend && (!p.resid || p.swiglu)) throw Error("part_sum: an addend goes with a residual");
    if (p.ntok < 1 || p.kp < 1 || p.rows < 1 || p.rows + p.swiglu > p.pstride || (p.swiglu && p.swiglu < p.rows))
        throw Error("part_sum: bad shape");
    hipLaunchKernelGGL(mmq::part_sum_kernel, dim3((p.rows + 255) / 256, p.ntok), dim3(256), 0, s, p.part, p.kp, p.ntok, p.rows,
                       p.pstride, p.resid, p.rstride, p.out, p.ostride, p.swiglu, p.addend);
    MI_HIP(hipGetLastError());
}

}  // namespace mi

