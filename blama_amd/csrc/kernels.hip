// HIP kernels for gfx950 (CDNA4, wave64) of a LLaMA-family GGUF model that have no file of
// their own: the v_dot4 batch GEMM, dequantisation and embedding rows, Q8_K quantisation, top-k,
// MoE routing and grouping, the load-time repack and the KV moves.  (Decode GEMVs: gemv.hip,
// dgemv.hip; attention over the f16 cache: attn.hip.)
//
// Numerics mirror the ggml CPU path of llama.cpp b5187 (the reference's
// verifier, Model::Params{.gpu=false}, inference/code/llama/Model.cpp:13-16):
// activations are quantised to Q8_K / Q8_0 exactly as quantize_row_q8_K_ref /
// quantize_row_q8_0 do, so every per-block integer dot product equals the
// CPU's bit for bit; only the fp32 accumulation order differs.  The whole
// file is compiled with -ffp-contract=off so that no a*b+c is silently fused
// where ggml rounds twice.
#include "kernels.h"
#include "qdot.h"
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <cstdlib>
#include <cstring>
#include <algorithm>

namespace mi {

// ---------------------------------------------------------------------------
// Batched GEMM (prompt ingestion): gemv_t's weight ring and integer dots, with every
// loaded weight chunk dotted against up to GEMM_NT tokens' activations in LDS.
// Correctness first: the prologue reads its parameters straight from kernarg and
// quantises the NT activation rows without the decode kernel's latency tricks
// (one launch streams the weights once for NT tokens).
// ---------------------------------------------------------------------------
// PRE: the instantiation that adds GemmParams::pre (launched only when it is set)
template <int T, int D, bool PRE>
__global__ __launch_bounds__(512) void gemm_t(const GemmParams P) {
    constexpr int NW = 8, NT = GEMM_NT;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    using Kk = Kq<T>;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int sbl = lane >> 3, j = lane & 7;
    const int nb = P.K >> 8;
    const int cpr = (nb + 7) >> 3;
    const int ntok = P.ntok;
    const ActLayout L = act_layout(P.K, P.need_q8k, P.need_q80);
    float* rope = reinterpret_cast<float*>(smem + NT * L.slot_bytes);            // [NT][n_rot/2][2]
    double* red = reinterpret_cast<double*>(rope + NT * ((P.n_rot / 2) * 2 + 2)); // [NT][NW]
    __shared__ int tp_pos[NT], tp_cell[NT];
    if (threadIdx.x < NT) {
        const int t = threadIdx.x < ntok ? threadIdx.x : ntok - 1;
        tp_pos[threadIdx.x] = P.tokpos ? P.tokpos[t * 4 + 1] : 0;
        tp_cell[threadIdx.x] = P.tokpos ? P.tokpos[t * 4 + 2] : 0;
    }
    // ---- prologue: RMSNorm (double sum, ggml order of rounding) + quantisation of NT rows
    const auto w4 = gptr(reinterpret_cast<const f32x4*>(P.norm_w));
    if (P.pro == PRO_RMSNORM) {
        for (int t = 0; t < NT; ++t) {
            double sacc = 0.0;
            if (t < ntok) {
                const auto x4 = gptr(reinterpret_cast<const f32x4*>(P.x + (long long)t * P.x_stride));
                for (int blk = wave; blk < nb; blk += NW) {
                    const f32x4 v = x4[blk * 64 + lane];
                    sacc += (double)(v.x * v.x);
                    sacc += (double)(v.y * v.y);
                    sacc += (double)(v.z * v.z);
                    sacc += (double)(v.w * v.w);
                }
            }
            sacc = wave_sum63_d(sacc);
            if (lane == 63) red[t * NW + wave] = sacc;
        }
    }
    __syncthreads();
    for (int t = 0; t < ntok; ++t) {
        float scale = 1.0f;
        if (P.pro == PRO_RMSNORM) {
            double tot = 0.0;
            for (int w = 0; w < NW; ++w) tot += red[t * NW + w];
            scale = 1.0f / sqrtf((float)(tot / (double)P.K) + P.eps);
        }
        char* base = smem + t * L.slot_bytes;
        const auto x4 = gptr(reinterpret_cast<const f32x4*>(P.x + (long long)t * P.x_stride));
        for (int blk = wave; blk < nb; blk += NW) {
            const f32x4 xv = x4[blk * 64 + lane];
            float v[4] = {xv.x, xv.y, xv.z, xv.w};
            if (P.pro == PRO_RMSNORM) {
                const f32x4 w = w4[blk * 64 + lane];
                v[0] = (v[0] * scale) * w.x;
                v[1] = (v[1] * scale) * w.y;
                v[2] = (v[2] * scale) * w.z;
                v[3] = (v[3] * scale) * w.w;
            }
            if (P.need_q8k)
                quant_q8k_block(v, lane, reinterpret_cast<int8_t*>(base + L.q8k) + blk * 256,
                                reinterpret_cast<int*>(base + L.bsum) + blk * 16,
                                reinterpret_cast<float*>(base + L.dk) + blk);
            if (P.need_q80)
                quant_q80_block(v, lane, reinterpret_cast<int8_t*>(base + L.q80) + blk * 256,
                                reinterpret_cast<float*>(base + L.d0) + blk * 8);
        }
    }
    __syncthreads();
    if (P.n_rot > 0) {   // RoPE table of each token's position (ggml_rope_cache_init)
        for (int t = wave; t < ntok; t += NW) {
            float* rt = rope + t * ((P.n_rot / 2) * 2 + 2);
            for (int i = lane; i < P.n_rot / 2; i += 64) {
                float theta = (float)tp_pos[t];
                for (int kk = 0; kk < i; ++kk) theta = theta * P.theta_scale;
                const float ff = P.freq_factors ? P.freq_factors[i] : 1.0f;
                const float th = P.freq_scale * (theta / ff);
                rt[2 * i] = cosf(th);
                rt[2 * i + 1] = sinf(th);
            }
        }
    }
    __syncthreads();

    // ---- weight stream: the gemv_t ring over this wave's units
    const int W = P.grid * NW;
    int u0, u1;
    unit_range(P.units, W, blockIdx.x * NW + wave, u0, u1);
    const int n_items = (u1 - u0) * cpr;
    const bool adj = P.pair == PAIR_ADJ;
    struct Slot { typename Kk::Ld a, b; };
    Slot ring[D];
    int iu = u0, ic = 0, park = 0;
    const uint8_t* pa[4];
    const uint8_t* pb[4];
    auto bases = [&](int u) {
        const long long ra = adj ? 2LL * u : u;
        long long rb = adj ? ra + 1 : u;
        if (adj && rb >= P.A.rows) rb = ra;   // odd tail: re-read row A, result unused
        const QMat& MB = adj ? P.A : P.B;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            pa[i] = P.A.p[i] + ra * nb * PlaneBytes<T>::b[i];
            pb[i] = MB.p[i] + rb * nb * PlaneBytes<T>::b[i];
        }
    };
    bases(u0 < P.units ? u0 : P.units - 1);
    auto issue = [&](Slot& S) {
        const int sb = park ? 0 : ic * 8 + sbl;
        const int jj = park ? 0 : j;
        S.a = Kk::load(pa, sb, jj);
        S.b = Kk::load(pb, sb, jj);
        if (iu < u1 && ++ic == cpr) {
            ic = 0;
            if (++iu < u1) bases(iu);
            else park = 1;
        }
    };
#pragma unroll
    for (int k = 0; k < D - 1; ++k) issue(ring[k]);

    int cu = u0, cc = 0;
    float accA[NT], accB[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) accA[t] = accB[t] = 0.0f;
    auto consume = [&](const Slot& S) {
        const int sb = cc * 8 + sbl;
        const bool lv = sb < nb;
        const int sbc = lv ? sb : nb - 1;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            if (t < ntok) {
                const typename Kk::AR ar = Kk::act(act_view(smem, L, t), sbc, j);
                const float da = Kk::dot(S.a, ar, j), db = Kk::dot(S.b, ar, j);
                accA[t] += lv ? da : 0.0f;
                accB[t] += lv ? db : 0.0f;
            }
        }
        if (++cc == cpr) {
            const long long ra = adj ? 2LL * cu : cu, rb = adj ? ra + 1 : cu;
            const bool hasB = !adj || rb < P.A.rows;
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                if (t >= ntok) continue;
                float yA = wave_sum63(accA[t]);
                float yB = wave_sum63(accB[t]);
                accA[t] = accB[t] = 0.0f;
                if (lane != 63) continue;
                if constexpr (PRE) {   // a LoRA adapter's term, before the epilogue
                    const float* pr = P.pre + (long long)t * P.pre_stride + P.pre_off;
                    yA += pr[ra];
                    if (hasB) yB += pr[adj ? rb : P.pre_up + rb];
                }
                float* out = P.out + (long long)t * P.out_stride;
                const float* res = P.resid ? P.resid + (long long)t * P.out_stride : nullptr;
                switch (P.epi) {
                case EPI_STORE:
                    out[ra] = yA;
                    if (hasB) out[rb] = yB;
                    break;
                case EPI_ADD: {
                    const float r0 = res[ra], r1 = hasB ? res[rb] : 0.0f;
                    float oA = yA + r0, oB = yB + r1;
                    if (P.addend) {   // (the control vector's direction, after the residual)
                        oA = oA + P.addend[ra];
                        if (hasB) oB = oB + P.addend[rb];
                    }
                    out[ra] = oA;
                    if (hasB) out[rb] = oB;
                    break;
                }
                case EPI_ROPE_Q:
                case EPI_ROPE_K: {
                    const float* rt = rope + t * ((P.n_rot / 2) * 2 + 2);
                    const int i0 = (int)(ra % P.head_dim);
                    float o0 = yA, o1 = yB;
                    if (i0 < P.n_rot) {
                        const float cs = rt[i0], sn = rt[i0 + 1];
                        o0 = yA * cs - yB * sn;
                        o1 = yA * sn + yB * cs;
                    }
                    if (P.epi == EPI_ROPE_Q) {
                        out[ra] = o0;
                        out[rb] = o1;
                    } else {
                        __half* kr = P.kcache + (long long)tp_cell[t] * P.kv_dim;
                        kr[ra] = __float2half_rn(o0);
                        kr[rb] = __float2half_rn(o1);
                        if (cu == 0) P.cell_pos[tp_cell[t]] = tp_pos[t];
                    }
                    break;
                }
                case EPI_V: {
                    __half* vr = P.vcache + (long long)tp_cell[t] * P.kv_dim;
                    vr[ra] = __float2half_rn(yA);
                    if (hasB) vr[rb] = __float2half_rn(yB);
                    break;
                }
                case EPI_SWIGLU:
                    out[cu] = silu_f(yA) * yB;
                    break;
                default: break;
                }
            }
            cc = 0;
            ++cu;
        }
    };
    for (int base = 0; base < n_items; base += D) {
#pragma unroll
        for (int k = 0; k < D; ++k) {
            issue(ring[(k + D - 1) % D]);
            if (base + k < n_items) consume(ring[k]);
        }
    }
}

typedef void (*GemmFn)(const GemmParams);
static GemmFn gemm_fn(int type, bool pre);
void init_gemm_attributes() {
    for (int t : {T_Q4_K, T_Q5_K, T_Q6_K, T_Q8_0, T_Q4_0, T_Q5_0})
        for (bool pre : {false, true})
            MI_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(gemm_fn(t, pre)),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024));
    // the int8-MFMA batch GEMMs and the batch attention, each from its own table
    init_mmq2_attributes();
    init_mmqs_attributes();
    init_attn_mfma_attributes();
}
static GemmFn gemm_fn(int type, bool pre) {
    switch (type) {
    case T_Q4_K: return pre ? gemm_t<T_Q4_K, 4, true> : gemm_t<T_Q4_K, 4, false>;
    case T_Q5_K: return pre ? gemm_t<T_Q5_K, 4, true> : gemm_t<T_Q5_K, 4, false>;
    case T_Q6_K: return pre ? gemm_t<T_Q6_K, 4, true> : gemm_t<T_Q6_K, 4, false>;
    case T_Q8_0: return pre ? gemm_t<T_Q8_0, 4, true> : gemm_t<T_Q8_0, 4, false>;
    case T_Q4_0: return pre ? gemm_t<T_Q4_0, 4, true> : gemm_t<T_Q4_0, 4, false>;
    case T_Q5_0: return pre ? gemm_t<T_Q5_0, 4, true> : gemm_t<T_Q5_0, 4, false>;
    default: return nullptr;
    }
}

static size_t gemm_smem_bytes(const GemmParams& p) {
    const ActLayout L = act_layout(p.K, p.need_q8k, p.need_q80);
    return (size_t)GEMM_NT * L.slot_bytes + (size_t)GEMM_NT * ((p.n_rot / 2) * 2 + 2) * 4 + GEMM_NT * 8 * 8 + 64;
}

void launch_gemm(const GemmParams& p_in, hipStream_t s) {
    GemmParams p = p_in;
    if (p.K % 256 != 0) throw Error("gemm: K must be a multiple of 256");
    if (p.ntok < 1 || p.ntok > GEMM_NT) throw Error("gemm: 1..GEMM_NT tokens per launch");
    if (p.pair == PAIR_AB && p.B.type != p.A.type) throw Error("gemm: a pair must share its quant type");
    if (p.epi == EPI_MOE_DOWN) throw Error("gemm: MoE launches are served token by token");
    p.need_q8k = !takes_q80(p.A.type);
    p.need_q80 = takes_q80(p.A.type);
    const int g = (p.units + 7) / 8;
    p.grid = g < 1 ? 1 : (g > 256 ? 256 : g);
    if ((long long)p.units * p.grid * 8 >= (1LL << 32)) throw Error("gemm: too many units");
    const size_t smem = gemm_smem_bytes(p);
    if (smem > 150 * 1024) throw Error("gemm: activations of GEMM_NT tokens do not fit LDS");
    GemmFn fn = gemm_fn(p.A.type, p.pre != nullptr);
    if (!fn) throw Error("gemm: unsupported quant type");
    hipLaunchKernelGGL(fn, dim3(p.grid), dim3(512), smem, s, p);
    MI_HIP(hipGetLastError());
}


// ---------------------------------------------------------------------------
// Exact ggml dequantisation of one element (dequantize_row_*, ggml-quants.c)
// ---------------------------------------------------------------------------
__device__ __forceinline__ void scale_min_k4(int t, const uint8_t* s, int& sc, int& m) {
    if (t < 4) { sc = s[t] & 63; m = s[t + 4] & 63; }
    else { sc = (s[t + 4] & 0xF) | ((s[t - 4] >> 6) << 4); m = (s[t + 4] >> 4) | ((s[t] >> 6) << 4); }
}

__device__ float dequant_elem(const QMat& M, long long row, int col) {
    const int sb = col >> 8, i = col & 255;
    const long long sbi = row * M.nb + sb;
    switch (M.type) {
    case T_Q4_K:
    case T_Q5_K: {
        const bool q5 = M.type == T_Q5_K;
        const uint8_t* qs = M.p[0] + sbi * 128;
        const uint8_t* hdr = M.p[q5 ? 2 : 1] + sbi * 16;
        const float d = h2f(hdr[0] | (hdr[1] << 8)), dmin = h2f(hdr[2] | (hdr[3] << 8));
        const int c = i >> 6, l = i & 63;
        const int t = 2 * c + (l >= 32);
        const int ll = l & 31;
        int q = (l < 32) ? (qs[32 * c + ll] & 0xF) : (qs[32 * c + ll] >> 4);
        if (q5) {
            const uint8_t* qh = M.p[1] + sbi * 32;
            q += ((qh[ll] >> t) & 1) ? 16 : 0;
        }
        int sc, m;
        scale_min_k4(t, hdr + 4, sc, m);
        const float d1 = d * (float)sc, m1 = dmin * (float)m;
        return d1 * (float)q - m1;
    }
    case T_Q6_K: {
        const uint8_t* ql = M.p[0] + sbi * 128;
        const uint8_t* qh = M.p[1] + sbi * 64;
        const int8_t* sc = reinterpret_cast<const int8_t*>(M.p[2] + sbi * 16);
        const uint8_t* dp = M.p[3] + sbi * 2;
        const float d = h2f(dp[0] | (dp[1] << 8));
        const int h = i >> 7, r = i & 127, quarter = r >> 5, l = r & 31;
        const int is = l / 16;
        const uint8_t L = ql[64 * h + l + ((quarter & 1) ? 32 : 0)];
        const int lo4 = (quarter < 2) ? (L & 0xF) : (L >> 4);
        const int hb = (qh[32 * h + l] >> (2 * quarter)) & 3;
        const int q = (lo4 | (hb << 4)) - 32;
        const int s = sc[8 * h + is + 2 * quarter];
        return (d * (float)s) * (float)q;
    }
    case T_Q8_0: {
        const int8_t q = reinterpret_cast<const int8_t*>(M.p[0] + sbi * 256)[i];
        const uint8_t* dp = M.p[1] + sbi * 16 + (i >> 5) * 2;
        return (float)q * h2f(dp[0] | (dp[1] << 8));
    }
    case T_Q4_0:
    case T_Q5_0: {   // dequantize_row_q4_0 / _q5_0: element l of block blk, (q - 8 or 16) * d
        const bool q5 = M.type == T_Q5_0;
        const int blk = i >> 5, l = i & 31;
        const uint8_t b = M.p[0][sbi * 128 + blk * 16 + (l & 15)];
        int q = l < 16 ? (b & 0xF) : (b >> 4);
        if (q5) {
            const uint8_t* h = M.p[1] + sbi * 32 + blk * 4;
            const unsigned qh = h[0] | (h[1] << 8) | (h[2] << 16) | ((unsigned)h[3] << 24);
            q |= (int)((qh >> l) & 1u) << 4;
        }
        const uint8_t* dp = M.p[q5 ? 2 : 1] + sbi * 16 + blk * 2;
        return (float)(q - (q5 ? 16 : 8)) * h2f(dp[0] | (dp[1] << 8));
    }
    case T_F32:
        return reinterpret_cast<const float*>(M.p[0])[row * M.K + col];
    case T_F16:
        return __half2float(reinterpret_cast<const __half*>(M.p[0])[row * M.K + col]);
    default:
        return 0.0f;
    }
}

// get_rows(tok_embd, token) (+ get_rows(position_embd, pos) for GPT-2, llm_build_gpt2's
// inpL = ggml_add(tok rows, pos rows))
__global__ void embed_kernel(const EmbedParams P) {
    const long long tok = P.tokpos[0];
    const long long pos = P.tokpos[1];
    if (P.step && blockIdx.x == 0 && threadIdx.x == 0) *P.step += 1u;
    for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < P.n_embd; c += gridDim.x * blockDim.x) {
        const float e = dequant_elem(P.E, tok, c);
        P.out[c] = P.has_pos ? e + dequant_elem(P.P, pos, c) : e;
    }
}

__global__ void embed_multi_kernel(const EmbedParams P) {
    const long long tok = P.tokpos[blockIdx.y * 4];
    const long long pos = P.tokpos[blockIdx.y * 4 + 1];
    float* out = P.out + (long long)blockIdx.y * P.n_embd;
    for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < P.n_embd; c += gridDim.x * blockDim.x) {
        const float e = dequant_elem(P.E, tok, c);
        out[c] = P.has_pos ? e + dequant_elem(P.P, pos, c) : e;
    }
}

void launch_embed_multi(const EmbedParams& p, int ntok, hipStream_t s) {
    hipLaunchKernelGGL(embed_multi_kernel, dim3((p.n_embd + 255) / 256, ntok), dim3(256), 0, s, p);
    MI_HIP(hipGetLastError());
}

void launch_embed(const EmbedParams& p, hipStream_t s) {
    hipLaunchKernelGGL(embed_kernel, dim3((p.n_embd + 255) / 256), dim3(256), 0, s, p);
    MI_HIP(hipGetLastError());
}

__global__ void dequant_rows_kernel(const QMat M, int row0, int nrows, float* out) {
    const long long n = (long long)nrows * M.K;
    for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x)
        out[e] = dequant_elem(M, row0 + e / M.K, (int)(e % M.K));
}

void launch_dequant_rows(const QMat& m, int row0, int nrows, float* out, hipStream_t s) {
    long long n = (long long)nrows * m.K;
    int grid = (int)std::min<long long>((n + 255) / 256, 4096);
    hipLaunchKernelGGL(dequant_rows_kernel, dim3(grid), dim3(256), 0, s, m, row0, nrows, out);
    MI_HIP(hipGetLastError());
}

__global__ void quantize_q8k_kernel(const float* x, int K, int8_t* q, float* d, int* bsums) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int blk = blockIdx.x * (blockDim.x >> 6) + wave;
    if (blk >= K / 256) return;
    const float4 xv = reinterpret_cast<const float4*>(x)[blk * 64 + lane];
    const float v[4] = {xv.x, xv.y, xv.z, xv.w};
    quant_q8k_block(v, lane, q + blk * 256, bsums + blk * 16, d + blk);
}

void launch_quantize_q8k(const float* x, int K, int8_t* q, float* d, int* bsums, hipStream_t s) {
    const int nb = K / 256;
    hipLaunchKernelGGL(quantize_q8k_kernel, dim3((nb + 3) / 4), dim3(256), 0, s, x, K, q, d, bsums);
    MI_HIP(hipGetLastError());
}

// ---------------------------------------------------------------------------
// Top-k: keys (orderable logit << 32 | ~id), larger key = better, so the order
// is logit descending then id ascending.  A wave holds 64 keys, one per lane,
// sorted descending by lane; two sorted lists merge into the top 64 of their
// union by c[i] = max(a[i], b[63-i]) (a bitonic sequence) and a 6-step
// half-cleaner.  Stage 1: each 1024-logit block -> 16 wave sorts -> LDS tree
// merge -> its top 64.  Stage 2: one workgroup merges the block lists.
// ---------------------------------------------------------------------------
typedef unsigned long long u64;
__device__ __forceinline__ u64 topk_key(float v, int id) {
    unsigned u = __float_as_uint(v);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((u64)u << 32) | (u64)(0xFFFFFFFFu - (unsigned)id);
}
__device__ __forceinline__ u64 shfl_xor64(u64 v, int m) {
    const unsigned lo = __shfl_xor((unsigned)v, m, 64), hi = __shfl_xor((unsigned)(v >> 32), m, 64);
    return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ u64 shfl64(u64 v, int src) {
    const unsigned lo = __shfl((unsigned)v, src, 64), hi = __shfl((unsigned)(v >> 32), src, 64);
    return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ u64 wave_sort_desc(u64 x, int lane) {
#pragma unroll
    for (int k = 2; k <= 64; k <<= 1) {
#pragma unroll
        for (int j = k >> 1; j > 0; j >>= 1) {
            const u64 y = shfl_xor64(x, j);
            const bool desc = (lane & k) == 0 || k == 64;
            const bool lower = (lane & j) == 0;
            const bool keep_max = lower == desc;
            x = keep_max ? (x > y ? x : y) : (x < y ? x : y);
        }
    }
    return x;
}
// a, b sorted descending across the wave -> top 64 of a U b, sorted descending
__device__ __forceinline__ u64 wave_merge_desc(u64 a, u64 b, int lane) {
    const u64 br = shfl64(b, 63 - lane);
    u64 x = a > br ? a : br;
#pragma unroll
    for (int j = 32; j > 0; j >>= 1) {
        const u64 y = shfl_xor64(x, j);
        x = (lane & j) == 0 ? (x > y ? x : y) : (x < y ? x : y);
    }
    return x;
}

// 16 waves each hold a sorted list; tree-merge them through LDS into wave 0.
__device__ __forceinline__ u64 block_merge16(u64 x, u64* lds, int wave, int lane) {
    for (int n = 16; n > 1; n >>= 1) {
        if (wave >= n / 2 && wave < n) lds[(wave - n / 2) * 64 + lane] = x;
        __syncthreads();
        if (wave < n / 2) x = wave_merge_desc(x, lds[wave * 64 + lane], lane);
        __syncthreads();
    }
    return x;
}

__global__ __launch_bounds__(1024) void topk_stage1(const float* logits, int n, u64* cand) {
    __shared__ u64 lds[8 * 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int id = blockIdx.x * TOPK_BLOCK + wave * 64 + lane;
    u64 x = id < n ? topk_key(logits[id], id) : 0ULL;
    x = wave_sort_desc(x, lane);
    x = block_merge16(x, lds, wave, lane);
    if (wave == 0) cand[blockIdx.x * 64 + lane] = x;
}

__global__ __launch_bounds__(1024) void topk_stage2(const u64* cand, int nblk, const float* logits, int* ids,
                                                   float* vals, int* h_ids, float* h_vals) {
    __shared__ u64 lds[8 * 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u64 x = wave < nblk ? cand[wave * 64 + lane] : 0ULL;
    for (int b = wave + 16; b < nblk; b += 16) x = wave_merge_desc(x, cand[b * 64 + lane], lane);
    x = block_merge16(x, lds, wave, lane);
    if (wave == 0) {
        const int i = x ? (int)(0xFFFFFFFFu - (unsigned)(x & 0xFFFFFFFFu)) : -1;
        const float v = i >= 0 ? logits[i] : -INFINITY;
        ids[lane] = i;
        vals[lane] = v;
        if (h_ids) {
            h_ids[lane] = i;
            h_vals[lane] = v;
        }
    }
}

void launch_topk(const TopkParams& p, hipStream_t s) {
    const int nblk = topk_blocks(p.n);
    hipLaunchKernelGGL(topk_stage1, dim3(nblk), dim3(1024), 0, s, p.logits, p.n, p.cand);
    MI_HIP(hipGetLastError());
    hipLaunchKernelGGL(topk_stage2, dim3(1), dim3(1024), 0, s, p.cand, nblk, p.logits, p.ids, p.vals, p.h_ids,
                       p.h_vals);
    MI_HIP(hipGetLastError());
}

__global__ void gather_kernel(const float* logits, const int* ids, int n, float* out) {
    const int i = threadIdx.x + blockIdx.x * blockDim.x;
    if (i < n) out[i] = logits[ids[i]];
}

// rows of logits: out[i] = base[(i / k) * row_stride + ids[i]]
__global__ void gather_rows_kernel(const float* base, long long row_stride, const int* ids, int n, int k, float* out) {
    const int i = threadIdx.x + blockIdx.x * blockDim.x;
    if (i < n) out[i] = base[(long long)(i / k) * row_stride + ids[i]];
}

void launch_gather_rows(const float* base, long long row_stride, const int* ids, int n, int k, float* out,
                        hipStream_t s) {
    if (n <= 0 || k <= 0) return;
    hipLaunchKernelGGL(gather_rows_kernel, dim3((n + 255) / 256), dim3(256), 0, s, base, row_stride, ids, n, k, out);
    MI_HIP(hipGetLastError());
}

void launch_gather(const float* logits, const int* ids, int n, float* out, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(gather_kernel, dim3((n + 255) / 256), dim3(256), 0, s, logits, ids, n, out);
    MI_HIP(hipGetLastError());
}

// ---------------------------------------------------------------------------
// MoE router (build_moe_ffn, softmax gating, norm_w): one workgroup.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void router_kernel(const RouterParams P0) {
    __shared__ double redd[4];
    __shared__ float logit[64];
    __shared__ float prs[64], topp[64];
    __shared__ int topi[64];
    // token blockIdx.x of a batch (launch_router_multi); one token for the decode step
    RouterParams P = P0;
    P.x += (long long)blockIdx.x * P.x_stride;
    P.sel += blockIdx.x * P.n_used;
    P.selw += blockIdx.x * P.n_used;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (P.part) {   // the split WO's halves: x = (p0 + p1) + x, written back for the experts
        const float* p0 = P.part + (long long)blockIdx.x * P.n_embd;
        const float* p1 = P.part + ((long long)P.part_ntok + blockIdx.x) * P.n_embd;
        float* xw = const_cast<float*>(P.x);
        for (int i = tid; i < P.n_embd; i += 256) xw[i] = (p0[i] + p1[i]) + xw[i];
        __syncthreads();
    }
    // every load of a phase issued before its arithmetic (a serial loop of dependent loads took
    // ~40 us per token, measured): the row as float4 per lane, kept in registers (n_embd <= 4096)
    constexpr int RK = 16;
    const f32x4* x4 = reinterpret_cast<const f32x4*>(P.x);
    const f32x4* n4 = reinterpret_cast<const f32x4*>(P.norm_w);
    const int nk = P.n_embd / 256;   // float4 per lane
    f32x4 xv[RK];
#pragma unroll
    for (int k = 0; k < RK; ++k)
        if (k < nk) xv[k] = x4[k * 64 + lane];
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < RK; ++k)
        if (k < nk) {
            s += (double)(xv[k].x * xv[k].x);
            s += (double)(xv[k].y * xv[k].y);
            s += (double)(xv[k].z * xv[k].z);
            s += (double)(xv[k].w * xv[k].w);
        }
    s = wave_sum_d(s);   // (every wave holds the whole row: each computes the same sum)
    const float mean = (float)(__shfl(s, 0, 64) / (double)P.n_embd);
    const float scale = 1.0f / sqrtf(mean + P.eps);
    (void)redd;
    {   // x * scale * norm_w, in place
        f32x4 nv[RK];
#pragma unroll
        for (int k = 0; k < RK; ++k)
            if (k < nk) nv[k] = n4[k * 64 + lane];
#pragma unroll
        for (int k = 0; k < RK; ++k)
            if (k < nk)
                xv[k] = f32x4{(xv[k].x * scale) * nv[k].x, (xv[k].y * scale) * nv[k].y, (xv[k].z * scale) * nv[k].z,
                              (xv[k].w * scale) * nv[k].w};
    }
    // expert e handled by wave e%4: logits = W_e . (x*scale*w)
    for (int e = wave; e < P.n_expert; e += 4) {
        const f32x4* we = reinterpret_cast<const f32x4*>(P.w + (long long)e * P.n_embd);
        f32x4 wv[RK];
#pragma unroll
        for (int k = 0; k < RK; ++k)
            if (k < nk) wv[k] = we[k * 64 + lane];
        float acc = 0.0f;
#pragma unroll
        for (int k = 0; k < RK; ++k)
            if (k < nk) {
                acc = fmaf(wv[k].x, xv[k].x, acc);
                acc = fmaf(wv[k].y, xv[k].y, acc);
                acc = fmaf(wv[k].z, xv[k].z, acc);
                acc = fmaf(wv[k].w, xv[k].w, acc);
            }
        acc = wave_sum(acc);
        if (lane == 0) logit[e] = acc;
    }
    __syncthreads();
    // softmax over the experts and the top n_used, in wave 0 with one lane per expert (per-thread
    // arrays here would live in scratch memory: ~45 us per call, measured)
    if (wave == 0) {
        const int E = P.n_expert;
        const float lg = lane < E ? logit[lane] : -INFINITY;
        float mx = lg;   // the max is order-free
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
        const float pe = lane < E ? expf(lg - mx) : 0.0f;
        prs[lane] = pe;
        __builtin_amdgcn_s_waitcnt(0xC07F);   // lgkmcnt(0)
        __builtin_amdgcn_wave_barrier();
        // soft_max's double sum in expert order, then p = e * (1/sum)
        double sum = 0.0;
        for (int e = 0; e < E; ++e) sum += (double)prs[e];
        const float inv = (float)(1.0 / sum);
        const float pr = pe * inv;
        // ggml_argsort (desc; the selection sort above kept ties in index order) as a rank
        int rank = 0;
        for (int e = 0; e < E; ++e) {
            const float pq = __shfl(pr, e, 64);
            rank += (pq > pr || (pq == pr && e < lane)) ? 1 : 0;
        }
        if (lane < E && rank < P.n_used) {
            topi[rank] = lane;
            topp[rank] = pr;
        }
        __builtin_amdgcn_s_waitcnt(0xC07F);
        __builtin_amdgcn_wave_barrier();
        if (lane == 0) {
            float wsum = 0.0f;
            for (int k = 0; k < P.n_used; ++k) wsum += topp[k];
            for (int k = 0; k < P.n_used; ++k) { P.sel[k] = topi[k]; P.selw[k] = topp[k] / wsum; }
        }
    }
}

void launch_router(const RouterParams& p, hipStream_t s) { launch_router_multi(p, 1, s); }

void launch_router_multi(const RouterParams& p, int ntok, hipStream_t s) {
    if (p.n_expert > 64) throw Error("router: too many experts");
    if (p.n_embd % 256 || p.n_embd > 4096) throw Error("router: n_embd must be a multiple of 256, at most 4096");
    if (ntok < 1) return;
    hipLaunchKernelGGL(router_kernel, dim3(ntok), dim3(256), 0, s, p);
    MI_HIP(hipGetLastError());
}

// One workgroup: 256 threads, each over a contiguous range of the picks (so that the rows of an
// expert come in pick order = token ascending), per-thread counts per expert in LDS, then an
// exclusive scan over the threads per expert, padded expert offsets, and the row assignment.
__global__ __launch_bounds__(256) void moe_group_kernel(const int* sel, int n, int U, int E, int* grp, int* rows,
                                                        int* rowsel, int* pos, int rows_cap) {
    __shared__ int cnt[256][MOE_GROUP_MAXE];
    __shared__ int off[MOE_GROUP_MAXE + 1];
    const int t = threadIdx.x;
    const int per = (n + 255) / 256;
    const int i0 = min(n, t * per), i1 = min(n, i0 + per);
    for (int e = 0; e < E; ++e) cnt[t][e] = 0;
    for (int i = i0; i < i1; ++i) {
        const int e = sel[i];
        if (e >= 0 && e < E) cnt[t][e] += 1;
    }
    __syncthreads();
    if (t < E) {   // exclusive scan over the threads: this expert's rows before thread th's
        int run = 0;
        for (int th = 0; th < 256; ++th) {
            const int c = cnt[th][t];
            cnt[th][t] = run;
            run += c;
        }
        grp[E + 1 + t] = run;
    }
    __syncthreads();
    if (t == 0) {
        off[0] = 0;
        for (int e = 0; e < E; ++e) off[e + 1] = off[e] + (grp[E + 1 + e] + 31) / 32 * 32;
        for (int e = 0; e <= E; ++e) grp[e] = off[e];
    }
    __syncthreads();
    // padding rows (and every row past the last expert's) first, then the picks' rows
    for (int r = t; r < rows_cap; r += 256) {
        rows[r] = -1;
        rowsel[r] = -1;
    }
    __syncthreads();
    int used[MOE_GROUP_MAXE];
    for (int e = 0; e < E; ++e) used[e] = 0;
    for (int i = i0; i < i1; ++i) {
        const int e = sel[i];
        if (e < 0 || e >= E) continue;   // the router never picks one (checked on the decode path)
        const int r = off[e] + cnt[t][e] + used[e]++;
        rows[r] = i / U;
        rowsel[r] = r;
        pos[i] = r;
    }
}

void launch_moe_group(const int* sel, int n, int U, int E, int* grp, int* rows, int* rowsel, int* pos, int rows_cap,
                      hipStream_t s) {
    if (E < 1 || E > MOE_GROUP_MAXE) throw Error("moe_group: 1..16 experts");
    if (rows_cap < moe_rows_cap(n, E)) throw Error("moe_group: row capacity too small");
    hipLaunchKernelGGL(moe_group_kernel, dim3(1), dim3(256), 0, s, sel, n, U, E, grp, rows, rowsel, pos, rows_cap);
    MI_HIP(hipGetLastError());
}

__global__ void moe_combine_kernel(const float* y, const int* pos, const float* w, float* x, int n_embd,
                                   const float* addend) {
    const int t = blockIdx.y;
    const float* y0 = y + (long long)pos[2 * t] * n_embd;
    const float* y1 = y + (long long)pos[2 * t + 1] * n_embd;
    const float w0 = w[2 * t], w1 = w[2 * t + 1];
    float* xr = x + (long long)t * n_embd;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n_embd; i += gridDim.x * blockDim.x) {
        float o = (y0[i] * w0 + y1[i] * w1) + xr[i];   // as the decode GEMV's EPI_MOE_DOWN
        if (addend) o = o + addend[i];
        xr[i] = o;
    }
}

void launch_moe_combine(const float* y, const int* pos, const float* w, float* x, int ntok, int n_embd,
                        hipStream_t s, const float* addend) {
    if (ntok < 1) return;
    hipLaunchKernelGGL(moe_combine_kernel, dim3((n_embd + 255) / 256, ntok), dim3(256), 0, s, y, pos, w, x, n_embd,
                       addend);
    MI_HIP(hipGetLastError());
}

// ---------------------------------------------------------------------------
// Load-time repack: GGUF blocks -> planes (one thread per superblock)
// ---------------------------------------------------------------------------
__global__ void repack_kernel(const uint8_t* raw, int type, long long nsb, uint8_t* p0, uint8_t* p1,
                              uint8_t* p2, uint8_t* p3) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < nsb;
         i += (long long)gridDim.x * blockDim.x) {
        if (type == T_Q4_K) {
            const uint8_t* b = raw + i * 144;
            for (int k = 0; k < 128; ++k) p0[i * 128 + k] = b[16 + k];
            for (int k = 0; k < 16; ++k) p1[i * 16 + k] = b[k];
        } else if (type == T_Q5_K) {
            const uint8_t* b = raw + i * 176;
            for (int k = 0; k < 128; ++k) p0[i * 128 + k] = b[48 + k];
            for (int k = 0; k < 32; ++k) p1[i * 32 + k] = b[16 + k];
            for (int k = 0; k < 16; ++k) p2[i * 16 + k] = b[k];
        } else if (type == T_Q6_K) {
            const uint8_t* b = raw + i * 210;
            for (int k = 0; k < 128; ++k) p0[i * 128 + k] = b[k];
            for (int k = 0; k < 64; ++k) p1[i * 64 + k] = b[128 + k];
            for (int k = 0; k < 16; ++k) p2[i * 16 + k] = b[192 + k];
            p3[i * 2] = b[208];
            p3[i * 2 + 1] = b[209];
        } else if (type == T_Q8_0) {
            const uint8_t* b = raw + i * 272;   // 8 blocks of 34
            for (int blk = 0; blk < 8; ++blk) {
                p1[i * 16 + blk * 2] = b[blk * 34];
                p1[i * 16 + blk * 2 + 1] = b[blk * 34 + 1];
                for (int k = 0; k < 32; ++k) p0[i * 256 + blk * 32 + k] = b[blk * 34 + 2 + k];
            }
        } else if (type == T_Q4_0) {
            const uint8_t* b = raw + i * 144;   // 8 blocks of 18: f16 d, qs[16]
            for (int blk = 0; blk < 8; ++blk) {
                p1[i * 16 + blk * 2] = b[blk * 18];
                p1[i * 16 + blk * 2 + 1] = b[blk * 18 + 1];
                for (int k = 0; k < 16; ++k) p0[i * 128 + blk * 16 + k] = b[blk * 18 + 2 + k];
            }
        } else if (type == T_Q5_0) {
            const uint8_t* b = raw + i * 176;   // 8 blocks of 22: f16 d, qh[4], qs[16]
            for (int blk = 0; blk < 8; ++blk) {
                p2[i * 16 + blk * 2] = b[blk * 22];
                p2[i * 16 + blk * 2 + 1] = b[blk * 22 + 1];
                for (int k = 0; k < 4; ++k) p1[i * 32 + blk * 4 + k] = b[blk * 22 + 2 + k];
                for (int k = 0; k < 16; ++k) p0[i * 128 + blk * 16 + k] = b[blk * 22 + 6 + k];
            }
        }
    }
}

void launch_repack(const uint8_t* raw, int type, long long rows, int K, uint8_t* const planes[4],
                   hipStream_t s) {
    const long long nsb = rows * (K / 256);
    const int grid = (int)std::min<long long>((nsb + 255) / 256, 8192);
    hipLaunchKernelGGL(repack_kernel, dim3(grid), dim3(256), 0, s, raw, type, nsb, planes[0], planes[1],
                       planes[2], planes[3]);
    MI_HIP(hipGetLastError());
}

// ---------------------------------------------------------------------------
// KV maintenance: K-shift (re-rotate cached K by a per-cell position delta,
// as llama.cpp's build_k_shift does with ggml_rope_ext on the f16 cache) and
// cell compaction (seq_rm).
// ---------------------------------------------------------------------------
__global__ void kv_shift_kernel(const KvShiftParams P) {
    const int cell = blockIdx.x, layer = blockIdx.y;
    const int delta = P.cell_delta[cell];
    if (delta == 0) return;
    __half* kr = P.kcache + ((long long)layer * P.n_ctx + cell) * P.kv_dim;
    const int pairs_per_head = P.head_dim / 2;
    for (int pi = threadIdx.x; pi < P.kv_dim / 2; pi += blockDim.x) {
        const int i = pi % pairs_per_head;          // pair index within head
        if (2 * i >= P.n_rot) continue;
        float theta = (float)delta;
        for (int k = 0; k < i; ++k) theta = theta * P.theta_scale;
        const float ff = P.freq_factors ? P.freq_factors[i] : 1.0f;
        const float th = P.freq_scale * (theta / ff);
        const float c = cosf(th), sn = sinf(th);
        const int head = pi / pairs_per_head;
        __half* e = kr + head * P.head_dim + 2 * i;
        const float x0 = __half2float(e[0]), x1 = __half2float(e[1]);
        e[0] = __float2half_rn(x0 * c - x1 * sn);
        e[1] = __float2half_rn(x0 * sn + x1 * c);
    }
}

void launch_kv_shift(const KvShiftParams& p, hipStream_t s) {
    if (p.n_cells <= 0) return;
    hipLaunchKernelGGL(kv_shift_kernel, dim3(p.n_cells, p.n_layer), dim3(256), 0, s, p);
    MI_HIP(hipGetLastError());
}

__global__ void kv_gather_kernel(const __half* cache, int n_ctx, int kv_dim, const int* src_cell, __half* dst) {
    const int cell = blockIdx.x, layer = blockIdx.y;
    const __half* sr = cache + ((long long)layer * n_ctx + src_cell[cell]) * kv_dim;
    __half* dr = dst + ((long long)layer * n_ctx + cell) * kv_dim;
    for (int i = threadIdx.x; i < kv_dim; i += blockDim.x) dr[i] = sr[i];
}

__global__ void kv_copy_kernel(const __half* src, int n_ctx, int kv_dim, int n, __half* dst) {
    const int cell = blockIdx.x, layer = blockIdx.y;
    const long long off = ((long long)layer * n_ctx + cell) * kv_dim;
    for (int i = threadIdx.x; i < kv_dim; i += blockDim.x) dst[off + i] = src[off + i];
}

void launch_kv_move(__half* cache, int n_layer, int n_ctx, int kv_dim, const int* src_cell, int n_dst,
                    __half* scratch, hipStream_t s) {
    if (n_dst <= 0) return;
    hipLaunchKernelGGL(kv_gather_kernel, dim3(n_dst, n_layer), dim3(256), 0, s, cache, n_ctx, kv_dim, src_cell,
                       scratch);
    MI_HIP(hipGetLastError());
    hipLaunchKernelGGL(kv_copy_kernel, dim3(n_dst, n_layer), dim3(256), 0, s, scratch, n_ctx, kv_dim, n_dst,
                       cache);
    MI_HIP(hipGetLastError());
}

}  // namespace mi
