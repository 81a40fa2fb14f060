// Short batches (<= MMQS_MAX tokens: the verification sizes, Session.cpp:231-244) on the int8
// MFMAs, streamed like the decode GEMV instead of tiled like mmq.hip's GEMM.  The arithmetic
// contract, the MFMA geometry and the tile layouts of the MFMA-order copy are mmq_common.h's.
//
// At 20-64 tokens a weight byte feeds at most 2 MFMA token tiles, so the launch is an HBM stream:
// every weight byte is read once, straight into registers (no LDS staging, no per-superblock
// barrier), and the grid is spread over K as well as over rows so that enough waves are in flight.
//   mmqs_t        workgroup = MS_NW waves = MS_NW row tiles (32 rows; a gate/up pair tile: 16 + 16)
//                 x one K-part of sbw superblocks; the part's activation tiles (all NT token tiles,
//                 bsums, d) are LDS-DMA'd once at entry, shared by the waves; each wave issues the
//                 weight loads of its first D superblocks at entry and refills the ring as it computes
//   mmqs1_t       the one-token-tile (<= 32 tokens) k-quant form with no LDS: a workgroup is ONE wave,
//   mmqs1_lean_t  the activation pieces streamed through registers next to the weights (below)
// Per superblock the arithmetic is the tiled GEMM's: the Q4_K / Q5_K weights as scaled int8 operand
// planes sc_j * q = P0 + 8 P1 (Q5_K: P0 + 128 P1) accumulated by the MFMA over the sub-blocks, the
// min terms by two more MFMAs, then y = fmaf(-dmin_x d_y, mins, fmaf(d_x d_y, S, y)) (Q6_K:
// fmaf(d_x d_y, S, y); Q8_0: one fmaf per 32-block) -- so the sum of a K-part's superblocks is what
// mmq2_t forms over the same superblocks, bit for bit.
// The K-parts write plain partial sums part[kp][ntok][pstride]; the consumer adds them in part
// order (quant_act.hip): launch_quant_act (residual x, or silu(gate) * up for the FFN down input),
// launch_qkv_finish (RoPE, KV append), launch_part_sum (output head, the last residual).
//
// Where a launch is chosen: mmqs_plan (mmq_plan's short form, below) from the launch's shape,
// mmqs_fn from the plan to the instantiation; init_mmqs_attributes walks the same table.
#include "mmq_common.h"

namespace mi {
namespace mmq {

// get_scale_min_k4 for the 8 sub-blocks of a Q4_K header {d, dmin, scales[12]}
__device__ __forceinline__ void q4k_scales(const u32x4 hd, int sc[8], int mn[8]) {
    const unsigned Y = hd.y, Z = hd.z, W = hd.w;   // bytes 0-3, 4-7, 8-11 of scales[12]
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        sc[j] = (Y >> (8 * j)) & 63;
        mn[j] = (Z >> (8 * j)) & 63;
        sc[4 + j] = ((W >> (8 * j)) & 0xF) | (((Y >> (8 * j + 6)) & 3) << 4);
        mn[4 + j] = ((W >> (8 * j + 4)) & 0xF) | (((Z >> (8 * j + 6)) & 3) << 4);
    }
}

constexpr int MS_NW = 4;     // waves (row tiles) per workgroup
constexpr int MS_SBW = 4;    // superblocks per K-part
struct MsArgs {
    const uint8_t* sw[MMQ_SEGS];   // MFMA-order copies
    int nrt[MMQ_SEGS];             // row tiles per segment
    int rows[MMQ_SEGS];
    int prow[MMQ_SEGS];            // the segment's first row in the partial row space
    int n;                         // segments
    int nrt_tot;
    int kp;                        // K-parts (grid = row blocks x kp)
    int sbw;                       // superblocks per K-part (<= MS_SBW)
    int nff;                       // pair launches: the up rows' offset in the partial row space
    float* part;                   // [kp][prows][pstride]
    int pstride;
    int prows;                     // rows of one part: the batch's tokens (grouped: the MoE rows)
    // grouped (MoE, mmqs1 only): blockIdx.y = expert e, whose rows [grp[e], + grp[grp_n + 1 + e])
    // of the activation (whole 32-row tiles, moe_group_kernel) read expert e's copy at
    // sw[0] + e * grp_stride; blockIdx.z = the 32-row tile within the expert
    const int* grp;
    int grp_n;
    long long grp_stride;
};
// 16-B weight loads per superblock of a row tile (NV) and the wave's ring depth (D)
template <int T> struct MsT;
template <> struct MsT<T_Q4_K> { static constexpr int NV = 5, D = 4; };    // qs [4] | header
template <> struct MsT<T_Q5_K> { static constexpr int NV = 6, D = 4; };    // qs [4] | qh | header
template <> struct MsT<T_Q6_K> { static constexpr int NV = 16, D = 2; };   // hi [8] | lo [8] (+ d)
template <> struct MsT<T_Q8_0> { static constexpr int NV = 9, D = 2; };    // qs [8] | d [8 x f16]
template <int T> struct MsW {
    u32x4 v[MsT<T>::NV];
    unsigned d6;   // Q6_K: the row's d
};
template <int T>
__device__ __forceinline__ MsW<T> ms_load(const uint8_t* tile, int lane) {
    const int col = lane & 31;
    MsW<T> w;
    auto ld = [&](int off) { return __builtin_nontemporal_load(gp(reinterpret_cast<const u32x4*>(tile + off))); };
    if (T == T_Q4_K || T == T_Q5_K) {
#pragma unroll
        for (int p = 0; p < 4; ++p) w.v[p] = ld(p * 1024 + lane * 16);
        if (T == T_Q5_K) w.v[4] = ld(4096 + lane * 16);
        w.v[MsT<T>::NV - 1] = ld((T == T_Q5_K ? 5120 : 4096) + col * 16);
        w.d6 = 0;
    } else if (T == T_Q6_K) {
#pragma unroll
        for (int sp = 0; sp < 8; ++sp) {
            w.v[sp] = ld(sp * 1024 + lane * 16);
            w.v[8 + sp] = ld(8192 + sp * 1024 + lane * 16);
        }
        w.d6 = __builtin_nontemporal_load(gp(reinterpret_cast<const unsigned short*>(tile + 16384 + col * 2)));
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) w.v[j] = ld(j * 1024 + lane * 16);
        w.v[8] = ld(8192 + col * 16);
        w.d6 = 0;
    }
    return w;
}
__device__ __forceinline__ v16i mfma_acc(v4i a, v4i b, v16i c) { return __builtin_amdgcn_mfma_i32_32x32x32_i8(a, b, c, 0, 0, 0); }
__device__ __forceinline__ v4i as_v4i(const unsigned p[4]) { return v4i{(int)p[0], (int)p[1], (int)p[2], (int)p[3]}; }

// one superblock (local index s of the part) of this wave's row tile into y[NT][16]
template <int T, int NT>
__device__ __forceinline__ void ms_sb(const MsW<T>& w, int s, const char* lds, int QB, int DB, int lane,
                                      float y[NT][16]) {
    typedef __attribute__((address_space(3))) const char lc;
    const lc* L = (const lc*)lds;
    const int col = lane & 31, h = lane >> 5;
    (void)col;
    auto act = [&](int t, int j) {
        return *reinterpret_cast<const __attribute__((address_space(3))) v4i*>(L + (s * NT + t) * 8192 + j * 1024 + lane * 16);
    };
    auto dx4 = [&](int off) { return *reinterpret_cast<const __attribute__((address_space(3))) f32x4*>(L + off); };
    if (T == T_Q4_K || T == T_Q5_K) {
        const u32x4 hd = w.v[MsT<T>::NV - 1];
        int sc[8], mn[8];
        q4k_scales(hd, sc, mn);
        const v16i z = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        // [hf]: even / odd sub-blocks in separate accumulators -- four independent MFMA chains per
        // token tile instead of two (a dependent MFMA waits out its predecessor's latency)
        v16i acc0[2][NT], acc1[2][NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) acc0[0][t] = acc1[0][t] = acc0[1][t] = acc1[1][t] = z;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const unsigned q[4] = {w.v[p].x, w.v[p].y, w.v[p].z, w.v[p].w};
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) {
                const int j = 2 * p + hf;
                unsigned P0[4], P1[4];
                if (T == T_Q4_K) {   // sc q = P0 + 8 P1 (P0 = q (sc & 7), P1 = q (sc >> 3), bytes <= 105)
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const unsigned nib = hf ? (q[i] >> 4) & 0x0F0F0F0Fu : q[i] & 0x0F0F0F0Fu;
                        P0[i] = bmul(nib, sc[j] & 7);
                        P1[i] = bmul(nib, sc[j] >> 3);
                    }
                } else {             // sc q = P0 + 128 P1 (q = lo4 + 16 hb <= 31)
                    const unsigned b[4] = {w.v[4].x, w.v[4].y, w.v[4].z, w.v[4].w};
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const unsigned q5 = ((hf ? q[i] >> 4 : q[i]) & 0x0F0F0F0Fu) | (((b[i] >> j) & 0x01010101u) << 4);
                        const unsigned m02 = wmul16(q5 & 0x00FF00FFu, sc[j]), m13 = wmul16((q5 >> 8) & 0x00FF00FFu, sc[j]);
                        P0[i] = (m02 & 0x007F007Fu) | ((m13 & 0x007F007Fu) << 8);
                        P1[i] = ((m02 >> 7) & 0x001F001Fu) | (((m13 >> 7) & 0x001F001Fu) << 8);
                    }
                }
                const v4i b0 = as_v4i(P0), b1 = as_v4i(P1);
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    const v4i a = act(t, j);
                    acc0[hf][t] = mfma_acc(a, b0, acc0[hf][t]);
                    acc1[hf][t] = mfma_acc(a, b1, acc1[hf][t]);
                }
            }
        }
        // sum_j m_j*bsum_j by MFMA (as mmq2_t, mmq.hip): bsums 64 hi + lo as A, the row's mins as B
        const unsigned Z = hd.z, W = hd.w;
        const int m03 = (int)(Z & 0x3F3F3F3Fu);
        const int m47 = (int)(((W >> 4) & 0x0F0F0F0Fu) | ((Z >> 2) & 0x30303030u));
        const v4i bm1 = h == 0 ? v4i{m03, m47, 0, 0} : v4i{0, 0, 0, 0};
        const v4i bm2 = h == 0 ? v4i{0, 0, m03, m47} : v4i{0, 0, 0, 0};
        const float dr = h2f(hd.x), dmr = h2f(hd.x >> 16);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const v4i ab = h == 0 ? *reinterpret_cast<const __attribute__((address_space(3))) v4i*>(L + QB + (s * NT + t) * 1024 + col * 16)
                                  : v4i{0, 0, 0, 0};
            const v16i x1 = mfma(ab, bm1);
            const v16i x2 = mfma(ab, bm2);
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 d4 = dx4(DB + s * 256 + (t * 32 + 8 * g + 4 * h) * 4);
                const float dx[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int e = 4 * g + i;
                    const int S = (acc0[0][t][e] + acc0[1][t][e]) + (T == T_Q5_K ? 128 : 8) * (acc1[0][t][e] + acc1[1][t][e]);
                    const float d = dr * dx[i], dm = dmr * dx[i];
                    y[t][e] = fmaf(-dm, (float)(64 * x1[e] + x2[e]), fmaf(d, (float)S, y[t][e]));
                }
            }
        }
    } else if (T == T_Q6_K) {
        const v16i z = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        v16i ah[2][NT], al[2][NT];   // [sp & 1]: four independent MFMA chains per token tile
#pragma unroll
        for (int t = 0; t < NT; ++t) ah[0][t] = al[0][t] = ah[1][t] = al[1][t] = z;
#pragma unroll
        for (int sp = 0; sp < 8; ++sp) {
            const unsigned ph[4] = {w.v[sp].x, w.v[sp].y, w.v[sp].z, w.v[sp].w};
            const unsigned pl[4] = {w.v[8 + sp].x, w.v[8 + sp].y, w.v[8 + sp].z, w.v[8 + sp].w};
            const v4i bh = as_v4i(ph), bl = as_v4i(pl);
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const v4i a = act(t, sp);
                ah[sp & 1][t] = mfma_acc(a, bh, ah[sp & 1][t]);
                al[sp & 1][t] = mfma_acc(a, bl, al[sp & 1][t]);
            }
        }
        const float dr = h2f(w.d6);
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 d4 = dx4(DB + s * 256 + (t * 32 + 8 * g + 4 * h) * 4);
                const float dx[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int e = 4 * g + i;
                    y[t][e] = fmaf(dr * dx[i], (float)((ah[0][t][e] + ah[1][t][e]) * 64 + (al[0][t][e] + al[1][t][e])), y[t][e]);
                }
            }
    } else {   // Q8_0: one MFMA per 32-block, vec_dot_q8_0_q8_0's per-block float update
        const u32x4 hdr = w.v[8];
        const unsigned hw[4] = {hdr.x, hdr.y, hdr.z, hdr.w};
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const unsigned pq[4] = {w.v[j].x, w.v[j].y, w.v[j].z, w.v[j].w};
            const v4i wq = as_v4i(pq);
            const float dwj = h2f(hw[j >> 1] >> (16 * (j & 1)));
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const v16i dj = mfma(act(t, j), wq);
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const f32x4 d4 = dx4(DB + (s * 8 + j) * 256 + (t * 32 + 8 * g + 4 * h) * 4);
                    const float dx[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
                    for (int i = 0; i < 4; ++i) y[t][4 * g + i] = fmaf((float)dj[4 * g + i], dwj * dx[i], y[t][4 * g + i]);
                }
            }
            // block j's updates before block j + 1's operand reads (volatile asm keeps its order, the
            // memory clobber keeps the LDS reads behind it): one block's MFMA results live at a time
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int e = 0; e < 16; ++e) asm volatile("" : "+v"(y[t][e]));
            asm volatile("" ::: "memory");
        }
    }
}

template <int T, bool AB, int NT>
__global__ __launch_bounds__(64 * MS_NW) void mmqs_t(const MsArgs M, const ActQ8 act) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr bool KQ = T != T_Q8_0;
    constexpr int D = MsT<T>::D;
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int col = lane & 31, h = lane >> 5;
    const int nb = act.K >> 8;
    const int kp = (int)blockIdx.x % M.kp, rb = (int)blockIdx.x / M.kp;
    const int sb0 = kp * M.sbw, nsb = min(M.sbw, nb - sb0);   // (the host sizes kp: nsb >= 1)
    // LDS: q [s][t] 8 KiB | k-quants: bsb [s][t] 1 KiB, dT [s] 256 B | Q8_0: dT [s][j] 256 B
    const int QB = M.sbw * NT * 8192;
    const int DB = QB + (KQ ? M.sbw * NT * 1024 : 0);
    typedef __attribute__((address_space(3))) void lv;
    // (1) this part's activation pieces (every token tile), LDS-DMA spread over the waves
    for (int i = wv; i < nsb * NT * 8; i += MS_NW) {
        const int s = i / (NT * 8), t = (i >> 3) % NT, j = i & 7;
        const int8_t* src = act.q + ((long long)t * nb + sb0 + s) * 8192 + j * 1024 + lane * 16;
        __builtin_amdgcn_global_load_lds(gp(src), (lv*)(smem + (s * NT + t) * 8192 + j * 1024), 16, 0, 0);
    }
    const int tl = min(lane, act.npad - 1);   // dT: token lane (a 32-token batch: lanes 32.. repeat)
    if (KQ) {
        for (int i = wv; i < nsb * NT; i += MS_NW) {   // bsb of (s, t) = i: 32 tokens x 16 B, twice
            const int s = i / NT, t = i % NT;
            const int8_t* src = act.bsb + ((long long)t * nb + sb0 + s) * 512 + col * 16;
            __builtin_amdgcn_global_load_lds(gp(src), (lv*)(smem + QB + i * 1024), 16, 0, 0);
        }
        for (int s = wv; s < nsb; s += MS_NW)
            __builtin_amdgcn_global_load_lds(gp(act.dT + (long long)(sb0 + s) * act.npad + tl), (lv*)(smem + DB + s * 256), 4, 0, 0);
    } else {
        for (int i = wv; i < nsb * 8; i += MS_NW)     // rows 8 (sb0 + s) + j of the per-32 d
            __builtin_amdgcn_global_load_lds(gp(act.dT + (long long)(8 * sb0 + i) * act.npad + tl), (lv*)(smem + DB + i * 256), 4, 0, 0);
    }
    // (2) this wave's row tile and the first D superblocks of its weights
    int g = rb * MS_NW + wv;
    const bool busy = g < M.nrt_tot;
    if (!busy) g = M.nrt_tot - 1;
    int seg = 0, rt = g;
#pragma unroll
    for (int i = 0; i < MMQ_SEGS - 1; ++i)
        if (i + 1 < M.n && seg == i && rt >= M.nrt[i]) {
            rt -= M.nrt[i];
            seg = i + 1;
        }
    const uint8_t* swA = seg == 0 ? M.sw[0] : seg == 1 ? M.sw[1] : M.sw[2];
    const int rows_s = seg == 0 ? M.rows[0] : seg == 1 ? M.rows[1] : M.rows[2];
    const int prow_s = seg == 0 ? M.prow[0] : seg == 1 ? M.prow[1] : M.prow[2];
    constexpr int TB = mmq32_tile_bytes_d(T);
    const uint8_t* tile0 = swA + ((long long)rt * nb + sb0) * TB;
    MsW<T> w[D];
    // a busy wave waits for its DMA only (issued before its NLD weight loads: loads retire in
    // order), so superblock 0's dots start while the later ones are still arriving
    constexpr int NLD = D * (MsT<T>::NV + (T == T_Q6_K ? 1 : 0));
    static_assert(NLD <= 63, "vmcnt range");
    if (busy) {
#pragma unroll
        for (int d = 0; d < D; ++d) w[d] = ms_load<T>(tile0 + (long long)min(d, nsb - 1) * TB, lane);
        asm volatile("" ::: "memory");   // every ring load issued before the wait
        __builtin_amdgcn_s_waitcnt((NLD & 0xF) | ((NLD >> 4) << 14) | (0x7 << 4) | (0xF << 8));   // vmcnt(NLD)
    } else {
        __builtin_amdgcn_s_waitcnt((0x7 << 4) | (0xF << 8));   // vmcnt(0)
    }
    __builtin_amdgcn_s_barrier();
    if (!busy) return;
    float y[NT][16];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int e = 0; e < 16; ++e) y[t][e] = 0.0f;
    for (int i = 0; i < nsb; i += D) {
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const int s = i + d;
            if (s < nsb) {
                const MsW<T> cur = w[d];
                if (s + D < nsb) w[d] = ms_load<T>(tile0 + (long long)(s + D) * TB, lane);
                ms_sb<T, NT>(cur, s, smem, QB, DB, lane, y);
            }
        }
    }
    // (3) the partial sums of this part: lane = weight row, 16 tokens per token tile
    const int rr = AB ? rt * 16 + (col & 15) : rt * 32 + col;
    if (rr >= rows_s) return;
    const int prow = prow_s + (AB && col >= 16 ? M.nff : 0) + rr;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int tok = t * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
            if (tok < act.ntok) M.part[((long long)kp * act.ntok + tok) * M.pstride + prow] = y[t][r];
        }
}

// mmqs1: the one-token-tile (<= 32 tokens) k-quant form with no LDS: a workgroup is ONE wave =
// one row tile x one K-part (4x the workgroups of mmqs_t, so a launch of few row blocks -- the 7B
// WO at 128 row tiles -- still covers every CU), and the wave streams its activation pieces
// (8 A operands, the bsums, the 16 token scales per superblock) through registers next to its
// weights, both DA / DW superblocks ahead.  No barrier, no LDS-DMA: every wait is the compiler's
// count of this wave's own loads.  Same arithmetic as ms_sb (sum for sum).
struct MsAct {
    v4i a[8];     // A operands of sub-blocks 0..7
    v4i ab;       // bsums (64 hi + lo) of token col (lanes h = 1: zero)
    f32x4 dx[4];  // d of tokens 8g + 4h .. + 3
};
__device__ __forceinline__ MsAct ms_act_load(const ActQ8& act, int sb, int lane) {
    const int col = lane & 31, h = lane >> 5;
    MsAct r;
    const int8_t* q = act.q + (long long)sb * 8192 + lane * 16;
#pragma unroll
    for (int j = 0; j < 8; ++j) r.a[j] = __builtin_nontemporal_load(gp(reinterpret_cast<const v4i*>(q + j * 1024)));
    const v4i b = *gp(reinterpret_cast<const v4i*>(act.bsb + (long long)sb * 512 + col * 16));
    r.ab = h == 0 ? b : v4i{0, 0, 0, 0};
#pragma unroll
    for (int g = 0; g < 4; ++g) r.dx[g] = *gp(reinterpret_cast<const f32x4*>(act.dT + (long long)sb * act.npad + 8 * g + 4 * h));
    return r;
}
template <int T>
__device__ __forceinline__ void ms1_sb(const MsW<T>& w, const MsAct& A, int lane, float y[16]) {
    const int h = lane >> 5;
    const v16i z = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (T == T_Q4_K || T == T_Q5_K) {
        const u32x4 hd = w.v[MsT<T>::NV - 1];
        int sc[8], mn[8];
        q4k_scales(hd, sc, mn);
        v16i acc0 = z, acc1 = z;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const unsigned q[4] = {w.v[p].x, w.v[p].y, w.v[p].z, w.v[p].w};
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) {
                const int j = 2 * p + hf;
                unsigned P0[4], P1[4];
                if (T == T_Q4_K) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const unsigned nib = hf ? (q[i] >> 4) & 0x0F0F0F0Fu : q[i] & 0x0F0F0F0Fu;
                        P0[i] = bmul(nib, sc[j] & 7);
                        P1[i] = bmul(nib, sc[j] >> 3);
                    }
                } else {
                    const unsigned b[4] = {w.v[4].x, w.v[4].y, w.v[4].z, w.v[4].w};
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const unsigned q5 = ((hf ? q[i] >> 4 : q[i]) & 0x0F0F0F0Fu) | (((b[i] >> j) & 0x01010101u) << 4);
                        const unsigned m02 = wmul16(q5 & 0x00FF00FFu, sc[j]), m13 = wmul16((q5 >> 8) & 0x00FF00FFu, sc[j]);
                        P0[i] = (m02 & 0x007F007Fu) | ((m13 & 0x007F007Fu) << 8);
                        P1[i] = ((m02 >> 7) & 0x001F001Fu) | (((m13 >> 7) & 0x001F001Fu) << 8);
                    }
                }
                acc0 = mfma_acc(A.a[j], as_v4i(P0), acc0);
                acc1 = mfma_acc(A.a[j], as_v4i(P1), acc1);
            }
        }
        const unsigned Z = hd.z, W = hd.w;
        const int m03 = (int)(Z & 0x3F3F3F3Fu);
        const int m47 = (int)(((W >> 4) & 0x0F0F0F0Fu) | ((Z >> 2) & 0x30303030u));
        const v4i bm1 = h == 0 ? v4i{m03, m47, 0, 0} : v4i{0, 0, 0, 0};
        const v4i bm2 = h == 0 ? v4i{0, 0, m03, m47} : v4i{0, 0, 0, 0};
        const v16i x1 = mfma(A.ab, bm1);
        const v16i x2 = mfma(A.ab, bm2);
        const float dr = h2f(hd.x), dmr = h2f(hd.x >> 16);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const float dx[4] = {A.dx[g].x, A.dx[g].y, A.dx[g].z, A.dx[g].w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int e = 4 * g + i;
                const int S = acc0[e] + (T == T_Q5_K ? 128 : 8) * acc1[e];
                const float d = dr * dx[i], dm = dmr * dx[i];
                y[e] = fmaf(-dm, (float)(64 * x1[e] + x2[e]), fmaf(d, (float)S, y[e]));
            }
        }
    } else {   // Q6_K
        v16i ah = z, al = z;
#pragma unroll
        for (int sp = 0; sp < 8; ++sp) {
            const unsigned ph[4] = {w.v[sp].x, w.v[sp].y, w.v[sp].z, w.v[sp].w};
            const unsigned pl[4] = {w.v[8 + sp].x, w.v[8 + sp].y, w.v[8 + sp].z, w.v[8 + sp].w};
            ah = mfma_acc(A.a[sp], as_v4i(ph), ah);
            al = mfma_acc(A.a[sp], as_v4i(pl), al);
        }
        const float dr = h2f(w.d6);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const float dx[4] = {A.dx[g].x, A.dx[g].y, A.dx[g].z, A.dx[g].w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int e = 4 * g + i;
                y[e] = fmaf(dr * dx[i], (float)(ah[e] * 64 + al[e]), y[e]);
            }
        }
    }
}
template <int T> struct Ms1D { static constexpr int DW = 2, DA = 2; };
template <> struct Ms1D<T_Q6_K> { static constexpr int DW = 1, DA = 2; };

// LEAN: one-deep rings, sized for two waves per SIMD (mmqs1_lean_t)
template <int T, bool AB, bool G, bool LEAN>
__device__ __forceinline__ void mmqs1_body(const MsArgs& M, const ActQ8& act_in) {
    constexpr int DW = LEAN ? 1 : Ms1D<T>::DW, DA = LEAN ? 1 : Ms1D<T>::DA;
    const int lane = threadIdx.x & 63;
    const int col = lane & 31, h = lane >> 5;
    const int nb = act_in.K >> 8;
    const int kp = (int)blockIdx.x % M.kp, g = (int)blockIdx.x / M.kp;
    const int sb0 = kp * M.sbw, nsb = min(M.sbw, nb - sb0);
    // this workgroup's token rows: [r0, r0 + ntk) of the partial row space, read from the
    // activation's 32-row tile r0 / 32 (grouped: expert e's tile z; exits past its rows)
    ActQ8 act = act_in;
    int r0 = 0, ntk = act_in.ntok;
    long long eoff = 0;
    if (G) {
        const int e = blockIdx.y, z = blockIdx.z;
        const int cnt = M.grp[M.grp_n + 1 + e];
        if (z * 32 >= cnt) return;
        r0 = M.grp[e] + z * 32;
        ntk = min(32, cnt - z * 32);
        const int tt = r0 >> 5;
        act.q += (long long)tt * nb * 8192;
        act.bsb += (long long)tt * nb * 512;
        act.dT += tt * 32;
        eoff = (long long)e * M.grp_stride;
    }
    int seg = 0, rt = g;
#pragma unroll
    for (int i = 0; i < MMQ_SEGS - 1; ++i)
        if (i + 1 < M.n && seg == i && rt >= M.nrt[i]) {
            rt -= M.nrt[i];
            seg = i + 1;
        }
    const uint8_t* swA = seg == 0 ? M.sw[0] : seg == 1 ? M.sw[1] : M.sw[2];
    const int rows_s = seg == 0 ? M.rows[0] : seg == 1 ? M.rows[1] : M.rows[2];
    const int prow_s = seg == 0 ? M.prow[0] : seg == 1 ? M.prow[1] : M.prow[2];
    constexpr int TB = mmq32_tile_bytes_d(T);
    const uint8_t* tile0 = swA + eoff + ((long long)rt * nb + sb0) * TB;
    // activation first, then weights (loads retire in order: superblock 0's act is never queued
    // behind later weights)
    MsAct a[DA];
#pragma unroll
    for (int d = 0; d < DA; ++d) a[d] = ms_act_load(act, sb0 + min(d, nsb - 1), lane);
    MsW<T> w[DW];
#pragma unroll
    for (int d = 0; d < DW; ++d) w[d] = ms_load<T>(tile0 + (long long)min(d, nsb - 1) * TB, lane);
    float y[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) y[e] = 0.0f;
    // fully unrolled over the part's (at most MS_SBW) superblocks: every ring slot is a value of its
    // own, so a refill issued before the slot's dots needs no register copy
#pragma unroll
    for (int s = 0; s < MS_SBW; ++s) {
        if (s < nsb) {
            const MsAct ca = a[s % DA];
            const MsW<T> cw = w[s % DW];
            if (s + DA < nsb) a[s % DA] = ms_act_load(act, sb0 + s + DA, lane);
            if (s + DW < nsb) w[s % DW] = ms_load<T>(tile0 + (long long)(s + DW) * TB, lane);
            ms1_sb<T>(cw, ca, lane, y);
        }
    }
    const int rr = AB ? rt * 16 + (col & 15) : rt * 32 + col;
    if (rr >= rows_s) return;
    const int prow = prow_s + (AB && col >= 16 ? M.nff : 0) + rr;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int tok = (r & 3) + 8 * (r >> 2) + 4 * h;
        if (tok < ntk) M.part[((long long)kp * M.prows + r0 + tok) * M.pstride + prow] = y[r];
    }
}
template <int T, bool AB, bool G>
__global__ __launch_bounds__(64) void mmqs1_t(const MsArgs M, const ActQ8 act) { mmqs1_body<T, AB, G, false>(M, act); }
template <int T, bool AB, bool G>
__global__ __launch_bounds__(64, 2) void mmqs1_lean_t(const MsArgs M, const ActQ8 act) { mmqs1_body<T, AB, G, true>(M, act); }


}  // namespace mmq

int mmqs_parts(int K) { return (K / 256 + mmq::MS_SBW - 1) / mmq::MS_SBW; }

bool mmqs_grouped_supported(int type) { return type == T_Q4_K || type == T_Q5_K || type == T_Q6_K; }

// ---------------------------------------------------------------------------
// Where a short launch is chosen.  mmqs_plan (mmq_plan's MMQ_SHORT form) is a pure function of the
// launch's shape; mmqs_fn is the one table from a plan to the instantiated kernel; the launchers
// check their arguments, fill MsArgs, ask for the plan and launch it.
// ---------------------------------------------------------------------------
namespace {
// mmqs_t's LDS: q [sbw][NT] 8 KiB | k-quants: bsb [sbw][NT] 1 KiB, dT [sbw] 256 B | Q8_0: dT [sbw][8] 256 B
size_t mmqs_lds(int T, int nt) {
    return mmq::MS_SBW * nt * 8192 + (T != T_Q8_0 ? mmq::MS_SBW * nt * 1024 + mmq::MS_SBW * 256 : mmq::MS_SBW * 8 * 256);
}
}  // namespace

MmqPlan mmqs_plan(const MmqShape& s) {
    const bool grouped = s.grp_n > 0;
    if (grouped && !mmqs_grouped_supported(s.type)) return mmq_no_plan("mmqs grouped: Q4_K / Q5_K / Q6_K experts only");
    if (!mmq32_supported(s.type)) return mmq_no_plan("mmqs: Q4_K / Q5_K / Q6_K / Q8_0 / Q4_0 / Q5_0 only");
    if (s.nseg < 1 || s.nseg > mmq::MMQ_SEGS || ((s.pair || grouped) && s.nseg != 1))
        return mmq_no_plan("mmqs: 1..3 matrices (a pair: one)");
    if (s.K % 256 || s.K <= 0) return mmq_no_plan("mmqs: K must be a multiple of 256");
    if (grouped && (s.npad % 32 || s.npad < 32)) return mmq_no_plan("mmqs grouped: the MoE rows are whole 32-row tiles");
    if (grouped && (s.grp_max < 1 || s.grp_max > MMQS_MAX)) return mmq_no_plan("mmqs grouped: bad expert / row count");
    if (!grouped && s.npad != 32 && s.npad != 64) return mmq_no_plan("mmqs: 1..64 tokens");
    MmqPlan k{};
    k.T = mmq::mmq_op_type(s.type);   // Q4_0 / Q5_0: their copies are Q8_0 tiles
    k.pair = s.pair;
    k.grouped = grouped;
    for (int i = 0; i < s.nseg; ++i) k.nrb += s.pair ? (s.rows[i] + 15) / 16 : (s.rows[i] + 31) / 32;   // row tiles
    // (half-width parts for the launches of few row blocks, 7B WO / V at 128 workgroups, measured no
    // faster: 20-token verify 3.46 vs 3.24 ms)
    k.kp = mmqs_parts(s.K);
    k.nt = grouped ? 1 : s.npad / 32;
    k.grid_y = k.grid_z = 1;
    if (k.nt == 1 && k.T != T_Q8_0) {
        // one token tile, k-quants: the one-wave register form (3.42 vs 3.50 ms for the LDS form, r05).
        // Q4_K / Q5_K on the one-deep-ring, two-waves-per-SIMD form (214-220 VGPRs instead of 246-256
        // at one wave: 20-token verify 7B 3.61 -> 3.40 ms, Mixtral 18.2 -> 15.7 ms, same box, r05);
        // Q6_K keeps its two-deep ring at one wave (the lean form at two waves spills).
        k.kernel = k.T == T_Q6_K ? MK_SHORT1 : MK_SHORT1_LEAN;
        k.grid_x = k.nrb * k.kp;
        if (grouped) {   // an expert holds at most grp_max rows (one per token routed to it)
            k.grid_y = s.grp_n;
            k.grid_z = (s.grp_max + 31) / 32;
        }
        k.block = 64;
        return k;
    }
    k.kernel = MK_SHORT;
    k.grid_x = (k.nrb + mmq::MS_NW - 1) / mmq::MS_NW * k.kp;
    k.block = 64 * mmq::MS_NW;
    k.lds = mmqs_lds(k.T, k.nt);
    return k;
}

namespace {
typedef void (*MmqsFn)(const mmq::MsArgs, const ActQ8);
template <int T>
MmqsFn mmqs_fn_t(const MmqPlan& k) {
    if (k.kernel == MK_SHORT) {
        if (k.nt == 2) return k.pair ? mmq::mmqs_t<T, true, 2> : mmq::mmqs_t<T, false, 2>;
        if constexpr (T == T_Q8_0) return k.pair ? mmq::mmqs_t<T, true, 1> : mmq::mmqs_t<T, false, 1>;
        return nullptr;   // (one token tile of k-quants is mmqs1's)
    }
    if constexpr (T == T_Q4_K || T == T_Q5_K) {
        if (k.kernel != MK_SHORT1_LEAN) return nullptr;
        if (k.grouped) return k.pair ? mmq::mmqs1_lean_t<T, true, true> : mmq::mmqs1_lean_t<T, false, true>;
        return k.pair ? mmq::mmqs1_lean_t<T, true, false> : mmq::mmqs1_lean_t<T, false, false>;
    }
    if constexpr (T == T_Q6_K) {
        if (k.kernel != MK_SHORT1) return nullptr;
        if (k.grouped) return k.pair ? mmq::mmqs1_t<T, true, true> : mmq::mmqs1_t<T, false, true>;
        return k.pair ? mmq::mmqs1_t<T, true, false> : mmq::mmqs1_t<T, false, false>;
    }
    return nullptr;
}
// the only place the short kernels are instantiated
MmqsFn mmqs_fn(const MmqPlan& k) {
    switch (k.T) {
    case T_Q4_K: return mmqs_fn_t<T_Q4_K>(k);
    case T_Q5_K: return mmqs_fn_t<T_Q5_K>(k);
    case T_Q6_K: return mmqs_fn_t<T_Q6_K>(k);
    case T_Q8_0: return mmqs_fn_t<T_Q8_0>(k);
    default: return nullptr;
    }
}

void mmqs_launch(const MmqShape& sh, mmq::MsArgs& M, const ActQ8& act, float* part, int pstride, int nff, hipStream_t s) {
    const MmqPlan k = mmq_plan(MMQ_SHORT, sh, 0);
    if (k.kernel == MK_NONE) throw Error(k.why);
    M.nrt_tot = k.nrb;
    M.sbw = mmq::MS_SBW;
    M.kp = k.kp;
    M.nff = nff;
    M.part = part;
    M.pstride = pstride;
    M.prows = act.ntok;
    hipLaunchKernelGGL(mmqs_fn(k), dim3(k.grid_x, k.grid_y, k.grid_z), dim3(k.block), k.lds, s, M, act);
    MI_HIP(hipGetLastError());
}
}  // namespace

// Once per device (init_gemm_attributes): the LDS limit of every mmqs_t instantiation a plan can name
// (the mmqs1 kernels use no LDS).
void init_mmqs_attributes() {
    for (int T : {T_Q4_K, T_Q5_K, T_Q6_K, T_Q8_0})
        for (int nt : {1, 2})
            for (bool pair : {false, true}) {
                MmqPlan k{};
                k.kernel = MK_SHORT;
                k.T = T;
                k.nt = nt;
                k.pair = pair;
                if (MmqsFn f = mmqs_fn(k))
                    MI_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(f), hipFuncAttributeMaxDynamicSharedMemorySize,
                                               (int)mmqs_lds(T, nt)));
            }
}

int launch_mmqs(const QMat* const* mats, const int* prow, int n, bool pair, int nff, const ActQ8& act, float* part,
                int pstride, hipStream_t s) {
    if (n < 1 || n > mmq::MMQ_SEGS || (pair && n != 1)) throw Error("mmqs: 1..3 matrices (a pair: one)");
    if (!mmq32_supported(mats[0]->type)) throw Error("mmqs: Q4_K / Q5_K / Q6_K / Q8_0 / Q4_0 / Q5_0 only");
    if (takes_q80(mats[0]->type) != (act.q80 != 0)) throw Error("mmqs: Q8_0 weights take Q8_0 activations, k-quants Q8_K");
    if (act.ntok < 1 || act.ntok > MMQS_MAX || (act.npad != 32 && act.npad != 64) || act.npad < act.ntok)
        throw Error("mmqs: 1..64 tokens");
    if (act.K % 256 || act.K <= 0) throw Error("mmqs: K must be a multiple of 256");
    mmq::MsArgs M{};
    MmqShape sh{};
    sh.type = mats[0]->type;
    sh.pair = pair;
    sh.nseg = M.n = n;
    sh.npad = act.npad;
    sh.K = act.K;
    for (int i = 0; i < n; ++i) {
        const QMat& A = *mats[i];
        if (A.type != mats[0]->type || A.K != act.K || !A.sw) throw Error("mmqs: the matrices share type and K, with MFMA-order copies");
        M.sw[i] = A.sw;
        sh.rows[i] = M.rows[i] = A.rows;
        M.nrt[i] = pair ? (A.rows + 15) / 16 : (A.rows + 31) / 32;
        M.prow[i] = prow[i];
        const int top = prow[i] + A.rows + (pair ? nff : 0);
        if (prow[i] < 0 || top > pstride || (pair && nff < A.rows)) throw Error("mmqs: partial rows past the stride");
    }
    mmqs_launch(sh, M, act, part, pstride, nff, s);
    return M.kp;
}

int launch_mmqs_grouped(const QMat& A, bool pair, int nff, const ActQ8& act, float* part, int pstride, const int* grp,
                        int n_expert, int max_rows, hipStream_t s) {
    if (!mmqs_grouped_supported(A.type)) throw Error("mmqs grouped: Q4_K / Q5_K / Q6_K experts only");
    if (act.q80) throw Error("mmqs grouped: k-quant experts take Q8_K activations");
    if (!A.sw || A.K != act.K || act.K % 256 || act.K <= 0) throw Error("mmqs grouped: the experts' MFMA-order copies, K a multiple of 256");
    if (act.ntok != act.npad || act.npad % 32 || act.npad < 32) throw Error("mmqs grouped: the MoE rows are whole 32-row tiles");
    if (n_expert < 1 || n_expert > A.n_exp || max_rows < 1 || max_rows > MMQS_MAX) throw Error("mmqs grouped: bad expert / row count");
    if (A.rows + (pair ? nff : 0) > pstride || (pair && nff < A.rows)) throw Error("mmqs grouped: partial rows past the stride");
    mmq::MsArgs M{};
    MmqShape sh{};
    sh.type = A.type;
    sh.pair = pair;
    sh.nseg = M.n = 1;
    sh.npad = act.npad;
    sh.K = act.K;
    sh.grp_n = n_expert;
    sh.grp_max = max_rows;
    M.sw[0] = A.sw;
    sh.rows[0] = M.rows[0] = A.rows;
    M.nrt[0] = pair ? (A.rows + 15) / 16 : (A.rows + 31) / 32;
    M.prow[0] = 0;
    M.grp = grp;
    M.grp_n = n_expert;
    M.grp_stride = A.sw_expert_stride;
    mmqs_launch(sh, M, act, part, pstride, nff, s);
    return M.kp;
}

}  // namespace mi
