// The tiled int8-MFMA GEMM of a physical batch of up to UB_MAX tokens (n_ubatch, reference
// Instance.hpp:24): prompt ingestion and batched verification past MMQS_MAX tokens (shorter
// batches: mmqs.hip).  The arithmetic contract and the MFMA geometry are mmq_common.h's.
//
// swizzle_kernel builds a matrix's MFMA-order copy once at load (the tile layouts: mmq_common.h).
//
// mmq2_t: a workgroup computes a 128-token x 32*RT-row block (8 waves: wave wv computes token tile
// wv & 3 x row tile wv >> 2, one 32x32 tile), its operands staged in LDS by LDS-DMA
// (global_load_lds_dwordx4):
//   * the weight tiles of the block's RT row tiles and the activation tiles of its 4 token tiles
//     for superblock sb + 1 land in one stage while superblock sb is computed from the other;
//     every piece address is a scalar base + a lane offset, computed once per token block;
//   * Q4_K / Q5_K: the 4 waves of a row tile first decode its superblock into int8 operand
//     planes of the SCALED weights sc_j * q (q45_planes, every plane byte <= 127), so the MFMAs
//     accumulate sum_j sc_j * dot_j over the 8 sub-blocks themselves: the nibble split and scale
//     work is done once per row tile instead of once per wave, and there is no integer multiply
//     per sub-block and result (VALU was the bound: ~310 VALU against 10 MFMAs per wave and
//     superblock); the min terms sum_j m_j * bsum_j are two more MFMAs (bsum = 64 hi + lo);
//   * Q6_K: the scaled hi/lo operands of the MFMA-order copy, accumulated by the MFMA; Q8_0:
//     one MFMA per 32-block and a float update per block (vec_dot_q8_0_q8_0's order);
//   * per 32x32 tile the integer sums are the contract's exact int32 values, and the float update
//     is one fmaf chain per superblock in superblock order: y = fmaf(-dmin_x d_y, mins,
//     fmaf(d_x d_y, S, y)) (Q6_K: fmaf(d_x d_y, S, y)).
// The token blocks of a row block are placed on one XCD (blockIdx % 8), so their weight reads
// share its L2.  LDS: NST stages of [RT weight slots of SLOT bytes][4 x 8 KiB activations][2 KiB
// bsb][dT: 1 KiB, Q8_0 4 KiB], then (Q4_K / Q5_K) the operand planes [RT][NPL][8 sub-blocks][64
// lanes x 16 B] (struct M2).
//
// Where a launch is chosen: mmq_plan (below) from the launch's shape, mmq2_fn from the plan to the
// instantiation; init_mmq2_attributes walks the same table once per device.
#include "mmq_common.h"
#include <algorithm>

namespace mi {
namespace mmq {

__global__ void swizzle_kernel(const QMat A, const QMat B, int pair, uint8_t* dst) {
    const int nb = A.nb;
    const long long tile = blockIdx.x;   // rt * nb + sb
    const int rt = (int)(tile / nb), sb = (int)(tile % nb);
    const int TB = mmq32_tile_bytes_d(A.type);
    uint8_t* o = dst + tile * TB;
    for (int off = threadIdx.x; off < TB; off += blockDim.x) {
        int plane, c, byte;
        if (A.type == T_Q4_0 || A.type == T_Q5_0) {
            const bool q5 = A.type == T_Q5_0;
            if (off < 8192) {   // element l = 16h + e of block jj as int8: the nibble (| the qh bit) - 8 (16)
                const int jj = off >> 10, ln = (off >> 4) & 63, e = off & 15;
                const int cc = ln & 31, l = 16 * (ln >> 5) + e;
                const QMat& M = (pair && cc >= 16) ? B : A;
                long long row = pair ? 16LL * rt + (cc & 15) : 32LL * rt + cc;
                if (row >= M.rows) row = M.rows - 1;
                const long long b = row * nb + sb;
                const uint8_t qb = M.p[0][b * 128 + jj * 16 + (l & 15)];
                int q = l < 16 ? (qb & 0xF) : (qb >> 4);
                if (q5) {
                    const uint8_t* hp = M.p[1] + b * 32 + jj * 4;
                    const unsigned qh = hp[0] | (hp[1] << 8) | (hp[2] << 16) | ((unsigned)hp[3] << 24);
                    q |= (int)((qh >> l) & 1u) << 4;
                }
                o[off] = (uint8_t)(int8_t)(q - (q5 ? 16 : 8));
                continue;
            }
            plane = q5 ? 2 : 1; c = (off - 8192) >> 4; byte = (off - 8192) & 15;
        } else if (A.type == T_Q8_0) {
            if (off < 8192) {
                const int jj = off >> 10, ln = (off >> 4) & 63, e = off & 15;
                plane = 0; c = ln & 31; byte = 32 * jj + 16 * (ln >> 5) + e;
            } else {
                plane = 1; c = (off - 8192) >> 4; byte = (off - 8192) & 15;
            }
        } else if (A.type == T_Q4_K) {
            if (off < 4096) {
                const int p = off >> 10, ln = (off >> 4) & 63, e = off & 15;
                plane = 0; c = ln & 31; byte = 32 * p + 16 * (ln >> 5) + e;
            } else {
                plane = 1; c = (off - 4096) >> 4; byte = (off - 4096) & 15;
            }
        } else if (A.type == T_Q5_K) {
            if (off < 4096) {
                const int p = off >> 10, ln = (off >> 4) & 63, e = off & 15;
                plane = 0; c = ln & 31; byte = 32 * p + 16 * (ln >> 5) + e;
            } else if (off < 5120) {
                const int ln = (off - 4096) >> 4, e = off & 15;
                plane = 1; c = ln & 31; byte = 16 * (ln >> 5) + e;
            } else {
                plane = 2; c = (off - 5120) >> 4; byte = (off - 5120) & 15;
            }
        } else {   // Q6_K
            if (off < 16384) {   // w = (q - 32) * scale of element 32s + 16h + e (dequantize_row_q6_K)
                const int lo = off >= 8192, o2 = off & 8191;
                const int sp = o2 >> 10, ln = (o2 >> 4) & 63, e = o2 & 15;
                const int cc = ln & 31, h = ln >> 5, l = 16 * h + e, hf = sp >> 2, qq = sp & 3;
                const QMat& M = (pair && cc >= 16) ? B : A;
                long long row = pair ? 16LL * rt + (cc & 15) : 32LL * rt + cc;
                if (row >= M.rows) row = M.rows - 1;
                const long long b = row * nb + sb;
                const int ql = M.p[0][b * 128 + 64 * hf + l + 32 * (qq & 1)];
                const int qh = M.p[1][b * 64 + 32 * hf + l];
                const int sc = (int)(signed char)M.p[2][b * 16 + 8 * hf + 2 * qq + h];
                const int q = ((qq >= 2 ? ql >> 4 : ql & 0xF) | (((qh >> (2 * qq)) & 3) << 4)) - 32;
                const int w = q * sc;
                o[off] = (uint8_t)(lo ? (w & 63) : (w >> 6));
                continue;
            }
            plane = 3; c = (off - 16384) >> 1; byte = (off - 16384) & 1;
        }
        const QMat& M = (pair && c >= 16) ? B : A;
        long long row = pair ? 16LL * rt + (c & 15) : 32LL * rt + c;
        if (row >= M.rows) row = M.rows - 1;
        const int pb = (A.type == T_Q4_0 || A.type == T_Q5_0) ? 16
                     : A.type == T_Q8_0 ? (plane == 0 ? 256 : 16)
                     : A.type == T_Q4_K ? (plane == 0 ? 128 : 16)
                     : A.type == T_Q5_K ? (plane == 0 ? 128 : plane == 1 ? 32 : 16)
                                        : (plane == 0 ? 128 : plane == 1 ? 64 : plane == 2 ? 16 : 2);
        o[off] = M.p[plane][(row * nb + sb) * pb + byte];
    }
}

// The epilogue of one 32-token x 32-row D tile (v: this lane's 16 results).
// GX: the GPT-2 instantiations (llm_build_gpt2): bias (the segment's rows; null: none) is added to
// y before everything else, and EPI_GELU is compiled in -- ggml_vec_gelu_f32 through the f16 table,
// gemv.hip's EPI_GELU expression.  The other instantiations carry no trace of either.
template <bool AB, bool GX>
__device__ __forceinline__ void mmq_epilogue(const GemmParams& P, int tend, const float2* rope, int ttok0,
                                             int lane, int row, const float v[16], int epi, int nrows,
                                             float* out, const float* pre, const float* bias) {
    const int col = lane & 31, h = lane >> 5;
    const bool roped = epi == EPI_ROPE_Q || epi == EPI_ROPE_K;
    float bv = 0.0f;
    if constexpr (GX) {
        if (bias && row < nrows) bv = bias[row];   // this lane's weight row
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int tok = ttok0 + (r & 3) + 8 * (r >> 2) + 4 * h;
        float vr = v[r];
        if constexpr (GX) {
            if (bias) vr += bv;   // ggml_add of the projection bias
        }
        if (pre && tok < tend && row < nrows)   // a LoRA adapter's term, before the epilogue
            vr += pre[(long long)tok * P.pre_stride + row];
        const float pv = __shfl_xor(vr, AB ? 16 : 1, 64);   // SwiGLU partner / RoPE partner
        if (tok >= tend) continue;
        if (AB) {
            if (col >= 16 || row >= nrows) continue;
            out[(long long)tok * P.out_stride + row] = silu(vr) * pv;   // silu(gate) * up
            continue;
        }
        if (row >= nrows) continue;
        float o = vr;
        if (roped) {
            const int i0 = row % P.head_dim;
            if (i0 < P.n_rot) {
                const float2 cs = rope[(long long)tok * (P.n_rot / 2) + i0 / 2];
                o = (col & 1) ? pv * cs.y + vr * cs.x : vr * cs.x - pv * cs.y;
            }
        }
        const int* tp = P.tokpos + tok * 4;
        switch (epi) {
        case EPI_STORE:
        case EPI_ROPE_Q: out[(long long)tok * P.out_stride + row] = o; break;
        case EPI_ADD: {
            const long long i = (long long)tok * P.out_stride + row;
            float s = o + P.resid[i];
            if (P.addend) s = s + P.addend[row];
            out[i] = s;
            break;
        }
        case EPI_ROPE_K: {
            const int cell = tp[2];
            P.kcache[(long long)cell * P.kv_dim + row] = __float2half_rn(o);
            if (row == 0) P.cell_pos[cell] = tp[1];
            break;
        }
        case EPI_V: P.vcache[(long long)tp[2] * P.kv_dim + row] = __float2half_rn(o); break;
        default:
            if constexpr (GX) {
                if (epi == EPI_GELU) {
                    const unsigned short hb = __half_as_ushort(__float2half_rn(o));
                    const float t = __half2float(__ushort_as_half(P.gelu_tab[hb]));
                    out[(long long)tok * P.out_stride + row] = o <= -10.0f ? 0.0f : (o >= 10.0f ? o : t);
                }
            }
            break;
        }
    }
}

// the matrices (row segments) of one launch: MMQ_SEGS at most, all of one type over one activation
struct MmqSegs {
    const uint8_t* sw[MMQ_SEGS];
    int rows[MMQ_SEGS];
    int epi[MMQ_SEGS];
    int n;
    int pre_off[MMQ_SEGS];    // GemmParams::pre_off of each segment
    int bias_off[MMQ_SEGS];   // the segment's first row in GemmParams::bias (launch_mmq32_rows)
};

template <int T> struct M2 {
    static constexpr int RT = 2;                                        // row tiles per block
    static constexpr int NW = 4 * RT;                                    // waves: one 32x32 tile each
    static constexpr int TB = mmq32_tile_bytes_d(T);                    // bytes of a tile-superblock
    static constexpr int SLOT = (TB + 1023) / 1024 * 1024;
    static constexpr int A_OFF = RT * SLOT;
    static constexpr int BSB_OFF = A_OFF + 4 * 8192;
    static constexpr int DT_OFF = BSB_OFF + 2048;
    static constexpr int DT_KB = T == T_Q8_0 ? 4 : 1;
    static constexpr int STAGE = DT_OFF + DT_KB * 1024;
    static constexpr int NI = STAGE / 1024;                             // 1 KiB LDS-DMA pieces
    static constexpr int NIW = (NI + NW - 1) / NW;                      // per wave (some repeat)
    static constexpr int NPL = 2;                                       // K-quant operand planes
    static constexpr int PLANES = (T == T_Q4_K || T == T_Q5_K) ? RT * NPL * 8 * 1024 : 0;
    static constexpr int lds(int nst) { return nst * STAGE + PLANES; }
};

// The two int8 operand planes of the scaled weights sc_j * q of sub-blocks 2w, 2w + 1 of one row
// (lane) of a Q4_K / Q5_K tile, every byte <= 127:
//   Q4_K (sc = 8 sh + sl, q <= 15):  P0 = q * sl, P1 = q * sh,  sc q = P0 + 8 P1
//   Q5_K (q = lo4 + 16 hb <= 31):    p = sc * q <= 1953 (16-bit products),
//                                    P0 = p & 127, P1 = p >> 7,  sc q = P0 + 128 P1
// hd: the row's header, wq: its qs piece w, qh (Q5_K): its high bits.  o0 / o1: P0 / P1 of
// sub-block 2w, o2 / o3: of sub-block 2w + 1.  (r06: a copy holding these planes pre-decoded,
// 3.7x the tile bytes, measured slower -- the L2->LDS copies bound this GEMM)
template <int T>
__device__ __forceinline__ void q45_planes(const u32x4 hd, const u32x4 wq, const u32x4 qh, int w, u32x4& o0, u32x4& o1,
                                           u32x4& o2, u32x4& o3) {
    const unsigned Y = hd.y, W = hd.w;
    // get_scale_min_k4 for j = 2w, 2w + 1
    int s0, s1;
    if (w < 2) {
        s0 = (Y >> (16 * w)) & 63;
        s1 = (Y >> (16 * w + 8)) & 63;
    } else {
        const int k = 2 * w - 4;
        s0 = ((W >> (8 * k)) & 0xF) | (((Y >> (8 * k + 6)) & 3) << 4);
        s1 = ((W >> (8 * k + 8)) & 0xF) | (((Y >> (8 * k + 14)) & 3) << 4);
    }
    const unsigned q[4] = {wq.x, wq.y, wq.z, wq.w};
    unsigned* p0 = reinterpret_cast<unsigned*>(&o0);
    unsigned* p1 = reinterpret_cast<unsigned*>(&o1);
    unsigned* p2 = reinterpret_cast<unsigned*>(&o2);
    unsigned* p3 = reinterpret_cast<unsigned*>(&o3);
    if (T == T_Q4_K) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const unsigned lo = q[i] & 0x0F0F0F0Fu, hi = (q[i] >> 4) & 0x0F0F0F0Fu;
            p0[i] = bmul(lo, s0 & 7);
            p1[i] = bmul(lo, s0 >> 3);
            p2[i] = bmul(hi, s1 & 7);
            p3[i] = bmul(hi, s1 >> 3);
        }
    } else {
        const unsigned b[4] = {qh.x, qh.y, qh.z, qh.w};
        // 4 elements q (bytes) times s as 16-bit products, split into lo7 / hi bytes
        auto split = [](unsigned q5, unsigned sc, unsigned& lo, unsigned& hi) {
            const unsigned m02 = wmul16(q5 & 0x00FF00FFu, sc), m13 = wmul16((q5 >> 8) & 0x00FF00FFu, sc);
            lo = (m02 & 0x007F007Fu) | ((m13 & 0x007F007Fu) << 8);
            hi = ((m02 >> 7) & 0x001F001Fu) | (((m13 >> 7) & 0x001F001Fu) << 8);
        };
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const unsigned q5a = (q[i] & 0x0F0F0F0Fu) | (((b[i] >> (2 * w)) & 0x01010101u) << 4);
            const unsigned q5b = ((q[i] >> 4) & 0x0F0F0F0Fu) | (((b[i] >> (2 * w + 1)) & 0x01010101u) << 4);
            split(q5a, s0, p0[i], p1[i]);
            split(q5b, s1, p2[i], p3[i]);
        }
    }
}

// NST 2: two stages (copy of sb + 1 during sb), one workgroup per CU.  NST 1: one stage, copy and
// compute in turn, sized (LDS, <= 128 VGPRs) for two workgroups per CU that overlap each other.
// PRE: the instantiation that adds GemmParams::pre (launched only when it is set: the other kernels
// carry no trace of it).  GX: the GPT-2 instantiation (GemmParams::bias, EPI_GELU), likewise its own.
template <int T, bool AB, int NST, bool PRE, bool GX>
__global__ __launch_bounds__(64 * M2<T>::NW) __attribute__((amdgpu_waves_per_eu(NST == 1 ? 4 : 2)))
void mmq2_t(const GemmParams P, const ActQ8 act, const float2* rope, const MmqSegs S) {
    using C = M2<T>;
    constexpr int RT = C::RT;
    constexpr int NPL = C::NPL;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int w = wv & 3;                             // this wave's token tile
    const int wr = wv >> 2;                           // this wave's row tile (of the block's RT)
    const int col = lane & 31, h = lane >> 5;
    const int nb = P.K >> 8;
    // segments: S.n matrices of this type over the same activation in one grid (Q / K / V),
    // their row blocks concatenated; segment s: S.rows[s] rows, MFMA-order copy S.sw[s],
    // epilogue S.epi[s].  A plain or grouped launch is one segment.
    int nrb = 0;
#pragma unroll
    for (int i = 0; i < MMQ_SEGS; ++i)
        if (i < S.n) nrb += ((AB ? (S.rows[i] + 15) / 16 : (S.rows[i] + 31) / 32) + RT - 1) / RT;
    const int ntb = (act.npad + 127) / 128;           // token blocks
    const int TB = C::TB;
    // split-K: part kh of the grid's ksplit parts takes superblocks [nb kh / ks, nb (kh + 1) / ks)
    const int ks = P.ksplit > 1 ? P.ksplit : 1;
    const int nbid = (int)gridDim.x / ks;
    const int kh = (int)blockIdx.x / nbid, bid = (int)blockIdx.x % nbid;
    const int sb0 = nb * kh / ks, sb1 = nb * (kh + 1) / ks;
    int rb, tb_b, tb_e, base, tend, grp_e = 0;
    if (P.grp) {
        // grouped (MoE): blockIdx -> (token block, expert, row block), token block slowest: the
        // first blocks of every expert go first, an expert's later blocks (its tokens past 128)
        // after them, and a block past its expert's tokens exits
        const int nrb8 = (nrb + 7) / 8 * 8;
        const int per = nrb8 * P.grp_n;
        const int tbi = bid / per, rem = bid % per;
        const int e = rem / nrb8;
        grp_e = e;
        rb = rem % nrb8;
        if (rb >= nrb) return;
        base = P.grp[e];
        const int cnt = P.grp[P.grp_n + 1 + e];
        if (tbi * 128 >= cnt) return;
        tend = base + cnt;
        tb_b = tbi;
        tb_e = tbi + 1;
    } else {
        // blockIdx -> (row block, token block): the token blocks of a row block on one XCD
        const int b = bid, xcd = b & 7, slot = b >> 3;
        rb = (slot / ntb) * 8 + xcd;
        tb_b = slot % ntb;
        tb_e = tb_b + 1;
        base = 0;
        tend = act.ntok;
        if (rb >= nrb) return;
    }
    // this row block's segment
    int seg = 0;
#pragma unroll
    for (int i = 0; i < MMQ_SEGS - 1; ++i) {
        const int nrb_i = ((AB ? (S.rows[i] + 15) / 16 : (S.rows[i] + 31) / 32) + RT - 1) / RT;
        if (i + 1 < S.n && seg == i && rb >= nrb_i) {
            rb -= nrb_i;
            seg = i + 1;
        }
    }
    const int rows_s = seg == 0 ? S.rows[0] : seg == 1 ? S.rows[1] : S.rows[2];
    const int epi_s = seg == 0 ? S.epi[0] : seg == 1 ? S.epi[1] : S.epi[2];
    const int nrt = AB ? (rows_s + 15) / 16 : (rows_s + 31) / 32;
    const uint8_t* swA = seg == 0 ? S.sw[0] : seg == 1 ? S.sw[1] : S.sw[2];
    if (P.grp) swA += (long long)grp_e * P.grp_stride;
    const int tile_end = (tend + 31) / 32;            // tiles past the batch's (group's) last: clamped
  for (int tb = tb_b; tb < tb_e; ++tb) {
    // (grouped: the previous token block's last stage may still be read by other waves)
    if (tb != tb_b) __builtin_amdgcn_s_barrier();
    const int tok0 = base + tb * 128;
    const int tile0 = tok0 / 32;
    const int ntt = min(4, tile_end - tile0);         // token tiles of this block

    // ---- the LDS-DMA copy of superblock sb into stage st: piece i (1 KiB) of the stage image.
    // Every piece is a wave-uniform base (scalar registers) + a per-lane 32-bit offset; the bases
    // of superblock 0 and their per-superblock steps are computed once per token block.
    auto ubase = [](const void* p) {
        const unsigned long long v = reinterpret_cast<unsigned long long>(p);
        const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
        return reinterpret_cast<const uint8_t*>(((unsigned long long)hi << 32) | lo);
    };
    const uint8_t* pbase[C::NIW];
    unsigned pstep[C::NIW], pvo[C::NIW];
#pragma unroll
    for (int k = 0; k < C::NIW; ++k) {
        int i = wv + C::NW * k;
        if (i >= C::NI) i = C::NI - 1;                // a repeated piece: same bytes, same place
        const int off = i * 1024;                     // byte offset of the piece in the stage
        if (off < C::A_OFF) {                         // weight slot r, bytes o.. within it
            const int r = off / C::SLOT, o = off % C::SLOT;
            const int rt = min(rb * RT + r, nrt - 1);
            pbase[k] = ubase(swA + (long long)rt * nb * TB + o);
            pstep[k] = TB;
            pvo[k] = o + lane * 16 < TB ? lane * 16 : 0;   // past the tile: any valid bytes (padding)
        } else if (off < C::BSB_OFF) {                // activation tile t, 1 KiB piece j
            const int o = off - C::A_OFF, t = o >> 13, j = (o >> 10) & 7;
            const int tt = min(tile0 + t, tile_end - 1);
            pbase[k] = ubase(act.q + (long long)tt * nb * 8192 + j * 1024);
            pstep[k] = 8192;
            pvo[k] = lane * 16;
        } else if (off < C::DT_OFF) {                 // bsb of tiles 2q, 2q+1 (512 B each)
            // (tiles past the batch's last are clamped to it: their slots are never read, and
            // a batch of one or three tiles has no tile pair to read)
            const int q = (off - C::BSB_OFF) >> 10;
            const int tt = min(tile0 + 2 * q, tile_end - 1), t2 = min(tile0 + 2 * q + (lane >> 5), tile_end - 1);
            pbase[k] = ubase(act.q80 ? reinterpret_cast<const int8_t*>(act.q) : act.bsb + (long long)tt * nb * 512);
            pstep[k] = act.q80 ? 0u : 512u;
            pvo[k] = act.q80 ? 0u : (unsigned)((t2 - tt) * nb * 512 + (lane & 31) * 16);
        } else {                                      // dT: 128 tokens x 4 B per row of dT
            const int q = (off - C::DT_OFF) >> 10;    // Q8_0: rows 8sb + 2q, 8sb + 2q + 1
            pbase[k] = ubase(act.dT + (long long)(act.q80 ? 2 * q : 0) * act.npad + tok0);
            pstep[k] = (unsigned)(act.q80 ? 8 : 1) * act.npad * 4u;
            const int tk = min(4 * (lane & 31), act.npad - 4 - tok0);
            pvo[k] = (unsigned)(tk * 4 + (act.q80 ? (lane >> 5) * act.npad * 4 : 0));
        }
    }
    auto copy_stage = [&](int sb, int st) {
        char* base = smem + st * C::STAGE;
#pragma unroll
        for (int k = 0; k < C::NIW; ++k) {
            int i = wv + C::NW * k;
            if (i >= C::NI) i = C::NI - 1;
            // (written as one offset: `ub + pvo[k]` here drops the kernel's host stub, hipcc 7.2)
            const uint8_t* ub = pbase[k] + (size_t)((unsigned long long)sb * pstep[k] + pvo[k]);
            __builtin_amdgcn_global_load_lds(gp(ub), (__attribute__((address_space(3))) void*)(base + i * 1024), 16, 0, 0);
        }
    };

    float y[1][16];
#pragma unroll
    for (int e = 0; e < 16; ++e) y[0][e] = 0.0f;

    copy_stage(sb0, NST == 2 ? (sb0 & 1) : 0);
#pragma unroll 1
    for (int sb = sb0; sb < sb1; ++sb) {
        // this wave's copy of superblock sb landed, then the workgroup's (barrier; LDS-DMA is a
        // pending LDS write on the VM counter).  Past the barrier every wave is done with
        // superblock sb - 1, whose stage takes the copy of sb + 1 (in flight during this step)
        // and whose operand planes take this step's decode.
        __builtin_amdgcn_s_waitcnt((0x7 << 4) | (0xF << 8));   // vmcnt(0)
        __builtin_amdgcn_s_barrier();
        if (NST == 2 && sb + 1 < sb1) copy_stage(sb + 1, (sb + 1) & 1);
        const lchar* stg = (const lchar*)(smem + (NST == 2 ? (sb & 1) : 0) * C::STAGE);
        const lchar* A0 = stg + C::A_OFF + w * 8192 + lane * 16;       // this wave's token tile
        const lchar* dTw = stg + C::DT_OFF + (w * 32 + 4 * h) * 4;
        // a wave whose token tile is past the block's tokens (or row tile past the matrix) skips
        // its MFMAs (it still copies and decodes for the others): partial blocks, MoE groups
        const bool busy = w < ntt && rb * RT + wr < nrt;
        if (T == T_Q8_0) {
          if (busy) {
#pragma unroll 2
            for (int j = 0; j < 8; ++j) {
                const v4i a = lds_ld<v4i>(A0 + j * 1024);
                {
                    constexpr int r = 0;
                    const lchar* wt = stg + wr * C::SLOT;
                    const v4i wq = lds_ld<v4i>(wt + j * 1024 + lane * 16);
                    const unsigned dwp = lds_ld<unsigned>(wt + 8192 + col * 16 + (j >> 1) * 4);
                    const float dwj = h2f(dwp >> (16 * (j & 1)));
                    const v16i dj = mfma(a, wq);
                    const lchar* dT8 = dTw + (j >> 1) * 1024 + (j & 1) * 512;
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const f32x4 dx4 = lds_ld<f32x4>(dT8 + 32 * g);
                        const float dx[4] = {dx4.x, dx4.y, dx4.z, dx4.w};
#pragma unroll
                        for (int i = 0; i < 4; ++i) y[r][4 * g + i] = fmaf((float)dj[4 * g + i], dwj * dx[i], y[r][4 * g + i]);
                    }
                    asm volatile("" ::: "memory");   // no LDS load hoisted across sub-blocks
                }
            }
          }
        } else if (T == T_Q4_K || T == T_Q5_K) {
            // (1) decode: the 4 waves of row tile wr turn its superblock into two int8 operand
            //     planes of the scaled weights sc_j * q, every byte <= 127:
            //       Q4_K (sc = 8 sh + sl, q <= 15):  P0 = q * sl, P1 = q * sh,  sc q = P0 + 8 P1
            //       Q5_K (q = lo4 + 16 hb <= 31):    p = sc * q <= 1953 (16-bit products),
            //                                        P0 = p & 127, P1 = p >> 7,  sc q = P0 + 128 P1
            //     and the MFMAs accumulate the scaled sub-block sums over all 8 sub-blocks exactly
            //     (no integer multiply per result); wave w decodes piece w (sub-blocks 2w, 2w + 1)
            //     for every lane's row.
            const lchar* wt = stg + wr * C::SLOT;
            lchar* pl = (lchar*)(smem + NST * C::STAGE) + wr * (NPL * 8 * 1024) + lane * 16;
            constexpr int HDO = T == T_Q5_K ? 5120 : 4096;
            {
                const u32x4 hd = lds_ld<u32x4>(wt + HDO + col * 16);
                const u32x4 wq = lds_ld<u32x4>(wt + w * 1024 + lane * 16);
                const u32x4 qh = T == T_Q5_K ? lds_ld<u32x4>(wt + 4096 + lane * 16) : u32x4{0, 0, 0, 0};
                u32x4 o0, o1, o2, o3;   // P0/P1 of sub-block 2w, P0/P1 of sub-block 2w + 1
                q45_planes<T>(hd, wq, qh, w, o0, o1, o2, o3);
                *reinterpret_cast<__attribute__((address_space(3))) u32x4*>(pl + (0 * 8 + 2 * w) * 1024) = o0;
                *reinterpret_cast<__attribute__((address_space(3))) u32x4*>(pl + (1 * 8 + 2 * w) * 1024) = o1;
                *reinterpret_cast<__attribute__((address_space(3))) u32x4*>(pl + (0 * 8 + 2 * w + 1) * 1024) = o2;
                *reinterpret_cast<__attribute__((address_space(3))) u32x4*>(pl + (1 * 8 + 2 * w + 1) * 1024) = o3;
                __builtin_amdgcn_s_waitcnt((0xF) | (0x3 << 14) | (0x7 << 4));   // lgkmcnt(0): planes written
                __builtin_amdgcn_s_barrier();
            }
            // (2) the MFMAs: token tile w x row tile wr, the planes accumulated over the sub-blocks
            if (busy) {
                constexpr int r = 0;
                const u32x4 hd = lds_ld<u32x4>(wt + HDO + col * 16);
                v16i acc0 = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, acc1 = acc0;
                const lchar* plr = (const lchar*)pl;
                // every operand of the superblock read first (at 2 waves per SIMD the LDS latency
                // is hidden only by reads in flight: counted waits, not lgkmcnt(0) per MFMA pair)
                v4i av[8], b0[8], b1[8];
                auto ld = [&](int j) {
                    av[j] = lds_ld<v4i>(A0 + j * 1024);
                    b0[j] = lds_ld<v4i>(plr + (0 * 8 + j) * 1024);
                    b1[j] = lds_ld<v4i>(plr + (1 * 8 + j) * 1024);
                };
                auto mm = [&](int j) {
                    if (NST == 2) {
                        pin(av[j]);
                        pin(b0[j]);
                        pin(b1[j]);
                    }
                    acc0 = __builtin_amdgcn_mfma_i32_32x32x32_i8(av[j], b0[j], acc0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_i32_32x32x32_i8(av[j], b1[j], acc1, 0, 0, 0);
                };
                // sub-blocks 0-3 read, then 4-7 read while 0-3 run
#pragma unroll
                for (int j = 0; j < 4; ++j) ld(j);
                if (NST == 2) pin_all();
#pragma unroll
                for (int j = 4; j < 8; ++j) ld(j);
#pragma unroll
                for (int j = 0; j < 8; ++j) mm(j);
                // sum_j m_j*bsum_j: mins as int8 B operands, k 0-7 (against hi) / k 8-15 (against lo)
                const unsigned Y = hd.y, Z = hd.z, W = hd.w;
                const int m03 = (int)(Z & 0x3F3F3F3Fu);
                const int m47 = (int)(((W >> 4) & 0x0F0F0F0Fu) | ((Z >> 2) & 0x30303030u));
                (void)Y;
                const v4i bm1 = h == 0 ? v4i{m03, m47, 0, 0} : v4i{0, 0, 0, 0};
                const v4i bm2 = h == 0 ? v4i{0, 0, m03, m47} : v4i{0, 0, 0, 0};
                const v4i ab = h == 0 ? lds_ld<v4i>(stg + C::BSB_OFF + w * 512 + col * 16) : v4i{0, 0, 0, 0};
                const v16i x1 = mfma(ab, bm1);
                const v16i x2 = mfma(ab, bm2);
                const float dr = h2f(hd.x), dmr = h2f(hd.x >> 16);
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const f32x4 dx4 = lds_ld<f32x4>(dTw + 32 * g);
                    const float dx[4] = {dx4.x, dx4.y, dx4.z, dx4.w};
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int e = 4 * g + i;
                        const int S = acc0[e] + (T == T_Q5_K ? 128 : 8) * acc1[e];
                        const float d = dr * dx[i], dm = dmr * dx[i];
                        y[r][e] = fmaf(-dm, (float)(64 * x1[e] + x2[e]), fmaf(d, (float)S, y[r][e]));
                    }
                }
            }
        } else {   // Q6_K: the 8 spans of w = 64*hi + lo, each operand accumulated by the MFMA
            if (busy) {
                constexpr int r = 0;
                const lchar* wt = stg + wr * C::SLOT;
                v16i ah = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, al = ah;
                v4i av[8], bh[8], bl[8];   // operands read first (counted LDS waits)
#pragma unroll
                for (int sp = 0; sp < 8; ++sp) {
                    av[sp] = lds_ld<v4i>(A0 + sp * 1024);
                    bh[sp] = lds_ld<v4i>(wt + sp * 1024 + lane * 16);
                    bl[sp] = lds_ld<v4i>(wt + 8192 + sp * 1024 + lane * 16);
                }
#pragma unroll
                for (int sp = 0; sp < 8; ++sp) {
                    if (NST == 2) {
                        pin(av[sp]);
                        pin(bh[sp]);
                        pin(bl[sp]);
                    }
                    ah = __builtin_amdgcn_mfma_i32_32x32x32_i8(av[sp], bh[sp], ah, 0, 0, 0);
                    al = __builtin_amdgcn_mfma_i32_32x32x32_i8(av[sp], bl[sp], al, 0, 0, 0);
                }
                const float dr = h2f(lds_ld<unsigned short>(wt + 16384 + col * 2));
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const f32x4 dx4 = lds_ld<f32x4>(dTw + 32 * g);
                    const float dx[4] = {dx4.x, dx4.y, dx4.z, dx4.w};
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int e = 4 * g + i;
                        y[r][e] = fmaf(dr * dx[i], (float)(ah[e] * 64 + al[e]), y[r][e]);
                    }
                }
            }
        }
        __builtin_amdgcn_s_waitcnt((0xF) | (0x3 << 14) | (0x7 << 4));   // lgkmcnt(0): this wave's LDS reads done
        if (NST == 1 && sb + 1 < sb1) {   // the one stage is free once every wave is past it
            __builtin_amdgcn_s_barrier();
            copy_stage(sb + 1, 0);
        }
    }
    // ---- epilogue: token tile w, row tile rb*RT + wr (no LDS: the next block's copy may start)
    const int rt = rb * RT + wr;
    if (w < ntt && rt < nrt) {
        const int row = AB ? rt * 16 + (col & 15) : rt * 32 + col;
        // split-K: this part's partial sums, stored plainly; else the segment's epilogue
        if (P.ksplit > 1)
            mmq_epilogue<AB, false>(P, tend, rope, tok0 + 32 * w, lane, row, y[0], EPI_STORE, rows_s,
                                    P.part + (long long)kh * P.ntok * P.out_stride, nullptr, nullptr);
        else {
            // (GemmParams::pre: this segment's rows; a pair's up lanes read the up rows' terms)
            const float* pre = nullptr;
            if constexpr (PRE) {
                const int po = seg == 0 ? S.pre_off[0] : seg == 1 ? S.pre_off[1] : S.pre_off[2];
                pre = P.pre + po + (AB && col >= 16 ? P.pre_up : 0);
            }
            const float* bias = nullptr;
            if constexpr (GX) {
                const int bo = seg == 0 ? S.bias_off[0] : seg == 1 ? S.bias_off[1] : S.bias_off[2];
                if (P.bias) bias = P.bias + bo;
            }
            mmq_epilogue<AB, GX>(P, tend, rope, tok0 + 32 * w, lane, row, y[0], epi_s, rows_s, P.out, pre, bias);
        }
    }
  }
}

}  // namespace mmq

bool mmq32_supported(int type) {
    return type == T_Q4_K || type == T_Q5_K || type == T_Q6_K || type == T_Q8_0 || is_legacy_quant(type);
}

int mmq32_tile_bytes(int type) { return mmq::mmq32_tile_bytes_d(type); }

size_t mmq32_copy_bytes(const QMat& A, bool pair) {
    const long long nrt = pair ? (A.rows + 15) / 16 : (A.rows + 31) / 32;
    return (size_t)nrt * A.nb * mmq32_tile_bytes(A.type);
}

void launch_mmq32_swizzle(const QMat& A, const QMat* B, uint8_t* dst, hipStream_t s) {
    if (!mmq32_supported(A.type)) throw Error("mmq32 swizzle: Q4_K / Q5_K / Q6_K / Q8_0 only");
    if (B && (B->type != A.type || B->rows != A.rows || B->K != A.K)) throw Error("mmq32 swizzle: bad pair");
    const long long nrt = B ? (A.rows + 15) / 16 : (A.rows + 31) / 32;
    hipLaunchKernelGGL(mmq::swizzle_kernel, dim3((unsigned)(nrt * A.nb)), dim3(256), 0, s, A, B ? *B : A, B ? 1 : 0, dst);
    MI_HIP(hipGetLastError());
}

// ---------------------------------------------------------------------------
// Where a tiled launch is chosen.  mmq_plan is a pure function of the launch's shape and the CU
// count; mmq2_fn is the one table from a plan to the instantiated kernel; launch_mmq2 fills the
// shape from its arguments, asks for the plan and launches it.
// ---------------------------------------------------------------------------
namespace {
const char* const MMQ32_TYPES = "mmq32: Q4_K / Q5_K / Q6_K / Q8_0 only";
const char* const MMQ2_SPLITK = "mmq2: split-K (2 or 4 parts) is for a single EPI_ADD matrix with a partials buffer";
const char* const MMQ2_GX = "mmq2: bias / GELU launches take one plain matrix, no pre, no split-K";

size_t mmq2_lds(int T, int nst) {
    switch (T) {
    case T_Q4_K: return mmq::M2<T_Q4_K>::lds(nst);
    case T_Q5_K: return mmq::M2<T_Q5_K>::lds(nst);
    case T_Q6_K: return mmq::M2<T_Q6_K>::lds(nst);
    default: return mmq::M2<T_Q8_0>::lds(nst);
    }
}
}  // namespace

MmqPlan mmqs_plan(const MmqShape& s);   // mmqs.hip

MmqPlan mmq_plan(MmqForm form, const MmqShape& s, int n_cu) {
    if (form == MMQ_SHORT) return mmqs_plan(s);
    if (!mmq32_supported(s.type)) return mmq_no_plan(MMQ32_TYPES);
    if (s.nseg < 1 || s.nseg > mmq::MMQ_SEGS || (s.pair && s.nseg != 1)) return mmq_no_plan("mmq2: 1..3 segments (a pair: one)");
    constexpr int RT = mmq::M2<T_Q4_K>::RT, NW = mmq::M2<T_Q4_K>::NW;   // (the same for every type)
    MmqPlan k{};
    k.kernel = MK_TILED;
    k.T = mmq::mmq_op_type(s.type);
    k.pair = s.pair;
    k.grouped = s.grp_n > 0;
    for (int i = 0; i < s.nseg; ++i) k.nrb += ((s.pair ? (s.rows[i] + 15) / 16 : (s.rows[i] + 31) / 32) + RT - 1) / RT;
    k.ntb = (s.npad + 127) / 128;
    // grouped (MoE): a workgroup per (token block, expert, row block)
    const int g1 = (k.nrb + 7) / 8 * 8 * (k.grouped ? s.grp_n * ((std::max(s.grp_max, 1) + 127) / 128) : k.ntb);
    if (s.ksplit > 1 && (k.grouped || s.pair || s.nseg != 1 || s.K / 256 < s.ksplit || (s.ksplit != 2 && s.ksplit != 4)))
        return mmq_no_plan(MMQ2_SPLITK);
    const int g2 = g1 * (s.ksplit > 1 ? s.ksplit : 1);
    // one stage (two workgroups per CU) when the grid fills two workgroups per CU, else two stages
    // (one per CU).  7B 512-token prefill, one vs two stages: 15.5 vs 16.8 ms (same box, r04)
    k.nst = g2 >= 2 * n_cu ? 1 : 2;
    k.pre = s.pre && s.ksplit <= 1;
    // the GPT-2 instantiations: a projection bias and / or GELU (single matrices; no pre, no split-K)
    k.gx = s.gx;
    if (k.gx && (k.pair || k.pre || s.ksplit > 1 || k.grouped)) return mmq_no_plan(MMQ2_GX);
    k.grid_x = g2;
    k.grid_y = k.grid_z = 1;
    k.block = 64 * NW;
    k.lds = mmq2_lds(k.T, k.nst);
    return k;
}

namespace {
typedef void (*Mmq2Fn)(const GemmParams, const ActQ8, const float2*, const mmq::MmqSegs);
template <int T, int NST>
Mmq2Fn mmq2_fn_tn(const MmqPlan& k) {
    if (k.gx) return mmq::mmq2_t<T, false, NST, false, true>;
    if (k.pre) return k.pair ? mmq::mmq2_t<T, true, NST, true, false> : mmq::mmq2_t<T, false, NST, true, false>;
    return k.pair ? mmq::mmq2_t<T, true, NST, false, false> : mmq::mmq2_t<T, false, NST, false, false>;
}
template <int T>
Mmq2Fn mmq2_fn_t(const MmqPlan& k) { return k.nst == 1 ? mmq2_fn_tn<T, 1>(k) : mmq2_fn_tn<T, 2>(k); }
// the only place mmq2_t is instantiated
Mmq2Fn mmq2_fn(const MmqPlan& k) {
    switch (k.T) {
    case T_Q4_K: return mmq2_fn_t<T_Q4_K>(k);
    case T_Q5_K: return mmq2_fn_t<T_Q5_K>(k);
    case T_Q6_K: return mmq2_fn_t<T_Q6_K>(k);
    case T_Q8_0: return mmq2_fn_t<T_Q8_0>(k);
    default: return nullptr;
    }
}

// the CU count of each device init_mmq2_attributes has run on (0: it has not)
constexpr int MMQ_MAX_DEV = 64;
int mmq_dev_cus[MMQ_MAX_DEV] = {};
int mmq_n_cu() {
    int dev = 0;
    MI_HIP(hipGetDevice(&dev));
    if (dev < 0 || dev >= MMQ_MAX_DEV || !mmq_dev_cus[dev]) throw Error("mmq2: init_gemm_attributes has not run on this device");
    return mmq_dev_cus[dev];
}
}  // namespace

// Once per device (init_gemm_attributes): the LDS limit of every instantiation a plan can name, and
// the device's CU count for the plans of its launches.
void init_mmq2_attributes() {
    for (int T : {T_Q4_K, T_Q5_K, T_Q6_K, T_Q8_0})
        for (int nst : {1, 2})
            for (int v = 0; v < 5; ++v) {   // plain, pair, pre, pair + pre, gx
                MmqPlan k{};
                k.kernel = MK_TILED;
                k.T = T;
                k.nst = nst;
                k.pair = v == 1 || v == 3;
                k.pre = v == 2 || v == 3;
                k.gx = v == 4;
                MI_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(mmq2_fn(k)), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)mmq2_lds(T, nst)));
            }
    int dev = 0, cus = 0;
    MI_HIP(hipGetDevice(&dev));
    MI_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    if (dev >= 0 && dev < MMQ_MAX_DEV) mmq_dev_cus[dev] = cus;
}

namespace {
// one mmq2 launch over the segments S (all of p.A's type; one segment unless launch_mmq32_multi /
// launch_mmq32_rows)
void launch_mmq2(const GemmParams& p, const mmq::MmqSegs& S, const ActQ8& act, const float2* rope, hipStream_t s) {
    MmqShape sh{};
    sh.type = p.A.type;
    sh.pair = p.pair == PAIR_AB;
    sh.nseg = S.n;
    for (int i = 0; i < S.n; ++i) sh.rows[i] = S.rows[i];
    sh.npad = act.npad;
    sh.K = p.A.nb * 256;
    sh.grp_n = p.grp ? p.grp_n : 0;
    sh.grp_max = p.grp_max;
    sh.ksplit = p.ksplit;
    sh.pre = p.pre != nullptr;
    sh.gx = p.bias != nullptr;
    for (int i = 0; i < S.n; ++i) sh.gx = sh.gx || S.epi[i] == EPI_GELU;
    if (p.grp && p.grp_n < 1) throw Error("mmq2: a grouped launch names its experts");
    if (p.ksplit > 1 && (p.epi != EPI_ADD || !p.part)) throw Error(MMQ2_SPLITK);
    const MmqPlan k = mmq_plan(MMQ_TILED, sh, mmq_n_cu());
    if (k.kernel == MK_NONE) throw Error(k.why);
    if (k.gx)
        for (int i = 0; i < S.n; ++i)
            if (S.epi[i] == EPI_GELU && !p.gelu_tab) throw Error("mmq2: the GELU epilogue needs the table");
    hipLaunchKernelGGL(mmq2_fn(k), dim3(k.grid_x), dim3(k.block), k.lds, s, p, act, rope, S);
    MI_HIP(hipGetLastError());
}

// the argument checks every tiled launch shares (a segment of launch_mmq32_multi: its own p);
// npad_max: UB_MAX, or the MoE rows' 4 * UB_MAX of a grouped launch
void mmq32_check(const GemmParams& p, int epi, const ActQ8& act, const float2* rope, int npad_max) {
    if (!mmq32_supported(p.A.type)) throw Error(MMQ32_TYPES);
    if (takes_q80(p.A.type) != (act.q80 != 0)) throw Error("mmq32: Q8_0 weights take Q8_0 activations, k-quants Q8_K");
    if (act.K != p.K || p.A.K != p.K) throw Error("mmq32: activation length differs from K");
    if (act.ntok < 1 || act.npad % 32 || act.npad > npad_max) throw Error("mmq32: bad token count");
    if (!p.A.sw) throw Error("mmq32: the matrix has no MFMA-order copy");
    if ((epi == EPI_ROPE_Q || epi == EPI_ROPE_K) && (!rope || p.head_dim % 2 || p.n_rot > p.head_dim))
        throw Error("mmq32: RoPE epilogue needs the rope table");
}
}  // namespace

void launch_mmq32_multi(const GemmParams* ps, int n, const ActQ8& act, const float2* rope, hipStream_t s) {
    bool one = n >= 2 && n <= mmq::MMQ_SEGS;
    for (int i = 0; i < n && one; ++i)
        one = ps[i].A.type == ps[0].A.type && ps[i].pair != PAIR_AB && !ps[i].grp && ps[i].K == ps[0].K &&
              ps[i].A.sw && ps[i].A.K == ps[0].K && ps[i].epi != EPI_SWIGLU;
    if (!one) {
        for (int i = 0; i < n; ++i) launch_mmq32(ps[i], act, rope, s);
        return;
    }
    mmq::MmqSegs S{};
    S.n = n;
    for (int i = 0; i < n; ++i) {   // the same checks as one launch each (the shared fields are ps[0]'s)
        const GemmParams& p = ps[i];
        mmq32_check(p, p.epi, act, rope, UB_MAX);
        if (p.out != ps[0].out || p.out_stride != ps[0].out_stride || p.resid != ps[0].resid)
            throw Error("mmq32 multi: the segments share one output buffer");
        if (p.pre != ps[0].pre || p.pre_stride != ps[0].pre_stride)
            throw Error("mmq32 multi: the segments share one pre-epilogue buffer");
        S.sw[i] = p.A.sw;
        S.rows[i] = p.A.rows;
        S.epi[i] = p.epi;
        S.pre_off[i] = p.pre_off;
    }
    launch_mmq2(ps[0], S, act, rope, s);
}

void launch_mmq32(const GemmParams& p, const ActQ8& act, const float2* rope, hipStream_t s) {
    mmq32_check(p, p.epi, act, rope, p.grp ? 4 * UB_MAX : UB_MAX);
    const bool ab = p.pair == PAIR_AB;
    if (ab && (p.B.type != p.A.type || p.B.rows != p.A.rows || p.epi != EPI_SWIGLU))
        throw Error("mmq32: a pair launch is gate/up SwiGLU of one type");
    if (!ab && p.epi == EPI_SWIGLU) throw Error("mmq32: SwiGLU needs a pair");
    mmq::MmqSegs S{};
    S.n = 1;
    S.sw[0] = p.A.sw;
    S.rows[0] = p.A.rows;
    S.epi[0] = p.epi;
    S.pre_off[0] = p.pre_off;
    launch_mmq2(p, S, act, rope, s);
}

void launch_mmq32_rows(const GemmParams& p, const int* row0, const int* nrows, const int* epi, int n, const ActQ8& act,
                       const float2* rope, hipStream_t s) {
    if (n < 1 || n > mmq::MMQ_SEGS) throw Error("mmq32 rows: 1..3 segments");
    for (int i = 0; i < n; ++i) mmq32_check(p, epi[i], act, rope, UB_MAX);
    if (p.pair == PAIR_AB || p.grp || p.ksplit > 1 || p.pre) throw Error("mmq32 rows: one plain matrix");
    mmq::MmqSegs S{};
    S.n = n;
    const size_t tile_row = (size_t)p.A.nb * mmq32_tile_bytes(p.A.type);   // one 32-row tile of the copy
    for (int i = 0; i < n; ++i) {
        if (row0[i] < 0 || row0[i] % 32 || nrows[i] < 1 || row0[i] + nrows[i] > p.A.rows)
            throw Error("mmq32 rows: a segment starts at a multiple of 32 rows, inside the matrix");
        // (a segment that ends inside a row tile reads the next segment's rows of that tile and
        // drops them: every tile of the copy is whole)
        S.sw[i] = p.A.sw + (size_t)(row0[i] / 32) * tile_row;
        S.rows[i] = nrows[i];
        S.epi[i] = epi[i];
        S.bias_off[i] = row0[i];
    }
    launch_mmq2(p, S, act, rope, s);
}

}  // namespace mi
