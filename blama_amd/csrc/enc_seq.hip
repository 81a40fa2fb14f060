// Several sequences per encoder call (gfx950, wave64): the segment-aware bidirectional attention
// and the per-sequence pooling of mi_encode_seqs.  The other launches of the pass (enc.hip) take
// the call's sequences laid end to end as so many token rows.
//
//  * enc_attn_seq_kernel<HD>: one workgroup of 4 waves per (head, 32-query tile of ONE sequence).
//    The host counts the tiles per sequence (enc_seq_lists), so a tile never straddles two
//    sequences; a tile reads the rows [start, start + len) of its sequence and nothing else.
//    The arithmetic is enc_attn_kernel's: q rounded to f16, KQ summed in f32, scaled; the two-pass
//    exact softmax over the sequence's keys (max, expf, the sum in double, p = e * (float)(1 / sum));
//    p rounded to f16; PV in f32.  Both products run on v_mfma_f32_32x32x16_f16, with the operand
//    and D layouts stated above enc_gemm_f16_kernel: A lane (row, half h) holds k = 8h .. 8h + 7
//    of its row, B lane (col, h) the same k of its column, D has the column on the lane and rows
//    (r & 3) + 8 (r >> 2) + 4 h in its registers.
//      QK^T: A = 32 keys straight from global memory (a lane's 16 bytes are 8 head dimensions of
//        its key; keys past the sequence's end are zero registers, never loaded), B = the tile's q,
//        rounded to f16 once into LDS.  HD / 16 chained MFMAs per 32-key block, the blocks dealt
//        round-robin to the waves.  D has the query on the lane and 4 x 4 consecutive keys in its
//        registers: the scaled scores go to LDS as 16-byte stores, [32][npad + 4] f32 (npad = len
//        rounded up to 32).
//      softmax: a wave per query row, 8 rows per wave; p is stored as f16, [32][npad + 8], zero
//        past the sequence's end and in the rows of queries past it.
//      PV: A = V transposed (row = head dimension, k = key), B = p (column = query, k = key).  V
//        streams through LDS in chunks of 128 keys, transposed on the way in: a thread loads the
//        same 8 head dimensions of two neighbouring keys and stores 8 dwords, each the pair of keys
//        of one head dimension, so a lane later reads 8 consecutive keys of its head dimension in
//        16 bytes.  HD 32: wave w takes the w-th 32-key block of every chunk.  HD 64: wave w takes
//        the 32-column half w & 1 and the key blocks 2 (w >> 1), 2 (w >> 1) + 1 of every chunk.
//        Each wave's partial 32 x 32 tile goes to LDS (over the scores, which are spent) and the
//        workgroup adds the partials in ascending wave order: ((p0 + p1) + p2) + p3 for HD 32,
//        p[half] + p[half + 2] for HD 64.
//    Batch invariance: every loop bound, every LDS offset and the order of every f32 and double
//    addition above is a function of (len, tile offset, HD) alone -- never of start, of the number
//    of sequences or of another sequence's contents.  A sequence's output rows therefore have the
//    same bits alone and in any batch.
//    ALIBI (jina-bert-v2; enc_jina.hip states the arithmetic): the scaled score takes slopes[head] *
//    -(float)|query - key| from the D layout's indices before it goes to LDS.  ALiBi makes the softmax
//    of a short sequence peaked, and the f16 rounding of a large p is then the pass's largest error
//    (2^-12 of p on average, straight into the output), so this variant carries the rounding's residual:
//    the softmax leaves p as f32 in the score row beside its f16 value, and PV runs a second MFMA on
//    lo = f16(p - (float)f16(p)) read from there.  The LDS layout is the same; the score rows are read
//    until the end of PV, so one barrier more stands before the partial tiles go over them.
//    LDS at len 512, HD 64: 66048 (scores) + 33280 (p) + 4608 (q) + 17408 (V chunk) = 121344 bytes
//    of the CU's 160 KiB.  The launch is sized by its longest sequence.
//  * enc_pool_seq_kernel: a workgroup per (sequence, 64 columns); embd_pool_kernel's arithmetic.
#include "enc_common.h"
#include "kernels.h"
#include "mi_engine.h"

#include <algorithm>
#include <cstring>
#include <string>

namespace mi {
namespace enc {

constexpr int SW = 4;          // waves per workgroup
constexpr int VC = 32 * SW;    // keys per staged V chunk
constexpr int VS = VC + 8;     // halves per row of the transposed chunk
constexpr int RS = 36;         // floats per row of a wave's partial output tile

// floats of the score region: the scores, or later the SW partial output tiles
__host__ __device__ inline int seq_sc_floats(int npad) { return 32 * (npad + 4) > SW * 32 * RS ? 32 * (npad + 4) : SW * 32 * RS; }

static size_t attn_seq_lds(int len, int hd) {
    const int npad = (len + 31) & ~31;
    return (size_t)seq_sc_floats(npad) * 4 + 32 * (size_t)(npad + 8) * 2 + 32 * (size_t)(hd + 8) * 2 + (size_t)hd * VS * 2;
}

template <int HD, bool ALIBI>
__global__ __launch_bounds__(64 * SW) void enc_attn_seq_kernel(const EncAttnSeq P) {
    constexpr int QS = HD + 8;           // halves per staged q row
    constexpr int NJ = HD / 16;          // MFMAs per 32-key block of QK^T
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int4 tile = reinterpret_cast<const int4*>(P.tiles)[blockIdx.y];
    const int start = tile.x, len = tile.y, off = tile.z;
    const int live = min(32, len - off);                         // queries of this tile
    const int npad = (len + 31) & ~31, SP = npad + 4, PS = npad + 8;
    float* sc = reinterpret_cast<float*>(smem);                  // [32][SP] scaled scores
    _Float16* ph = reinterpret_cast<_Float16*>(sc + seq_sc_floats(npad));   // [32][PS] p
    _Float16* qs = ph + 32 * PS;                                 // [32][QS] f16 q
    _Float16* vt = qs + 32 * QS;                                 // [HD][VS] V chunk, transposed
    const int head = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int col = lane & 31, h = lane >> 5;

    for (int i = tid; i < 32 * (HD / 4); i += 64 * SW) {
        const int t = i / (HD / 4), c = i - t * (HD / 4);
        float4 v = float4{0.0f, 0.0f, 0.0f, 0.0f};               // queries past the end: zero rows, never stored
        if (t < live) v = *reinterpret_cast<const float4*>(P.q + (long long)(start + off + t) * P.q_stride + head * HD + 4 * c);
        *reinterpret_cast<u32x2*>(qs + t * QS + 4 * c) = u32x2{pack2(v.x, v.y), pack2(v.z, v.w)};
    }
    __syncthreads();

    // ---- QK^T: D lane = query, registers = keys of the block ----
    const __half* kbase = P.k + (long long)start * P.kv_stride + head * HD + 8 * h;
    for (int kb = w; kb < (npad >> 5); kb += SW) {
        const int key = kb * 32 + col;
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            u32x4 a = u32x4{0u, 0u, 0u, 0u};
            if (key < len) a = *reinterpret_cast<const u32x4*>(kbase + (long long)key * P.kv_stride + 16 * j);
            const u32x4 b = *reinterpret_cast<const u32x4*>(qs + col * QS + 16 * j + 8 * h);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(as_h8(a), as_h8(b), acc, 0, 0, 0);
        }
        float* srow = sc + col * SP + kb * 32 + 4 * h;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            float4 v = float4{acc[4 * q] * P.scale, acc[4 * q + 1] * P.scale, acc[4 * q + 2] * P.scale, acc[4 * q + 3] * P.scale};
            if (ALIBI) {   // register 4 q + e of the lane's query off + col is key 32 kb + 8 q + 4 h + e
                const float m = P.slopes[head];
                const int qi = off + col, k0 = kb * 32 + 8 * q + 4 * h;
                v.x = v.x + m * alibi_dist(qi, k0);
                v.y = v.y + m * alibi_dist(qi, k0 + 1);
                v.z = v.z + m * alibi_dist(qi, k0 + 2);
                v.w = v.w + m * alibi_dist(qi, k0 + 3);
            }
            *reinterpret_cast<float4*>(srow + 8 * q) = v;
        }
    }
    __syncthreads();

    // ---- the exact softmax of each live query row (a wave per row), p rounded to f16 ----
    for (int j = 0; j < 8; ++j) {
        const int r = 8 * w + j;
        float* row = sc + r * SP;
        _Float16* prow = ph + r * PS;
        if (r >= live) {
            for (int c = lane; c < npad; c += 64) {
                prow[c] = (_Float16)0.0f;
                if (ALIBI) row[c] = 0.0f;
            }
            continue;
        }
        float mx = -INFINITY;
        for (int c = lane; c < len; c += 64) mx = fmaxf(mx, row[c]);
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
        double sum = 0.0;
        for (int c = lane; c < len; c += 64) {
            const float e = expf(row[c] - mx);
            row[c] = e;
            sum += (double)e;
        }
        sum = wave_sum_d(sum);
        const float inv = (float)(1.0 / sum);
        for (int c = lane; c < npad; c += 64) {
            const float p = c < len ? row[c] * inv : 0.0f;
            prow[c] = (_Float16)p;
            if (ALIBI) row[c] = p;   // the f32 value, for the residual of the rounding
        }
    }

    // ---- PV: D lane = query, registers = head dimensions of this wave's 32-column half ----
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    const __half* vbase = P.v + (long long)start * P.kv_stride + head * HD;
    for (int c0 = 0; c0 < npad; c0 += VC) {
        if (c0) __syncthreads();   // the previous chunk is read
        for (int i = tid; i < (VC / 2) * (HD / 8); i += 64 * SW) {
            const int kp = i & (VC / 2 - 1), ch = i / (VC / 2);
            const int key = c0 + 2 * kp;
            if (key >= npad) continue;   // blocks past npad are never read
            u32x4 a = u32x4{0u, 0u, 0u, 0u}, b = a;   // keys past the end: zero columns
            if (key < len) a = *reinterpret_cast<const u32x4*>(vbase + (long long)key * P.kv_stride + 8 * ch);
            if (key + 1 < len) b = *reinterpret_cast<const u32x4*>(vbase + (long long)(key + 1) * P.kv_stride + 8 * ch);
            unsigned* dst = reinterpret_cast<unsigned*>(vt + (8 * ch) * VS + 2 * kp);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                dst[(2 * e) * (VS / 2)] = (a[e] & 0xffffu) | (b[e] << 16);
                dst[(2 * e + 1) * (VS / 2)] = (a[e] >> 16) | (b[e] & 0xffff0000u);
            }
        }
        __syncthreads();
        auto block = [&](int kbl, int dh) {
            if (c0 + 32 * kbl >= npad) return;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const u32x4 a = *reinterpret_cast<const u32x4*>(vt + (32 * dh + col) * VS + 32 * kbl + 16 * j + 8 * h);
                const u32x4 b = *reinterpret_cast<const u32x4*>(ph + col * PS + c0 + 32 * kbl + 16 * j + 8 * h);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(as_h8(a), as_h8(b), acc, 0, 0, 0);
                if (ALIBI) {   // + V (p - f16(p)): the same 8 keys of the lane's query, from the f32 row
                    const float* pf = sc + col * SP + c0 + 32 * kbl + 16 * j + 8 * h;
                    const float4 x = *reinterpret_cast<const float4*>(pf), y = *reinterpret_cast<const float4*>(pf + 4);
                    const half8 hi = as_h8(b);
                    const u32x4 lo = u32x4{pack2(x.x - (float)hi[0], x.y - (float)hi[1]), pack2(x.z - (float)hi[2], x.w - (float)hi[3]),
                                           pack2(y.x - (float)hi[4], y.y - (float)hi[5]), pack2(y.z - (float)hi[6], y.w - (float)hi[7])};
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(as_h8(a), as_h8(lo), acc, 0, 0, 0);
                }
            }
        };
        if (HD == 32) {
            block(w, 0);
        } else {
            block(2 * (w >> 1), w & 1);
            block(2 * (w >> 1) + 1, w & 1);
        }
    }
    // every wave passed a barrier since its last read of the scores: the partial tiles go there
    if (ALIBI) __syncthreads();   // (this variant read them in PV)
    float* red = sc;   // [SW][32][RS]
#pragma unroll
    for (int q = 0; q < 4; ++q)
        *reinterpret_cast<float4*>(red + (w * 32 + col) * RS + 8 * q + 4 * h) = float4{acc[4 * q], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]};
    __syncthreads();
    for (int i = tid; i < 32 * (HD / 4); i += 64 * SW) {
        const int t = i / (HD / 4), d = 4 * (i - t * (HD / 4));
        if (t >= live) continue;
        const int w0 = HD == 32 ? 0 : d >> 5, dw = HD == 32 ? 1 : 2;    // the first partial and the step to the next
        const float* src = red + (w0 * 32 + t) * RS + (d & 31);
        float4 o = *reinterpret_cast<const float4*>(src);
#pragma unroll
        for (int k = dw; w0 + k < SW; k += dw) {
            const float4 p = *reinterpret_cast<const float4*>(src + k * 32 * RS);
            o.x = o.x + p.x;
            o.y = o.y + p.y;
            o.z = o.z + p.z;
            o.w = o.w + p.w;
        }
        *reinterpret_cast<float4*>(P.out + (long long)(start + off + t) * P.out_stride + head * HD + d) = o;
    }
}

__global__ __launch_bounds__(64) void enc_pool_seq_kernel(const EncPoolSeq P) {
    const int j = blockIdx.y * 64 + threadIdx.x;
    if (j >= P.K) return;
    const int4 s = reinterpret_cast<const int4*>(P.seqs)[blockIdx.x];
    const float* rows = P.rows + (long long)s.x * P.stride;
    float* out = P.out + (long long)blockIdx.x * P.K;
    if (P.pooling == MI_POOLING_CLS) {
        out[j] = rows[j];
    } else if (P.pooling == MI_POOLING_LAST) {
        out[j] = rows[(long long)(s.y - 1) * P.stride + j];
    } else {   // MEAN: each term rounded to f32, added in ascending token order
        const float inv = __int_as_float(s.z);
        float acc = 0.0f;
        for (int t = 0; t < s.y; ++t) acc = __fadd_rn(acc, __fmul_rn(rows[(long long)t * P.stride + j], inv));
        out[j] = acc;
    }
}

void init_attn_seq_attributes() {
    const int lds = (int)attn_seq_lds(ENC_MAX_TOK, 64);
    for (const void* f : {reinterpret_cast<const void*>(enc_attn_seq_kernel<32, false>), reinterpret_cast<const void*>(enc_attn_seq_kernel<64, false>),
                          reinterpret_cast<const void*>(enc_attn_seq_kernel<32, true>), reinterpret_cast<const void*>(enc_attn_seq_kernel<64, true>)})
        MI_HIP(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
}

}  // namespace enc

// the launch group of a sequence by its own length alone: 0 short, 1 long, 2 past ENC_MAX_LONG
static int seq_group(int len) { return len > ENC_MAX_LONG ? 2 : len > ENC_MAX_TOK ? 1 : 0; }

int enc_seq_lists(const int* seq_len, int n_seq, int* seqs, int* tiles, int* n_long, int* n_xlong) {
    int start = 0, cnt[3] = {0, 0, 0};
    for (int s = 0; s < n_seq; ++s) {
        const int len = seq_len[s];
        if (len < 1 || len > ENC_MAX_SEQ)
            throw Error("encoder sequences: sequence " + std::to_string(s) + " has " + std::to_string(len) + " tokens (1 to 8192)");
        const int g = seq_group(len), step = g == 2 ? ENC_XL_Q : 32;
        cnt[g] += (len + step - 1) / step;
        const float inv = 1.0f / (float)len;
        int bits;
        std::memcpy(&bits, &inv, sizeof bits);
        if (seqs) {
            int* q = seqs + 4 * s;
            q[0] = start, q[1] = len, q[2] = bits, q[3] = 0;
        }
        start += len;
    }
    if (n_long) *n_long = cnt[1];
    if (n_xlong) *n_xlong = cnt[2];
    const int total = cnt[0] + cnt[1] + cnt[2];
    if (!tiles) return total;
    // the short sequences' tiles from 0, then the long sequences', then the 128-query groups of the
    // sequences past ENC_MAX_LONG; each group in sequence order
    int at[3] = {0, cnt[0], cnt[0] + cnt[1]};
    start = 0;
    for (int s = 0; s < n_seq; ++s) {
        const int len = seq_len[s], g = seq_group(len);
        int& nt = at[g];
        for (int off = 0; off < len; off += g == 2 ? ENC_XL_Q : 32, ++nt) {
            int* t = tiles + 4 * nt;
            t[0] = start, t[1] = len, t[2] = off, t[3] = s;
        }
        start += len;
    }
    return total;
}

void launch_enc_attn_seq(const EncAttnSeq& p, hipStream_t s) {
    if (!enc_attn_supported(p.head_dim)) throw Error("enc attention: head_dim 32 or 64");
    if (p.n_head < 1 || p.n_seq < 1 || !p.seq_len || !p.tiles || !p.q || !p.k || !p.v || !p.out)
        throw Error("enc attention: unsupported shape");
    if (p.kv_stride % 8 || p.q_stride % 4 || p.out_stride % 4) throw Error("enc attention: kv_stride % 8, q_stride % 4, out_stride % 4");
    int n_long = 0, n_xlong = 0;
    const int n_tiles = enc_seq_lists(p.seq_len, p.n_seq, nullptr, nullptr, &n_long, &n_xlong);   // throws on a length outside 1 .. 8192
    long long total = 0;
    int longest = 0;   // of the sequences this file's kernel takes
    for (int i = 0; i < p.n_seq; ++i) {
        total += p.seq_len[i];
        if (p.seq_len[i] <= ENC_MAX_TOK) longest = std::max(longest, p.seq_len[i]);
    }
    if (total != p.ntok) throw Error("enc attention: the sequence lengths do not sum to ntok");
    const int n_short = n_tiles - n_long - n_xlong;
    if (n_short) {
        const dim3 grid(p.n_head, n_short), block(64 * enc::SW);
        const size_t lds = enc::attn_seq_lds(longest, p.head_dim);
        if (p.slopes) {
            if (p.head_dim == 32) hipLaunchKernelGGL((enc::enc_attn_seq_kernel<32, true>), grid, block, lds, s, p);
            else hipLaunchKernelGGL((enc::enc_attn_seq_kernel<64, true>), grid, block, lds, s, p);
        } else {
            if (p.head_dim == 32) hipLaunchKernelGGL((enc::enc_attn_seq_kernel<32, false>), grid, block, lds, s, p);
            else hipLaunchKernelGGL((enc::enc_attn_seq_kernel<64, false>), grid, block, lds, s, p);
        }
        MI_HIP(hipGetLastError());
    }
    if (n_long) {   // the long sequences' tiles follow the short ones' in the list
        EncAttnSeq l = p;
        l.tiles = p.tiles + 4 * n_short;
        launch_enc_attn_long(l, n_long, s);
    }
    if (n_xlong) {  // and the groups of the sequences past ENC_MAX_LONG follow those
        EncAttnSeq l = p;
        l.tiles = p.tiles + 4 * (n_short + n_long);
        launch_enc_attn_xlong(l, n_xlong, s);
    }
}

void launch_enc_pool_seq(const EncPoolSeq& p, hipStream_t s) {
    if (p.n_seq < 1 || p.K < 1 || !p.rows || !p.seqs || !p.out) throw Error("enc pool: unsupported shape");
    if (p.pooling != MI_POOLING_MEAN && p.pooling != MI_POOLING_CLS && p.pooling != MI_POOLING_LAST)
        throw Error("enc pool: pooling MEAN, CLS or LAST");
    hipLaunchKernelGGL(enc::enc_pool_seq_kernel, dim3(p.n_seq, (p.K + 63) / 64), dim3(64), 0, s, p);
    MI_HIP(hipGetLastError());
}

}  // namespace mi
