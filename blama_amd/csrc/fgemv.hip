// Batch-1 decode GEMV over F16 matrices, streaming form (gfx950, wave64): ggml_mul_mat of one token
// against an unquantised F16 matrix [rows][K] for the decode step of an all-F16 LLaMA model.
//
// Arithmetic (ggml's CPU path for F16 weights): the f32 activation is rounded to f16 once (RNE);
// the product of two f16 values is exact in f32; the products are added in f32.  The order of the
// additions is fixed by K alone: lane l of the row's wave adds the elements of its 16-byte pieces
// l, l + 64, l + 128, ... in ascending order, and the 64 lanes are combined by the DPP scan of
// wave_sum63.  Neither the grid, the role nor the kernel variant changes it: a row's result is
// bit-reproducible, and the same whether it is computed alone or among others.
//
// Shape, after dgemv.hip: one unit (a row, a RoPE row pair, a gate/up row pair) per wave, 8-wave
// workgroups, a grid of units / 8.  A wave requests every weight load of its unit at entry (up to
// FG_PASS 16-byte pieces per row and lane, 128 VGPRs; a gate/up or RoPE pair over K > 8192 takes a
// second pass) through a buffer resource bounded by the row, so pieces past the row's end and the
// waves past the last unit cost no memory access.  The activation arrives as f32 (the normed row a
// small launch wrote, the attention output, or h) and is requested ahead of the weights; the
// workgroup rounds it to f16 into LDS once, behind the weight loads.
#include "qdot.h"
#include <hip/hip_ext.h>

#include <cstring>

namespace mi {

namespace {

constexpr int FG_NW = 8;              // waves per workgroup
constexpr int FG_THREADS = FG_NW * 64;
constexpr int FG_PIECE = 64 * 8;      // halves one wave load covers (16 bytes per lane)

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));

struct FgArgs {
    const __half* w[3];
    int rows[3];
    int nmat, K, units;
    int nq, nk;                 // FG_QKV: rows of Q and K among the matrices' rows in order
    const float* x;             // [K]
    float* out;
    const float* resid;         // FG_ADD
    const float* addend;        // FG_ADD, optional
    const int* tokpos;          // FG_QKV: {token, pos, cell, -}
    int* cell_pos;
    __half* kcache;
    __half* vcache;
    const float* freq_factors;
    float theta_scale, freq_scale;
    int n_rot, head_dim, kv_dim;
};

__device__ __forceinline__ void fg_lds_barrier() {
    __builtin_amdgcn_s_waitcnt((0xF) | (0x3 << 14) | (0x7 << 4));   // lgkmcnt(0); vmcnt untouched
    __builtin_amdgcn_s_barrier();
}

// NC: 16-byte pieces per row and lane requested together (K <= NC * 512 in one pass);
// NX: 16-byte pieces of x per thread (K <= NX * 2048)
template <int ROLE, int NC, int NX>
__global__ __launch_bounds__(FG_THREADS) void fgemv_kernel(const FgArgs a) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    constexpr int RW = (ROLE == FG_QKV || ROLE == FG_SWIGLU) ? 2 : 1;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int u = (int)blockIdx.x * FG_NW + wave;
    const bool uv = u < a.units;
    const int uc = uv ? u : a.units - 1;
    const int K = a.K;
    const unsigned row_bytes = (unsigned)K * 2u;

    // ---- 1. the activation and the epilogue's inputs, requested before any weight
    f32x4 xv[NX];
    {
        const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.x), 0, K * 4, 0x00020000);
#pragma unroll
        for (int k = 0; k < NX; ++k)   // (pieces past K: out of the descriptor's range, zeros)
            xv[k] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(xr, (unsigned)(tid + FG_THREADS * k) * 16u, 0, 0));
    }
    i32x4 tp = {0, 0, 0, 0};
    if (ROLE == FG_QKV) tp = *gptr(reinterpret_cast<const i32x4*>(a.tokpos));
    float res = 0.0f;
    if (ROLE == FG_ADD) {
        const uint8_t* rb = reinterpret_cast<const uint8_t*>(rfl_ptr(a.resid));
        res = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(buf_rsrc(rb), oob((unsigned)uc * 4, !uv), 0, 0));
    }
    // the unit's rows: FG_SWIGLU gate row uc and up row uc; FG_QKV rows 2 uc, 2 uc + 1 of the
    // matrices laid end to end (every matrix has an even row count: a pair never straddles two)
    const int r0 = RW * uc;
    const __half* wrow[RW];
    if (ROLE == FG_SWIGLU) {
        wrow[0] = a.w[0] + (long long)uc * K;
        wrow[RW - 1] = a.w[1] + (long long)uc * K;
    } else {
        int r = ROLE == FG_QKV ? r0 : uc, mi = 0;
        if (a.nmat > 1 && r >= a.rows[0]) {
            r -= a.rows[0];
            mi = 1;
            if (a.nmat > 2 && r >= a.rows[1]) {
                r -= a.rows[1];
                mi = 2;
            }
        }
        wrow[0] = a.w[mi] + (long long)r * K;
        if (RW == 2) wrow[RW - 1] = wrow[0] + K;
    }
    const bool isq = ROLE == FG_QKV && r0 < a.nq;
    const bool isk = ROLE == FG_QKV && !isq && r0 < a.nq + a.nk;
    const int i0 = (ROLE == FG_QKV && (isq || isk)) ? (isq ? r0 : r0 - a.nq) % a.head_dim : 0;
    const bool roped = (isq || isk) && i0 < a.n_rot;
    float ff = 1.0f;
    if (ROLE == FG_QKV && a.freq_factors) {
        const uint8_t* fb = reinterpret_cast<const uint8_t*>(rfl_ptr(a.freq_factors));
        ff = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(buf_rsrc(fb), oob((unsigned)(i0 / 2) * 4, !roped), 0, 0));
    }
    asm volatile("" ::: "memory");

    // ---- 2. the first pass's weight loads (K <= NC * 512: all of them)
    __amdgpu_buffer_rsrc_t wr[RW];
#pragma unroll
    for (int r = 0; r < RW; ++r)
        wr[r] = __builtin_amdgcn_make_buffer_rsrc(const_cast<__half*>(rfl_ptr(wrow[r])), 0, (int)row_bytes, 0x00020000);
    u32x4 w[RW][NC];
    auto load_pass = [&](int k0) {
#pragma unroll
        for (int r = 0; r < RW; ++r)
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const unsigned off = ((unsigned)(k0 + c * FG_PIECE) + 8u * lane) * 2u;   // past the row: zeros
                w[r][c] = __builtin_amdgcn_raw_buffer_load_b128(wr[r], oob(off, !uv), 0, 0);
            }
    };
    load_pass(0);

    // ---- 3. the activation, rounded to f16 (RNE), into LDS
#pragma unroll
    for (int k = 0; k < NX; ++k) {
        const int i = tid + FG_THREADS * k;
        if (i * 4 < K) {
            const f16x4 hv = {(_Float16)xv[k].x, (_Float16)xv[k].y, (_Float16)xv[k].z, (_Float16)xv[k].w};
            *reinterpret_cast<f16x4*>(lds + i * 8) = hv;
        }
    }
    fg_lds_barrier();

    // ---- 4. the dot products: lane 63 holds each row's sum
    float acc[RW];
#pragma unroll
    for (int r = 0; r < RW; ++r) acc[r] = 0.0f;
    for (int k0 = 0; k0 < K; k0 += NC * FG_PIECE) {
        if (k0) load_pass(k0);
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const int e0 = k0 + c * FG_PIECE + 8 * lane;
            if (e0 < K) {   // (K % 8 == 0: a piece is whole or absent)
                const f16x8 xh = *reinterpret_cast<const f16x8*>(lds + e0 * 2);
#pragma unroll
                for (int r = 0; r < RW; ++r) {
                    const f16x8 wh = __builtin_bit_cast(f16x8, w[r][c]);
#pragma unroll
                    for (int e = 0; e < 8; ++e) acc[r] = acc[r] + (float)xh[e] * (float)wh[e];
                }
            }
        }
    }
    float y[RW];
#pragma unroll
    for (int r = 0; r < RW; ++r) y[r] = wave_sum63(acc[r]);

    // ---- 5. epilogue (lane 63)
    if (lane != 63 || !uv) return;
    if (ROLE == FG_QKV) {
        float o0 = y[0], o1 = y[RW - 1];
        if (roped) {   // ggml_rope_cache_init (ext_factor 0, mscale 1) for this pair, then rotate
            float theta = (float)tp.y;
            for (int k = 0; k < i0 / 2; ++k) theta = theta * a.theta_scale;
            const float th = a.freq_scale * (theta / ff);
            const float cs = cosf(th), sn = sinf(th);
            o0 = y[0] * cs - y[RW - 1] * sn;
            o1 = y[0] * sn + y[RW - 1] * cs;
        }
        const int cell = tp.z;
        if (isq) {
            a.out[r0] = o0;
            a.out[r0 + 1] = o1;
        } else if (isk) {
            const int rk = r0 - a.nq;
            __half* kr = a.kcache + (long long)cell * a.kv_dim;
            kr[rk] = __float2half_rn(o0);
            kr[rk + 1] = __float2half_rn(o1);
            if (rk == 0) a.cell_pos[cell] = tp.y;
        } else {
            const int rv = r0 - a.nq - a.nk;
            __half* vr = a.vcache + (long long)cell * a.kv_dim;
            vr[rv] = __float2half_rn(o0);
            vr[rv + 1] = __float2half_rn(o1);
        }
    } else if (ROLE == FG_SWIGLU) {
        a.out[u] = silu_f(y[0]) * y[RW - 1];
    } else if (ROLE == FG_ADD) {
        float o = y[0] + res;
        if (a.addend) o = o + gptr(a.addend)[u];
        a.out[u] = o;
    } else {
        a.out[u] = y[0];
    }
}

typedef void (*FgFn)(const FgArgs);

// pieces per pass: K <= 2048 -> 4, <= 4096 -> 8, <= 8192 -> 16; a single row also 32 (<= 16384),
// a pair past 8192 two passes of 16
template <int ROLE>
FgFn fg_fn(int K) {
    constexpr bool pair = ROLE == FG_QKV || ROLE == FG_SWIGLU;
    if (K <= 2048) return fgemv_kernel<ROLE, 4, 1>;
    if (K <= 4096) return fgemv_kernel<ROLE, 8, 2>;
    if (K <= 8192) return fgemv_kernel<ROLE, 16, 4>;
    return fgemv_kernel<ROLE, pair ? 16 : 32, 8>;
}

}  // namespace

bool fgemv_supported(int K) { return K >= 32 && K % 32 == 0 && K <= FGEMV_MAX_K; }

void launch_fgemv(const FgemvParams& p, hipStream_t s, hipEvent_t ev_start, hipEvent_t ev_stop) {
    if (!fgemv_supported(p.K)) throw Error("fgemv: K must be a multiple of 32, 32 .. 16384");
    if (p.role < FG_QKV || p.role > FG_STORE) throw Error("fgemv: role 0 .. 3");
    if (!p.x || !p.out) throw Error("fgemv: no activation or output");
    const int nmat_max = p.role == FG_QKV ? 3 : p.role == FG_SWIGLU ? 2 : 1;
    if (p.nmat < 1 || p.nmat > nmat_max || (p.role == FG_SWIGLU && p.nmat != 2)) throw Error("fgemv: matrix count does not fit the role");
    FgArgs a;
    std::memset(&a, 0, sizeof(a));
    long long rows = 0;
    for (int i = 0; i < p.nmat; ++i) {
        if (!p.w[i] || p.rows[i] < 1) throw Error("fgemv: empty matrix");
        if (p.role == FG_QKV && (p.rows[i] & 1)) throw Error("fgemv: Q/K/V rows must be even");
        a.w[i] = p.w[i];
        a.rows[i] = p.rows[i];
        rows += p.rows[i];
    }
    if (p.role == FG_SWIGLU && p.rows[0] != p.rows[1]) throw Error("fgemv: SwiGLU needs a gate/up pair of one shape");
    if (p.role == FG_ADD && !p.resid) throw Error("fgemv: residual epilogue without resid");
    if (p.role == FG_QKV) {
        if (!p.tokpos) throw Error("fgemv: QKV epilogue needs tokpos");
        if (p.nq < 0 || p.nk < 0 || (p.nq & 1) || (p.nk & 1) || p.nq + p.nk > rows) throw Error("fgemv: Q/K row counts");
        if (p.nq < rows && (!p.kcache || !p.vcache || !p.cell_pos || p.kv_dim < 2)) throw Error("fgemv: K/V rows need the caches");
    }
    a.nmat = p.nmat;
    a.K = p.K;
    a.units = (int)(p.role == FG_QKV ? rows / 2 : p.role == FG_SWIGLU ? p.rows[0] : rows);
    a.nq = p.nq;
    a.nk = p.nk;
    a.x = p.x;
    a.out = p.out;
    a.resid = p.resid;
    a.addend = p.role == FG_ADD ? p.addend : nullptr;
    a.tokpos = p.tokpos;
    a.cell_pos = p.cell_pos;
    a.kcache = p.kcache;
    a.vcache = p.vcache;
    a.freq_factors = p.freq_factors;
    a.theta_scale = p.theta_scale;
    a.freq_scale = p.freq_scale;
    a.n_rot = p.n_rot;
    a.head_dim = p.head_dim > 0 ? p.head_dim : 2;
    a.kv_dim = p.kv_dim;
    const FgFn fn = p.role == FG_QKV ? fg_fn<FG_QKV>(p.K) : p.role == FG_ADD ? fg_fn<FG_ADD>(p.K)
                  : p.role == FG_SWIGLU ? fg_fn<FG_SWIGLU>(p.K) : fg_fn<FG_STORE>(p.K);
    const int grid = (a.units + FG_NW - 1) / FG_NW;
    const size_t smem = ((size_t)p.K * 2 + 15) / 16 * 16;
    if (ev_start || ev_stop)
        hipExtLaunchKernelGGL(fn, dim3(grid), dim3(FG_THREADS), smem, s, ev_start, ev_stop, 0, a);
    else
        hipLaunchKernelGGL(fn, dim3(grid), dim3(FG_THREADS), smem, s, a);
    MI_HIP(hipGetLastError());
}

}  // namespace mi
