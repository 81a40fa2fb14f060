// The op-level entry points of include/mi_engine.h (mi_op_*): one kernel, or one short chain of
// launches, on host inputs and outputs, for the tests.  Synchronous; what the engine builds for
// itself (expert layout, MFMA-order copies, launch parameter blocks) is built by the engine's own
// functions.
#include "engine.h"
#include "qdot.h"   // act_layout: where a published activation keeps its parts

#include <algorithm>
#include <cmath>
#include <cstring>
#include <list>
#include <vector>

using namespace mi;

namespace {
// n elements of T on the device (at least 16 bytes), uploaded from `host` when given.
template <class T> struct Dev {
    T* p = nullptr;
    size_t n;
    explicit Dev(size_t count, const T* host = nullptr) : n(count) {
        MI_HIP(hipMalloc(reinterpret_cast<void**>(&p), std::max<size_t>(n * sizeof(T), 16)));
        if (!host) return;
        const hipError_t e = hipMemcpy(p, host, n * sizeof(T), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            hipFree(p);
            MI_HIP(e);
        }
    }
    Dev(const Dev&) = delete;
    Dev& operator=(const Dev&) = delete;
    ~Dev() { hipFree(p); }
    void fill(int byte) { MI_HIP(hipMemset(p, byte, n * sizeof(T))); }
    void copy_device(const T* src) { MI_HIP(hipMemcpy(p, src, n * sizeof(T), hipMemcpyDeviceToDevice)); }
    void download(T* host) const { MI_HIP(hipMemcpy(host, p, n * sizeof(T), hipMemcpyDeviceToHost)); }
};
using Keep = std::list<Dev<uint8_t>>;   // the planes and copies a QMat views

const __half* f16(const uint16_t* p) { return reinterpret_cast<const __half*>(p); }

void check_quant(int type, int K) {
    if (!is_quant(type)) throw Error("op: unsupported quant type");
    if (K % 256) throw Error("op: K must be a multiple of 256");
}

size_t plane_bytes(int type, int rows, int K, int k) {
    return ((size_t)rows * (K / 256) + kPlanePadSb) * plane_sb_bytes(type, k);
}

// Upload GGUF blocks and repack them into planes; returns the QMat view.
QMat upload_qmat(int type, const void* raw, int rows, int K, Keep& keep) {
    check_quant(type, K);
    const Dev<uint8_t> staging((size_t)rows * (K / block_elems(type)) * block_bytes(type), static_cast<const uint8_t*>(raw));
    QMat m{};
    m.type = type;
    m.rows = rows;
    m.K = K;
    m.nb = K / 256;
    uint8_t* planes[4] = {nullptr, nullptr, nullptr, nullptr};
    for (int k = 0; k < plane_count(type); ++k) {
        keep.emplace_back(plane_bytes(type, rows, K, k));
        keep.back().fill(0);
        m.p[k] = planes[k] = keep.back().p;
    }
    launch_repack(staging.p, type, rows, K, planes, nullptr);
    MI_HIP(hipDeviceSynchronize());
    return m;
}

// The E experts of a MoE *_exps tensor ([E][rows] rows of GGUF blocks) as one QMat
QMat upload_experts(int type, const void* raw, int n_expert, int rows, int K, Keep& keep) {
    QMat m = upload_qmat(type, raw, n_expert * rows, K, keep);
    split_experts(m, n_expert);
    return m;
}

// A's MFMA-order copies (a pair: gate and up in one)
void swizzle(QMat& A, const QMat* B, Keep& keep) {
    keep.emplace_back(mmq32_copy_bytes(A, B != nullptr) * std::max(1, A.n_exp));
    build_mmq_copies(A, B, keep.back().p);
    MI_HIP(hipDeviceSynchronize());
}

GemvParams gemv_of(int pro, const float* x, int K) {
    GemvParams p;
    std::memset(&p, 0, sizeof(p));
    p.pro = pro;
    p.nslots = 1;
    p.x[0] = x;
    p.K = K;
    return p;
}

GemvParams single_gemv(const QMat& m, const float* x, float* y) {
    GemvParams p = gemv_of(PRO_PLAIN, x, m.K);
    p.nseg = 1;
    p.seg[0] = seg_of(m, PAIR_ADJ, EPI_STORE, y);
    return p;
}

// The router's picks of ntok tokens: two distinct experts of [0, n_expert) each (an expert then
// holds at most ntok rows, the bound the grouped launches size their grids with).
void check_picks(const int32_t* sel, int ntok, int n_expert) {
    for (int t = 0; t < ntok; ++t) {
        const int a = sel[2 * t], b = sel[2 * t + 1];
        if (a < 0 || a >= n_expert || b < 0 || b >= n_expert) throw Error("op_moe: expert out of range");
        if (a == b) throw Error("op_moe: a token's two picks must differ");
    }
}
}  // namespace

extern "C" {

int32_t mi_op_gemv(int32_t device, int32_t type, const void* raw, int32_t rows, int32_t K, const float* x, float* y) {
    try {
        check_quant(type, K);
        MI_HIP(hipSetDevice(device));
        ensure_kernel_attributes(device);
        Keep keep;
        const QMat m = upload_qmat(type, raw, rows, K, keep);
        Dev<float> dx(K, x), dy(rows);
        launch_gemv(single_gemv(m, dx.p, dy.p), nullptr);
        MI_HIP(hipDeviceSynchronize());
        dy.download(y);
        return 0;
    }
    MI_TRY(-1)
}

// The decode step's streaming GEMV (dgemv.hip) for one launch of a given role: x quantised on the
// device by dv_quant_kernel (no norm), then dgemv_kernel.  role 0 (Q/K/V, no RoPE: every row a Q
// row; a second matrix = a second segment of another type), 1 (residual add), 2 (SwiGLU of the pair
// A = gate, B = up), 3 (store), 4 (residual add with x quantised inside the launch, by every
// workgroup: the small models' FFN down), 5 (role 4 in 16-wave workgroups of 16 rows: the large
// models' FFN down).
int32_t mi_op_dgemv(int32_t device, int32_t role, int32_t type, const void* raw, int32_t rows, int32_t K, int32_t type2,
                    const void* raw2, int32_t rows2, const float* x, const float* resid, float* y) {
    try {
        if (role < 0 || role > 5) throw Error("op_dgemv: role");
        const bool wide = role == 5;
        const bool addq = role == 4 || wide;
        if (addq) role = 1;
        const bool two = raw2 && rows2 > 0;
        check_quant(type, K);
        if (two) check_quant(type2, K);
        if (role == 2 && (!two || type2 != type || rows2 != rows)) throw Error("op_dgemv: SwiGLU needs a pair");
        if ((role == 1 || role == 3) && two) throw Error("op_dgemv: one matrix for this role");
        if (role == 1 && !resid) throw Error("op_dgemv: residual role needs resid");
        MI_HIP(hipSetDevice(device));
        ensure_kernel_attributes(device);
        Keep keep;
        const QMat a = upload_qmat(type, raw, rows, K, keep);
        QMat b{};
        if (two) b = upload_qmat(type2, raw2, rows2, K, keep);
        const int out_rows = role == 0 ? rows + (two ? rows2 : 0) : rows;
        Dev<float> dx(K, x), dy(out_rows), dr(out_rows, role == 1 ? resid : nullptr);
        Dev<int> dtp(4);
        dtp.fill(0);
        const int fmt = act_fmt({type, two ? type2 : type});
        Dev<char> act(dv_act_bytes(K, fmt & 1, fmt >> 1));
        launch_dv_quant(dx.p, ActOut{K, fmt & 1, fmt >> 1, act.p, nullptr, 1e-5f}, nullptr);
        GemvParams p;
        std::memset(&p, 0, sizeof(p));
        p.K = K;
        p.act_in = addq ? nullptr : act.p;
        p.x[0] = addq ? dx.p : nullptr;
        p.act_q8k = fmt & 1;
        p.act_q80 = fmt >> 1;
        p.act_wide = wide;
        p.tokpos = dtp.p;
        p.head_dim = 128;
        p.nseg = role == 0 && two ? 2 : 1;
        const int epi[4] = {EPI_QKV, EPI_ADD, EPI_SWIGLU, EPI_STORE};
        for (int s = 0; s < p.nseg; ++s) {
            GemvSeg& g = p.seg[s];
            g = seg_of(s == 0 ? a : b, role == 2 ? PAIR_AB : PAIR_ADJ, epi[role], dy.p + (s == 0 ? 0 : rows));
            if (role == 2) g.B = b;
            g.nq = g.A.rows;   // Q/K/V: every row a Q row, n_rot 0 (no rotation)
            g.resid = role == 1 ? dr.p : nullptr;
        }
        if (!dgemv_supported(p)) throw Error("op_dgemv: no compiled variant for this launch");
        launch_dgemv(p, nullptr);
        MI_HIP(hipDeviceSynchronize());
        dy.download(y);
        return 0;
    }
    MI_TRY(-1)
}

// The F16 decode step's streaming GEMV (fgemv.hip) for one launch of a given role, mi_op_dgemv's
// roles 0-3: role 0 without RoPE, every row a Q row (a second matrix: further rows).
int32_t mi_op_fgemv(int32_t device, int32_t role, const uint16_t* w, int32_t rows, int32_t K, const uint16_t* w2,
                    int32_t rows2, const float* x, const float* resid, float* y) {
    try {
        if (role < 0 || role > 3) throw Error("op_fgemv: role");
        if (!w || !x || !y || rows < 1) throw Error("op_fgemv: null argument");
        if (!fgemv_supported(K)) throw Error("op_fgemv: K must be a multiple of 32, 32 .. 16384");
        const bool two = w2 && rows2 > 0;
        if (role == 2 && (!two || rows2 != rows)) throw Error("op_fgemv: SwiGLU needs a pair");
        if ((role == 1 || role == 3) && two) throw Error("op_fgemv: one matrix for this role");
        if (role == 1 && !resid) throw Error("op_fgemv: residual role needs resid");
        MI_HIP(hipSetDevice(device));
        const int out_rows = role == 0 ? rows + (two ? rows2 : 0) : rows;
        Dev<uint16_t> da((size_t)rows * K, w), db(two ? (size_t)rows2 * K : 8, two ? w2 : nullptr);
        Dev<float> dx(K, x), dy(out_rows), dr(out_rows, role == 1 ? resid : nullptr);
        Dev<int> dtp(4);
        dtp.fill(0);
        FgemvParams p;
        std::memset(&p, 0, sizeof(p));
        p.role = role;
        p.w[0] = f16(da.p);
        p.rows[0] = rows;
        p.nmat = 1;
        if (two) {
            p.w[1] = f16(db.p);
            p.rows[1] = rows2;
            p.nmat = 2;
        }
        p.K = K;
        p.nq = out_rows;   // Q/K/V: every row a Q row, n_rot 0 (no rotation)
        p.x = dx.p;
        p.out = dy.p;
        p.resid = role == 1 ? dr.p : nullptr;
        p.tokpos = dtp.p;
        p.head_dim = 128;
        launch_fgemv(p, nullptr);
        MI_HIP(hipDeviceSynchronize());
        dy.download(y);
        return 0;
    }
    MI_TRY(-1)
}

// Median time of one fgemv launch of `role` over rows x K F16 matrices (role 0: one matrix, every
// row a Q row; role 2: a gate/up pair of rows each), from events recorded at the kernel's own start
// and end, after a warm-up; consecutive launches read different copies so that they stream from
// HBM, not from the Infinity Cache.  bytes_out: the matrix bytes one launch reads.
int32_t mi_op_fgemv_bench(int32_t device, int32_t role, int32_t rows, int32_t K, int32_t iters, float* median_us,
                          int64_t* bytes_out) {
    try {
        if (role < 0 || role > 3 || rows < 2 || (rows & 1) || iters < 1 || !median_us) throw Error("op_fgemv_bench: arguments");
        if (!fgemv_supported(K)) throw Error("op_fgemv_bench: K must be a multiple of 32, 32 .. 16384");
        MI_HIP(hipSetDevice(device));
        const int nmat = role == 2 ? 2 : 1;
        const size_t one = (size_t)rows * K * nmat;   // halves of one copy
        const int copies = (int)std::min<size_t>(64, std::max<size_t>(1, (768ull << 20) / (one * 2) + 1));
        // random f16 weights of the models' scale: a 1 Mi-element block tiled over the copies
        std::vector<uint16_t> blk(1 << 20);
        unsigned long long st = 0x9E3779B97F4A7C15ull;
        for (uint16_t& v : blk) {
            st = st * 6364136223846793005ull + 1442695040888963407ull;
            const _Float16 h = (_Float16)(((float)((st >> 40) & 0xFFFF) / 65536.0f - 0.5f) * 0.1f);
            std::memcpy(&v, &h, 2);
        }
        Dev<uint16_t> w(one * copies);
        for (size_t o = 0; o < one * copies; o += blk.size())
            MI_HIP(hipMemcpy(w.p + o, blk.data(), std::min(blk.size(), one * copies - o) * 2, hipMemcpyHostToDevice));
        std::vector<float> hx(K);
        for (int i = 0; i < K; ++i) hx[i] = 0.5f - 0.01f * (float)(i % 97);
        Dev<float> dx(K, hx.data()), dy(rows), dr(rows);
        dr.fill(0);
        Dev<int> dtp(4);
        dtp.fill(0);
        auto params = [&](int c) {
            FgemvParams p;
            std::memset(&p, 0, sizeof(p));
            p.role = role;
            p.w[0] = f16(w.p + (size_t)c * one);
            p.rows[0] = rows;
            p.nmat = nmat;
            if (nmat == 2) {
                p.w[1] = p.w[0] + (size_t)rows * K;
                p.rows[1] = rows;
            }
            p.K = K;
            p.nq = rows;
            p.x = dx.p;
            p.out = dy.p;
            p.resid = role == 1 ? dr.p : nullptr;
            p.tokpos = dtp.p;
            p.head_dim = 128;
            return p;
        };
        hipEvent_t a, b;
        MI_HIP(hipEventCreate(&a));
        MI_HIP(hipEventCreate(&b));
        std::vector<float> t;
        for (int i = 0; i < copies + 4; ++i) launch_fgemv(params(i % copies), nullptr);
        for (int i = 0; i < iters; ++i) {
            launch_fgemv(params(i % copies), nullptr, a, b);
            MI_HIP(hipEventSynchronize(b));
            float ms = 0;
            MI_HIP(hipEventElapsedTime(&ms, a, b));
            t.push_back(ms * 1000.0f);
        }
        hipEventDestroy(a);
        hipEventDestroy(b);
        std::sort(t.begin(), t.end());
        *median_us = t[t.size() / 2];
        if (bytes_out) *bytes_out = (int64_t)one * 2;
        return 0;
    }
    MI_TRY(-1)
}

int32_t mi_op_gemv_bench(int32_t device, int32_t type, const void* raw, int32_t rows, int32_t K, int32_t iters,
                         float* median_us) {
    try {
        check_quant(type, K);
        MI_HIP(hipSetDevice(device));
        ensure_kernel_attributes(device);
        Keep keep;
        const QMat m0 = upload_qmat(type, raw, rows, K, keep);
        // enough copies that consecutive launches stream from HBM, not the 256 MiB Infinity Cache
        size_t mbytes = 0;
        for (int k = 0; k < plane_count(type); ++k) mbytes += plane_bytes(type, rows, K, k);
        const int copies = (int)std::min<size_t>(64, std::max<size_t>(1, (768ull << 20) / mbytes + 1));
        std::vector<QMat> mats(copies, m0);
        for (int c = 1; c < copies; ++c)
            for (int k = 0; k < plane_count(type); ++k) {
                keep.emplace_back(plane_bytes(type, rows, K, k));
                keep.back().copy_device(m0.p[k]);
                mats[c].p[k] = keep.back().p;
            }
        std::vector<float> hx(K);
        for (int i = 0; i < K; ++i) hx[i] = 0.5f + 0.001f * (float)(i % 97);
        Dev<float> dx(K, hx.data()), dy(rows);
        hipEvent_t a, b;
        MI_HIP(hipEventCreate(&a));
        MI_HIP(hipEventCreate(&b));
        std::vector<float> t;
        for (int i = 0; i < copies + 2; ++i) launch_gemv(single_gemv(mats[i % copies], dx.p, dy.p), nullptr);
        for (int i = 0; i < iters; ++i) {
            const GemvParams p = single_gemv(mats[i % copies], dx.p, dy.p);
            MI_HIP(hipEventRecord(a, nullptr));
            launch_gemv(p, nullptr);
            MI_HIP(hipEventRecord(b, nullptr));
            MI_HIP(hipEventSynchronize(b));
            float ms = 0;
            MI_HIP(hipEventElapsedTime(&ms, a, b));
            t.push_back(ms * 1000.0f);
        }
        hipEventDestroy(a);
        hipEventDestroy(b);
        std::sort(t.begin(), t.end());
        *median_us = t.empty() ? 0.0f : t[t.size() / 2];
        return 0;
    }
    MI_TRY(-1)
}

int32_t mi_op_dequant(int32_t device, int32_t type, const void* raw, int32_t rows, int32_t K, float* out) {
    try {
        check_quant(type, K);
        MI_HIP(hipSetDevice(device));
        Keep keep;
        const QMat m = upload_qmat(type, raw, rows, K, keep);
        Dev<float> d((size_t)rows * K);
        launch_dequant_rows(m, 0, rows, d.p, nullptr);
        MI_HIP(hipDeviceSynchronize());
        d.download(out);
        return 0;
    }
    MI_TRY(-1)
}

int32_t mi_op_quantize_q8_K(int32_t device, const float* x, int32_t K, int8_t* qs, float* d, int32_t* bsums) {
    try {
        if (K % 256) throw Error("K must be a multiple of 256");
        MI_HIP(hipSetDevice(device));
        const int nb = K / 256;
        Dev<float> dx(K, x), dd(nb);
        Dev<int8_t> dq(K);
        Dev<int> db((size_t)nb * 16);
        launch_quantize_q8k(dx.p, K, dq.p, dd.p, db.p, nullptr);
        MI_HIP(hipDeviceSynchronize());
        dq.download(qs);
        dd.download(d);
        db.download(bsums);
        return 0;
    }
    MI_TRY(-1)
}

int32_t mi_op_topk(int32_t device, const float* logits, int32_t n, int32_t k, int32_t* ids, float* vals) {
    try {
        if (k < 0 || k > TOPK_MAX) throw Error("k must be in [0, 64]");
        if (n < 1) throw Error("n must be positive");
        MI_HIP(hipSetDevice(device));
        Dev<float> dl(n, logits), dv(TOPK_MAX);
        Dev<unsigned long long> dc((size_t)topk_blocks(n) * TOPK_MAX);
        Dev<int> di(TOPK_MAX);
        TopkParams tp{dl.p, n, dc.p, di.p, dv.p, nullptr, nullptr};
        launch_topk(tp, nullptr);
        MI_HIP(hipDeviceSynchronize());
        std::vector<int> hi(TOPK_MAX);
        std::vector<float> hv(TOPK_MAX);
        di.download(hi.data());
        dv.download(hv.data());
        for (int i = 0; i < k; ++i) { ids[i] = hi[i]; vals[i] = hv[i]; }
        return k;
    }
    MI_TRY(-1)
}

int32_t mi_op_attention(int32_t device, int32_t n_head, int32_t n_head_kv, int32_t head_dim, int32_t n_cells,
                        const float* q, const uint16_t* k_f16, const uint16_t* v_f16, const int32_t* cell_pos,
                        int32_t pos, float* out) {
    try {
        if (n_head <= 0 || n_head_kv <= 0 || n_head % n_head_kv || n_cells <= 0 || head_dim <= 0)
            throw Error("attention: bad shape");
        MI_HIP(hipSetDevice(device));
        const int kv_dim = n_head_kv * head_dim, d = n_head * head_dim;
        const size_t kvn = (size_t)n_cells * kv_dim, xn = (size_t)n_head * ATTN_SMAX;
        const int tp[4] = {0, pos, n_cells - 1, 0};   // {token, query position, last cell}
        Dev<float> dq(d, q), dsc((size_t)n_head * n_cells), dsm(xn), dpo((size_t)ATTN_SMAX * d), dout(d);
        Dev<__half> dk(kvn, f16(k_f16)), dv(kvn, f16(v_f16));
        Dev<int> dcp(n_cells, cell_pos), dtp(4, tp);
        AttnParams a{dq.p, dk.p, dv.p, dtp.p, dcp.p, dsc.p, dsm.p, dpo.p, n_head, n_head_kv, head_dim, kv_dim,
                     n_cells, 1.0f / std::sqrt((float)head_dim)};
        a.fused = n_cells <= ATTN_SHORT ? 1 : 0;   // the decode graph's choice for this cell count
        // the decode graph's single-launch long-context kernel (exchange buffers zeroed, step 0)
        Dev<unsigned> dxf(xn * 32), dst(4);
        Dev<float> dxm(xn);
        Dev<double> dxs(xn);
        dxf.fill(0);
        dst.fill(0);
        a.xflags = dxf.p;
        a.xmax = dxm.p;
        a.xsum = dxs.p;
        a.step = dst.p;
        launch_attn(a, nullptr);
        launch_attn_combine(AttnPartials{dpo.p, n_head, head_dim}, dtp.p, dout.p, nullptr);
        MI_HIP(hipDeviceSynchronize());
        dout.download(out);
        return 0;
    }
    MI_TRY(-1)
}

int32_t mi_op_attn_plan(int32_t mode, int32_t n_head, int32_t n_head_kv, int32_t head_dim, int32_t n_ctx, int32_t ntok,
                        int32_t long_ok, int32_t* out) {
    try {
        if (mode < ATTN_DECODE_QUANT || mode > ATTN_BATCH_FUSED) throw Error("attn_plan: bad mode");
        const AttnPlan k = attn_plan((AttnMode)mode, n_head, n_head_kv, head_dim, n_ctx, ntok, long_ok != 0);
        const int v[10] = {k.kernel, k.R, k.LPC, k.HG, k.NWV, k.grid_x, k.grid_y, k.block, (int)k.lds, k.qsplit};
        std::copy(v, v + 10, out);
        return 0;
    }
    MI_TRY(-1)
}

// mmq_plan for one shape: out[16] = {kernel, T, pair, pre, gx, grouped, nst, nt, nrb, ntb, kp, grid_x, grid_y,
// grid_z, block, lds}.  form: 0 tiled, 1 short.  Opens no device.
int32_t mi_op_mmq_plan(int32_t form, int32_t type, int32_t pair, const int32_t* rows, int32_t nseg, int32_t npad, int32_t K,
                       int32_t grp_n, int32_t grp_max, int32_t ksplit, int32_t pre, int32_t gx, int32_t n_cu, int32_t* out) {
    try {
        if (form != MMQ_TILED && form != MMQ_SHORT) throw Error("mmq_plan: form 0 (tiled) or 1 (short)");
        if (nseg < 0 || nseg > 3) throw Error("mmq_plan: at most 3 segments");
        MmqShape sh{};
        sh.type = type;
        sh.pair = pair != 0;
        sh.nseg = nseg;
        for (int i = 0; i < nseg; ++i) sh.rows[i] = rows[i];
        sh.npad = npad;
        sh.K = K;
        sh.grp_n = grp_n;
        sh.grp_max = grp_max;
        sh.ksplit = ksplit;
        sh.pre = pre != 0;
        sh.gx = gx != 0;
        const MmqPlan k = mmq_plan((MmqForm)form, sh, n_cu);
        const int v[16] = {k.kernel, k.T, k.pair, k.pre, k.gx, k.grouped, k.nst, k.nt, k.nrb, k.ntb, k.kp,
                           k.grid_x, k.grid_y, k.grid_z, k.block, (int)k.lds};
        std::copy(v, v + 16, out);
        if (k.kernel == MK_NONE) set_last_error(k.why);   // (mi_last_error: the message the launcher throws)
        return 0;
    }
    MI_TRY(-1)
}

// One decode step's attention through launch_attn in a given mode, with the output the engine's next
// launch reads: the activation published in act_layout (ATTN_DECODE_QUANT: by the attention kernel;
// ATTN_DECODE_SPLIT: by attn_combine_quant over the two launches' partials), unpacked.  Returns the
// plan's kernel (AK_*).
int32_t mi_op_attention_decode(int32_t device, int32_t mode, int32_t n_head, int32_t n_head_kv, int32_t head_dim,
                               int32_t n_ctx, int32_t cell, int32_t pos, const float* q, const uint16_t* k_f16,
                               const uint16_t* v_f16, const int32_t* cell_pos, int32_t fmt, int32_t want_f32, float* out,
                               int8_t* q8k, int32_t* bsums, float* dk, int8_t* q80, float* d0) {
    try {
        if (mode != ATTN_DECODE_QUANT && mode != ATTN_DECODE_FUSED && mode != ATTN_DECODE_SPLIT)
            throw Error("attention_decode: mode 0 (quantising), 1 (fused) or 2 (two launches)");
        if (!q || !k_f16 || !v_f16 || !cell_pos) throw Error("attention_decode: null argument");
        if (n_head <= 0 || n_head_kv <= 0 || n_head % n_head_kv || head_dim <= 0 || n_ctx <= 0)
            throw Error("attention_decode: bad shape");
        if (cell < 0 || cell >= n_ctx) throw Error("attention_decode: cell outside the cache");
        const bool split = mode == ATTN_DECODE_SPLIT;
        if (split ? cell < ATTN_SHORT : cell >= ATTN_SHORT)
            throw Error("attention_decode: the single launch serves up to 512 cells, the two launches more");
        if (fmt < 0 || fmt > 3 || (mode == ATTN_DECODE_QUANT && !fmt) || (mode == ATTN_DECODE_FUSED && fmt))
            throw Error("attention_decode: fmt bit 0 Q8_K, bit 1 Q8_0 (the fused mode: 0)");
        const int wk = fmt & 1, w0 = fmt >> 1;
        if ((want_f32 || !fmt) && !out) throw Error("attention_decode: no f32 output buffer");
        if ((wk && (!q8k || !bsums || !dk)) || (w0 && (!q80 || !d0))) throw Error("attention_decode: no buffer for a format asked for");
        const AttnPlan plan = attn_plan((AttnMode)mode, n_head, n_head_kv, head_dim, n_ctx, 1, false);
        if (plan.kernel == AK_NONE) throw Error("attention_decode: no kernel serves this head geometry in this mode");
        const int kv_dim = n_head_kv * head_dim, K = n_head * head_dim;
        if (fmt && K % 256) throw Error("attention_decode: a quantised output needs n_head * head_dim in whole 256-blocks");
        MI_HIP(hipSetDevice(device));
        const size_t kvn = (size_t)n_ctx * kv_dim;
        const int tp[4] = {0, pos, cell, 0};   // {token, query position, last cell}
        Dev<float> dq(K, q), dsc(split ? (size_t)n_head * n_ctx : 1), dsm((size_t)ATTN_SMAX * n_head);
        Dev<float> dpo((size_t)(split ? ATTN_SMAX : 1) * K), dout(K);
        Dev<__half> dkc(kvn, f16(k_f16)), dvc(kvn, f16(v_f16));
        Dev<int> dcp(n_ctx, cell_pos), dtp(4, tp);
        Dev<char> act(fmt ? dv_act_bytes(K, wk, w0) : 16);
        // what the launches do not write stays recognisable: NaN floats, quants of -128
        dpo.fill(0xFF);
        dout.fill(0xFF);
        act.fill(0x80);
        AttnParams a{dq.p, dkc.p, dvc.p, dtp.p, dcp.p, dsc.p, dsm.p, dpo.p, n_head, n_head_kv, head_dim, kv_dim,
                     n_ctx, 1.0f / std::sqrt((float)head_dim)};
        a.fused = split ? 0 : 1;
        a.long_off = 1;   // past 512 cells: the two launches (the exchange kernel is mi_op_attention's)
        const ActOut ao{K, wk, w0, act.p, nullptr, 0.0f};
        const AttnPartials parts{dpo.p, n_head, head_dim};
        const float* f32 = dout.p;
        if (split) {
            launch_attn(a, nullptr);
            launch_attn_combine(parts, dtp.p, dout.p, nullptr);
            if (fmt) launch_attn_combine_quant(parts, dtp.p, ao, nullptr);
        } else {
            if (fmt) a.act_out = ao;
            // the decode kernel stores the f32 row on request only; the fused kernel always, as split 0
            if (plan.kernel == AK_DEC) a.out_f32 = want_f32 ? dout.p : nullptr;
            else f32 = dpo.p;
            launch_attn(a, nullptr);
        }
        MI_HIP(hipDeviceSynchronize());
        if (want_f32 || !fmt) MI_HIP(hipMemcpy(out, f32, (size_t)K * sizeof(float), hipMemcpyDeviceToHost));
        if (fmt) {
            std::vector<char> h(act.n);
            act.download(h.data());
            const ActLayout L = act_layout(K, wk, w0);
            if (wk) {
                std::memcpy(q8k, h.data() + L.q8k, (size_t)K);
                std::memcpy(bsums, h.data() + L.bsum, (size_t)L.nb * 16 * sizeof(int32_t));
                std::memcpy(dk, h.data() + L.dk, (size_t)L.nb * sizeof(float));
            }
            if (w0) {
                std::memcpy(q80, h.data() + L.q80, (size_t)K);
                std::memcpy(d0, h.data() + L.d0, (size_t)L.nb * 8 * sizeof(float));
            }
        }
        return plan.kernel;
    }
    MI_TRY(-1)
}

// A short batch's attention through launch_attn_multi: ntok tokens over up to ATTN_SHORT cells, one
// grid row per token; with `quant` each token's output also quantised into the batch GEMMs' format
// (ActQ8, sized as mi_op_gemm sizes it), brought back to token order.  Returns the plan's kernel.
int32_t mi_op_attention_short(int32_t device, int32_t n_head, int32_t n_head_kv, int32_t head_dim, int32_t n_cells,
                              int32_t ntok, const float* q, const uint16_t* k_f16, const uint16_t* v_f16,
                              const int32_t* cell_pos, const int32_t* tok_cell, const int32_t* tok_pos, int32_t quant,
                              float* out, int8_t* q_out, float* d_out, int32_t* bsums_out) {
    try {
        if (!q || !k_f16 || !v_f16 || !cell_pos || !tok_cell || !tok_pos || !out) throw Error("attention_short: null argument");
        if (n_head <= 0 || n_head_kv <= 0 || n_head % n_head_kv || head_dim <= 0 || n_cells <= 0)
            throw Error("attention_short: bad shape");
        if (ntok < 1 || ntok > MMQS_MAX) throw Error("attention_short: 1..64 tokens");
        if (quant < 0 || quant > 2) throw Error("attention_short: quant 0 (none), 1 (Q8_K) or 2 (Q8_0)");
        if (quant && (!q_out || !d_out || (quant == 1 && !bsums_out))) throw Error("attention_short: no buffer for the quantised rows");
        for (int t = 0; t < ntok; ++t) {
            if (tok_cell[t] < 0 || tok_cell[t] >= n_cells || tok_cell[t] >= ATTN_SHORT)
                throw Error("attention_short: token cell out of range (the cache, and 512 cells)");
            if (t && tok_cell[t] <= tok_cell[t - 1]) throw Error("attention_short: token cells must ascend");
        }
        const AttnPlan plan = attn_plan(quant ? ATTN_BATCH_QUANT : ATTN_BATCH_FUSED, n_head, n_head_kv, head_dim, n_cells, ntok, false);
        if (plan.kernel == AK_NONE) throw Error("attention_short: no kernel serves this head geometry in this mode");
        const int kv_dim = n_head_kv * head_dim, K = n_head * head_dim;
        if (quant && K % 256) throw Error("attention_short: a quantised output needs n_head * head_dim in whole 256-blocks");
        MI_HIP(hipSetDevice(device));
        const size_t kvn = (size_t)n_cells * kv_dim;
        std::vector<int> tp((size_t)ntok * 4, 0);
        for (int t = 0; t < ntok; ++t) {
            tp[t * 4 + 1] = tok_pos[t];
            tp[t * 4 + 2] = tok_cell[t];
        }
        const bool q80 = quant == 2;
        const size_t npad = (size_t)(ntok + 31) / 32 * 32;
        const int nb = K / 256, nd = q80 ? K / 32 : nb;   // scales per row
        Dev<float> dq((size_t)ntok * K, q), dout((size_t)ntok * K), ddT(quant ? npad * (K / 32) : 1);
        Dev<int8_t> dqa(quant ? npad * K : 1), dbs(quant ? npad * nb * 16 : 1);
        Dev<__half> dkc(kvn, f16(k_f16)), dvc(kvn, f16(v_f16));
        Dev<int> dcp(n_cells, cell_pos), dtp(tp.size(), tp.data());
        // what the launch does not write stays recognisable: NaN floats, quants and sum bytes of -128
        dout.fill(0xFF);
        ddT.fill(0xFF);
        dqa.fill(0x80);
        dbs.fill(0x80);
        AttnParams a{dq.p, dkc.p, dvc.p, dtp.p, dcp.p, nullptr, nullptr, nullptr, n_head, n_head_kv, head_dim, kv_dim,
                     n_cells, 1.0f / std::sqrt((float)head_dim)};
        if (quant) {
            a.act_q8 = ActQ8{dqa.p, ddT.p, dbs.p, K, ntok, (int)npad, q80 ? 1 : 0};
            if (plan.kernel == AK_DEC) a.out_f32 = dout.p;   // the fused kernel stores the rows at `out` anyway
        }
        launch_attn_multi(a, ntok, dout.p, nullptr);
        MI_HIP(hipDeviceSynchronize());
        dout.download(out);
        if (!quant) return plan.kernel;
        // the MFMA-fragment order back to token order: element 32 j + 16 h + e of superblock sb
        std::vector<int8_t> hq(dqa.n), hb(dbs.n);
        std::vector<float> hd(ddT.n);
        dqa.download(hq.data());
        dbs.download(hb.data());
        ddT.download(hd.data());
        for (int t = 0; t < ntok; ++t)
            for (int sb = 0; sb < nb; ++sb) {
                for (int j = 0; j < 8; ++j)
                    for (int h = 0; h < 2; ++h)
                        std::memcpy(q_out + (size_t)t * K + sb * 256 + 32 * j + 16 * h,
                                    hq.data() + (((size_t)(t / 32) * nb + sb) * 8 + j) * 1024 + (h * 32 + t % 32) * 16, 16);
                if (q80) continue;
                // the 32-element sums, byte-split: 64 * hi (bytes 0-7) + lo (bytes 8-15)
                const int8_t* b = hb.data() + (((size_t)(t / 32) * nb + sb) * 32 + t % 32) * 16;
                for (int j = 0; j < 8; ++j) bsums_out[((size_t)t * nb + sb) * 8 + j] = 64 * (int)b[j] + (int)b[8 + j];
            }
        for (int t = 0; t < ntok; ++t)   // dT [scale][npad] -> [ntok][scale]
            for (int b = 0; b < nd; ++b) d_out[(size_t)t * nd + b] = hd[(size_t)b * npad + t];
        return plan.kernel;
    }
    MI_TRY(-1)
}

int32_t mi_op_gemm(int32_t device, int32_t type, const void* raw, const void* raw_up, int32_t rows, int32_t K,
                   int32_t ntok, const float* x, float* y) {
    try {
        if (!mmq32_supported(type)) throw Error("op_gemm: Q4_K / Q5_K / Q6_K / Q8_0 / Q4_0 / Q5_0 only");
        if (ntok < 1 || ntok > UB_MAX) throw Error("op_gemm: 1..512 token rows");
        if (rows < 1 || K < 256 || K % 256) throw Error("op_gemm: bad shape");
        MI_HIP(hipSetDevice(device));
        ensure_kernel_attributes(device);
        Keep keep;
        QMat A = upload_qmat(type, raw, rows, K, keep);
        QMat B = A;
        const bool pair = raw_up != nullptr;
        if (pair) B = upload_qmat(type, raw_up, rows, K, keep);
        swizzle(A, pair ? &B : nullptr, keep);
        const size_t npad = (size_t)(ntok + 31) / 32 * 32;
        Dev<float> dx((size_t)ntok * K, x), dy((size_t)ntok * rows), ddT(npad * (K / 32));
        Dev<int8_t> dq(npad * K), dbs(npad * (K / 256) * 16);
        Dev<int> dtp((size_t)ntok * 4);
        dtp.fill(0);
        ActQ8 act{dq.p, ddT.p, dbs.p, K, ntok, (int)npad, takes_q80(type) ? 1 : 0};
        QuantAct qa{};
        qa.x = dx.p;
        qa.x_stride = K;
        launch_quant_act(qa, act, nullptr);
        // up to the short-batch limit: the short-batch GEMM (K-part sums, added by part_sum) as the
        // engine's verification batches take it; MI_MMQS_MAX=0: the tiled GEMM for every count
        if (ntok <= mmqs_token_limit()) {
            const int pst = pair ? 2 * rows : rows;
            Dev<float> part((size_t)mmqs_parts(K) * ntok * pst);
            const QMat* mats[1] = {&A};
            const int prow[1] = {0};
            const int kp = launch_mmqs(mats, prow, 1, pair, rows, act, part.p, pst, nullptr);
            PartSum ps{};
            ps.part = part.p;
            ps.kp = kp;
            ps.ntok = ntok;
            ps.rows = rows;
            ps.pstride = pst;
            ps.out = dy.p;
            ps.ostride = rows;
            ps.swiglu = pair ? rows : 0;
            launch_part_sum(ps, nullptr);
            MI_HIP(hipDeviceSynchronize());
        } else {
            launch_mmq32(mmq32_params(A, pair ? &B : nullptr, ntok, dtp.p, dy.p, rows), act, nullptr, nullptr);
        }
        MI_HIP(hipDeviceSynchronize());
        dy.download(y);
        return 0;
    }
    MI_TRY(-1)
}

int32_t mi_op_gemm_bias(int32_t device, int32_t type, const void* raw, int32_t rows, int32_t K, int32_t ntok,
                        const float* x, const float* norm_w, const float* norm_b, float eps, const float* bias,
                        const float* resid, int32_t epilogue, float* y, int8_t* q_out, float* d_out) {
    try {
        if (!mmq32_supported(type)) throw Error("op_gemm_bias: Q4_K / Q5_K / Q6_K / Q8_0 / Q4_0 / Q5_0 only");
        if (ntok < 1 || ntok > UB_MAX) throw Error("op_gemm_bias: 1..512 token rows");
        if (rows < 1 || K < 256 || K % 256) throw Error("op_gemm_bias: bad shape");
        if (epilogue < 0 || epilogue > 2 || (epilogue == 1 && !resid)) throw Error("op_gemm_bias: epilogue 0 / 1 (with resid) / 2");
        if ((norm_w == nullptr) != (norm_b == nullptr)) throw Error("op_gemm_bias: LayerNorm takes its weight and its bias");
        if (!x || !y) throw Error("op_gemm_bias: null argument");
        MI_HIP(hipSetDevice(device));
        ensure_kernel_attributes(device);
        Keep keep;
        QMat A = upload_qmat(type, raw, rows, K, keep);
        swizzle(A, nullptr, keep);
        const bool q80 = takes_q80(type);
        const size_t npad = (size_t)(ntok + 31) / 32 * 32;
        const int nb = K / 256, nd = q80 ? K / 32 : nb;   // scales per row
        Dev<float> dx((size_t)ntok * K, x), dy((size_t)ntok * rows), ddT(npad * (K / 32));
        Dev<float> dnw(K, norm_w), dnb(K, norm_b), dbias(rows, bias), dres((size_t)ntok * rows, epilogue == 1 ? resid : nullptr);
        Dev<int8_t> dq(npad * K), dbs(npad * nb * 16);
        Dev<int> dtp((size_t)ntok * 4);
        dtp.fill(0);
        const std::vector<unsigned short> tab = gelu_table_host();
        Dev<unsigned short> dtab(tab.size(), tab.data());
        ActQ8 act{dq.p, ddT.p, dbs.p, K, ntok, (int)npad, q80 ? 1 : 0};
        QuantAct qa{};
        qa.x = dx.p;
        qa.x_stride = K;
        qa.norm_w = norm_w ? dnw.p : nullptr;
        qa.norm_b = norm_b ? dnb.p : nullptr;
        qa.eps = eps;
        launch_quant_act(qa, act, nullptr);
        GemmParams p = mmq32_params(A, nullptr, ntok, dtp.p, dy.p, rows);
        const int epis[3] = {EPI_STORE, EPI_ADD, EPI_GELU};
        p.epi = epis[epilogue];
        p.resid = epilogue == 1 ? dres.p : nullptr;
        p.bias = bias ? dbias.p : nullptr;
        p.gelu_tab = dtab.p;
        launch_mmq32(p, act, nullptr, nullptr);
        MI_HIP(hipDeviceSynchronize());
        dy.download(y);
        if (q_out) {   // the MFMA-fragment order back to token order: element 32 j + 16 h + e of superblock sb
            std::vector<int8_t> hq(dq.n);
            dq.download(hq.data());
            for (int t = 0; t < ntok; ++t)
                for (int sb = 0; sb < nb; ++sb)
                    for (int j = 0; j < 8; ++j)
                        for (int h = 0; h < 2; ++h)
                            std::memcpy(q_out + (size_t)t * K + sb * 256 + 32 * j + 16 * h,
                                        hq.data() + (((size_t)(t / 32) * nb + sb) * 8 + j) * 1024 + (h * 32 + t % 32) * 16, 16);
        }
        if (d_out) {   // dT [scale][npad] -> [ntok][scale]
            std::vector<float> hd(ddT.n);
            ddT.download(hd.data());
            for (int t = 0; t < ntok; ++t)
                for (int b = 0; b < nd; ++b) d_out[(size_t)t * nd + b] = hd[(size_t)b * npad + t];
        }
        return 0;
    }
    MI_TRY(-1)
}

int32_t mi_op_attention_batch(int32_t device, int32_t n_head, int32_t n_head_kv, int32_t head_dim, int32_t n_cells,
                              int32_t ntok, const float* q, const uint16_t* k_f16, const uint16_t* v_f16,
                              const int32_t* cell_pos, const int32_t* tok_cell, const int32_t* tok_pos, float* out) {
    try {
        if (n_head <= 0 || n_head_kv <= 0 || n_head % n_head_kv || n_cells <= 0 || ntok <= 0)
            throw Error("attention_batch: bad shape");
        if (!attn_mfma_supported(head_dim)) throw Error("attention_batch: head_dim 64 or 128");
        for (int t = 0; t < ntok; ++t) {
            if (tok_cell[t] < 0 || tok_cell[t] >= n_cells) throw Error("attention_batch: token cell out of range");
            if (t && tok_cell[t] <= tok_cell[t - 1]) throw Error("attention_batch: token cells must ascend");
        }
        MI_HIP(hipSetDevice(device));
        ensure_kernel_attributes(device);
        const int kv_dim = n_head_kv * head_dim, d = n_head * head_dim;
        const size_t kvn = (size_t)n_cells * kv_dim;
        std::vector<int> tp((size_t)ntok * 4, 0);
        for (int t = 0; t < ntok; ++t) {
            tp[t * 4 + 1] = tok_pos[t];
            tp[t * 4 + 2] = tok_cell[t];
        }
        Dev<float> dq((size_t)ntok * d, q), dout((size_t)ntok * d);
        Dev<__half> dk(kvn, f16(k_f16)), dv(kvn, f16(v_f16));
        Dev<int> dcp(n_cells, cell_pos), dtp(tp.size(), tp.data());
        AttnParams a{dq.p, dk.p, dv.p, dtp.p, dcp.p, nullptr, nullptr, nullptr, n_head, n_head_kv, head_dim, kv_dim,
                     n_cells, 1.0f / std::sqrt((float)head_dim)};
        launch_attn_mfma(a, ntok, dout.p, nullptr);
        MI_HIP(hipDeviceSynchronize());
        dout.download(out);
        return 0;
    }
    MI_TRY(-1)
}

// ---- the MoE kernels, op by op ----
int32_t mi_op_router(int32_t device, int32_t n_embd, int32_t n_expert, int32_t ntok, const float* x, int32_t x_stride,
                     const float* norm_w, float eps, const float* w, const float* part, int32_t* sel_out,
                     float* selw_out, float* x_out) {
    try {
        if (!x || !norm_w || !w || !sel_out || !selw_out) throw Error("op_router: null argument");
        if (ntok < 1 || ntok > UB_MAX) throw Error("op_router: 1..512 token rows");
        if (n_embd < 1 || n_expert < 2) throw Error("op_router: bad shape");
        if (x_stride < n_embd || x_stride % 4) throw Error("op_router: x_stride must cover n_embd, in whole float4s");
        MI_HIP(hipSetDevice(device));
        Dev<float> dx((size_t)ntok * x_stride, x), dn(n_embd, norm_w), dw((size_t)n_expert * n_embd, w);
        Dev<float> dp((size_t)2 * ntok * n_embd, part), dselw((size_t)ntok * 2);
        Dev<int> dsel((size_t)ntok * 2);
        dsel.fill(0x80);
        dselw.fill(0xFF);
        RouterParams rp{dx.p, dn.p, eps, dw.p, n_embd, n_expert, 2, dsel.p, dselw.p, x_stride, part ? dp.p : nullptr, ntok};
        launch_router_multi(rp, ntok, nullptr);
        MI_HIP(hipDeviceSynchronize());
        dsel.download(sel_out);
        dselw.download(selw_out);
        if (x_out) dx.download(x_out);
        return 0;
    }
    MI_TRY(-1)
}

int32_t mi_op_moe_group(int32_t device, const int32_t* sel, int32_t n, int32_t U, int32_t E, int32_t rows_cap,
                        int32_t* grp_out, int32_t* rows_out, int32_t* rowsel_out, int32_t* pos_out) {
    try {
        if (!sel || !grp_out || !rows_out || !rowsel_out || !pos_out) throw Error("op_moe_group: null argument");
        if (n < 1 || n > 4 * UB_MAX || U < 1 || n % U) throw Error("op_moe_group: 1..2048 picks, whole tokens");
        if (rows_cap < 1 || rows_cap > 8 * UB_MAX) throw Error("op_moe_group: bad row capacity");
        MI_HIP(hipSetDevice(device));
        Dev<int> dsel(n, sel), dgrp(2 * std::max(E, 0) + 1), drows(rows_cap), drs(rows_cap), dpos(n);
        // a sentinel (0x80808080) in everything the kernel should write
        for (Dev<int>* d : {&dgrp, &drows, &drs, &dpos}) d->fill(0x80);
        launch_moe_group(dsel.p, n, U, E, dgrp.p, drows.p, drs.p, dpos.p, rows_cap, nullptr);
        MI_HIP(hipDeviceSynchronize());
        dgrp.download(grp_out);
        drows.download(rows_out);
        drs.download(rowsel_out);
        dpos.download(pos_out);
        return 0;
    }
    MI_TRY(-1)
}

int32_t mi_op_moe_gemm(int32_t device, int32_t mode, int32_t type, const void* raw, const void* raw_up, int32_t n_expert,
                       int32_t rows, int32_t K, int32_t ntok, const float* x, int32_t per_pick, const int32_t* sel,
                       float* y) {
    try {
        if (!raw || !x || !sel || !y) throw Error("op_moe_gemm: null argument");
        if (mode != 0 && mode != 1) throw Error("op_moe_gemm: mode 0 (tiled) or 1 (short)");
        if (!mmq32_supported(type) || is_legacy_quant(type)) throw Error("op_moe_gemm: Q4_K / Q5_K / Q6_K / Q8_0 only");
        if (mode == 1 && !mmqs_grouped_supported(type)) throw Error("op_moe_gemm: the short form takes Q4_K / Q5_K / Q6_K experts");
        if (ntok < 1 || ntok > (mode == 1 ? MMQS_MAX : UB_MAX)) throw Error("op_moe_gemm: 1..512 tokens (short form: 1..64)");
        if (n_expert < 2 || n_expert > MOE_GROUP_MAXE) throw Error("op_moe_gemm: 2..16 experts");
        if (rows < 1 || K < 256 || K % 256) throw Error("op_moe_gemm: bad shape");
        check_picks(sel, ntok, n_expert);
        MI_HIP(hipSetDevice(device));
        ensure_kernel_attributes(device);
        const bool pair = raw_up != nullptr;
        const int n = 2 * ntok, cap = moe_rows_cap(n, n_expert);
        Keep keep;
        QMat A = upload_experts(type, raw, n_expert, rows, K, keep);
        QMat B = A;
        if (pair) B = upload_experts(type, raw_up, n_expert, rows, K, keep);
        swizzle(A, pair ? &B : nullptr, keep);
        // the picks grouped by expert
        Dev<int> dsel(n, sel), dgrp(2 * n_expert + 1), drows(cap), drs(cap), dpos(n);
        launch_moe_group(dsel.p, n, 2, n_expert, dgrp.p, drows.p, drs.p, dpos.p, cap, nullptr);
        MI_HIP(hipDeviceSynchronize());
        std::vector<int> pos(n);
        dpos.download(pos.data());
        for (int i = 0; i < n; ++i)
            if (pos[i] < 0 || pos[i] >= cap) throw Error("op_moe_gemm: the grouping left a pick without a row");
        // the MoE rows quantised: the tokens' rows through moe_rows (gate/up), or one row per pick,
        // already in its compact place, through moe_rowsel (down)
        std::vector<float> hx;
        if (per_pick) {
            hx.assign((size_t)cap * K, 0.0f);
            for (int i = 0; i < n; ++i) std::memcpy(&hx[(size_t)pos[i] * K], x + (size_t)i * K, (size_t)K * sizeof(float));
        }
        Dev<float> dx((size_t)(per_pick ? cap : ntok) * K, per_pick ? hx.data() : x);
        Dev<float> ddT((size_t)cap * (K / 32)), dy((size_t)cap * rows);
        Dev<int8_t> dq((size_t)cap * K), dbs((size_t)cap * (K / 256) * 16);
        ActQ8 act{dq.p, ddT.p, dbs.p, K, cap, cap, type == T_Q8_0 ? 1 : 0};
        QuantAct qa{};
        qa.x = dx.p;
        qa.x_stride = K;
        qa.rows = per_pick ? drs.p : drows.p;
        launch_quant_act(qa, act, nullptr);
        dy.fill(0);
        if (mode == 0) {   // the tiled grouped launch of a physical batch
            Dev<int> dtp((size_t)cap * 4);
            dtp.fill(0);
            launch_mmq32(mmq32_params(A, pair ? &B : nullptr, cap, dtp.p, dy.p, rows, dgrp.p, ntok), act, nullptr, nullptr);
            MI_HIP(hipDeviceSynchronize());
        } else {           // the short batch's grouped launch, its K-parts added by part_sum
            const int pst = pair ? 2 * rows : rows;
            Dev<float> part((size_t)mmqs_parts(K) * cap * pst);
            part.fill(0);
            const int kp = launch_mmqs_grouped(A, pair, pair ? rows : 0, act, part.p, pst, dgrp.p, n_expert, ntok, nullptr);
            PartSum ps{};
            ps.part = part.p;
            ps.kp = kp;
            ps.ntok = cap;
            ps.rows = rows;
            ps.pstride = pst;
            ps.out = dy.p;
            ps.ostride = rows;
            ps.swiglu = pair ? rows : 0;
            launch_part_sum(ps, nullptr);
            MI_HIP(hipDeviceSynchronize());
        }
        std::vector<float> hy((size_t)cap * rows);
        dy.download(hy.data());
        for (int i = 0; i < n; ++i) std::memcpy(y + (size_t)i * rows, &hy[(size_t)pos[i] * rows], (size_t)rows * sizeof(float));
        return 0;
    }
    MI_TRY(-1)
}

int32_t mi_op_moe_decode(int32_t device, int32_t type, const void* gate, const void* up, const void* down,
                         int32_t n_expert, int32_t n_embd, int32_t n_ff, const float* x, const float* norm_w, float eps,
                         const int32_t* sel, const float* selw, const float* addend, float* h_out, float* x_out) {
    try {
        if (!gate || !up || !down || !x || !norm_w || !sel || !selw || !h_out || !x_out) throw Error("op_moe_decode: null argument");
        if (!is_quant(type) || is_legacy_quant(type)) throw Error("op_moe_decode: unsupported quant type");
        if (n_expert < 1 || n_embd < 256 || n_embd % 256 || n_ff < 256 || n_ff % 256) throw Error("op_moe_decode: bad shape");
        for (int k = 0; k < 2; ++k)
            if (sel[k] < 0 || sel[k] >= n_expert) throw Error("op_moe_decode: expert out of range");
        MI_HIP(hipSetDevice(device));
        ensure_kernel_attributes(device);
        Keep keep;
        const QMat G = upload_experts(type, gate, n_expert, n_ff, n_embd, keep);
        const QMat Up = upload_experts(type, up, n_expert, n_ff, n_embd, keep);
        const QMat D = upload_experts(type, down, n_expert, n_embd, n_ff, keep);
        Dev<float> dx(n_embd, x), dn(n_embd, norm_w), dh((size_t)2 * n_ff), dselw(2, selw), dadd(n_embd, addend);
        Dev<int> dsel(2, sel);
        dh.fill(0xFF);
        float* h = dh.p;
        float* h2 = h + n_ff;
        GemvParams p = gemv_of(PRO_RMSNORM, dx.p, n_embd);
        p.norm_w = dn.p;
        p.eps = eps;
        moe_gate_up_segs(p, G, Up, dsel.p, dselw.p, h, h2);
        launch_gemv(p, nullptr);
        GemvParams d = gemv_of(PRO_PLAIN, h, n_ff);
        d.eps = eps;
        moe_down_seg(d, D, dsel.p, dselw.p, h2, dx.p, addend ? dadd.p : nullptr);
        launch_gemv(d, nullptr);
        MI_HIP(hipDeviceSynchronize());
        dh.download(h_out);
        dx.download(x_out);
        return 0;
    }
    MI_TRY(-1)
}

// One launch of the encoder GEMM (enc.hip enc_gemm_f16_kernel): y[t][r] = sum_k f16(x[t][k]) w[r][k],
// then the epilogue (0 none, 1 bias, 2 bias + gelu, 3 bias + resid).
int32_t mi_op_gemm_f16(int32_t device, const uint16_t* w_f16, int32_t rows, int32_t K, int32_t ntok, const float* x,
                       const float* bias, const float* resid, int32_t epilogue, float* y) {
    try {
        if (!w_f16 || !x || !y) throw Error("op_gemm_f16: null argument");
        if (epilogue < ENC_NONE || epilogue > ENC_RESID) throw Error("op_gemm_f16: epilogue 0 .. 3");
        if (epilogue != ENC_NONE && !bias) throw Error("op_gemm_f16: this epilogue needs a bias");
        if (epilogue == ENC_RESID && !resid) throw Error("op_gemm_f16: residual epilogue without resid");
        if (rows < 32 || rows % 32 || K < 32 || K % 32 || ntok < 1 || ntok > ENC_MAX_TOK)
            throw Error("op_gemm_f16: rows % 32, K % 32, 1 <= ntok <= 512");
        MI_HIP(hipSetDevice(device));
        const size_t ny = (size_t)ntok * rows;
        Dev<__half> dw((size_t)rows * K, f16(w_f16));
        Dev<float> dx((size_t)ntok * K, x), dy(ny), db(rows, epilogue != ENC_NONE ? bias : nullptr);
        Dev<float> dr(ny, epilogue == ENC_RESID ? resid : nullptr);
        Dev<unsigned short> dt(65536, epilogue == ENC_GELU ? gelu_table_host().data() : nullptr);   // ggml_table_gelu_f16
        EncGemm g{};
        g.m[0] = EncMat{dw.p, epilogue != ENC_NONE ? db.p : nullptr, rows, dy.p, nullptr};
        g.nmat = 1;
        g.epi = epilogue;
        g.K = K;
        g.ntok = ntok;
        g.x = dx.p;
        g.x_stride = K;
        g.out_stride = rows;
        g.resid = epilogue == ENC_RESID ? dr.p : nullptr;
        g.gelu_tab = dt.p;
        launch_enc_gemm(g, nullptr);
        MI_HIP(hipDeviceSynchronize());
        dy.download(y);
        return 0;
    }
    MI_TRY(-1)
}

// Bidirectional attention of ntok tokens over themselves (enc.hip enc_attn_kernel): q f32 [ntok][n_head *
// head_dim], k / v f16 of the same shape -> out f32; scale 1 / sqrtf(head_dim).
int32_t mi_op_attention_enc(int32_t device, int32_t n_head, int32_t head_dim, int32_t ntok, const float* q,
                            const uint16_t* k_f16, const uint16_t* v_f16, float* out) {
    try {
        if (!q || !k_f16 || !v_f16 || !out) throw Error("op_attention_enc: null argument");
        if (n_head < 1 || ntok < 1 || ntok > ENC_MAX_TOK || !enc_attn_supported(head_dim))
            throw Error("op_attention_enc: head_dim 32 or 64, 1 <= ntok <= 512");
        MI_HIP(hipSetDevice(device));
        init_enc_attributes();
        const int ne = n_head * head_dim;
        const size_t n = (size_t)ntok * ne;
        Dev<float> dq(n, q), dout(n);
        Dev<__half> dk(n, f16(k_f16)), dv(n, f16(v_f16));
        launch_enc_attn(EncAttn{dq.p, dk.p, dv.p, ne, ne, ne, n_head, head_dim, ntok, 1.0f / std::sqrt((float)head_dim), dout.p},
                        nullptr);
        MI_HIP(hipDeviceSynchronize());
        dout.download(out);
        return 0;
    }
    MI_TRY(-1)
}

}  // extern "C"
