"""The float64 restatements the op-level GEMM / GEMV tests share (test_gpu_batch_ops.py,
test_gpu_dgemv.py, test_gpu_moe_ops.py): a quantised matrix times Q8_K / Q8_0 activations with the
bound sum_b |term_b| every fp32 summation order stays within, and the SwiGLU bounds built on it."""
import numpy as np

import ggml_ref as R

GEMM_TOL = 2e-5


def _act_blocks(t, X):
    """Dequantised activations per quant block: (blk_elems, A[T, nblk, blk_elems] f64)."""
    T, K = X.shape
    if t == R.Q8_0:
        a = [R.quantize_q8_0(x) for x in X]
        A = np.stack([q.d[:, None].astype(np.float64) * q.qs for q in a])          # (T, K/32, 32)
        return 32, A
    a = [R.quantize_q8_K(x) for x in X]
    A = np.stack([q.d[:, None].astype(np.float64) * q.qs for q in a])              # (T, K/256, 256)
    return 256, A


def _weight_blocks(t, raw, rows, K):
    """(Wp, Wm): the per-block weights split into the d*scale*q part and the -dmin*m part
    (Q4_K only; None otherwise), f64 (rows, nblk, blk_elems)."""
    if t in (R.Q4_K, R.Q5_K):
        d, dmin, sc, m, q = (R.unpack_q4_K if t == R.Q4_K else R.unpack_q5_K)(raw)
        nb = K // 256
        q = q.reshape(rows, nb, 8, 32).astype(np.float64)
        Wp = d.reshape(rows, nb, 1, 1).astype(np.float64) * sc.reshape(rows, nb, 8, 1) * q
        Wm = np.broadcast_to((dmin.reshape(rows, nb, 1, 1).astype(np.float64) * m.reshape(rows, nb, 8, 1)),
                             (rows, nb, 8, 32))
        return Wp.reshape(rows, nb, 256), -Wm.reshape(rows, nb, 256)
    if t == R.Q6_K:
        d, sc, q = R.unpack_q6_K(raw)
        nb = K // 256
        Wp = d.reshape(rows, nb, 1, 1).astype(np.float64) * sc.reshape(rows, nb, 16, 1) * \
            q.reshape(rows, nb, 16, 16).astype(np.float64)
        return Wp.reshape(rows, nb, 256), None
    d, q = R.unpack_q8_0(raw)
    nb = K // 32
    return d.reshape(rows, nb, 1).astype(np.float64) * q.reshape(rows, nb, 32), None


def gemm_ref(t, raw, rows, K, X, act=None):
    """y[T, rows] and the bound sum_b |term_b| (f64), all tokens at once.  act: X's blocks as
    _act_blocks(t, X)[1] returns them, when the caller already has them (several matrices over one
    activation)."""
    A = _act_blocks(t, X)[1] if act is None else act
    Wp, Wm = _weight_blocks(t, raw, rows, K)
    T = A.shape[0]
    y = np.zeros((T, rows))
    bound = np.zeros((T, rows))
    for b in range(A.shape[1]):
        yp = A[:, b] @ Wp[:, b].T
        y += yp
        bound += np.abs(yp)
        if Wm is not None:
            ym = A[:, b] @ Wm[:, b].T
            y += ym
            bound += np.abs(ym)
    return y, bound


def gemm_swiglu_ref(g, bg, u, bu):
    """silu(g) * u (f64) of a gate/up pair of gemm_ref results and its bound:
    d(silu(g) u) <= |silu'(g)| |u| eg + |silu(g)| eu, |silu'| <= 1.1; plus the fp32 epilogue."""
    s = g / (1.0 + np.exp(-g))
    ref = s * u
    lim = GEMM_TOL * (1.1 * np.abs(u) * bg + np.abs(s) * bu) + 1e-6 * np.abs(ref) + 1e-30
    return ref, lim


def gemv_ref(t, raw, K, x, sel=None):
    """(y f64 of R.mul_mat_vec's f32 result, sum_b |term_b|) of one activation; sel: a row subset."""
    if sel is not None:
        raw = raw.reshape(-1, R.row_bytes(t, K))[sel].reshape(-1)
    return R.mul_mat_vec(raw, t, K, x).astype(np.float64), R.mul_mat_vec_abs(raw, t, K, x)


def gemv_swiglu_ref(g, ga, u, ua, tol):
    """silu(g) * u in fp32 (ggml_vec_swiglu_f32 of b5187: silu then mul) of a gate/up pair of
    gemv_ref results, and the bound that propagates the GEMV bounds of g and u through the product."""
    g32, u32 = g.astype(np.float32), u.astype(np.float32)
    ref = (g32 / (np.float32(1) + np.exp(-g32))) * u32
    sg = 1.0 / (1.0 + np.exp(-g))
    dsilu = np.abs(sg * (1 + g * (1 - sg)))
    bound = (dsilu * np.abs(u) * ga + np.abs(g * sg) * ua) * tol + np.abs(ref) * 3e-7 + 1e-30
    return ref.astype(np.float64), bound
