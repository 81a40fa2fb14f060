"""Op-level parity of the F16 decode step's streaming GEMV (blama_amd/csrc/fgemv.hip, mi_op_fgemv)
against the float64 dot of the f16-rounded operands.

Bar (derived, as tests/test_gpu_bert_ops.py's GEMM bar; no free tolerance): the kernel rounds x to
f16 as ggml does and adds exact f16 products in f32, so a dot is off by at most
K * 2^-24 * sum_k |x16_k w_k|, plus one f32 ulp of the reference for each separate f32 operation of
the epilogue (the residual add of role 1).  SwiGLU (role 2) is checked in two steps that add nothing
to that rule: its gate and up dots under the plain bar (role 0 over the same two matrices: the sum
order is K's alone, so these are the bits role 2 sums), and its output against silu(g) * u formed in
float64 from those dots, within one f32 ulp for each of the epilogue's four separate f32 operations
(expf, the add, the divide, the multiply).  The wrong product of the two dots is about 4e6 ulps away."""
import numpy as np
import pytest

from blama_amd import engine

pytestmark = pytest.mark.gpu

SHAPES = [(40, 96), (256, 256), (768, 2048), (512, 11008), (4096, 256)]


def _ulp32(a):
    a = np.abs(np.asarray(a, np.float64)).astype(np.float32)
    return (np.nextafter(a, np.float32(np.inf)) - a).astype(np.float64)


def _data(rows, K, seed):
    rng = np.random.default_rng(seed)
    w = (rng.standard_normal((rows, K)) * 0.03).astype(np.float16)
    x = rng.standard_normal(K).astype(np.float32)
    return w, x


def _dot(w, x):
    """(float64 dot of the f16-rounded operands, its bar) per row."""
    x16 = x.astype(np.float16).astype(np.float64)
    W = w.astype(np.float64)
    return W @ x16, w.shape[1] * 2.0 ** -24 * (np.abs(W) @ np.abs(x16))


def _assert_within(got, ref, bar, tag):
    d = np.abs(got.astype(np.float64) - ref)
    worst = float(np.max(d / np.maximum(bar, 1e-300)))
    print(f"{tag}: max err / bar = {worst:.3f}")
    assert np.all(d <= bar), (tag, worst)


@pytest.mark.parametrize("rows,K", SHAPES)
def test_role_store(gpu_lib, rows, K):
    w, x = _data(rows, K, 1)
    ref, bar = _dot(w, x)
    _assert_within(engine.op_fgemv(3, w, x), ref, bar, f"store {rows}x{K}")


@pytest.mark.parametrize("rows,K", SHAPES)
def test_role_qkv_two_matrices(gpu_lib, rows, K):
    rows2 = rows // 2 + 2   # a second matrix of other (even) rows
    w, x = _data(rows, K, 2)
    w2, _ = _data(rows2, K, 3)
    ref = np.concatenate([_dot(w, x)[0], _dot(w2, x)[0]])
    bar = np.concatenate([_dot(w, x)[1], _dot(w2, x)[1]])
    got = engine.op_fgemv(0, w, x, w2=w2)
    assert got.shape == (rows + rows2,)
    _assert_within(got, ref, bar, f"qkv {rows}+{rows2}x{K}")


@pytest.mark.parametrize("rows,K", SHAPES)
def test_role_residual(gpu_lib, rows, K):
    w, x = _data(rows, K, 4)
    resid = np.random.default_rng(5).standard_normal(rows).astype(np.float32)
    ref, bar = _dot(w, x)
    ref = ref + resid.astype(np.float64)
    _assert_within(engine.op_fgemv(1, w, x, resid=resid), ref, bar + _ulp32(ref), f"add {rows}x{K}")


@pytest.mark.parametrize("rows,K", SHAPES)
def test_role_swiglu(gpu_lib, rows, K):
    w, x = _data(rows, K, 6)
    w = (w.astype(np.float32) * 8).astype(np.float16)   # gate values of O(1): silu away from its linear range
    u, _ = _data(rows, K, 7)
    g, bg = _dot(w, x)
    up, bu = _dot(u, x)
    dots = engine.op_fgemv(0, w, x, w2=u)
    _assert_within(dots, np.concatenate([g, up]), np.concatenate([bg, bu]), f"swiglu dots {rows}x{K}")
    gd, ud = dots[:rows].astype(np.float64), dots[rows:].astype(np.float64)
    ref = gd / (1.0 + np.exp(-gd)) * ud
    _assert_within(engine.op_fgemv(2, w, x, w2=u), ref, 4 * _ulp32(ref), f"swiglu {rows}x{K}")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("rows,K", [(40, 96), (768, 2048), (512, 11008)])
def test_bit_reproducible_and_grid_independent(gpu_lib, rows, K):
    """The same inputs give the same bits; a row's result does not depend on the launch it is
    part of: role 3 over the rows split into two calls equals the one-call result bit for bit, and
    so do the other roles' dots (role 0: its rows; role 1 with a zero residual)."""
    w, x = _data(rows, K, 8)
    one = engine.op_fgemv(3, w, x)
    assert np.array_equal(_bits(one), _bits(engine.op_fgemv(3, w, x)))
    cut = (rows // 3) | 1   # an odd split: other workgroups, other waves
    two = np.concatenate([engine.op_fgemv(3, w[:cut], x), engine.op_fgemv(3, w[cut:], x)])
    assert np.array_equal(_bits(one), _bits(two))
    assert np.array_equal(_bits(one), _bits(engine.op_fgemv(0, w, x)))
    zero = np.zeros(rows, np.float32)
    assert np.array_equal(_bits(one + zero), _bits(engine.op_fgemv(1, w, x, resid=zero)))


def test_bad_shapes_are_refused(gpu_lib):
    w, x = _data(8, 48, 9)   # K not a multiple of 32
    with pytest.raises(engine.EngineError, match="multiple of 32"):
        engine.op_fgemv(3, w, x)
    w, x = _data(7, 64, 9)   # role 0 needs even row counts
    with pytest.raises(engine.EngineError, match="even"):
        engine.op_fgemv(0, w, x)
