"""Op-level parity of the IQ4_NL / IQ4_XS kernels: dequantisation, the decode GEMVs (gemv_kernel
through mi_op_gemv, the streaming dgemv_kernel through mi_op_dgemv) and the prompt-batch GEMMs (the
one-wave short, two-tile short and tiled MFMA forms through mi_op_gemm).

Reference (iq4_util): IQ4_NL is the existing oracle on its exact Q8_0 re-encoding; IQ4_XS the
restatement of vec_dot_iq4_xs_q8_K over the oracle's Q8_K activations.  Both give the (ref, sum
|terms|) pair that test_gpu_dgemv's _check / GEMV_TOL and gemm_ref_util's GEMM_TOL take."""
import numpy as np
import pytest

import ggml_ref as R
import iq4_util as U
import legacy_quant_util
import q3_k_util
from blama_amd import engine
from gemm_ref_util import GEMM_TOL, gemm_swiglu_ref, gemv_ref, gemv_swiglu_ref
from test_gpu_dgemv import GEMV_TOL, ROLE_ADD, ROLE_ADDQ, ROLE_QKV, ROLE_STORE, ROLE_SWIGLU, _check
from util import rand_matrix, rand_x

pytestmark = pytest.mark.gpu

TYPES = pytest.mark.parametrize("t", [U.IQ4_NL, U.IQ4_XS], ids=["iq4_nl", "iq4_xs"])
KS = (256, 768, 2048)          # one superblock, an odd count, a whole 8-superblock pass
ROWS = (2, 34, 320)
ROLES = [ROLE_QKV, ROLE_ADD, ROLE_SWIGLU, ROLE_STORE, ROLE_ADDQ]
EXTREME_X = {U.IQ4_NL: legacy_quant_util.extreme_x, U.IQ4_XS: q3_k_util.extreme_x}   # +-127 only, per Q8_0 / Q8_K block


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _dgemv(t, role, rows, K, w, x, w2, res):
    """mi_op_dgemv in `role` under test_gpu_dgemv's rule of that role (w2: SwiGLU's up; res: the adds' residual)."""
    w2, res = w2 if role == ROLE_SWIGLU else None, res if role in (ROLE_ADD, ROLE_ADDQ) else None
    y = engine.op_dgemv(role, t, w, rows, K, x, type2=t, raw2=w2, rows2=rows, resid=res)
    ref, absb = U.gemv_ref(t, w, K, x)
    if w2 is None and res is None:
        return _check(y, ref, absb, (t, role, rows, K))
    if w2 is not None:
        ref, bound = gemv_swiglu_ref(ref, absb, *U.gemv_ref(t, w2, K, x), GEMV_TOL)
    else:   # y = fl(dot + resid): the GEMV bound plus the rounding of the add
        bound = absb * GEMV_TOL + (np.abs(ref) + np.abs(res)) * 1.2e-7 + 1e-30
        ref = ref + res
    err = np.abs(y.astype(np.float64) - ref)
    assert np.all(err <= bound), (t, role, rows, K, float((err / bound).max()))


def _gemm(t, raw, up, rows, K, X):
    got = engine.op_gemm(t, raw, rows, K, X, raw_up=up).astype(np.float64)
    ref, bg = U.gemm_ref(t, raw, rows, K, X)
    lim = GEMM_TOL * bg + 1e-30
    if up is not None:
        ref, lim = gemm_swiglu_ref(ref, bg, *U.gemm_ref(t, up, rows, K, X))
    assert np.all(np.abs(got - ref) <= lim), (t, rows, K, len(X), up is not None, float((np.abs(got - ref) / lim).max()))


@TYPES
@pytest.mark.parametrize("rows,K,kind", [(3, 256, "rand"), (2, 768, "rand"), (4, 512, "extreme")])
def test_dequant_bit_exact(gpu_lib, t, rows, K, kind):
    w = U.rand_matrix(t, rows, K, 12 + K) if kind == "rand" else U.extreme_matrix(t, rows, K, 3)
    assert np.array_equal(_bits(engine.op_dequant(t, w, rows, K)), _bits(U.dequantize(w, t)))


@TYPES
@pytest.mark.parametrize("K", KS)
def test_gemv_matches_oracle(gpu_lib, t, K):
    x = rand_x(K, seed=K)
    for rows in ROWS:
        w = U.rand_matrix(t, rows, K, rows * 7 + K)
        _check(engine.op_gemv(t, w, rows, K, x), *U.gemv_ref(t, w, K, x), (t, rows, K))


@TYPES
@pytest.mark.parametrize("role", ROLES)
def test_dgemv_roles_match_oracle(gpu_lib, t, role):
    for K in KS:
        x = rand_x(K, seed=K + 3)
        for rows in ROWS:
            _dgemv(t, role, rows, K, U.rand_matrix(t, rows, K, rows + K), x, U.rand_matrix(t, rows, K, rows + K + 50),
                   rand_x(rows, seed=rows + 1))


@TYPES
def test_dgemv_inlaunch_quant_same_bits(gpu_lib, t):
    rows, K = 34, 768
    w, x, res = U.rand_matrix(t, rows, K, 5), rand_x(K, seed=6), rand_x(rows, seed=7)
    assert np.array_equal(_bits(engine.op_dgemv(ROLE_ADD, t, w, rows, K, x, resid=res)),
                          _bits(engine.op_dgemv(ROLE_ADDQ, t, w, rows, K, x, resid=res)))


def test_dgemv_mixed_qkv(gpu_lib, tv=R.Q5_K):
    """The streaming step's Q/K/V launch of an IQ4_XS file: Q and K rows as IQ4_XS, V rows as Q5_K, both
    segments of one launch (test_gpu_iq4.py holds a model to the decode path that issues it)."""
    rows0, rows1, K = 320, 34, 768
    w0, w1, x = U.rand_matrix(U.IQ4_XS, rows0, K, 31), rand_matrix(tv, rows1, K, seed=32), rand_x(K, seed=33)
    y = engine.op_dgemv(ROLE_QKV, U.IQ4_XS, w0, rows0, K, x, type2=tv, raw2=w1, rows2=rows1)
    _check(y[:rows0], *U.gemv_ref(U.IQ4_XS, w0, K, x), "IQ4_XS segment")
    _check(y[rows0:], *gemv_ref(tv, w1, K, x), "Q5_K segment")


# 2 and 20 tokens: one token tile, the one-wave short form; 64: two tiles, the short form; 130: the
# tiled form, one full token block and a partial one (test_mmq_plan's boundaries)
@TYPES
@pytest.mark.parametrize("pair", [False, True], ids=["one", "pair"])
@pytest.mark.parametrize("ntok", [2, 20, 64, 130])
def test_gemm_matches_oracle(gpu_lib, t, ntok, pair):
    for K in (256, 768):
        X = np.stack([rand_x(K, seed=K * 1000 + i) for i in range(ntok)])
        X[ntok // 2, :256] = 0.0                           # an all-zero activation superblock (d = 0)
        for rows in (32, 77, 320):
            _gemm(t, U.rand_matrix(t, rows, K, rows + K + ntok), U.rand_matrix(t, rows, K, rows + K + ntok + 1) if pair else None,
                  rows, K, X)


@TYPES
def test_adversarial_extremes(gpu_lib, t):
    """Codebook indices 0 / 15 and (IQ4_XS) scales -32 / +31 only, activations of +-127 only: w reaches
    both ends of the hi / lo split, -3937 and +4064; a wrong table half, nibble or scale bit moves every sum
    by a large part of its size.  Once through the GEMV and once through each GEMM form."""
    rows, K = 34, 768
    w, w2 = U.extreme_matrix(t, rows, K, 9), U.extreme_matrix(t, rows, K, 10)
    parts = U.unpack(w, t)
    assert set(np.unique(parts[0])) == {-127, 113}
    if t == U.IQ4_XS:
        assert set(np.unique(parts[1])) == {0, 63}
        sw = parts[0].reshape(-1, 8, 32) * (parts[1] - 32)[:, :, None]
        assert sw.min() == 31 * -127 and sw.max() == -32 * -127   # -3937 .. +4064: the range's two ends
    x = EXTREME_X[t](K, 11)
    _check(engine.op_gemv(t, w, rows, K, x), *U.gemv_ref(t, w, K, x), "gemv")
    _dgemv(t, ROLE_SWIGLU, rows, K, w, x, w2, None)
    for ntok in (20, 64, 130):
        _gemm(t, w, w2, rows, K, np.stack([EXTREME_X[t](K, 30 + i) for i in range(ntok)]))
