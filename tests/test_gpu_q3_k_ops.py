"""Op-level parity of the Q3_K kernels: dequantisation, the decode GEMVs (gemv_kernel through
mi_op_gemv, the streaming dgemv_kernel through mi_op_dgemv) and the prompt-batch GEMMs (the
short-batch and the tiled MFMA forms through mi_op_gemm).

Reference: the existing oracle on the Q6_K re-encoding of the same blocks (q3_k_util.to_q6_k: the
same d, scales sc6 - 32, values q + 32), with the helper and the bar of the Q6_K case of the same op:
test_gpu_dgemv's rules for the GEMVs, gemm_ref_util for mi_op_gemm."""
import numpy as np
import pytest

import ggml_ref as R
import q3_k_util as U
from blama_amd import engine
from gemm_ref_util import GEMM_TOL, gemm_ref, gemm_swiglu_ref, gemv_ref, gemv_swiglu_ref
from test_gpu_dgemv import GEMV_TOL, ROLE_ADD, ROLE_ADDQ, ROLE_QKV, ROLE_STORE, ROLE_SWIGLU, _check
from util import rand_matrix, rand_x

pytestmark = pytest.mark.gpu

T = U.Q3_K
KS = (256, 768, 2048)          # one superblock, an odd count, a whole 8-superblock pass
ROWS = (2, 34, 320)
ROLES = [ROLE_QKV, ROLE_ADD, ROLE_SWIGLU, ROLE_STORE, ROLE_ADDQ]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _ref(w, K, x):
    return gemv_ref(R.Q6_K, U.to_q6_k(w), K, x)


def _dgemv(role, rows, K, w, x, w2, res):
    """mi_op_dgemv in `role` under test_gpu_dgemv's rule of that role (w2: SwiGLU's up; res: the adds' residual)."""
    w2, res = w2 if role == ROLE_SWIGLU else None, res if role in (ROLE_ADD, ROLE_ADDQ) else None
    y = engine.op_dgemv(role, T, w, rows, K, x, type2=T, raw2=w2, rows2=rows, resid=res)
    ref, absb = _ref(w, K, x)
    if w2 is None and res is None:
        return _check(y, ref, absb, (role, rows, K))
    if w2 is not None:
        ref, bound = gemv_swiglu_ref(ref, absb, *_ref(w2, K, x), GEMV_TOL)
    else:   # y = fl(dot + resid): the GEMV bound plus the rounding of the add
        bound = absb * GEMV_TOL + (np.abs(ref) + np.abs(res)) * 1.2e-7 + 1e-30
        ref = ref + res
    err = np.abs(y.astype(np.float64) - ref)
    assert np.all(err <= bound), (role, rows, K, float((err / bound).max()))


def _gemm(raw, up, rows, K, X):
    got = engine.op_gemm(T, raw, rows, K, X, raw_up=up).astype(np.float64)
    ref, bg = gemm_ref(R.Q6_K, U.to_q6_k(raw), rows, K, X)
    lim = GEMM_TOL * bg + 1e-30
    if up is not None:
        ref, lim = gemm_swiglu_ref(ref, bg, *gemm_ref(R.Q6_K, U.to_q6_k(up), rows, K, X))
    assert np.all(np.abs(got - ref) <= lim), (rows, K, len(X), up is not None, float((np.abs(got - ref) / lim).max()))


@pytest.mark.parametrize("rows,K,w", [(3, 256, U.rand_matrix(3, 256, 12)), (2, 768, U.rand_matrix(2, 768, 13)),
                                      (4, 512, U.extreme_matrix(4, 512, 3))], ids=["256", "768", "extreme"])
def test_dequant_bit_exact(gpu_lib, rows, K, w):
    assert np.array_equal(_bits(engine.op_dequant(T, w, rows, K)), _bits(R.dequantize(U.to_q6_k(w), R.Q6_K)))


@pytest.mark.parametrize("K", KS)
def test_gemv_matches_oracle(gpu_lib, K):
    x = rand_x(K, seed=K)
    for rows in ROWS:
        w = U.rand_matrix(rows, K, rows * 7 + K)
        _check(engine.op_gemv(T, w, rows, K, x), *_ref(w, K, x), (rows, K))


@pytest.mark.parametrize("role", ROLES)
def test_dgemv_roles_match_oracle(gpu_lib, role):
    for K in KS:
        x = rand_x(K, seed=K + 3)
        for rows in ROWS:
            _dgemv(role, rows, K, U.rand_matrix(rows, K, rows + K), x, U.rand_matrix(rows, K, rows + K + 50),
                   rand_x(rows, seed=rows + 1))


def test_dgemv_inlaunch_quant_same_bits(gpu_lib):
    rows, K = 34, 768
    w, x, res = U.rand_matrix(rows, K, 5), rand_x(K, seed=6), rand_x(rows, seed=7)
    assert np.array_equal(_bits(engine.op_dgemv(ROLE_ADD, T, w, rows, K, x, resid=res)),
                          _bits(engine.op_dgemv(ROLE_ADDQ, T, w, rows, K, x, resid=res)))


def test_dgemv_mixed_qkv(gpu_lib, tv=R.Q4_K):
    """The Q3_K_M launch: Q and K rows as Q3_K, V rows as Q4_K, both segments of one launch."""
    rows0, rows1, K = 320, 34, 768
    w0, w1, x = U.rand_matrix(rows0, K, 31), rand_matrix(tv, rows1, K, seed=32), rand_x(K, seed=33)
    y = engine.op_dgemv(ROLE_QKV, T, w0, rows0, K, x, type2=tv, raw2=w1, rows2=rows1)
    _check(y[:rows0], *_ref(w0, K, x), "Q3_K segment")
    _check(y[rows0:], *gemv_ref(tv, w1, K, x), "Q4_K segment")


# <= 64 tokens: the short-batch split-K form (one and two token tiles); above: the tiled form, 160 =
# one full token block and a partial one
@pytest.mark.parametrize("pair", [False, True], ids=["one", "pair"])
@pytest.mark.parametrize("ntok", [1, 33, 64, 65, 160])
def test_gemm_matches_oracle(gpu_lib, ntok, pair):
    for K in (256, 768):
        X = np.stack([rand_x(K, seed=K * 1000 + i) for i in range(ntok)])
        X[ntok // 2, :256] = 0.0                           # an all-zero activation superblock (d = 0)
        for rows in (32, 77, 320):
            _gemm(U.rand_matrix(rows, K, rows + K + ntok), U.rand_matrix(rows, K, rows + K + ntok + 1) if pair else None,
                  rows, K, X)


def test_gemm_tiled_form_at_a_short_count(gpu_lib, monkeypatch):
    monkeypatch.setenv("MI_MMQS_MAX", "0")
    rows, K, ntok = 77, 768, 40
    X = np.stack([rand_x(K, seed=70 + i) for i in range(ntok)])
    for up in (None, U.rand_matrix(rows, K, 22)):
        _gemm(U.rand_matrix(rows, K, 21), up, rows, K, X)


def test_adversarial_extremes(gpu_lib):
    """Weights at -4 / +3 and scales at -32 / +31 only, whole sub-blocks at (-4)(-32) = +128, Q8_K
    activations of +-127 only: an operand that wraps at +128, a wrong mask bit or a wrong scale nibble
    moves the sums by a large part of their size."""
    rows, K = 34, 768
    w, w2 = U.extreme_matrix(rows, K, 9), U.extreme_matrix(rows, K, 10)
    q, sc6, _ = U.unpack(w)
    assert set(np.unique(q)) == {-4, 3} and set(np.unique(sc6)) == {0, 63}
    assert ((q.reshape(-1, 16, 16) * (sc6 - 32)[:, :, None]) == 128).all(2).any()
    x = U.extreme_x(K, 11)
    assert set(np.unique(R.quantize_q8_K(x).qs)) <= {-127, 127}
    _check(engine.op_gemv(T, w, rows, K, x), *_ref(w, K, x), "gemv")
    for role in ROLES:
        _dgemv(role, rows, K, w, x, w2, rand_x(rows, seed=12))
    for ntok in (20, 65):
        X = np.stack([U.extreme_x(K, 30 + i) for i in range(ntok)])
        for up in (None, w2):
            _gemm(w, up, rows, K, X)


def test_deterministic(gpu_lib):
    rows, K = 96, 2048
    w, x = U.rand_matrix(rows, K, 3), rand_x(K, seed=4)
    X = np.stack([rand_x(K, seed=60 + i) for i in range(33)])
    for f in (lambda: engine.op_gemv(T, w, rows, K, x),
              lambda: engine.op_dgemv(ROLE_QKV, T, w, rows, K, x),
              lambda: engine.op_gemm(T, w, rows, K, X),
              lambda: engine.op_gemm(T, w, rows, K, np.concatenate([X, X, X]))):
        assert np.array_equal(_bits(f()), _bits(f()))
