"""Op-level parity of the Q4_0 / Q5_0 kernels: dequantisation, the decode GEMVs (gemv_kernel through
mi_op_gemv, the streaming dgemv_kernel in roles 0-4 through mi_op_dgemv) and the prompt-batch GEMMs
(the short-batch and the tiled MFMA forms through mi_op_gemm).

Reference: the existing oracle on the Q8_0 re-encoding of the same blocks (legacy_quant_util.to_q8_0:
the same d, qs = the signed weights -- the arithmetic ggml's vec_dot_q4_0_q8_0 / vec_dot_q5_0_q8_0
share with vec_dot_q8_0_q8_0), with the helper and the bar of the Q8_0 case of the same op:
test_gpu_ops.GEMV_TOL / test_gpu_dgemv's helpers for the GEMVs, gemm_ref_util for mi_op_gemm."""
import numpy as np
import pytest

import ggml_ref as R
import legacy_quant_util as U
from blama_amd import engine
from gemm_ref_util import GEMM_TOL, gemm_ref, gemm_swiglu_ref, gemv_ref, gemv_swiglu_ref
from test_gpu_dgemv import GEMV_TOL, ROLE_ADD, ROLE_ADDQ, ROLE_QKV, ROLE_STORE, ROLE_SWIGLU
from util import rand_x

pytestmark = pytest.mark.gpu

TYPES = [U.Q4_0, U.Q5_0]
IDS = [U.NAME[t] for t in TYPES]
KS = (256, 768, 2048)          # one superblock, an odd count, a whole 8-superblock pass
ROWS = (2, 34, 320)
Q8 = R.Q8_0


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _gemv_ratio(got, raw8, K, x):
    """max err / bound of a GEMV result against the Q8_0 oracle (the bar of test_gemv_matches_oracle)."""
    ref, absb = gemv_ref(Q8, raw8, K, x)
    return float((np.abs(got.astype(np.float64) - ref) / (absb * GEMV_TOL + 1e-30)).max())


@pytest.mark.parametrize("t", TYPES, ids=IDS)
def test_dequant_bit_exact(gpu_lib, t):
    for rows, K, seed in ((5, 1024, 11), (3, 256, 12), (2, 768, 13)):
        w = U.rand_matrix(t, rows, K, seed=seed)
        got = engine.op_dequant(t, w, rows, K)
        ref = R.dequantize(U.to_q8_0(w, t), Q8)
        assert np.array_equal(_bits(got), _bits(ref)), (U.NAME[t], rows, K)
    w = U.extreme_matrix(t, 4, 512, seed=3)
    assert np.array_equal(_bits(engine.op_dequant(t, w, 4, 512)), _bits(R.dequantize(U.to_q8_0(w, t), Q8)))


@pytest.mark.parametrize("t", TYPES, ids=IDS)
def test_gemv_matches_oracle(gpu_lib, t):
    for K in KS:
        x = rand_x(K, seed=K)
        for rows in ROWS:
            w = U.rand_matrix(t, rows, K, seed=rows * 7 + K)
            r = _gemv_ratio(engine.op_gemv(t, w, rows, K, x), U.to_q8_0(w, t), K, x)
            print(f"gemv {U.NAME[t]} {rows}x{K}: err / bound = {r:.3f}")
            assert r <= 1.0, (U.NAME[t], rows, K, r)


def _dgemv_case(t, role, rows, K, w, x, w2=None, res=None):
    """Runs mi_op_dgemv in `role` and returns max err / bound by test_gpu_dgemv's rule of that role."""
    w8 = U.to_q8_0(w, t)
    if role == ROLE_SWIGLU:
        y = engine.op_dgemv(role, t, w, rows, K, x, type2=t, raw2=w2, rows2=rows)
        g, ga = gemv_ref(Q8, w8, K, x)
        u, ua = gemv_ref(Q8, U.to_q8_0(w2, t), K, x)
        ref, bound = gemv_swiglu_ref(g, ga, u, ua, GEMV_TOL)
        return y, float((np.abs(y.astype(np.float64) - ref) / bound).max())
    y = engine.op_dgemv(role, t, w, rows, K, x, resid=res)
    ref, absb = gemv_ref(Q8, w8, K, x)
    if role in (ROLE_ADD, ROLE_ADDQ):   # y = fl(dot + resid): the GEMV bound plus the rounding of the add
        r = res.astype(np.float64)
        bound = absb * GEMV_TOL + (np.abs(ref) + np.abs(r)) * 1.2e-7 + 1e-30
        return y, float((np.abs(y.astype(np.float64) - (ref + r)) / bound).max())
    return y, float((np.abs(y.astype(np.float64) - ref) / (absb * GEMV_TOL + 1e-30)).max())


@pytest.mark.parametrize("role", [ROLE_QKV, ROLE_ADD, ROLE_SWIGLU, ROLE_STORE, ROLE_ADDQ])
@pytest.mark.parametrize("t", TYPES, ids=IDS)
def test_dgemv_roles_match_oracle(gpu_lib, t, role):
    for K in KS:
        x = rand_x(K, seed=K + 3)
        for rows in ROWS:
            w = U.rand_matrix(t, rows, K, seed=rows + K + t)
            w2 = U.rand_matrix(t, rows, K, seed=rows + K + t + 50) if role == ROLE_SWIGLU else None
            res = rand_x(rows, seed=rows + 1) if role in (ROLE_ADD, ROLE_ADDQ) else None
            _, r = _dgemv_case(t, role, rows, K, w, x, w2, res)
            print(f"dgemv role {role} {U.NAME[t]} {rows}x{K}: err / bound = {r:.3f}")
            assert r <= 1.0, (U.NAME[t], role, rows, K, r)


@pytest.mark.parametrize("t", TYPES, ids=IDS)
def test_dgemv_inlaunch_quant_same_bits(gpu_lib, t):
    """Role 4 quantises x in every workgroup with dv_quant_kernel's arithmetic: role 1's bits."""
    rows, K = 34, 768
    w = U.rand_matrix(t, rows, K, seed=5)
    x, res = rand_x(K, seed=6), rand_x(rows, seed=7)
    y1 = engine.op_dgemv(ROLE_ADD, t, w, rows, K, x, resid=res)
    y4 = engine.op_dgemv(ROLE_ADDQ, t, w, rows, K, x, resid=res)
    assert np.array_equal(_bits(y1), _bits(y4))


def _gemm_ratio(t, got, raw, up, rows, K, X):
    g, bg = gemm_ref(Q8, U.to_q8_0(raw, t), rows, K, X)
    if up is None:
        return float((np.abs(got - g) / (GEMM_TOL * bg + 1e-30)).max())
    u, bu = gemm_ref(Q8, U.to_q8_0(up, t), rows, K, X)
    ref, lim = gemm_swiglu_ref(g, bg, u, bu)
    return float((np.abs(got - ref) / lim).max())


# <= 64 tokens: the short-batch split-K form (one and two token tiles); above: the tiled form
@pytest.mark.parametrize("pair", [False, True], ids=["one", "pair"])
@pytest.mark.parametrize("ntok", [1, 20, 33, 64, 65, 512])
@pytest.mark.parametrize("t", TYPES, ids=IDS)
def test_gemm_matches_oracle(gpu_lib, t, ntok, pair):
    for K in (256, 768):
        X = np.stack([rand_x(K, seed=K * 1000 + i) for i in range(ntok)])
        X[ntok // 2, :256] = 0.0                           # an all-zero activation block (d = 0)
        for rows in (32, 96, 320):
            raw = U.rand_matrix(t, rows, K, seed=rows + K + ntok)
            up = U.rand_matrix(t, rows, K, seed=rows + K + ntok + 1) if pair else None
            got = engine.op_gemm(t, raw, rows, K, X, raw_up=up).astype(np.float64)
            r = _gemm_ratio(t, got, raw, up, rows, K, X)
            print(f"gemm {U.NAME[t]} {rows}x{K} x {ntok}{' pair' if pair else ''}: err / bound = {r:.3f}")
            assert r <= 1.0, (U.NAME[t], rows, K, ntok, pair, r)


@pytest.mark.parametrize("t", TYPES, ids=IDS)
def test_gemm_tiled_form_at_a_short_count(gpu_lib, monkeypatch, t):
    """The tiled GEMM pinned at a count mi_op_gemm would send to the short form, rows that leave a
    partial tile."""
    monkeypatch.setenv("MI_MMQS_MAX", "0")
    rows, K, ntok = 77, 768, 40
    X = np.stack([rand_x(K, seed=70 + i) for i in range(ntok)])
    for pair in (False, True):
        raw = U.rand_matrix(t, rows, K, seed=21)
        up = U.rand_matrix(t, rows, K, seed=22) if pair else None
        got = engine.op_gemm(t, raw, rows, K, X, raw_up=up).astype(np.float64)
        assert _gemm_ratio(t, got, raw, up, rows, K, X) <= 1.0


@pytest.mark.parametrize("t", TYPES, ids=IDS)
def test_adversarial_extremes(gpu_lib, t):
    """Weights at -8 / +7 (-16 / +15) only, activations that quantise to +-127 only: every block sum
    is at the size where a wrong offset, sign or nibble half is far outside the bar."""
    rows, K = 34, 768
    w = U.extreme_matrix(t, rows, K, seed=9)
    w2 = U.extreme_matrix(t, rows, K, seed=10)
    x = U.extreme_x(K, seed=11)
    assert set(np.unique(R.quantize_q8_0(x).qs)) <= {-127, 127}
    w8 = U.to_q8_0(w, t)
    assert np.array_equal(_bits(engine.op_dequant(t, w, rows, K)), _bits(R.dequantize(w8, Q8)))
    assert _gemv_ratio(engine.op_gemv(t, w, rows, K, x), w8, K, x) <= 1.0
    res = rand_x(rows, seed=12)
    for role in (ROLE_QKV, ROLE_ADD, ROLE_SWIGLU, ROLE_STORE, ROLE_ADDQ):
        _, r = _dgemv_case(t, role, rows, K, w, x, w2, res if role in (ROLE_ADD, ROLE_ADDQ) else None)
        assert r <= 1.0, (U.NAME[t], role, r)
    for ntok in (20, 65):
        X = np.stack([U.extreme_x(K, seed=30 + i) for i in range(ntok)])
        for up in (None, w2):
            got = engine.op_gemm(t, w, rows, K, X, raw_up=up).astype(np.float64)
            assert _gemm_ratio(t, got, w, up, rows, K, X) <= 1.0, (U.NAME[t], ntok, up is not None)


def _wrong_q8_0(raw, t, how):
    """The Q8_0 re-encoding a faulty kernel would match: the offset one short (7 / 15 instead of
    8 / 16), or the low-nibble and the high-nibble halves of every block swapped."""
    b = U.to_q8_0(raw, t).reshape(-1, 34).copy()
    q = b[:, 2:].view(np.int8)
    if how == "offset":
        q += 1
    else:
        q[:] = np.concatenate([q[:, 16:], q[:, :16]], axis=1)
    return b.reshape(-1)


@pytest.mark.parametrize("how", ["offset", "halves"])
@pytest.mark.parametrize("t", TYPES, ids=IDS)
def test_a_fault_would_be_detected(gpu_lib, t, how):
    """Test of the test: against the GPU result of a random case, references built with the offset
    one short and with the block halves swapped fail the bar of every op."""
    rows, K, ntok = 34, 768, 20
    w = U.rand_matrix(t, rows, K, seed=41)
    x = rand_x(K, seed=42)
    bad = _wrong_q8_0(w, t, how)
    assert not np.array_equal(_bits(engine.op_dequant(t, w, rows, K)), _bits(R.dequantize(bad, Q8)))
    for got in (engine.op_gemv(t, w, rows, K, x), engine.op_dgemv(ROLE_STORE, t, w, rows, K, x)):
        assert _gemv_ratio(got, U.to_q8_0(w, t), K, x) <= 1.0
        r = _gemv_ratio(got, bad, K, x)
        print(f"{U.NAME[t]} wrong {how}: gemv err / bound = {r:.1f}")
        assert r > 10.0
    X = np.stack([rand_x(K, seed=50 + i) for i in range(ntok)])
    got = engine.op_gemm(t, w, rows, K, X).astype(np.float64)
    g, bg = gemm_ref(Q8, bad, rows, K, X)
    r = float((np.abs(got - g) / (GEMM_TOL * bg + 1e-30)).max())
    print(f"{U.NAME[t]} wrong {how}: gemm err / bound = {r:.1f}")
    assert r > 10.0


@pytest.mark.parametrize("t", TYPES, ids=IDS)
def test_deterministic(gpu_lib, t):
    rows, K = 96, 2048
    w = U.rand_matrix(t, rows, K, seed=3)
    x = rand_x(K, seed=4)
    X = np.stack([rand_x(K, seed=60 + i) for i in range(33)])
    for f in (lambda: engine.op_gemv(t, w, rows, K, x),
              lambda: engine.op_dgemv(ROLE_QKV, t, w, rows, K, x),
              lambda: engine.op_gemm(t, w, rows, K, X),
              lambda: engine.op_gemm(t, w, rows, K, np.concatenate([X, X, X]))):
        assert np.array_equal(_bits(f()), _bits(f()))


def test_moe_ops_keep_refusing(gpu_lib):
    w = U.rand_matrix(U.Q4_0, 2 * 32, 256, seed=1)
    with pytest.raises(engine.EngineError):
        engine.op_moe_gemm(0, U.Q4_0, w, 2, 32, 256, np.zeros((4, 256), np.float32), np.zeros(4, np.int32))
