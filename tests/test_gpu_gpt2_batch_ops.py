"""Op-level parity of the GPT-2 prompt-batch launches through mi_op_gemm_bias: launch_quant_act
(plain and LayerNorm mode) and the tiled int8-MFMA GEMM with a projection bias and the store /
residual-add / GELU epilogues (mmq.hip: quant_act_kernel<.., LN>, mmq2_t<.., GX>).

GEMM bar: the project's GEMM op bar, GEMM_TOL x sum_b |term_b| (gemm_ref_util / test_gpu_batch_ops.py):
the per-block integer dots are exact, only the fp32 order of the block sums differs, and the bias and
the residual are added to that sum as the oracle adds them (one more f32 rounding each, 1e-6 |.|).
GELU: the table is indexed by fp16(p); an output is accepted when it lies between the smallest and
the largest R.gelu value over the f16 neighbours of p +- bar.
LayerNorm mode: the quantised activation itself, for inputs on which the oracle does not sit on a
rounding boundary (its float32 and float64 evaluations agree): equal quants, d within 2 ulp."""
import functools

import numpy as np
import pytest

import ggml_ref as R
from blama_amd import engine
from gemm_ref_util import GEMM_TOL, gemv_ref
from util import rand_matrix, rand_x

pytestmark = pytest.mark.gpu

SHAPES = [(40, 256), (2304, 768), (81, 768)]   # (rows, K): a partial row tile, the 117M fused QKV, a 17-row tail
NTOKS = [1, 33, 129]
TYPES = [R.Q6_K, R.Q8_0]


@functools.lru_cache(maxsize=None)
def _case(t, rows, K):
    """The matrix, 129 activation rows, bias, residual, and the oracle's y = W q(x) per row with its
    bound -- computed once; the token counts read prefixes."""
    seed = 7 * rows + K + t
    raw = rand_matrix(t, rows, K, seed=seed)
    X = np.stack([rand_x(K, seed=seed * 1000 + i) for i in range(max(NTOKS))])
    X[5, :256] = 0.0   # an all-zero activation block (d = 0)
    rng = np.random.default_rng(seed)
    bias = rng.standard_normal(rows).astype(np.float32)
    resid = rng.standard_normal((max(NTOKS), rows)).astype(np.float32)
    ys, bs = zip(*(gemv_ref(t, raw, K, x) for x in X))
    out = raw, X, bias, resid, np.stack(ys), np.stack(bs)
    for a in out:
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("ntok", NTOKS)
@pytest.mark.parametrize("rows,K", SHAPES)
@pytest.mark.parametrize("t", TYPES, ids=lambda t: R.TYPE_NAME[t])
def test_bias_plain_and_residual(gpu_lib, t, rows, K, ntok):
    raw, X, bias, resid, y, bound = _case(t, rows, K)
    X, resid, y, bound = X[:ntok], resid[:ntok], y[:ntok], bound[:ntok]
    yb = (y.astype(np.float32) + bias).astype(np.float32)
    got, _, _ = engine.op_gemm_bias(t, raw, rows, K, X, bias=bias)
    lim = GEMM_TOL * (bound + np.abs(bias)) + 1e-6 * np.abs(yb) + 1e-30
    err = np.abs(got.astype(np.float64) - yb)
    assert np.all(err <= lim), ("store", float((err / lim).max()), np.argwhere(err > lim)[:5].tolist())
    ref = (yb + resid).astype(np.float32)
    got, _, _ = engine.op_gemm_bias(t, raw, rows, K, X, bias=bias, resid=resid, epilogue=engine.GEMM_BIAS_ADD)
    lim = GEMM_TOL * (bound + np.abs(bias)) + 1e-6 * (np.abs(yb) + np.abs(ref)) + 1e-30
    err = np.abs(got.astype(np.float64) - ref)
    assert np.all(err <= lim), ("add", float((err / lim).max()), np.argwhere(err > lim)[:5].tolist())
    # no bias: the plain store
    got, _, _ = engine.op_gemm_bias(t, raw, rows, K, X)
    err = np.abs(got.astype(np.float64) - y)
    assert np.all(err <= GEMM_TOL * bound + 1e-30)


@pytest.mark.parametrize("rows,K", [(40, 256), (81, 768)])
@pytest.mark.parametrize("t", TYPES, ids=lambda t: R.TYPE_NAME[t])
def test_bias_gelu(gpu_lib, t, rows, K):
    raw, X, _, _, y, bound = _case(t, rows, K)
    ntok = 33
    X, y, bound = X[:ntok], y[:ntok], bound[:ntok]
    bias = np.linspace(-8.0, 8.0, rows).astype(np.float32)   # pre-activations spanning |p| up to 8 and past
    p = (y.astype(np.float32) + bias).astype(np.float32)
    assert np.abs(p).max() >= 8.0 and np.abs(p).min() < 0.05
    bar = GEMM_TOL * (bound + np.abs(bias)) + 1e-6 * np.abs(p) + 1e-30
    got, _, _ = engine.op_gemm_bias(t, raw, rows, K, X, bias=bias, epilogue=engine.GEMM_BIAS_GELU)
    # the f16 values from the one below fp16(p - bar) to the one above fp16(p + bar), as index ranges
    # into the ascending list of the finite f16 values
    allh = np.arange(65536, dtype=np.uint16).view(np.float16)
    allh = np.sort(allh[np.isfinite(allh)])
    g = np.append(R.gelu(allh.astype(np.float32)).astype(np.float64), 0.0)   # (one past the end for reduceat)
    a32 = allh.astype(np.float32)
    lo = np.maximum(np.searchsorted(a32, (p - bar).astype(np.float16).astype(np.float32), "left") - 1, 0).reshape(-1)
    hi = np.minimum(np.searchsorted(a32, (p + bar).astype(np.float16).astype(np.float32), "right") + 1, allh.size).reshape(-1)
    assert np.all(hi > lo)
    idx = np.stack([lo, hi], axis=1).reshape(-1)
    gmin = np.minimum.reduceat(g, idx)[::2].reshape(p.shape)
    gmax = np.maximum.reduceat(g, idx)[::2].reshape(p.shape)
    # (past +-10 the epilogue returns 0 / the f32 value itself: between its f16 neighbours too)
    ok = (got >= gmin) & (got <= gmax)
    assert np.all(ok), (np.argwhere(~ok)[:5].tolist(), got[~ok][:5], gmin[~ok][:5], gmax[~ok][:5])


# ---- LayerNorm mode: the quantised activation ----
LN_NTOK = 33
# seeds on which the oracle's float32 and float64 evaluations give the same quants and the same
# arg-amax in every block (picked on the CPU with _ln_stable; the test checks it again)
LN_SEEDS = {(R.Q6_K, 256): 1, (R.Q6_K, 768): 1, (R.Q8_0, 256): 1, (R.Q8_0, 768): 1}


def _ln_inputs(K, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((LN_NTOK, K)).astype(np.float32)
    X[3] += 40.0                       # a large mean offset
    X[4] -= 100.0                      # a larger one
    X[7, K // 3] = 500.0               # a single outlier
    w = (1.0 + 0.3 * rng.standard_normal(K)).astype(np.float32)
    b = (0.2 * rng.standard_normal(K)).astype(np.float32)
    return X, w, b


def _ln32(x, w, b, eps):
    return ((R.layer_norm(x, eps) * w).astype(np.float32) + b).astype(np.float32)


def _ln64(x, w, b, eps):
    x = x.astype(np.float64)
    v = x - x.mean()
    return v / np.sqrt((v * v).mean() + eps) * w + b


def _quant(t, y):
    """(q [K] int, d per block f64, arg-amax per block) of quantize_row_q8_K / q8_0's rules on y
    (f32: the oracle's functions; f64: the same rules in float64)."""
    if y.dtype == np.float32:
        a = R.quantize_q8_0(y) if t == R.Q8_0 else R.quantize_q8_K(y)
        n = 32 if t == R.Q8_0 else 256
        return a.qs.reshape(-1).astype(np.int64), a.d.astype(np.float64), np.argmax(np.abs(y.reshape(-1, n)), axis=1)
    n = 32 if t == R.Q8_0 else 256
    yb = y.reshape(-1, n)
    am = np.argmax(np.abs(yb), axis=1)
    mx = yb[np.arange(yb.shape[0]), am]
    if t == R.Q8_0:
        amax = np.abs(mx)
        idv = np.where(amax != 0, 127.0 / np.where(amax != 0, amax, 1.0), 0.0)
        return np.rint(yb * idv[:, None]).astype(np.int64).reshape(-1), amax / 127.0, am
    isc = np.where(mx != 0, -127.0 / np.where(mx != 0, mx, 1.0), 0.0)
    q = np.minimum(127, np.rint(yb * isc[:, None])).astype(np.int64)
    return q.reshape(-1), np.where(mx != 0, 1.0 / np.where(isc != 0, isc, 1.0), 0.0), am


def _ln_stable(t, K, seed, eps=1e-5):
    X, w, b = _ln_inputs(K, seed)
    for x in X:
        q32, _, a32 = _quant(t, _ln32(x, w, b, eps))
        q64, _, a64 = _quant(t, _ln64(x, w, b, eps))
        if not (np.array_equal(q32, q64) and np.array_equal(a32, a64)):
            return False
    return True


@pytest.mark.parametrize("K", [256, 768])
@pytest.mark.parametrize("t", TYPES, ids=lambda t: R.TYPE_NAME[t])
def test_layernorm_quantised_activation(gpu_lib, t, K):
    eps = 1e-5
    seed = LN_SEEDS[(t, K)]
    assert _ln_stable(t, K, seed, eps), "the oracle's float32 and float64 evaluations differ on this seed"
    X, w, b = _ln_inputs(K, seed)
    raw = rand_matrix(t, 32, K, seed=3)
    _, q, d = engine.op_gemm_bias(t, raw, 32, K, X, norm_w=w, norm_b=b, eps=eps)
    for i, x in enumerate(X):
        rq, rd, _ = _quant(t, _ln32(x, w, b, eps))
        assert np.array_equal(q[i].astype(np.int64), rq), (i, np.argwhere(q[i] != rq)[:5].tolist())
        rd32 = rd.astype(np.float32)
        ulp = np.abs(d[i].view(np.int32).astype(np.int64) - rd32.view(np.int32).astype(np.int64))
        assert np.all(ulp <= 2), (i, int(ulp.max()))
