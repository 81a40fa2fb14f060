"""Op-level parity of the encoder kernels (enc.hip) through mi_op_gemm_f16 / mi_op_attention_enc.

GEMM bar (derived, no free tolerance).  The kernel rounds x to f16 as ggml does and adds exact f16
products in f32, so against the float64 dot of the f16-rounded operands an output is off by at most
K * 2^-24 * sum_k |w x| (K f32 additions, each within 2^-24 relative of a partial sum bounded by
sum |w x|), plus one f32 ulp of the result for each separate add of the epilogue (bias, residual).
GELU: the kernel looks fp16(pre-activation) up in ggml's table, so its result must lie between the
smallest and the largest table value over every f16 within the linear bar of the reference
pre-activation, widened by one f16 neighbour on each side.
Attention bar: the project's own (test_gpu_batch_ops.py): max err <= 2^-10 max|V|, mean <= 1e-5."""
import numpy as np
import pytest

import ggml_ref as R
from blama_amd import engine
from test_gpu_batch_ops import attn_batch_ref

pytestmark = pytest.mark.gpu

NONE, BIAS, GELU, RESID = 0, 1, 2, 3
GEMM_CASES = [
    (384, 384, 1, BIAS), (384, 384, 33, BIAS), (384, 384, 70, BIAS),
    (1536, 384, 70, GELU),
    (384, 1536, 33, RESID),
    (320, 128, 5, BIAS),
    (128, 320, 64, RESID),
    (96, 32, 3, NONE),
    (384, 384, 512, BIAS),
]


def _inputs(rows, K, ntok, seed):
    rng = np.random.default_rng(seed)
    w16 = (rng.standard_normal((rows, K)) / np.sqrt(K)).astype(np.float16)
    x = rng.standard_normal((ntok, K)).astype(np.float32)
    if ntok > 1:
        x[ntok // 2] = 0.0      # an all-zero activation row
    w16[rows // 3] = 0.0        # an all-zero weight row
    bias = (rng.standard_normal(rows) * 0.1).astype(np.float32)
    resid = rng.standard_normal((ntok, rows)).astype(np.float32)
    return w16, x, bias, resid


def _ulp32(a):
    a = np.abs(np.asarray(a, np.float64)).astype(np.float32)
    return (np.nextafter(a, np.float32(np.inf)) - a).astype(np.float64)


_F16 = None


def _f16_line():
    """Every finite f16 in ascending order and the GELU table's value at each."""
    global _F16
    if _F16 is None:
        v = np.arange(65536, dtype=np.uint16).view(np.float16)
        v = np.unique(v[np.isfinite(v)])                      # ascending, -0 / +0 merged
        g = R.gelu(v.astype(np.float32)).astype(np.float64)
        # sparse tables: lo[k][i] / hi[k][i] = min / max of g[i : i + 2^k]
        lo, hi = [g], [g]
        while 2 ** len(lo) <= g.size:
            s = 2 ** (len(lo) - 1)
            lo.append(np.minimum(lo[-1][:-s], lo[-1][s:]))
            hi.append(np.maximum(hi[-1][:-s], hi[-1][s:]))
        _F16 = (v.astype(np.float64), lo, hi)
    return _F16


def _gelu_range(lo, hi):
    """min and max of the table over every f16 in [lo, hi] widened by one f16 neighbour each side."""
    vals, tlo, thi = _f16_line()
    i0 = np.clip(np.searchsorted(vals, lo, "left") - 1, 0, vals.size - 1)    # the f16 below lo
    i1 = np.clip(np.searchsorted(vals, hi, "right"), 0, vals.size - 1)       # the f16 above hi
    i0 = np.maximum(i0 - 1, 0)
    i1 = np.minimum(i1 + 1, vals.size - 1)
    k = np.floor(np.log2(i1 - i0 + 1)).astype(np.int64)                      # two 2^k windows cover [i0, i1]
    mn = np.empty(lo.shape)
    mx = np.empty(lo.shape)
    for kk in np.unique(k):
        m = k == kk
        a, b = i0[m], i1[m] - 2 ** kk + 1
        mn[m] = np.minimum(tlo[kk][a], tlo[kk][b])
        mx[m] = np.maximum(thi[kk][a], thi[kk][b])
    return mn, mx


@pytest.mark.parametrize("rows,K,ntok,epi", GEMM_CASES, ids=[f"{c[0]}x{c[1]}-n{c[2]}-e{c[3]}" for c in GEMM_CASES])
def test_gemm_f16_matches_float64(gpu_lib, rows, K, ntok, epi):
    w16, x, bias, resid = _inputs(rows, K, ntok, seed=rows + 7 * K + 31 * ntok + epi)
    got = engine.op_gemm_f16(w16, x, bias if epi else None, resid if epi == RESID else None, epi).astype(np.float64)
    again = engine.op_gemm_f16(w16, x, bias if epi else None, resid if epi == RESID else None, epi)
    assert np.array_equal(got.astype(np.float32).view(np.uint32), again.view(np.uint32)), "two calls differ in bits"
    x16 = R.f32_to_f16(x).astype(np.float64)
    W = w16.astype(np.float64)
    dot = x16 @ W.T
    mag = np.abs(x16) @ np.abs(W).T
    bar = K * 2.0 ** -24 * mag
    ref = dot
    if epi != NONE:
        ref = ref + bias.astype(np.float64)
        bar = bar + _ulp32(ref)
    if epi == RESID:
        ref = ref + resid.astype(np.float64)
        bar = bar + _ulp32(ref)
    if epi == GELU:
        mn, mx = _gelu_range(ref - bar, ref + bar)
        bad = np.argwhere((got < mn) | (got > mx))
        print(f"gelu {rows}x{K} n{ntok}: {bad.shape[0]} outside the table range; widest range {float((mx - mn).max()):.3g}")
        assert bad.size == 0, (bad[:5].tolist(), got[tuple(bad[0])], mn[tuple(bad[0])], mx[tuple(bad[0])])
        return
    err = np.abs(got - ref)
    print(f"gemm {rows}x{K} n{ntok} e{epi}: worst err / bar {float((err / np.maximum(bar, 1e-300)).max()):.3g}")
    bad = np.argwhere(err > bar)
    assert bad.size == 0, (len(bad), bad[:5].tolist(), float((err / np.maximum(bar, 1e-300)).max()))
    assert ntok == 1 or np.all(got[ntok // 2] == ((bias if epi else 0) + (resid[ntok // 2] if epi == RESID else 0))), "zero activation row"


ATTN_CASES = [(12, 32, 1), (12, 32, 33), (12, 32, 70), (12, 32, 512), (2, 64, 5), (2, 64, 128)]


@pytest.mark.parametrize("n_head,hd,ntok", ATTN_CASES, ids=[f"h{c[0]}-hd{c[1]}-n{c[2]}" for c in ATTN_CASES])
def test_attention_enc_matches_oracle(gpu_lib, n_head, hd, ntok):
    rng = np.random.default_rng(ntok + hd + n_head)
    q = (rng.standard_normal((ntok, n_head, hd)) * 0.6).astype(np.float32)
    k16 = (rng.standard_normal((ntok, n_head * hd)) * 0.6).astype(np.float16)
    v16 = rng.standard_normal((ntok, n_head * hd)).astype(np.float16)
    got = engine.op_attention_enc(q, k16, v16)
    again = engine.op_attention_enc(q, k16, v16)
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32)), "two calls differ in bits"
    # every cell visible to every token: each token sits in the last cell at the last position
    last = np.full(ntok, ntok - 1, np.int32)
    ref = attn_batch_ref(q, k16, v16, n_head, last, last, np.arange(ntok, dtype=np.int32))
    err = np.abs(got - ref)
    print(f"attention h{n_head} hd{hd} n{ntok}: max err {float(err.max()):.3g}, mean {float(err.mean()):.3g}")
    assert err.max() <= 2.0 ** -10 * np.abs(v16.astype(np.float32)).max(), float(err.max())
    assert err.mean() <= 1e-5, float(err.mean())
