"""Op-level parity of the kernels the jina-bert-v2 graph adds: the ALiBi variants of the three encoder attention
kernels and enc_attn_xlong_kernel (past 2048 tokens) through mi_op_attention_enc_alibi, the GELU-gated pair
launch through mi_op_gemm_f16_geglu.

Attention: every sequence against attn_alibi_ref (float64, q rounded to f16) on its own rows at the project's
attention bar as test_gpu_enc_seqs_ops.py states it: max err <= 2^-10 max|V of the sequence|, mean <= 1e-5
max(1, max|V|).  The bar holds whether or not a compiler contracts score * scale + slope * mask: that moves a
score by one f32 ulp, 2^-24 relative at |s| < 1000 here, against p's f16 rounding of 2^-11.
The reference does not round p to f16.  A peaked softmax over a few keys rounded that way alone misses the mean
bar (33 tokens x 3 heads: 3.67e-5 against 3.2e-5), so the ALiBi variants of the short kernels carry the rounding's
residual through PV; past 512 tokens p is f16 as the issue states it and the mean sits at half the bar.
GEGLU: against float64 gelu_table(g) u.  g and u lie within their derived GEMM bars bg, bu (K 2^-24 sum|w x|,
test_gpu_bert_ops.py).  The device rounds its g to f16 and reads the table there: its g is within bg of the
true one and each rounding moves at most half an f16 ulp, so the two table arguments differ by at most bg +
ulp16(g); |gelu'| <= 1.13, and both table entries are themselves rounded to f16 (half an ulp each), so the
gate term differs by at most tg = 1.13 (bg + ulp16(g)) + ulp16(gelu).  Bar: tg (|u| + bu) + |gelu(g)| bu, plus
2 x 2^-24 |ref| for the product."""
import numpy as np
import pytest

import ggml_ref as R
from blama_amd import engine
from jina_ref_util import alibi_slopes, attn_alibi_ref

gpu = pytest.mark.gpu      # (the slope-telling test below needs no GPU)

CASES = [(3, 32, (1,)), (3, 32, (33,)), (2, 64, (70, 7, 512)), (3, 64, (513,)), (2, 32, (1100, 33)), (3, 32, (2049,)),
         (2, 64, (2100, 600, 5)), (2, 64, (8192,))]


def _inputs(n_head, hd, lens, seed):
    rng = np.random.default_rng(seed)
    ntok = sum(lens)
    q = (rng.standard_normal((ntok, n_head, hd)) * 0.6).astype(np.float32)
    k16 = (rng.standard_normal((ntok, n_head * hd)) * 0.6).astype(np.float16)
    v16 = rng.standard_normal((ntok, n_head * hd)).astype(np.float16)
    for i, (a, n) in enumerate(zip(np.cumsum((0,) + lens), lens)):
        v16[a:a + n] *= np.float16((1.0, 64.0, 1.0 / 64.0)[i % 3])
    return q, k16, v16


def _within_bar(err, v16):
    vmax = float(np.abs(v16.astype(np.float32)).max())
    return err.max() <= 2.0 ** -10 * vmax and err.mean() <= 1e-5 * max(1.0, vmax)


@gpu
@pytest.mark.parametrize("n_head,hd,lens", CASES, ids=[f"h{c[0]}-hd{c[1]}-" + "_".join(map(str, c[2])) for c in CASES])
def test_alibi_attention_matches_float64(gpu_lib, n_head, hd, lens):
    q, k16, v16 = _inputs(n_head, hd, lens, seed=sum(lens) + hd)
    got = engine.op_attention_enc_alibi(q, k16, v16, lens, 8.0)
    slopes = alibi_slopes(n_head)
    for a, n in zip(np.cumsum((0,) + lens), lens):
        s = slice(a, a + n)
        # 8192 tokens: the first, the last and two groups of 32 queries that straddle a tile and a workgroup edge
        rows = np.concatenate([np.arange(r, r + 32) for r in (0, 2032, 4208, 8160)]) if n == 8192 else np.arange(n)
        err = np.abs(got[s][rows] - attn_alibi_ref(q[s], k16[s], v16[s], slopes, rows))
        print(f"h{n_head} hd{hd} seq at {a} len {n}: max err {float(err.max()):.3g}, mean {float(err.mean()):.3g}")
        assert _within_bar(err, v16[s]), (a, n, float(err.max()), float(err.mean()))


def test_references_tell_the_slopes_apart():
    """CPU only: at 33 tokens a reference without bias, and one with m0^(h + 1) for head 2, each miss the bar there."""
    q, k16, v16 = _inputs(3, 32, (33,), seed=65)
    slopes = alibi_slopes(3)
    assert slopes.tolist() == [2.0 ** -4, 2.0 ** -8, 2.0 ** -2]
    ref = attn_alibi_ref(q, k16, v16, slopes)
    for wrong in (np.zeros(3), np.float32(2.0 ** -4) ** np.arange(1, 4)):
        assert not _within_bar(np.abs(attn_alibi_ref(q, k16, v16, wrong) - ref)[:, 2], v16)


@gpu
def test_max_bias_zero_is_the_plain_kernel(gpu_lib):
    q, k16, v16 = _inputs(2, 64, (70, 600), seed=1)
    a, b = engine.op_attention_enc_alibi(q, k16, v16, (70, 600), 0.0), engine.op_attention_enc_seqs(q, k16, v16, (70, 600))
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


@gpu
@pytest.mark.parametrize("n_head,hd", [(2, 32), (2, 64)])
def test_xlong_batch_invariance(gpu_lib, n_head, hd):
    """A 2100-token sequence alone, between a short and a long neighbour, and among sequences that hold only NaN."""
    lens = (33, 2100, 600)
    q, k16, v16 = _inputs(n_head, hd, lens, seed=hd)
    s = slice(33, 2133)
    alone = engine.op_attention_enc_alibi(q[s], k16[s], v16[s], (2100,))
    between = engine.op_attention_enc_alibi(q, k16, v16, lens)[s]
    nq, nk, nv = np.full_like(q, np.nan), np.full_like(k16, np.nan), np.full_like(v16, np.nan)
    nq[s], nk[s], nv[s] = q[s], k16[s], v16[s]
    among_nan = engine.op_attention_enc_alibi(nq, nk, nv, lens)[s]
    assert np.isfinite(alone).all()
    for other in (between, among_nan):
        assert np.array_equal(alone.view(np.uint32), other.view(np.uint32))


def _ulp16(a):
    a = np.abs(np.asarray(a, np.float64)).astype(np.float16)
    return (np.nextafter(a, np.float16(np.inf)) - a).astype(np.float64)


@gpu
@pytest.mark.parametrize("rows,K,ntok", [(320, 128, 33), (2048, 512, 70)])
def test_gemm_f16_geglu_matches_float64(gpu_lib, rows, K, ntok):
    rng = np.random.default_rng(rows + 7 * K + ntok)
    g16, u16 = ((rng.standard_normal((rows, K)) * a / np.sqrt(K)).astype(np.float16) for a in (2.0, 1.0))
    x = rng.standard_normal((ntok, K)).astype(np.float32)
    got = engine.op_gemm_f16_geglu(g16, u16, x).astype(np.float64)
    x16 = R.f32_to_f16(x).astype(np.float64)
    g, u = x16 @ g16.astype(np.float64).T, x16 @ u16.astype(np.float64).T
    bg, bu = (K * 2.0 ** -24 * (np.abs(x16) @ np.abs(w.astype(np.float64)).T) for w in (g16, u16))
    gl = R.gelu(g).astype(np.float64)
    ref = gl * u
    tg = 1.13 * (bg + _ulp16(g)) + _ulp16(gl)
    bar = tg * (np.abs(u) + bu) + np.abs(gl) * bu + 2 * 2.0 ** -24 * np.abs(ref)
    err = np.abs(got - ref)
    print(f"geglu {rows}x{K} n{ntok}: worst err / bar {float((err / bar).max()):.3g}")
    assert np.all(err <= bar), (np.argwhere(err > bar)[:5].tolist(), float((err / bar).max()))
    assert not np.all(np.abs(got - g / (1.0 + np.exp(-g)) * u) <= bar)      # a silu gate sits outside the bar
