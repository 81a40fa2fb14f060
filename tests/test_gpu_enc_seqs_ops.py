"""Op-level parity of the segmented encoder attention (enc_seq.hip) through mi_op_attention_enc_seqs,
and the encoder GEMM past 512 token rows.

Attention: every sequence against attn_batch_ref on its own rows alone, at the project's attention
bar taken per sequence (max err <= 2^-10 max|V of the sequence|, mean <= 1e-5 max(1, max|V|)).  Each
sequence's V is scaled by another power of two, so a key leaked across a boundary cannot hide.
GEMM: the derived bar of test_gpu_bert_ops.py (K * 2^-24 * sum|w x| plus an f32 ulp per epilogue add)."""
import numpy as np
import pytest

import ggml_ref as R
from blama_amd import engine
from test_gpu_batch_ops import attn_batch_ref

pytestmark = pytest.mark.gpu

CASES = [(12, 32, (1,)), (12, 32, (33, 1, 31, 64)), (2, 64, (65, 5, 32)), (12, 32, (512,)), (2, 64, (7, 512))]
V_SCALES = (1.0, 64.0, 1.0 / 64.0, 4096.0, 1.0 / 4096.0)


def _inputs(n_head, hd, lens, seed):
    rng = np.random.default_rng(seed)
    ntok = sum(lens)
    q = (rng.standard_normal((ntok, n_head, hd)) * 0.6).astype(np.float32)
    k16 = (rng.standard_normal((ntok, n_head * hd)) * 0.6).astype(np.float16)
    v16 = rng.standard_normal((ntok, n_head * hd)).astype(np.float16)
    for i, (a, n) in enumerate(zip(np.cumsum((0,) + lens), lens)):
        v16[a:a + n] *= np.float16(V_SCALES[i % len(V_SCALES)])
    return q, k16, v16


def _ref(q, k16, v16, n_head):
    n = q.shape[0]
    last = np.full(n, n - 1, np.int32)      # every cell visible to every token, as test_gpu_bert_ops.py
    return attn_batch_ref(q, k16, v16, n_head, last, last, np.arange(n, dtype=np.int32))


@pytest.mark.parametrize("n_head,hd,lens", CASES, ids=[f"h{c[0]}-hd{c[1]}-" + "_".join(map(str, c[2])) for c in CASES])
def test_attention_enc_seqs_matches_oracle(gpu_lib, n_head, hd, lens):
    q, k16, v16 = _inputs(n_head, hd, lens, seed=sum(lens) + hd + n_head)
    got = engine.op_attention_enc_seqs(q, k16, v16, lens)
    again = engine.op_attention_enc_seqs(q, k16, v16, lens)
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32)), "two calls differ in bits"
    for a, n in zip(np.cumsum((0,) + lens), lens):
        s = slice(a, a + n)
        err = np.abs(got[s] - _ref(q[s], k16[s], v16[s], n_head))
        vmax = float(np.abs(v16[s].astype(np.float32)).max())
        print(f"h{n_head} hd{hd} seq at {a} len {n}: max err / max|V| {float(err.max()) / vmax:.3g}, mean {float(err.mean()):.3g}")
        assert err.max() <= 2.0 ** -10 * vmax, (a, n, float(err.max()), vmax)
        assert err.mean() <= 1e-5 * max(1.0, vmax), (a, n, float(err.mean()))


@pytest.mark.parametrize("n_head,hd", [(12, 32), (2, 64)])
def test_batch_invariance(gpu_lib, n_head, hd):
    """A 33-token sequence alone, as the third of four, and among sequences that hold only NaN."""
    lens = (64, 5, 33, 1)
    q, k16, v16 = _inputs(n_head, hd, lens, seed=hd)
    s = slice(69, 102)
    alone = engine.op_attention_enc_seqs(q[s], k16[s], v16[s], (33,))
    third = engine.op_attention_enc_seqs(q, k16, v16, lens)[s]
    nq, nk, nv = np.full_like(q, np.nan), np.full_like(k16, np.nan), np.full_like(v16, np.nan)
    nq[s], nk[s], nv[s] = q[s], k16[s], v16[s]
    among_nan = engine.op_attention_enc_seqs(nq, nk, nv, lens)[s]
    assert np.isfinite(alone).all()
    assert np.array_equal(alone.view(np.uint32), third.view(np.uint32))
    assert np.array_equal(alone.view(np.uint32), among_nan.view(np.uint32))


@pytest.mark.parametrize("rows,K,ntok,epi", [(384, 384, 545, 1), (384, 1536, 1000, 3)])
def test_gemm_f16_past_512_rows(gpu_lib, rows, K, ntok, epi):
    rng = np.random.default_rng(rows + 7 * K + 31 * ntok + epi)
    w16 = (rng.standard_normal((rows, K)) / np.sqrt(K)).astype(np.float16)
    x = rng.standard_normal((ntok, K)).astype(np.float32)
    bias = (rng.standard_normal(rows) * 0.1).astype(np.float32)
    resid = rng.standard_normal((ntok, rows)).astype(np.float32)
    got = engine.op_gemm_f16(w16, x, bias, resid if epi == 3 else None, epi).astype(np.float64)
    x16, W = R.f32_to_f16(x).astype(np.float64), w16.astype(np.float64)

    def ulp32(a):
        a = np.abs(a).astype(np.float32)
        return (np.nextafter(a, np.float32(np.inf)) - a).astype(np.float64)

    ref = x16 @ W.T + bias.astype(np.float64)
    bar = K * 2.0 ** -24 * (np.abs(x16) @ np.abs(W).T) + ulp32(ref)
    if epi == 3:
        ref = ref + resid.astype(np.float64)
        bar = bar + ulp32(ref)
    err = np.abs(got - ref)
    print(f"gemm {rows}x{K} n{ntok} e{epi}: worst err / bar {float((err / bar).max()):.3g}")
    assert np.all(err <= bar), float((err / bar).max())
