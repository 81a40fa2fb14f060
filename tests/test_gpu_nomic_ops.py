"""Op-level parity of the kernels of enc_nomic.hip: the long-sequence attention through
mi_op_attention_enc_seqs / mi_op_attention_enc, the fused Q|K|V launch with the NEOX rotation through
mi_op_gemm_f16_rope, the gate/up pair launch through mi_op_gemm_f16_swiglu.

Attention: every sequence against attn_batch_ref on its own rows, at the project's attention bar as
test_gpu_enc_seqs_ops.py states it (max err <= 2^-10 max|V of the sequence|, mean <= 1e-5 max(1,
max|V|)), each sequence's V scaled by another power of two.
RoPE GEMM: against the float64 GEMM of the f16-rounded activation, rotated with ggml_rope_cache_init's
table.  Bar of a rotated element: the derived GEMM bars (test_gpu_bert_ops.py: K 2^-24 sum|w x|) of both
partners through |cos| and |sin|, plus test_gpu_rope.py's TRIG_TOL (|y0| + |y1|) for the device's cosf /
sinf and the two products, plus one f32 ulp for the add; K and V, stored as f16, one f16 ulp more.
SwiGLU: against float64 silu(g) u.  With g, u within their GEMM bars bg, bu and |silu'| <= 1.1:
1.1 bg (|u| + bu) + |silu(g)| bu, plus 8 x 2^-24 |ref| for expf (2 ulp), the add, the division and
the product of the epilogue."""
import numpy as np
import pytest

import ggml_ref as R
from blama_amd import engine
from nomic_ref_util import rope_neox
from test_gpu_batch_ops import attn_batch_ref
from test_gpu_rope import TRIG_TOL

pytestmark = pytest.mark.gpu

V_SCALES = (1.0, 64.0, 1.0 / 64.0, 4096.0)
LONG_CASES = [(2, 64, (513,)), (2, 32, (545,)), (2, 64, (2048,)), (2, 32, (7, 600, 33, 1030))]


def _attn_inputs(n_head, hd, lens, seed):
    rng = np.random.default_rng(seed)
    ntok = sum(lens)
    q = (rng.standard_normal((ntok, n_head, hd)) * 0.6).astype(np.float32)
    k16 = (rng.standard_normal((ntok, n_head * hd)) * 0.6).astype(np.float16)
    v16 = rng.standard_normal((ntok, n_head * hd)).astype(np.float16)
    for i, (a, n) in enumerate(zip(np.cumsum((0,) + lens), lens)):
        v16[a:a + n] *= np.float16(V_SCALES[i % len(V_SCALES)])
    return q, k16, v16


def _check_attn(got, q, k16, v16, n_head, what):
    n = q.shape[0]
    last = np.full(n, n - 1, np.int32)      # every cell visible to every token
    err = np.abs(got - attn_batch_ref(q, k16, v16, n_head, last, last, np.arange(n, dtype=np.int32)))
    vmax = float(np.abs(v16.astype(np.float32)).max())
    print(f"{what} len {n}: max err / max|V| {float(err.max()) / vmax:.3g}, mean {float(err.mean()):.3g}")
    assert err.max() <= 2.0 ** -10 * vmax, (what, n, float(err.max()), vmax)
    assert err.mean() <= 1e-5 * max(1.0, vmax), (what, n, float(err.mean()))


@pytest.mark.parametrize("n_head,hd,lens", LONG_CASES, ids=[f"h{c[0]}-hd{c[1]}-" + "_".join(map(str, c[2])) for c in LONG_CASES])
def test_long_attention_matches_oracle(gpu_lib, n_head, hd, lens):
    q, k16, v16 = _attn_inputs(n_head, hd, lens, seed=sum(lens) + hd)
    got = engine.op_attention_enc_seqs(q, k16, v16, lens)
    for a, n in zip(np.cumsum((0,) + lens), lens):
        s = slice(a, a + n)
        _check_attn(got[s], q[s], k16[s], v16[s], n_head, f"h{n_head} hd{hd} seq at {a}")


@pytest.mark.parametrize("n_head,hd", [(2, 32), (2, 64)])
def test_long_batch_invariance(gpu_lib, n_head, hd):
    """A 600-token sequence alone, between a short and a long neighbour, and among sequences that hold
    only NaN; and two calls."""
    lens = (33, 600, 1030)
    q, k16, v16 = _attn_inputs(n_head, hd, lens, seed=hd)
    s = slice(33, 633)
    alone = engine.op_attention_enc_seqs(q[s], k16[s], v16[s], (600,))
    again = engine.op_attention_enc_seqs(q[s], k16[s], v16[s], (600,))
    between = engine.op_attention_enc_seqs(q, k16, v16, lens)[s]
    nq, nk, nv = np.full_like(q, np.nan), np.full_like(k16, np.nan), np.full_like(v16, np.nan)
    nq[s], nk[s], nv[s] = q[s], k16[s], v16[s]
    among_nan = engine.op_attention_enc_seqs(nq, nk, nv, lens)[s]
    assert np.isfinite(alone).all()
    for other in (again, between, among_nan):
        assert np.array_equal(alone.view(np.uint32), other.view(np.uint32))


@pytest.mark.parametrize("n_head,hd,ntok", [(2, 64, 513), (2, 32, 1025)])
def test_attention_enc_past_512(gpu_lib, n_head, hd, ntok):
    q, k16, v16 = _attn_inputs(n_head, hd, (ntok,), seed=ntok)
    _check_attn(engine.op_attention_enc(q, k16, v16), q, k16, v16, n_head, f"h{n_head} hd{hd} one call")


def _ulp32(a):
    a = np.abs(np.asarray(a, np.float64)).astype(np.float32)
    return (np.nextafter(a, np.float32(np.inf)) - a).astype(np.float64)


def _ulp16(a):
    a = np.abs(np.asarray(a, np.float64)).astype(np.float16)
    return (np.nextafter(a, np.float16(np.inf)) - a).astype(np.float64)


@pytest.mark.parametrize("n_head,hd,n_rot", [(2, 64, 64), (3, 32, 32), (2, 64, 32)])
def test_gemm_f16_rope_matches_float64(gpu_lib, n_head, hd, n_rot):
    ne, ntok, base = n_head * hd, 33, 1000.0
    K, half = ne, n_rot // 2
    rng = np.random.default_rng(ne + n_rot)
    w16 = (rng.standard_normal((3 * ne, K)) / np.sqrt(K)).astype(np.float16)
    x = rng.standard_normal((ntok, K)).astype(np.float32)
    pos = rng.permutation(np.r_[2047, 0, 1, rng.integers(2, 2047, ntok - 3)]).astype(np.int32)
    q, k16, v16 = engine.op_gemm_f16_rope(w16, x, pos, n_head, hd, n_rot, freq_base=base)
    got = np.concatenate([q, k16.astype(np.float32), v16.astype(np.float32)], axis=1).astype(np.float64)

    x16, W = R.f32_to_f16(x).astype(np.float64), w16.astype(np.float64)
    y = (x16 @ W.T).reshape(ntok, 3 * n_head, hd)                     # heads of Q, of K, of V
    by = (K * 2.0 ** -24 * (np.abs(x16) @ np.abs(W).T)).reshape(y.shape)
    cs = np.stack([np.stack(R.rope_cache(int(p), n_rot, base)) for p in pos]).astype(np.float64)   # (ntok, 2, half)
    c, s = cs[:, None, 0], cs[:, None, 1]
    ref, bar = y.copy(), by.copy()
    rot = slice(0, 2 * n_head)                                        # Q and K heads
    y0, y1, b0, b1 = y[:, rot, :half], y[:, rot, half:n_rot], by[:, rot, :half], by[:, rot, half:n_rot]
    ref[:, rot, :half], ref[:, rot, half:n_rot] = y0 * c - y1 * s, y0 * s + y1 * c
    trig = TRIG_TOL * (np.abs(y0) + np.abs(y1))
    bar[:, rot, :half] = b0 * np.abs(c) + b1 * np.abs(s) + trig
    bar[:, rot, half:n_rot] = b0 * np.abs(s) + b1 * np.abs(c) + trig
    bar[:, rot, :n_rot] += _ulp32(ref[:, rot, :n_rot])
    bar[:, n_head:] += _ulp16(ref[:, n_head:])                        # K and V are stored as f16
    ref, bar = ref.reshape(ntok, -1), bar.reshape(ntok, -1)
    err = np.abs(got - ref)
    print(f"rope gemm h{n_head} hd{hd} n_rot{n_rot}: worst err / bar {float((err / bar).max()):.3g}")
    assert np.all(err <= bar), (np.argwhere(err > bar)[:5].tolist(), float((err / bar).max()))
    # the inputs tell the mistakes apart: a NORM pairing, a swapped sign and an unrotated K each sit many bars away
    y32 = y.astype(np.float32)
    norm_paired = np.stack([R.rope_norm(y32[t, rot], int(pos[t]), n_rot, base) for t in range(ntok)])
    swapped = rope_neox(y32[:, rot].reshape(ntok, -1), -pos.astype(np.int64), 2 * n_head, n_rot, base).reshape(ntok, 2 * n_head, hd)
    for wrong in (norm_paired, swapped, y32[:, rot]):
        off = np.abs(wrong - ref.reshape(y.shape)[:, rot])[pos > 1][..., :n_rot] / bar.reshape(y.shape)[:, rot][pos > 1][..., :n_rot]
        assert np.median(off[:, n_head:]) > 100 and np.median(off[:, :n_head]) > 100


@pytest.mark.parametrize("rows,K,ntok", [(320, 128, 33), (1536, 384, 70), (320, 384, 70)])
def test_gemm_f16_swiglu_matches_float64(gpu_lib, rows, K, ntok):
    rng = np.random.default_rng(rows + 7 * K + ntok)
    g16, u16 = ((rng.standard_normal((rows, K)) * a / np.sqrt(K)).astype(np.float16) for a in (2.0, 1.0))
    x = rng.standard_normal((ntok, K)).astype(np.float32)
    got = engine.op_gemm_f16_swiglu(g16, u16, x).astype(np.float64)
    x16 = R.f32_to_f16(x).astype(np.float64)
    g, u = x16 @ g16.astype(np.float64).T, x16 @ u16.astype(np.float64).T
    bg, bu = (K * 2.0 ** -24 * (np.abs(x16) @ np.abs(w.astype(np.float64)).T) for w in (g16, u16))
    sg = g / (1.0 + np.exp(-g))
    ref = sg * u
    bar = 1.1 * bg * (np.abs(u) + bu) + np.abs(sg) * bu + 8 * 2.0 ** -24 * np.abs(ref)
    err = np.abs(got - ref)
    print(f"swiglu {rows}x{K} n{ntok}: worst err / bar {float((err / bar).max()):.3g}")
    assert np.all(err <= bar), (np.argwhere(err > bar)[:5].tolist(), float((err / bar).max()))
