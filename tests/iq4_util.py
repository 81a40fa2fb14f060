"""Helpers of the IQ4_NL / IQ4_XS tests.

An IQ4_NL block is exactly a Q8_0 block with the same d and qs[i] = kv[nibble]
(vec_dot_iq4_nl_q8_0 and vec_dot_q8_0_q8_0 form the same int32 sum times the same d_x * d_y), so
every IQ4_NL reference is the existing oracle on the Q8_0 re-encoding, as legacy_quant_util's.
IQ4_XS has no such twin among the oracle's types (its scaled weight reaches +-4064), so its dot is
restated here in the shape of ggml_ref.block_sums: per superblock coef = f32(d * d8) and the exact
integer S = sum_ib (ls_ib - 32) sum_j kv a over ggml_ref.quantize_q8_K(x)."""
import numpy as np

import gemm_ref_util
import ggml_ref as R
from blama_amd import gguf, synthetic
from legacy_quant_util import _add_kv
from lora_util import LoraOracle, _mat_vec
from util import oracle_from_gguf

IQ4_NL, IQ4_XS = 20, 23
KV = synthetic.IQ4_KV
BLOCK = {IQ4_NL: (32, 18), IQ4_XS: (256, 136)}


def unpack(raw, t):
    """IQ4_NL: (kv (n, 32), d f32 (n,)); IQ4_XS: (kv (n, 256), ls (n, 8) in 0..63, d f32 (n,)).  Per 32
    weights, byte j of qs holds the index of weight j (low nibble) and of weight j + 16 (high)."""
    b = np.ascontiguousarray(raw, np.uint8).reshape(-1, BLOCK[t][1])
    d = b[:, 0:2].copy().view(np.float16).reshape(-1).astype(np.float32)
    qs = (b[:, 2:] if t == IQ4_NL else b[:, 8:]).reshape(b.shape[0], -1, 16)
    kv = KV[np.concatenate([qs & 0xF, qs >> 4], axis=2)].reshape(b.shape[0], -1)
    if t == IQ4_NL:
        return kv, d
    sh = b[:, 2:4].copy().view("<u2").reshape(-1).astype(np.int32)
    sl = b[:, 4:8].astype(np.int32)
    ls = np.stack([((sl[:, ib // 2] >> (4 * (ib % 2))) & 0xF) | (((sh >> (2 * ib)) & 3) << 4) for ib in range(8)], 1)
    return kv, ls, d


def dequantize(raw, t):
    """dequantize_row_iq4_nl / _iq4_xs in f32: d * kv, (d * (ls - 32)) * kv."""
    if t == IQ4_NL:
        kv, d = unpack(raw, t)
        return (d[:, None] * kv.astype(np.float32)).astype(np.float32).reshape(-1)
    kv, ls, d = unpack(raw, t)
    dl = (d[:, None] * (ls - 32).astype(np.float32)).astype(np.float32)
    return (np.repeat(dl, 32, axis=1) * kv.astype(np.float32)).astype(np.float32).reshape(-1)


def to_q8_0(raw) -> np.ndarray:
    """The Q8_0 blocks (f16 d, int8 qs[32]) with an IQ4_NL matrix's d and qs[i] = kv[nibble]."""
    b = np.ascontiguousarray(raw, np.uint8).reshape(-1, 18)
    out = np.empty((b.shape[0], 34), np.uint8)
    out[:, 0:2] = b[:, 0:2]
    out[:, 2:] = unpack(raw, IQ4_NL)[0].astype(np.int8).view(np.uint8)
    return out.reshape(-1)


def block_sums_xs(raw, K, x):
    """[(coef, isum)] of an IQ4_XS matrix over one activation: vec_dot_iq4_xs_q8_K per superblock."""
    nb = K // 256
    kv, ls, d = unpack(raw, IQ4_XS)
    a = R.quantize_q8_K(x)
    dots = (kv.reshape(-1, nb, 8, 32).astype(np.int64) * a.qs.reshape(1, nb, 8, 32)).sum(-1)
    S = (dots * (ls.reshape(-1, nb, 8) - 32)).sum(-1)
    return [((d.reshape(-1, nb) * a.d[None]).astype(np.float32), S)]


def gemv_ref(t, raw, K, x):
    """(y f64 of the f32 result, sum_b |term_b|): gemm_ref_util.gemv_ref for the two types."""
    if t == IQ4_NL:
        q8 = to_q8_0(raw)
        return R.mul_mat_vec(q8, R.Q8_0, K, x).astype(np.float64), R.mul_mat_vec_abs(q8, R.Q8_0, K, x)
    (coef, S), = block_sums_xs(raw, K, x)
    terms = coef.astype(np.float64) * S
    return terms.sum(-1).astype(np.float32).astype(np.float64), np.abs(terms).sum(-1)


def gemm_ref(t, raw, rows, K, X):
    """(y[T, rows] f64, bound[T, rows]) as gemm_ref_util.gemm_ref, token by token."""
    if t == IQ4_NL:
        return gemm_ref_util.gemm_ref(R.Q8_0, to_q8_0(raw), rows, K, X)
    T = np.stack([c.astype(np.float64) * s for c, s in (block_sums_xs(raw, K, x)[0] for x in X)])
    return T.sum(-1), np.abs(T).sum(-1)


class Iq4Oracle(LoraOracle):
    """The oracle for a model with IQ4_XS tensors (with adapters and a control vector when set, as
    LoraOracle): `xs` holds their raw blocks by name; a matrix among them multiplies through
    block_sums_xs, and the token table is read from its exact f32 dequantisation."""
    xs: dict = {}

    def _mm(self, name, x):
        raw = self.xs.get(name)
        if raw is None:
            return super()._mm(name, x)
        y = gemv_ref(IQ4_XS, raw, self.tensors[name].shape[0], np.asarray(x, np.float32).reshape(-1))[0].astype(np.float32)
        for ad, scale in self.loras:   # LoraOracle._mm's term on this base
            if name in ad.pairs:
                A, B = ad.pairs[name]
                s = scale if ad.alpha == 0.0 else scale * ad.alpha / A.shape[0]
                y = (y + (_mat_vec(B, _mat_vec(A, x)) * np.float32(s)).astype(np.float32)).astype(np.float32)
        return y


def iq4_oracle(image, n_ctx, loras=(), vec=None):
    """The oracle of an IQ4 image: IQ4_NL tensors re-encoded as Q8_0; IQ4_XS matrices through
    Iq4Oracle._mm, an IQ4_XS token table as the F32 tensor of its dequantised values."""
    rd = gguf.GGUFReader(image)
    w = gguf.GGUFWriter()
    for k, v in rd.kv.items():
        if k != "general.alignment":
            _add_kv(w, k, v)
    xs = {}
    for name, t in rd.tensors.items():
        data = np.asarray(t.data)
        if t.type == IQ4_NL:
            w.add_tensor(name, R.Q8_0, t.shape, to_q8_0(data))
        elif t.type == IQ4_XS:
            xs[name] = data
            w.add_tensor(name, R.F32, t.shape, dequantize(data, IQ4_XS).view(np.uint8))
        else:
            w.add_tensor(name, t.type, t.shape, data)
    o = oracle_from_gguf(w.to_bytes(), n_ctx=n_ctx)
    c = Iq4Oracle(o.hp, o.tensors, n_ctx=n_ctx)
    c.xs, c.loras, c.vec = xs, list(loras), dict(vec or {})
    return c


def rand_matrix(t, rows, K, seed=0):
    buf = np.empty(K // BLOCK[t][0] * BLOCK[t][1] * rows, np.uint8)
    synthetic.fill_quant(buf, t, np.random.default_rng(seed))
    return buf


def extreme_matrix(t, rows, K, seed=0):
    """Every codebook index 0 or 15 (-127 / +113), every IQ4_XS scale -32 or +31, each sub-block
    mostly of one end with a few weights of the other: w = (ls - 32) kv reaches 31 x -127 = -3937 and -32 x -127 = +4064."""
    rng = np.random.default_rng(seed)
    n = rows * K // 32
    idx = np.where(rng.integers(0, 2, (n, 1)).astype(bool) ^ (rng.random((n, 32)) < 0.1), 0, 15)
    if t == IQ4_NL:
        return synthetic.pack_iq4_nl(idx, rng.uniform(0.0002, 0.0004, n).astype(np.float16)).reshape(-1)
    ls = np.where(rng.integers(0, 2, (n // 8, 8)).astype(bool), 0, 63)
    return synthetic.pack_iq4_xs(idx.reshape(n // 8, 256), ls, rng.uniform(0.0001, 0.0002, n // 8).astype(np.float16)).reshape(-1)
