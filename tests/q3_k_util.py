"""Helpers of the Q3_K tests.  A Q3_K block is exactly a Q6_K block: the same d, scales[s] =
sc6(s) - 32, 6-bit value q + 32, the same element order and 16-element scale groups (ggml's
dequantize_row_q3_K / _q6_K both evaluate (d * sc) * q, and vec_dot_q3_K_q8_K / _q6_K_q8_K share
their integer arithmetic), so the reference of every test is the existing oracle run on the Q6_K
re-encoding this file produces."""
import numpy as np

import ggml_ref as R
from blama_amd import gguf, synthetic
from legacy_quant_util import _add_kv

Q3_K = 11


def unpack(raw):
    """(q (n, 256) in -4..3, sc6 (n, 16) in 0..63, d bytes (n, 2)) of block_q3_K: hmask[32], qs[64],
    scales[12], f16 d; weight 128 n + 32 j + l = ((qs[32 n + l] >> 2 j) & 3) - (bit 4 n + j of hmask[l] ? 0 : 4)."""
    b = np.ascontiguousarray(raw, np.uint8).reshape(-1, 110)
    hm, qs, sc = b[:, 0:32].astype(np.int32), b[:, 32:96].astype(np.int32), b[:, 96:108].astype(np.int32)
    q = np.empty((b.shape[0], 256), np.int32)
    for n in range(2):
        for j in range(4):
            low2 = (qs[:, 32 * n:32 * n + 32] >> (2 * j)) & 3
            q[:, 128 * n + 32 * j:128 * n + 32 * j + 32] = low2 - np.where((hm >> (4 * n + j)) & 1, 0, 4)
    sc6 = np.empty((b.shape[0], 16), np.int32)
    for s in range(16):
        low4 = (sc[:, s] & 0xF) if s < 8 else (sc[:, s - 8] >> 4)
        sc6[:, s] = low4 | (((sc[:, 8 + (s & 3)] >> (2 * (s >> 2))) & 3) << 4)
    return q, sc6, b[:, 108:110]


def to_q6_k(raw) -> np.ndarray:
    """The Q6_K blocks (ql[128], qh[64], i8 scales[16], f16 d) with the same d, scales sc6 - 32 and values q + 32."""
    q, sc6, d = unpack(raw)
    q = q + 32
    out = np.zeros((q.shape[0], 210), np.uint8)
    for h in range(2):
        a, b, c, e = (q[:, 128 * h + 32 * k:128 * h + 32 * k + 32] for k in range(4))
        out[:, 64 * h:64 * h + 32] = (a & 0xF) | ((c & 0xF) << 4)
        out[:, 64 * h + 32:64 * h + 64] = (b & 0xF) | ((e & 0xF) << 4)
        out[:, 128 + 32 * h:160 + 32 * h] = (a >> 4) | ((b >> 4) << 2) | ((c >> 4) << 4) | ((e >> 4) << 6)
    out[:, 192:208] = (sc6 - 32).astype(np.int8).view(np.uint8)
    out[:, 208:210] = d
    return out.reshape(-1)


def transcode_gguf(image) -> np.ndarray:
    """The image with every Q3_K tensor rewritten as Q6_K; the other tensors byte for byte."""
    rd = gguf.GGUFReader(image)
    w = gguf.GGUFWriter()
    for k, v in rd.kv.items():
        if k != "general.alignment":   # the writer's own first key
            _add_kv(w, k, v)
    for name, t in rd.tensors.items():
        if t.type == Q3_K:
            w.add_tensor(name, R.Q6_K, t.shape, to_q6_k(np.asarray(t.data)))
        else:
            w.add_tensor(name, t.type, t.shape, np.asarray(t.data))
    return w.to_bytes()


def rand_matrix(rows: int, K: int, seed: int = 0) -> np.ndarray:   # util.rand_matrix (its row_bytes stops at the oracle's types)
    buf = np.empty(K // 256 * 110 * rows, np.uint8)
    synthetic.fill_quant(buf, Q3_K, np.random.default_rng(seed))
    return buf


def extreme_matrix(rows: int, K: int, seed: int = 0) -> np.ndarray:
    """Every weight -4 or +3, every scale -32 or +31.  A sub-block of scale -32 holds -4 throughout:
    its scaled weights all sit at +128, the one value past int8.  A sub-block of scale +31 is mostly of
    one end with a few weights of the other."""
    rng = np.random.default_rng(seed)
    n = rows * K // 256
    neg_scale = rng.integers(0, 2, (n, 16)).astype(bool)
    end = rng.integers(0, 2, (n, 16, 1)).astype(bool) ^ (rng.random((n, 16, 16)) < 0.1)
    q = np.where(neg_scale[:, :, None] | end, -4, 3).reshape(n, 256)
    return synthetic.pack_q3_K(q, np.where(neg_scale, 0, 63), rng.uniform(0.0004, 0.0008, n).astype(np.float16)).reshape(-1)


def extreme_x(K: int, seed: int = 0) -> np.ndarray:
    """Activations whose Q8_K values are +-127 only: one magnitude per 256-block."""
    rng = np.random.default_rng(seed)
    s = rng.integers(0, 2, K) * 2 - 1
    return (s * np.repeat(rng.uniform(0.5, 2.0, K // 256), 256)).astype(np.float32)
