"""Helpers of the Q4_0 / Q5_0 tests.  Every block of the two types is exactly a Q8_0 block with
the same d and qs[i] = the signed weight (ggml's vec_dot_q4_0_q8_0, vec_dot_q5_0_q8_0 and
vec_dot_q8_0_q8_0 share their arithmetic, as the dequantize_row_* do), so the reference of every
test is the existing oracle run on the Q8_0 re-encoding this file produces."""
import numpy as np

import ggml_ref as R
from blama_amd import gguf, synthetic

Q4_0, Q5_0 = 2, 6
LEGACY = (Q4_0, Q5_0)
NAME = {Q4_0: "Q4_0", Q5_0: "Q5_0"}
BLOCK_BYTES = {Q4_0: 18, Q5_0: 22}


def row_bytes(t: int, K: int) -> int:
    return K // 32 * BLOCK_BYTES[t]


def signed_weights(raw, t: int) -> np.ndarray:
    """(n blocks, 32) int8: weight j = (qs[j] & 0xF) - 8, weight j + 16 = (qs[j] >> 4) - 8; Q5_0 adds
    bit j (bit j + 16) of the little-endian u32 qh as the fifth bit, offset 16."""
    b = np.ascontiguousarray(raw, np.uint8).reshape(-1, BLOCK_BYTES[t])
    qs = b[:, 2:18] if t == Q4_0 else b[:, 6:22]
    q = np.concatenate([qs & 0xF, qs >> 4], axis=1).astype(np.int32)
    if t == Q5_0:
        qh = b[:, 2:6].copy().view("<u4").reshape(-1, 1)
        q |= (((qh >> np.arange(32, dtype=np.uint32)) & 1) << 4).astype(np.int32)
    return (q - (8 if t == Q4_0 else 16)).astype(np.int8)


def to_q8_0(raw, t: int) -> np.ndarray:
    """The Q8_0 blocks (34 B: f16 d, int8 qs[32]) holding the same d and the same signed weights."""
    b = np.ascontiguousarray(raw, np.uint8).reshape(-1, BLOCK_BYTES[t])
    out = np.empty((b.shape[0], 34), np.uint8)
    out[:, 0:2] = b[:, 0:2]
    out[:, 2:] = signed_weights(raw, t).view(np.uint8)
    return out.reshape(-1)


def transcode_gguf(image) -> np.ndarray:
    """The synthetic image with every Q4_0 / Q5_0 tensor rewritten as Q8_0 (same names, shapes,
    metadata values and order; the other tensors byte for byte)."""
    rd = gguf.GGUFReader(image)
    w = gguf.GGUFWriter()
    for k, v in rd.kv.items():
        if k != "general.alignment":   # the writer's own first key
            _add_kv(w, k, v)
    for name, t in rd.tensors.items():
        if t.type in LEGACY:
            w.add_tensor(name, R.Q8_0, t.shape, to_q8_0(np.asarray(t.data), t.type))
        else:
            w.add_tensor(name, t.type, t.shape, np.asarray(t.data))
    return w.to_bytes()


def _add_kv(w, k, v):
    if isinstance(v, bool):
        w.add_bool(k, v)
    elif isinstance(v, str):
        w.add_str(k, v)
    elif isinstance(v, (list, tuple, np.ndarray)):
        v = list(v)
        if v and isinstance(v[0], str):
            w.add_array(k, gguf.T_STRING, v)
        elif v and isinstance(v[0], (float, np.floating)):
            w.add_array(k, gguf.T_FLOAT32, [float(x) for x in v])
        else:
            w.add_array(k, gguf.T_INT32, [int(x) for x in v])
    elif isinstance(v, (float, np.floating)):
        w.add_f32(k, float(v))
    else:
        w.add_u32(k, int(v))


def rand_matrix(t: int, rows: int, K: int, seed: int = 0, std: float = 0.03) -> np.ndarray:
    """Seeded random valid blocks (util.rand_matrix for the two types)."""
    buf = np.empty(row_bytes(t, K) * rows, np.uint8)
    synthetic.fill_quant(buf, t, np.random.default_rng(seed), std=std)
    return buf


def quantize_rows(X, t: int) -> np.ndarray:
    return synthetic.quantize_rows(X, t)


def pack_blocks(q, d16, t: int) -> np.ndarray:
    """Blocks from signed weights q (n, 32) in -8..7 (-16..15) and f16 scales d16 (n,)."""
    q = np.asarray(q, np.int32) + (8 if t == Q4_0 else 16)
    n = q.shape[0]
    out = np.empty((n, BLOCK_BYTES[t]), np.uint8)
    out[:, 0:2] = np.asarray(d16, np.float16).view(np.uint8).reshape(n, 2)
    qs = ((q[:, :16] & 0xF) | ((q[:, 16:] & 0xF) << 4)).astype(np.uint8)
    if t == Q5_0:
        qh = (((q >> 4) & 1).astype(np.uint32) << np.arange(32, dtype=np.uint32)).sum(1, dtype=np.uint32)
        out[:, 2:6] = qh.astype("<u4").view(np.uint8).reshape(n, 4)
        out[:, 6:22] = qs
    else:
        out[:, 2:18] = qs
    return out.reshape(-1)


def extreme_matrix(t: int, rows: int, K: int, seed: int = 0) -> np.ndarray:
    """Blocks at both ends of the range, -8 / +7 (-16 / +15): each weight one of the two, the
    low-nibble half and the high-nibble half of a block mostly of opposite ends, so that a wrong
    offset, a wrong sign or swapped halves moves every block sum by a large part of its size."""
    rng = np.random.default_rng(seed)
    n = rows * K // 32
    lo = 16 if t == Q5_0 else 8
    half = rng.integers(0, 2, (n, 1))                                   # which half is the negative one
    flip = rng.random((n, 32)) < 0.1                                    # a few weights of the other end
    neg = ((np.arange(32)[None, :] < 16) == (half == 1)) ^ flip
    q = np.where(neg, -lo, lo - 1)
    return pack_blocks(q, rng.uniform(0.002, 0.004, n).astype(np.float16), t)


def extreme_x(K: int, seed: int = 0) -> np.ndarray:
    """Activations whose every block quantises to +-127 only."""
    rng = np.random.default_rng(seed)
    s = rng.integers(0, 2, K) * 2 - 1
    a = np.repeat(rng.uniform(0.5, 2.0, K // 32), 32)
    return (s * a).astype(np.float32)
