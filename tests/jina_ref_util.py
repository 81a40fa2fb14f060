"""References for the jina-bert-v2 tests: the ALiBi slopes of ggml_compute_forward_soft_max_f32, a plain float64
attention with the ALiBi bias, and the encoder pass (llm_build_bert's jina branch, llama.cpp b5187, flash_attn
off) in ggml's CPU arithmetic on BertRef's helpers: no position table, score * scale + slope * -|i - j| as two
f32 steps, h = gelu(gate x) * (up x) by the f16 table, no bias on ffn_up / ffn_gate.  acc as BertRef's."""
import numpy as np

import ggml_ref as R
from bert_ref_util import BertRef
from blama_amd import gguf


def alibi_slopes(n_head, max_bias=8.0):
    n2 = 1 << int(np.floor(np.log2(n_head)))
    m0, m1 = (np.power(np.float32(2.0), np.float32(-b) / np.float32(n2), dtype=np.float32) for b in (max_bias, max_bias / 2))
    return np.array([np.power(m0, np.float32(h + 1)) if h < n2 else np.power(m1, np.float32(2 * (h - n2) + 1))
                     for h in range(n_head)], np.float32)


def attn_alibi_ref(q, k16, v16, slopes, rows=None):
    """q (n, n_head, hd) f32, rounded to f16; k16 / v16 (n, n_head * hd): softmax_j(q_i . k_j / sqrt(hd) - slope_h
    |i - j|) v in float64, for the query rows `rows` (default all) -> (len(rows), n_head, hd) float64."""
    n, n_head, hd = q.shape
    rows = np.arange(n) if rows is None else np.asarray(rows)
    q16 = q[rows].astype(np.float16).astype(np.float64)
    dist = np.abs(rows[:, None] - np.arange(n)[None, :]).astype(np.float64)
    out = np.empty((rows.size, n_head, hd))
    for h in range(n_head):
        K, V = (a[:, h * hd:(h + 1) * hd].astype(np.float64) for a in (k16, v16))
        s = q16[:, h] @ K.T / np.sqrt(hd) - float(slopes[h]) * dist
        e = np.exp(s - s.max(axis=1, keepdims=True))
        out[:, h] = (e / e.sum(axis=1, keepdims=True)) @ V
    return out


class JinaRef(BertRef):
    def __init__(self, buf):
        rd = gguf.GGUFReader(np.asarray(buf, np.uint8))
        kv, a = rd.kv, "jina-bert-v2."
        self.n_embd, self.n_layer = int(kv[a + "embedding_length"]), int(kv[a + "block_count"])
        self.n_head, self.n_ff = int(kv[a + "attention.head_count"]), int(kv[a + "feed_forward_length"])
        self.eps = float(np.float32(kv[a + "attention.layer_norm_epsilon"]))
        self.hd = self.n_embd // self.n_head
        self.slopes = alibi_slopes(self.n_head)
        self.t = {}
        for name, ti in rd.tensors.items():
            arr = np.frombuffer(ti.data.tobytes(), {0: np.float32, 1: np.float16}[ti.type])
            self.t[name] = arr.reshape(ti.shape[::-1]) if len(ti.shape) > 1 else arr

    def attention(self, q, k, v, acc):
        n = q.shape[0]
        k16, v16 = R.f32_to_f16(k), R.f32_to_f16(v)
        scale = np.float32(1.0) / np.sqrt(np.float32(self.hd), dtype=np.float32)
        mask = -np.abs(np.arange(n)[:, None] - np.arange(n)[None, :]).astype(np.float32)
        out = np.empty_like(q)
        for h in range(self.n_head):
            sl = slice(h * self.hd, (h + 1) * self.hd)
            s = (self.mm(k16[:, sl], q[:, sl], acc) * scale).astype(np.float32)
            s = (s + (self.slopes[h] * mask).astype(np.float32)).astype(np.float32)
            p = np.stack([R.soft_max(s[t], 1.0) for t in range(n)])
            out[:, sl] = self.mm(np.ascontiguousarray(v16[:, sl].T), p, acc)
        return out

    def forward(self, tokens, acc="f64"):
        """The rows after the last layer, f32 [n][n_embd]: token i at position i, token type 0."""
        T = self.t
        tok = np.asarray(tokens, np.int64)
        f = lambda a: a.astype(np.float32)   # noqa: E731
        x = self.norm((f(T["token_embd.weight"][tok]) + f(T["token_types.weight"][0])[None, :]).astype(np.float32), "token_embd_norm")
        for l in range(self.n_layer):
            p = f"blk.{l}."
            lin = lambda name, a: (self.mm(T[p + name + ".weight"], a, acc) + T[p + name + ".bias"]).astype(np.float32)   # noqa: E731
            att = self.attention(lin("attn_q", x), lin("attn_k", x), lin("attn_v", x), acc)
            x1 = self.norm((lin("attn_output", att) + x).astype(np.float32), p + "attn_output_norm")
            h = (R.gelu(self.mm(T[p + "ffn_gate.weight"], x1, acc)) * self.mm(T[p + "ffn_up.weight"], x1, acc)).astype(np.float32)
            x = self.norm((lin("ffn_down", h) + x1).astype(np.float32), p + "layer_output_norm")
        return x
