"""A numpy reference of the encoder pass (llm_build_bert, llama.cpp b5187, flash_attn off) in ggml's
CPU arithmetic: the f32 operand of an F16 matrix rounded to f16, the bias and the residual separate
f32 adds, LayerNorm and GELU as oracle/ggml_ref.py states them, attention with f16 q / k / v / p and
the exact f32 softmax with a double sum.  Dots accumulate in float64 (acc="f64") -- or, for the
rounding floor of a comparison, in f32 in index order (acc="f32")."""
import numpy as np

import ggml_ref as R
from blama_amd import gguf

LOGIT_TOL = 2e-3   # the project's embedding rule: max|d| <= LOGIT_TOL x rms of the reference row


class BertRef:
    def __init__(self, buf):
        rd = gguf.GGUFReader(np.asarray(buf, np.uint8))
        kv = rd.kv
        self.n_embd = int(kv["bert.embedding_length"])
        self.n_layer = int(kv["bert.block_count"])
        self.n_head = int(kv["bert.attention.head_count"])
        self.n_ff = int(kv["bert.feed_forward_length"])
        self.n_ctx_train = int(kv["bert.context_length"])
        self.eps = float(np.float32(kv["bert.attention.layer_norm_epsilon"]))
        self.hd = self.n_embd // self.n_head
        self.t = {}
        for name, ti in rd.tensors.items():
            dt = {0: np.float32, 1: np.float16}[ti.type]
            a = np.frombuffer(ti.data.tobytes(), dt)
            self.t[name] = a.reshape(ti.shape[::-1]) if len(ti.shape) > 1 else a

    # y[t][r] = sum_k f16(x[t][k]) W[r][k], rounded to f32 once (f64) or after every add (f32)
    def mm(self, W16, x, acc):
        x16 = R.f32_to_f16(x)
        if acc == "f64":
            return (x16.astype(np.float64) @ W16.astype(np.float64).T).astype(np.float32)
        Wf = W16.astype(np.float32)
        out = np.empty((x.shape[0], W16.shape[0]), np.float32)
        for t in range(x.shape[0]):
            out[t] = np.cumsum(Wf * x16[t].astype(np.float32)[None, :], axis=1, dtype=np.float32)[:, -1]
        return out

    def norm(self, x, name):
        w, b = self.t[name + ".weight"], self.t[name + ".bias"]
        y = np.stack([R.layer_norm(r, self.eps) for r in x])
        return ((y * w).astype(np.float32) + b).astype(np.float32)

    def attention(self, q, k, v, acc):
        n = q.shape[0]
        k16, v16 = R.f32_to_f16(k), R.f32_to_f16(v)
        scale = np.float32(1.0) / np.sqrt(np.float32(self.hd), dtype=np.float32)
        out = np.empty_like(q)
        for h in range(self.n_head):
            sl = slice(h * self.hd, (h + 1) * self.hd)
            s = self.mm(k16[:, sl], q[:, sl], acc)                    # (n, n): token x key
            p = np.stack([R.soft_max(s[t], scale) for t in range(n)])
            out[:, sl] = self.mm(np.ascontiguousarray(v16[:, sl].T), p, acc)
        return out

    def forward(self, tokens, acc="f64"):
        """The rows after the last layer, f32 [n][n_embd]: token i at position i, token type 0."""
        T = self.t
        tok = np.asarray(tokens, np.int64)
        n = tok.size
        f = lambda a: a.astype(np.float32)   # noqa: E731
        x = (f(T["token_embd.weight"][tok]) + f(T["token_types.weight"][0])[None, :]).astype(np.float32)
        x = (f(T["position_embd.weight"][:n]) + x).astype(np.float32)
        x = self.norm(x, "token_embd_norm")
        for l in range(self.n_layer):
            p = f"blk.{l}."
            lin = lambda name, a: (self.mm(T[p + name + ".weight"], a, acc) + T[p + name + ".bias"]).astype(np.float32)   # noqa: E731
            q, k, v = lin("attn_q", x), lin("attn_k", x), lin("attn_v", x)
            a = (lin("attn_output", self.attention(q, k, v, acc)) + x).astype(np.float32)
            x1 = self.norm(a, p + "attn_output_norm")
            hmid = R.gelu(lin("ffn_up", x1))
            ff = (lin("ffn_down", hmid) + x1).astype(np.float32)
            x = self.norm(ff, p + "layer_output_norm")
        return x


def rms(row):
    return float(np.sqrt(np.mean(np.asarray(row, np.float64) ** 2)))
