"""A numpy reference of the nomic-bert encoder pass (llm_build_bert's nomic branch, llama.cpp b5187,
flash_attn off) in ggml's CPU arithmetic, on BertRef's helpers: no position table, the fused attn_qkv
without bias, ggml_rope_ext in mode NEOX on Q and K (the table of ggml_rope_cache_init, theta iterated
in f32), h = silu(gate x) * (up x), no projection bias anywhere.  acc as BertRef's."""
import numpy as np

import ggml_ref as R
from bert_ref_util import BertRef
from blama_amd import gguf


def rope_neox(x, pos, n_head, n_rot, freq_base, freq_scale=1.0):
    """x (n, n_head * hd) f32 rotated per head at pos[t]: pair ic is (ic, ic + n_rot / 2); elements
    from n_rot on are copied."""
    n = x.shape[0]
    y = np.array(x, np.float32).reshape(n, n_head, -1)
    half = n_rot // 2
    for t in range(n):
        cos, sin = R.rope_cache(int(pos[t]), n_rot, freq_base, freq_scale)
        x0, x1 = y[t, :, :half].copy(), y[t, :, half:n_rot].copy()
        y[t, :, :half] = ((x0 * cos).astype(np.float32) - (x1 * sin).astype(np.float32)).astype(np.float32)
        y[t, :, half:n_rot] = ((x0 * sin).astype(np.float32) + (x1 * cos).astype(np.float32)).astype(np.float32)
    return y.reshape(n, -1)


class NomicRef(BertRef):
    def __init__(self, buf):
        rd = gguf.GGUFReader(np.asarray(buf, np.uint8))
        kv, a = rd.kv, "nomic-bert."
        self.n_embd = int(kv[a + "embedding_length"])
        self.n_layer = int(kv[a + "block_count"])
        self.n_head = int(kv[a + "attention.head_count"])
        self.n_ff = int(kv[a + "feed_forward_length"])
        self.n_ctx_train = int(kv[a + "context_length"])
        self.eps = float(np.float32(kv[a + "attention.layer_norm_epsilon"]))
        self.hd = self.n_embd // self.n_head
        self.freq_base = float(np.float32(kv.get(a + "rope.freq_base", 10000.0)))
        self.n_rot = int(kv.get(a + "rope.dimension_count", self.hd))
        self.t = {}
        for name, ti in rd.tensors.items():
            arr = np.frombuffer(ti.data.tobytes(), {0: np.float32, 1: np.float16}[ti.type])
            self.t[name] = arr.reshape(ti.shape[::-1]) if len(ti.shape) > 1 else arr

    def forward(self, tokens, acc="f64"):
        """The rows after the last layer, f32 [n][n_embd]: token i at position i, token type 0."""
        T, d = self.t, self.n_embd
        tok = np.asarray(tokens, np.int64)
        pos = np.arange(tok.size)
        f = lambda a: a.astype(np.float32)   # noqa: E731
        x = (f(T["token_embd.weight"][tok]) + f(T["token_types.weight"][0])[None, :]).astype(np.float32)
        x = self.norm(x, "token_embd_norm")
        for l in range(self.n_layer):
            p = f"blk.{l}."
            qkv = self.mm(T[p + "attn_qkv.weight"], x, acc)
            q, k = (rope_neox(qkv[:, i * d:(i + 1) * d], pos, self.n_head, self.n_rot, self.freq_base) for i in (0, 1))
            att = self.attention(q, k, qkv[:, 2 * d:], acc)
            a = (self.mm(T[p + "attn_output.weight"], att, acc) + x).astype(np.float32)
            x1 = self.norm(a, p + "attn_output_norm")
            h = (R.silu(self.mm(T[p + "ffn_gate.weight"], x1, acc)) * self.mm(T[p + "ffn_up.weight"], x1, acc)).astype(np.float32)
            ff = (self.mm(T[p + "ffn_down.weight"], h, acc) + x1).astype(np.float32)
            x = self.norm(ff, p + "layer_output_norm")
        return x
