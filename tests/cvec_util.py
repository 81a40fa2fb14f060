"""Control-vector reference for the tests: the CPU oracle's llm_build_llama / llm_build_gpt2 with
build_cvec after the FFN residual add, x = ((ffn + x) + v_il), and llama_adapter_cvec's layer rule
(llama.cpp b5187: apply / tensor_for / apply_to)."""
import numpy as np

import ggml_ref as R
import util
from util import oracle_from_gguf


def layer_vectors(data, n_embd, n_layer, il_start, il_end, shift=0):
    """{layer: vector} of llama_adapter_cvec::apply(data, len, n_embd, il_start, il_end): layer il
    (0-based) carries data[(il-1)*n_embd : il*n_embd] when 1 <= il <= n_layer-1, il_start <= il <=
    il_end and il*n_embd <= len.  shift = -1 is the off-by-one a power check wants rejected: the
    slice of layer il lands on layer il - 1 (data[0:n_embd] on layer 0)."""
    data = np.ascontiguousarray(data, np.float32).reshape(-1)
    out = {}
    for il in range(1, n_layer):
        if il_start <= il <= il_end and il * n_embd <= data.size:
            out[il + shift] = data[(il - 1) * n_embd:il * n_embd]
    return out


class CvecOracle(R.LlamaOracle):
    """LlamaOracle whose layers add their control-vector direction after the FFN residual add.
    vec: {layer: f32[n_embd]} (empty: the plain oracle's arithmetic).  x_rms: rms of the residual
    stream after the last layer of the last token decoded."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.vec = {}
        self.x_rms = 0.0

    def _cvec(self, x, il):
        v = self.vec.get(il)
        return x if v is None else (x + np.asarray(v, np.float32)).astype(np.float32)

    def _decode_one_gpt2(self, token):
        hp = self.hp
        hd = hp.head_dim
        d = hp.n_embd
        pos = (max(self.cell_pos) + 1) if self.n_past else 0
        cell = self.n_past
        assert cell < self.n_ctx and pos < hp.n_ctx_train
        x = (self._row("token_embd.weight", token) + self._row("position_embd.weight", pos)).astype(np.float32)
        scale = np.float32(1.0) / np.sqrt(np.float32(hd), dtype=np.float32)
        ratio = hp.n_head // hp.n_head_kv
        for il in range(hp.n_layer):
            b = f"blk.{il}."
            cur = self._norm(x, b + "attn_norm")
            qkv = (self._mm(b + "attn_qkv.weight", cur) + self._vec(b + "attn_qkv.bias")).astype(np.float32)
            q = qkv[:d].reshape(hp.n_head, hd)
            self.kcache[il][cell] = R.f32_to_f16(qkv[d:2 * d])
            self.vcache[il][cell] = R.f32_to_f16(qkv[2 * d:3 * d])
            vis = [c for c in range(cell + 1) if c == cell or self.cell_pos[c] <= pos]
            Kc = self.kcache[il][vis].reshape(len(vis), hp.n_head_kv, hd)
            Vc = self.vcache[il][vis].reshape(len(vis), hp.n_head_kv, hd)
            att = np.empty((hp.n_head, hd), np.float32)
            for h in range(hp.n_head):
                att[h] = R.attention_head(q[h], Kc[:, h // ratio], Vc[:, h // ratio], scale)
            cur = (self._mm(b + "attn_output.weight", att.reshape(-1)) + self._vec(b + "attn_output.bias")).astype(np.float32)
            x = (cur + x).astype(np.float32)
            cur = self._norm(x, b + "ffn_norm")
            u = (self._mm(b + "ffn_up.weight", cur) + self._vec(b + "ffn_up.bias")).astype(np.float32)
            cur = (self._mm(b + "ffn_down.weight", R.gelu(u)) + self._vec(b + "ffn_down.bias")).astype(np.float32)
            x = self._cvec((cur + x).astype(np.float32), il)
        self.x_rms = float(np.sqrt(np.mean(x.astype(np.float64) ** 2)))
        cur = self._norm(x, "output_norm")
        out = self.tensors.get("output.weight", self.tensors["token_embd.weight"])
        logits = R.mul_mat_vec(out.data, out.type, out.shape[0], cur)
        self.cell_pos.append(pos)
        self.n_past += 1
        return logits

    def decode_one(self, token):
        if self.hp.arch == "gpt2":
            return self._decode_one_gpt2(token)
        hp = self.hp
        hd = hp.head_dim
        pos = (max(self.cell_pos) + 1) if self.n_past else 0
        cell = self.n_past
        assert cell < self.n_ctx
        x = self._row("token_embd.weight", token)
        scale = np.float32(1.0) / np.sqrt(np.float32(hd), dtype=np.float32)
        ff = self.tensors.get("rope_freqs.weight")
        ffv = None if ff is None else R.dequantize(ff.data, ff.type)
        ratio = hp.n_head // hp.n_head_kv
        for il in range(hp.n_layer):
            cur = (R.rms_norm(x, hp.eps) * self._w(f"blk.{il}.attn_norm.weight")).astype(np.float32)
            q = self._rope(self._mm(f"blk.{il}.attn_q.weight", cur).reshape(hp.n_head, hd), pos, ffv, "q")
            k = self._rope(self._mm(f"blk.{il}.attn_k.weight", cur).reshape(hp.n_head_kv, hd), pos, ffv, "k")
            v = self._mm(f"blk.{il}.attn_v.weight", cur)
            self.kcache[il][cell] = R.f32_to_f16(k.reshape(-1))
            self.vcache[il][cell] = R.f32_to_f16(v)
            vis = [c for c in range(cell + 1) if c == cell or self.cell_pos[c] <= pos]
            Kc = self.kcache[il][vis].reshape(len(vis), hp.n_head_kv, hd)
            Vc = self.vcache[il][vis].reshape(len(vis), hp.n_head_kv, hd)
            att = np.empty((hp.n_head, hd), np.float32)
            for h in range(hp.n_head):
                att[h] = R.attention_head(q[h], Kc[:, h // ratio], Vc[:, h // ratio], scale)
            x = (self._mm(f"blk.{il}.attn_output.weight", att.reshape(-1)) + x).astype(np.float32)
            cur = (R.rms_norm(x, hp.eps) * self._w(f"blk.{il}.ffn_norm.weight")).astype(np.float32)
            x = self._cvec((self._ffn(il, cur) + x).astype(np.float32), il)
        self.x_rms = float(np.sqrt(np.mean(x.astype(np.float64) ** 2)))
        cur = (R.rms_norm(x, hp.eps) * self._w("output_norm.weight")).astype(np.float32)
        out = self.tensors.get("output.weight", self.tensors["token_embd.weight"])
        logits = R.mul_mat_vec(out.data, out.type, out.shape[0], cur)
        self.cell_pos.append(pos)
        self.n_past += 1
        return logits


def cvec_oracle(buf, n_ctx, vec=None) -> CvecOracle:
    o = oracle_from_gguf(buf, n_ctx=n_ctx)
    c = CvecOracle(o.hp, o.tensors, n_ctx=n_ctx)
    c.vec = dict(vec or {})
    return c


def cvec_ulp_floor(buf, n_ctx, prompt, tokens, vec, runs=4):
    """util.oracle_ulp_floor with the steered oracle: its perturbed re-runs build their oracle
    through util.oracle_from_gguf, which for the length of the call returns a CvecOracle."""
    orig = util.oracle_from_gguf
    util.oracle_from_gguf = lambda b, n_ctx=0: cvec_oracle(b, n_ctx, vec)
    try:
        return util.oracle_ulp_floor(buf, n_ctx, prompt, tokens, runs=runs)
    finally:
        util.oracle_from_gguf = orig
