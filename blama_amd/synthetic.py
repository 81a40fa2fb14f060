"""Synthetic LLaMA-family GGUF images for the BASELINE.json configs.

No checkpoint can be downloaded here, so tests and the
bench use GGUF images with the *exact* tensor names, shapes and per-tensor
quant types of the named models, filled with seeded random -- but valid and
realistically scaled -- quant blocks.

Per-tensor type rules follow llama.cpp b5187 ``llama_tensor_get_type``
(src/llama-quant.cpp) as summarised in SURVEY.md §8 "Q4_K_M tensor mix":
Q4_K_M -> output Q6_K; attn_v / ffn_down Q6_K where use_more_bits(i, n);
everything else Q4_K; 8-expert models bump attn_k/attn_v to Q8_0 and
attn_output to Q5_K (Q4_K_M) ; norms F32.
"""
from __future__ import annotations

import hashlib
from dataclasses import dataclass, replace

import os

import numpy as np

from . import gguf

F32, F16, Q8_0, Q4_K, Q5_K, Q6_K = 0, 1, 8, 12, 13, 14
Q4_0, Q5_0 = 2, 6


@dataclass(frozen=True)
class LlamaConfig:
    name: str
    n_vocab: int
    n_embd: int
    n_layer: int
    n_head: int
    n_head_kv: int
    n_ff: int
    n_ctx_train: int
    rope_base: float
    eps: float
    ftype: str            # "Q4_K_M", "Q5_K_M", "Q6_K", "Q8_0", "Q4_K"...
    n_expert: int = 0
    n_expert_used: int = 0
    arch: str = "llama"   # "llama" or "gpt2" (llm_build_gpt2)
    # RoPE variants, all off by default (an existing config's image stays byte-identical)
    n_rot: int = 0                    # rope.dimension_count; 0 = head_dim (partial rotary when smaller)
    rope_scale: float = 0.0           # > 0: linear RoPE scaling, rope.scaling.type "linear" + rope.scaling.factor
    rope_scale_legacy: bool = False   # write the factor as rope.scale_linear instead, with no type key
    rope_scaling_type: str = "linear"  # the rope.scaling.type written beside rope.scaling.factor
    rope_freqs: bool = False          # an F32 rope_freqs.weight of n_rot/2 frequency factors (Llama-3.1)
    init: str = ""                    # _init_params overrides of this config, "key=value,..." as BLAMA_SYNTH_INIT
    pooling_type: int = -1            # >= 0: written as {arch}.pooling_type (llama_pooling_type)
    tied_head: bool = False           # ftype "F16": no output.weight, the head is token_embd (Llama-3.2)

    @property
    def head_dim(self):
        return self.n_embd // self.n_head

    @property
    def rot_dim(self):
        return self.n_rot or self.head_dim


CONFIGS = {
    # BASELINE.json configs[0..4]
    "tinyllama-1.1b-q8_0": LlamaConfig("TinyLlama-1.1B", 32000, 2048, 22, 32, 4, 5632, 2048,
                                        10000.0, 1e-5, "Q8_0"),
    "llama2-7b-q4_k_m": LlamaConfig("Llama-2-7B", 32000, 4096, 32, 32, 32, 11008, 4096,
                                     10000.0, 1e-5, "Q4_K_M"),
    "llama3-8b-q6_k": LlamaConfig("Llama-3-8B", 128256, 4096, 32, 32, 8, 14336, 8192,
                                   500000.0, 1e-5, "Q6_K"),
    "mixtral-8x7b-q5_k_m": LlamaConfig("Mixtral-8x7B", 32000, 4096, 32, 32, 8, 14336, 32768,
                                        1e6, 1e-5, "Q5_K_M", n_expert=8, n_expert_used=2),
    # small shapes for parity tests (same code paths, seconds on the CPU oracle)
    "tiny-q4_k_m": LlamaConfig("tiny", 512, 256, 4, 4, 2, 512, 256, 10000.0, 1e-5, "Q4_K_M"),
    "tiny-q5_k_m": LlamaConfig("tiny", 512, 256, 2, 4, 2, 512, 256, 10000.0, 1e-5, "Q5_K_M"),
    "tiny-q6_k": LlamaConfig("tiny", 640, 256, 2, 4, 1, 768, 256, 500000.0, 1e-5, "Q6_K"),
    "tiny-q8_0": LlamaConfig("tiny", 384, 256, 2, 8, 4, 768, 256, 10000.0, 1e-6, "Q8_0"),
    "tiny1-q4_k_m": LlamaConfig("tiny1", 512, 256, 1, 4, 2, 512, 256, 10000.0, 1e-5, "Q4_K_M"),
    "tiny-moe-q5_k_m": LlamaConfig("tiny-moe", 512, 256, 2, 4, 2, 512, 256, 1e6, 1e-5,
                                    "Q5_K_M", n_expert=4, n_expert_used=2),
    # RoPE variants (tests/test_gpu_rope.py): frequency factors, linear scaling under both key
    # spellings, partial rotary -- on the streaming step (hd 64), the gemv_kernel step (hd 32), MoE.
    # Q/K weights 30 x the default scale: with the default's near-uniform softmax a wrong rotation
    # barely reaches the logits (test_rope_fault_would_be_detected measures that it does here)
    "tiny-rf-q4_k_m": LlamaConfig("tiny-rf", 512, 256, 2, 4, 2, 512, 256, 10000.0, 1e-5, "Q4_K_M",
                                   rope_scale=4.0, rope_freqs=True, init="qk=0.3"),
    "tiny-prot-q4_k_m": LlamaConfig("tiny-prot", 512, 256, 2, 4, 2, 512, 256, 10000.0, 1e-5, "Q4_K_M",
                                     n_rot=32, rope_scale=2.0, rope_scale_legacy=True, init="qk=0.3"),
    "tiny-rf-q8_0": LlamaConfig("tiny-rf", 512, 256, 2, 8, 4, 768, 256, 10000.0, 1e-6, "Q8_0",
                                 n_rot=16, rope_scale=4.0, rope_freqs=True, init="qk=0.3"),
    "tiny-rf-moe-q5_k_m": LlamaConfig("tiny-rf-moe", 512, 256, 2, 4, 2, 512, 256, 1e6, 1e-5, "Q5_K_M",
                                       n_expert=4, n_expert_used=2, rope_scale=2.0, rope_freqs=True, init="qk=0.3"),
    # GQA ratio 2 with 16 kv heads of 64: the quantising decode attention has no
    # kernel for two kv heads per 256-block, so decode takes the gemv_kernel step and short
    # batches the plain fused attention + quant_act -- both must still run
    "tiny-gqa16-q4_k_m": LlamaConfig("tiny-gqa16", 512, 2048, 2, 32, 16, 512, 256, 10000.0, 1e-5, "Q4_K_M"),
    # the reference's own KAT model shape (gpt2-117m-q6_k, t-integration.cpp:25): 12 x 768,
    # 12 heads of 64, n_ff 3072, V 50257, 1024 positions, every matrix Q6_K, tied output head
    "gpt2-117m-q6_k": LlamaConfig("GPT-2-117M", 50257, 768, 12, 12, 12, 3072, 1024, 10000.0, 1e-5,
                                  "Q6_K", arch="gpt2"),
    "tiny-gpt2-q6_k": LlamaConfig("tiny-gpt2", 700, 256, 2, 4, 4, 768, 128, 10000.0, 1e-5, "Q6_K",
                                  arch="gpt2"),
    "tiny-gpt2-q8_0": LlamaConfig("tiny-gpt2", 600, 512, 2, 8, 8, 1024, 128, 10000.0, 1e-5, "Q8_0",
                                  arch="gpt2"),
}

# Unquantised F16 files (every matrix F16; a table of their own: CONFIGS' "tiny-" names are the
# quantised decode paths): GQA 2 with heads of 64; heads of 128 with a tied output head (no
# output.weight); rope_freqs + linear scaling + partial rotary with O(1) scores
F16_CONFIGS = {
    "tiny-f16": LlamaConfig("tiny-f16", 512, 256, 2, 4, 2, 768, 1024, 10000.0, 1e-5, "F16"),
    "tiny-f16-hd128": LlamaConfig("tiny-f16-hd128", 384, 512, 2, 4, 4, 1024, 1024, 10000.0, 1e-5, "F16",
                                  tied_head=True),
    "tiny-rf-f16": LlamaConfig("tiny-rf-f16", 512, 256, 2, 4, 2, 768, 1024, 10000.0, 1e-5, "F16",
                               n_rot=32, rope_scale=4.0, rope_freqs=True, init="qk=0.3"),
    # benchmark shapes (scripts/f16_bench.py)
    "tinyllama-1.1b-f16": LlamaConfig("TinyLlama-1.1B", 32000, 2048, 22, 32, 4, 5632, 2048, 10000.0, 1e-5, "F16"),
    "llama2-7b-f16": LlamaConfig("Llama-2-7B", 32000, 4096, 32, 32, 32, 11008, 4096, 10000.0, 1e-5, "F16"),
}

# llama-quantize's classic Q4_0 / Q5_0 files (general.file_type 2 / 8): every matrix of the type,
# output.weight Q6_K.  A table of their own, as F16_CONFIGS.  GQA 2 with heads of 64 (the streaming
# decode step) and, in the shape of tiny-q8_0, heads of 32 (the gemv_kernel step)
LEGACY_CONFIGS = {
    "tiny-q4_0": LlamaConfig("tiny-q4_0", 512, 256, 2, 4, 2, 512, 256, 10000.0, 1e-5, "Q4_0"),
    "tiny-q5_0": LlamaConfig("tiny-q5_0", 512, 256, 2, 4, 2, 512, 256, 10000.0, 1e-5, "Q5_0"),
    "tiny-hd32-q4_0": LlamaConfig("tiny-hd32-q4_0", 384, 256, 2, 8, 4, 768, 256, 10000.0, 1e-6, "Q4_0"),
    "tiny-hd32-q5_0": LlamaConfig("tiny-hd32-q5_0", 384, 256, 2, 8, 4, 768, 256, 10000.0, 1e-6, "Q5_0"),
    # benchmark shapes (scripts/legacy_quant_bench.py)
    "tinyllama-1.1b-q4_0": LlamaConfig("TinyLlama-1.1B", 32000, 2048, 22, 32, 4, 5632, 2048, 10000.0, 1e-5, "Q4_0"),
    "tinyllama-1.1b-q5_0": LlamaConfig("TinyLlama-1.1B", 32000, 2048, 22, 32, 4, 5632, 2048, 10000.0, 1e-5, "Q5_0"),
}


def use_more_bits(i: int, n: int) -> bool:
    # llama-quant.cpp use_more_bits
    return i < n // 8 or i >= 7 * n // 8 or (i - n // 8) % 3 == 2


def _gpt2_types(cfg, base) -> dict:
    """llm_build_gpt2's tensors (LLM_ARCH_GPT2 in src/llama-arch.cpp): every matrix of the
    file type, LayerNorm weights / biases and the matrix biases F32, no output.weight (the
    head is token_embd, TENSOR_DUPLICATED in llama-model.cpp)."""
    t = {"token_embd.weight": base, "position_embd.weight": base,
         "output_norm.weight": F32, "output_norm.bias": F32}
    for i in range(cfg.n_layer):
        p = f"blk.{i}."
        for n in ("attn_norm", "ffn_norm"):
            t[p + n + ".weight"] = F32
            t[p + n + ".bias"] = F32
        for n in ("attn_qkv", "attn_output", "ffn_up", "ffn_down"):
            t[p + n + ".weight"] = base
            t[p + n + ".bias"] = F32
    return t


def _gpt2_shapes(cfg) -> dict:
    d = cfg.n_embd
    s = {"token_embd.weight": (d, cfg.n_vocab), "position_embd.weight": (d, cfg.n_ctx_train),
         "output_norm.weight": (d,), "output_norm.bias": (d,)}
    for i in range(cfg.n_layer):
        p = f"blk.{i}."
        for n in ("attn_norm", "ffn_norm"):
            s[p + n + ".weight"] = (d,)
            s[p + n + ".bias"] = (d,)
        s[p + "attn_qkv.weight"] = (d, 3 * d)
        s[p + "attn_qkv.bias"] = (3 * d,)
        s[p + "attn_output.weight"] = (d, d)
        s[p + "attn_output.bias"] = (d,)
        s[p + "ffn_up.weight"] = (d, cfg.n_ff)
        s[p + "ffn_up.bias"] = (cfg.n_ff,)
        s[p + "ffn_down.weight"] = (cfg.n_ff, d)
        s[p + "ffn_down.bias"] = (d,)
    return s


def tensor_types(cfg: LlamaConfig) -> dict:
    """name -> ggml type for every weight (the Q*_K_M mixes of llama_tensor_get_type)."""
    base = {"Q4_K_M": Q4_K, "Q5_K_M": Q5_K, "Q6_K": Q6_K, "Q8_0": Q8_0, "Q4_K": Q4_K,
            "Q5_K": Q5_K, "F16": F16, "Q4_0": Q4_0, "Q5_0": Q5_0}[cfg.ftype]
    if cfg.arch == "gpt2":
        return _gpt2_types(cfg, base)
    if base == F16:   # the unquantised file convert_hf_to_gguf writes: every matrix F16, the rest F32
        t = {n: (F32 if len(sh) == 1 or n.endswith("ffn_gate_inp.weight") else F16) for n, sh in tensor_shapes(cfg).items()}
        return t
    mixed = cfg.ftype in ("Q4_K_M", "Q5_K_M")
    t = {"token_embd.weight": base, "output_norm.weight": F32,
         "output.weight": Q8_0 if base == Q8_0 else Q6_K}
    if cfg.rope_freqs:
        t["rope_freqs.weight"] = F32
    n = cfg.n_layer
    for i in range(n):
        p = f"blk.{i}."
        t[p + "attn_norm.weight"] = F32
        t[p + "ffn_norm.weight"] = F32
        t[p + "attn_q.weight"] = base
        t[p + "attn_k.weight"] = base
        t[p + "attn_v.weight"] = base
        t[p + "attn_output.weight"] = base
        if mixed and use_more_bits(i, n):
            t[p + "attn_v.weight"] = Q6_K
        if cfg.n_expert == 8 and base != Q8_0:
            t[p + "attn_k.weight"] = Q8_0
            t[p + "attn_v.weight"] = Q8_0
            if cfg.ftype == "Q4_K_M":
                t[p + "attn_output.weight"] = Q5_K
        down = Q6_K if (mixed and use_more_bits(i, n)) else base
        if cfg.n_expert:
            t[p + "ffn_gate_inp.weight"] = F32
            t[p + "ffn_gate_exps.weight"] = base
            t[p + "ffn_up_exps.weight"] = base
            t[p + "ffn_down_exps.weight"] = down
        else:
            t[p + "ffn_gate.weight"] = base
            t[p + "ffn_up.weight"] = base
            t[p + "ffn_down.weight"] = down
    return t


def tensor_shapes(cfg: LlamaConfig) -> dict:
    """name -> ggml ne shape (ne0 = input dim K)."""
    if cfg.arch == "gpt2":
        return _gpt2_shapes(cfg)
    d, kv = cfg.n_embd, cfg.n_head_kv * cfg.head_dim
    s = {"token_embd.weight": (d, cfg.n_vocab), "output_norm.weight": (d,),
         "output.weight": (d, cfg.n_vocab)}
    if cfg.tied_head:
        del s["output.weight"]
    if cfg.rope_freqs:
        s["rope_freqs.weight"] = (cfg.rot_dim // 2,)
    for i in range(cfg.n_layer):
        p = f"blk.{i}."
        s[p + "attn_norm.weight"] = (d,)
        s[p + "ffn_norm.weight"] = (d,)
        s[p + "attn_q.weight"] = (d, d)
        s[p + "attn_k.weight"] = (d, kv)
        s[p + "attn_v.weight"] = (d, kv)
        s[p + "attn_output.weight"] = (d, d)
        if cfg.n_expert:
            s[p + "ffn_gate_inp.weight"] = (d, cfg.n_expert)
            s[p + "ffn_gate_exps.weight"] = (d, cfg.n_ff, cfg.n_expert)
            s[p + "ffn_up_exps.weight"] = (d, cfg.n_ff, cfg.n_expert)
            s[p + "ffn_down_exps.weight"] = (cfg.n_ff, d, cfg.n_expert)
        else:
            s[p + "ffn_gate.weight"] = (d, cfg.n_ff)
            s[p + "ffn_up.weight"] = (d, cfg.n_ff)
            s[p + "ffn_down.weight"] = (cfg.n_ff, d)
    return s


def _rng(seed: int, name: str):
    h = hashlib.sha256(f"{seed}:{name}".encode()).digest()
    return np.random.default_rng(int.from_bytes(h[:8], "little"))


def _pack_scales_k4(sc: np.ndarray, m: np.ndarray) -> np.ndarray:
    """Inverse of get_scale_min_k4 (the packing of quantize_row_q4_K_ref)."""
    nb = sc.shape[0]
    s = np.zeros((nb, 12), np.uint8)
    for j in range(4):
        s[:, j] = sc[:, j]
        s[:, j + 4] = m[:, j]
    for j in range(4, 8):
        s[:, j + 4] = (sc[:, j] & 0xF) | ((m[:, j] & 0xF) << 4)
        s[:, j - 4] |= (sc[:, j] >> 4) << 6
        s[:, j] |= (m[:, j] >> 4) << 6
    return s


def fill_quant(view: np.ndarray, t: int, rng, std: float = 0.03):
    """Fill a tensor's bytes with valid random blocks whose dequantised values
    are roughly zero-mean with standard deviation ``std``."""
    be, bb = gguf.GGML_BLOCK[t]
    if t == F32:
        v = view.view(np.float32)
        v[:] = rng.standard_normal(v.size, dtype=np.float32) * np.float32(std)
        return
    if t == F16:
        v = view.view(np.float16)
        v[:] = (rng.standard_normal(v.size, dtype=np.float32) * np.float32(std)).astype(np.float16)
        return
    nb = view.size // bb
    bl = view.reshape(nb, bb)
    CH = 1 << 16   # blocks per chunk (bounded temporaries)
    for a in range(0, nb, CH):
        b = bl[a:a + CH]
        n = b.shape[0]
        b[:] = rng.integers(0, 256, size=b.shape, dtype=np.uint8)
        if t in (Q4_K, Q5_K):
            qmax = 15 if t == Q4_K else 31
            sc = rng.integers(24, 64, size=(n, 8), dtype=np.int32)
            d = (std / (40.0 * (qmax + 1) / np.sqrt(12.0))) * rng.uniform(0.8, 1.2, n)
            ratio = 16.0 if t == Q4_K else 32.0      # dmin = d*ratio
            dmin = d * ratio
            m = np.clip(np.rint(sc * (qmax / 2.0) / ratio), 0, 63).astype(np.int32)
            b[:, 0:2] = d.astype(np.float16).view(np.uint8).reshape(n, 2)
            b[:, 2:4] = dmin.astype(np.float16).view(np.uint8).reshape(n, 2)
            b[:, 4:16] = _pack_scales_k4(sc.astype(np.uint8), m.astype(np.uint8))
        elif t == Q6_K:
            sc = rng.integers(16, 48, size=(n, 16), dtype=np.int32)
            sgn = rng.integers(0, 2, size=(n, 16), dtype=np.int32) * 2 - 1
            b[:, 192:208] = (sc * sgn).astype(np.int8).view(np.uint8)
            d = (std / (32.0 * 64 / np.sqrt(12.0))) * rng.uniform(0.8, 1.2, n)
            b[:, 208:210] = d.astype(np.float16).view(np.uint8).reshape(n, 2)
        elif t == Q8_0:
            d = (std / (256 / np.sqrt(12.0))) * rng.uniform(0.8, 1.2, n)
            b[:, 0:2] = d.astype(np.float16).view(np.uint8).reshape(n, 2)
        elif t in (Q4_0, Q5_0):   # uniform 4- / 5-bit values around 8 / 16: std = d * levels / sqrt(12)
            d = (std / ((16 if t == Q4_0 else 32) / np.sqrt(12.0))) * rng.uniform(0.8, 1.2, n)
            b[:, 0:2] = d.astype(np.float16).view(np.uint8).reshape(n, 2)
        else:
            raise NotImplementedError(t)


# ---------------------------------------------------------------------------
# Float -> block quantisers (simple, valid blocks; not ggml's rmse-searching
# quantize_row_*_ref -- any valid block is valid model data).  X: (n, 256)
# float32 superblocks (Q8_0: (n, 32) blocks); returns (n, block_bytes) uint8.
# ---------------------------------------------------------------------------
def _f16(a):
    return np.asarray(a, np.float32).astype(np.float16)


def quantize_q8_0_rows(X):
    X = X.reshape(-1, 32)
    amax = np.abs(X).max(1)
    d16 = _f16(amax / 127.0)
    d = d16.astype(np.float32)
    q = np.clip(np.rint(np.divide(X, d[:, None], out=np.zeros_like(X), where=d[:, None] > 0)), -127, 127)
    out = np.empty((X.shape[0], 34), np.uint8)
    out[:, 0:2] = d16.view(np.uint8).reshape(-1, 2)
    out[:, 2:] = q.astype(np.int8).view(np.uint8)
    return out


def quantize_q45_0_rows(X, q5: bool):
    """(n, 32) blocks -> block_q4_0 (18 B) / block_q5_0 (22 B): d = amax / 7 (15), the level
    nearest to x / d (within half a quantum of x), stored + 8 (+ 16): weight j in the low nibble of qs[j],
    weight j + 16 in the high one, the fifth bits of weights 0..31 in the little-endian u32 qh."""
    X = X.reshape(-1, 32)
    n = X.shape[0]
    off = 16 if q5 else 8
    d16 = _f16(np.abs(X).max(1) / (off - 1.0))
    d = d16.astype(np.float32)
    q = np.clip(np.rint(np.divide(X, d[:, None], out=np.zeros_like(X), where=d[:, None] > 0)), -off, off - 1)
    q = q.astype(np.int32) + off
    lo, hi = q[:, :16], q[:, 16:]
    out = np.empty((n, 22 if q5 else 18), np.uint8)
    out[:, 0:2] = d16.view(np.uint8).reshape(n, 2)
    qs = ((lo & 0xF) | ((hi & 0xF) << 4)).astype(np.uint8)
    if q5:
        qh = (((q >> 4) & 1).astype(np.uint32) << np.arange(32, dtype=np.uint32)).sum(1, dtype=np.uint32)
        out[:, 2:6] = qh.astype("<u4").view(np.uint8).reshape(n, 4)
        out[:, 6:22] = qs
    else:
        out[:, 2:18] = qs
    return out


def quantize_q6_K_rows(X):
    X = X.reshape(-1, 256)
    n = X.shape[0]
    s = np.abs(X.reshape(n, 16, 16)).max(2) / 31.0            # per-16 scale
    d16 = _f16(s.max(1) / 127.0)
    d = d16.astype(np.float32)
    sc = np.clip(np.rint(np.divide(s, d[:, None], out=np.zeros_like(s), where=d[:, None] > 0)), 1, 127)
    eff = np.repeat(d[:, None] * sc, 16, axis=1)
    q = np.clip(np.rint(np.divide(X, eff, out=np.zeros_like(X), where=eff > 0)), -32, 31).astype(np.int32) + 32
    ql = np.zeros((n, 128), np.uint8)
    qh = np.zeros((n, 64), np.uint8)
    for h in range(2):
        e = q[:, 128 * h:128 * h + 128]
        a, b, c, dd = e[:, 0:32], e[:, 32:64], e[:, 64:96], e[:, 96:128]
        ql[:, 64 * h:64 * h + 32] = (a & 0xF) | ((c & 0xF) << 4)
        ql[:, 64 * h + 32:64 * h + 64] = (b & 0xF) | ((dd & 0xF) << 4)
        qh[:, 32 * h:32 * h + 32] = (a >> 4) | ((b >> 4) << 2) | ((c >> 4) << 4) | ((dd >> 4) << 6)
    out = np.empty((n, 210), np.uint8)
    out[:, 0:128] = ql
    out[:, 128:192] = qh
    out[:, 192:208] = sc.astype(np.int8).view(np.uint8)
    out[:, 208:210] = d16.view(np.uint8).reshape(n, 2)
    return out


def quantize_q45_K_rows(X, q5: bool):
    X = X.reshape(-1, 256)
    n = X.shape[0]
    qmax = 31 if q5 else 15
    sub = X.reshape(n, 8, 32)
    mn = np.maximum(0.0, -sub.min(2))
    s = (sub.max(2) + mn) / qmax
    d16 = _f16(s.max(1) / 63.0)
    m16 = _f16(mn.max(1) / 63.0)
    d, dm = d16.astype(np.float32), m16.astype(np.float32)
    sc = np.clip(np.rint(np.divide(s, d[:, None], out=np.zeros_like(s), where=d[:, None] > 0)), 0, 63)
    m = np.clip(np.rint(np.divide(mn, dm[:, None], out=np.zeros_like(mn), where=dm[:, None] > 0)), 0, 63)
    eff = d[:, None] * sc
    off = dm[:, None] * m
    q = np.clip(np.rint(np.divide(sub + off[:, :, None], eff[:, :, None], out=np.zeros_like(sub),
                                  where=eff[:, :, None] > 0)), 0, qmax).astype(np.int32).reshape(n, 256)
    qs = np.zeros((n, 128), np.uint8)
    qh = np.zeros((n, 32), np.uint8)
    for j in range(4):
        lo, hi = q[:, 64 * j:64 * j + 32], q[:, 64 * j + 32:64 * j + 64]
        qs[:, 32 * j:32 * j + 32] = (lo & 0xF) | ((hi & 0xF) << 4)
        if q5:
            qh |= (((lo >> 4) & 1) << (2 * j)).astype(np.uint8)
            qh |= (((hi >> 4) & 1) << (2 * j + 1)).astype(np.uint8)
    out = np.empty((n, 176 if q5 else 144), np.uint8)
    out[:, 0:2] = d16.view(np.uint8).reshape(n, 2)
    out[:, 2:4] = m16.view(np.uint8).reshape(n, 2)
    out[:, 4:16] = _pack_scales_k4(sc.astype(np.uint8), m.astype(np.uint8))
    if q5:
        out[:, 16:48] = qh
        out[:, 48:176] = qs
    else:
        out[:, 16:144] = qs
    return out


def quantize_rows(X, t: int) -> np.ndarray:
    X = np.ascontiguousarray(X, np.float32)
    if t == Q8_0:
        return quantize_q8_0_rows(X).reshape(-1)
    if t == Q6_K:
        return quantize_q6_K_rows(X).reshape(-1)
    if t in (Q4_K, Q5_K):
        return quantize_q45_K_rows(X, t == Q5_K).reshape(-1)
    if t in (Q4_0, Q5_0):
        return quantize_q45_0_rows(X, t == Q5_0).reshape(-1)
    if t == F32:
        return X.reshape(-1).view(np.uint8)
    if t == F16:
        return X.reshape(-1).astype(np.float16).view(np.uint8)
    raise NotImplementedError(t)


# ---------------------------------------------------------------------------
# Token structure.  A random-weight 32-layer quantised network is chaotic: two
# correct CPU implementations that differ only in fp32 summation order end up
# with LogitComparer similarity ~0.7 (measured; DESIGN.md "synthetic weights"),
# because its top-10 logits are tightly packed in a flat distribution.  Trained
# LMs have peaked next-token distributions.  The synthetic model gets one:
# a per-token direction B[t] (unit-variance Gaussian) is the embedding of t,
# and output row t' carries sum_k alpha/sqrt(k) * B[t'-k], k = 1..10, on top of
# the random part -- after token t the model "prefers" t+1 > t+2 > ... > t+10.
# ---------------------------------------------------------------------------
_BCHUNK = 1024


def _token_dirs(seed: int, lo: int, hi: int, V: int, d: int) -> np.ndarray:
    """B[t mod V] for t in [lo, hi) (lo may be negative); float32 (hi-lo, d)."""
    out = np.empty((hi - lo, d), np.float32)
    t = lo
    while t < hi:
        tm = t % V
        c = tm // _BCHUNK
        base = c * _BCHUNK
        rows = min(_BCHUNK, V - base)
        blk = _rng(seed, f"tokdir:{c}").standard_normal((rows, d), dtype=np.float32)
        take = min(hi - t, base + rows - tm)
        out[t - lo:t - lo + take] = blk[tm - base:tm - base + take]
        t += take
    return out


def _init_params(cfg):
    env = dict(kv.split("=") for kv in (cfg.init + "," + os.environ.get("BLAMA_SYNTH_INIT", "")).split(",") if kv)
    p = {"base": 0.03, "qk": 0.01, "resid": 0.03 / np.sqrt(2.0 * cfg.n_layer), "embd": 8.0,
         "alpha": 0.01, "nsucc": 10}
    if cfg.arch == "gpt2" or cfg.tied_head:
        p["embd"] = 1.0   # the embedding is also the (tied) output head: logits O(sqrt(d))
    for k, v in env.items():
        p[k] = float(v)
    return p


def _fill_structured(cfg, seed, name, t, view, P):
    V, d = cfg.n_vocab, cfg.n_embd
    be, bb = gguf.GGML_BLOCK[t]
    row_b = d // be * bb
    rows = view.reshape(V, row_b)
    CH = 2048
    ns = int(P["nsucc"])

    def chunk(a):
        b = min(V, a + CH)
        if name == "token_embd.weight":
            X = _token_dirs(seed, a, b, V, d) * np.float32(P["embd"])
        else:
            # chunk 0 draws from the tensor's own stream (as every small-vocab model always
            # did); later chunks from streams of their own, so chunks fill in parallel
            rng = _rng(seed, name) if a == 0 else _rng(seed, f"{name}:{a}")
            X = rng.standard_normal((b - a, d), dtype=np.float32) * np.float32(P["base"])
            Bw = _token_dirs(seed, a - ns, b, V, d)
            for k in range(1, ns + 1):
                X += np.float32(P["alpha"] / np.sqrt(k)) * Bw[ns - k:ns - k + (b - a)]
        rows[a:b] = quantize_rows(X, t).reshape(b - a, row_b)

    starts = list(range(0, V, CH))
    if len(starts) == 1:
        chunk(0)
        return
    from concurrent.futures import ThreadPoolExecutor   # numpy releases the GIL in these ops
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        list(ex.map(chunk, starts))


def vocab_tokens(n_vocab: int):
    toks = ["<unk>", "<s>", "</s>"] + ["<0x%02X>" % i for i in range(256)]
    toks += ["▁t%d" % i for i in range(n_vocab - len(toks))]
    return toks[:n_vocab]


RESIDUAL_OUT = ("attn_output.weight", "ffn_down.weight", "ffn_down_exps.weight")


def _init_std(P, name):
    if name.endswith(("attn_q.weight", "attn_k.weight")):
        return P["qk"]      # attention scores O(1): softmax not saturated
    if name.endswith(RESIDUAL_OUT):
        return P["resid"]   # residual branches scaled by 1/sqrt(2 n_layer)
    return P["base"]


BPE_CORPUS = [
    "The quick brown fox jumps over the lazy dog. It's a test, isn't it? We'll see.",
    "Verification sessions run concurrently on every replica of the model.",
    "request number 0 1 2 3 4 5 6 7 8 9 10 11 12 13 14 15 and 3.14159 pies",
    "Hello world! Numbers 1 22 333 4444, naive cafe, resume -- quotes and text.",
]


def bpe_vocab(n_vocab: int, n_merges_vocab: int = 800) -> dict:
    """A Llama-3-shaped byte-level BPE vocabulary of exactly n_vocab entries ("gpt2" tokenizer,
    pre-tokenizer "llama-bpe"): a BPE model trained here with HuggingFace `tokenizers` (the
    byte alphabet and up to n_merges_vocab pieces with their merges), then
    <|begin_of_text|> / <|end_of_text|> / <|eot_id|> and <|reserved_special_token_i|> control
    tokens up to n_vocab, as Llama-3's 128256-entry vocabulary ends in 256 reserved specials.
    Returns tokens, token types, merges, bos/eos ids and the trained `tokenizers.Tokenizer`
    (which encodes prompts exactly as the host mirror does, tests/test_tokenizer_bpe.py)."""
    import json
    from tokenizers import Regex, Tokenizer, decoders, models, pre_tokenizers, trainers
    llama3 = (r"(?:'[sS]|'[tT]|'[rR][eE]|'[vV][eE]|'[mM]|'[lL][lL]|'[dD])|[^\r\n\p{L}\p{N}]?\p{L}+|"
              r"\p{N}{1,3}| ?[^\s\p{L}\p{N}]+[\r\n]*|\s*[\r\n]+|\s+(?!\S)|\s+")
    tok = Tokenizer(models.BPE(ignore_merges=True))
    tok.pre_tokenizer = pre_tokenizers.Sequence([
        pre_tokenizers.Split(Regex(llama3), behavior="isolated", invert=False),
        pre_tokenizers.ByteLevel(add_prefix_space=False, trim_offsets=False, use_regex=False)])
    tok.decoder = decoders.ByteLevel()
    trainer = trainers.BpeTrainer(vocab_size=n_merges_vocab, min_frequency=1,
                                  initial_alphabet=pre_tokenizers.ByteLevel.alphabet(), show_progress=False)
    tok.train_from_iterator(BPE_CORPUS * 20, trainer=trainer)
    model = json.loads(tok.to_str())["model"]
    toks = [None] * len(model["vocab"])
    for t, i in model["vocab"].items():
        toks[i] = t
    merges = [m if isinstance(m, str) else " ".join(m) for m in model["merges"]]
    types = [1] * len(toks)
    specials = ["<|begin_of_text|>", "<|end_of_text|>", "<|eot_id|>"]
    k = 0
    while len(toks) + len(specials) < n_vocab:
        specials.append("<|reserved_special_token_%d|>" % k)
        k += 1
    base = len(toks)
    toks += specials
    types += [3] * len(specials)
    assert len(toks) == n_vocab
    return dict(tokens=toks, types=types, merges=merges, pre="llama-bpe", bos=base, eos=base + 1,
                eot=base + 2, tokenizer=tok)


def build_gguf(cfg: LlamaConfig, seed: int = 0, header_only: bool = False, vocab: dict | None = None,
               types_override: dict | None = None) -> np.ndarray:
    """The whole synthetic GGUF file as one uint8 array (header_only: just the
    metadata + tensor table, enough for a vocab-only or no_upload replica load).
    vocab: a byte-level BPE vocabulary from bpe_vocab() instead of the SPM one.
    types_override: name -> ggml type written in place of tensor_types' (header_only: files a
    loader must refuse; a full image: a file with a tensor of another served type)."""
    w = gguf.GGUFWriter()
    arch = cfg.arch
    w.add_str("general.architecture", arch)
    w.add_str("general.name", f"synthetic {cfg.name} {cfg.ftype}")
    w.add_u32("general.file_type", {"Q8_0": 7, "Q4_K_M": 15, "Q5_K_M": 17, "Q6_K": 18,
                                    "Q4_K": 15, "Q5_K": 17, "F16": 1, "Q4_0": 2, "Q5_0": 8}[cfg.ftype])
    w.add_u32(f"{arch}.context_length", cfg.n_ctx_train)
    w.add_u32(f"{arch}.embedding_length", cfg.n_embd)
    w.add_u32(f"{arch}.block_count", cfg.n_layer)
    w.add_u32(f"{arch}.feed_forward_length", cfg.n_ff)
    w.add_u32(f"{arch}.attention.head_count", cfg.n_head)
    if arch == "gpt2":   # LLM_KV_ATTENTION_LAYERNORM_EPS; no RoPE keys
        w.add_f32(f"{arch}.attention.layer_norm_epsilon", cfg.eps)
    else:
        w.add_u32(f"{arch}.attention.head_count_kv", cfg.n_head_kv)
        w.add_f32(f"{arch}.attention.layer_norm_rms_epsilon", cfg.eps)
        w.add_f32(f"{arch}.rope.freq_base", cfg.rope_base)
        w.add_u32(f"{arch}.rope.dimension_count", cfg.rot_dim)
        if cfg.rope_scale > 0 and cfg.rope_scale_legacy:
            w.add_f32(f"{arch}.rope.scale_linear", cfg.rope_scale)
        elif cfg.rope_scale > 0:
            w.add_str(f"{arch}.rope.scaling.type", cfg.rope_scaling_type)
            w.add_f32(f"{arch}.rope.scaling.factor", cfg.rope_scale)
    w.add_u32(f"{arch}.vocab_size", cfg.n_vocab)
    if cfg.n_expert:
        w.add_u32(f"{arch}.expert_count", cfg.n_expert)
        w.add_u32(f"{arch}.expert_used_count", cfg.n_expert_used)
    if cfg.pooling_type >= 0:
        w.add_u32(f"{arch}.pooling_type", cfg.pooling_type)
    if vocab is None:
        w.add_str("tokenizer.ggml.model", "llama")
        toks = vocab_tokens(cfg.n_vocab)
        w.add_array("tokenizer.ggml.tokens", gguf.T_STRING, toks)
        w.add_array("tokenizer.ggml.scores", gguf.T_FLOAT32, [-float(i) for i in range(len(toks))])
        ttype = [2, 3, 3] + [6] * 256 + [1] * (len(toks) - 259)
        w.add_array("tokenizer.ggml.token_type", gguf.T_INT32, ttype[:len(toks)])
        w.add_u32("tokenizer.ggml.bos_token_id", 1)
        w.add_u32("tokenizer.ggml.eos_token_id", 2)
        w.add_u32("tokenizer.ggml.unknown_token_id", 0)
    else:
        assert len(vocab["tokens"]) == cfg.n_vocab
        w.add_str("tokenizer.ggml.model", "gpt2")
        w.add_str("tokenizer.ggml.pre", vocab["pre"])
        w.add_array("tokenizer.ggml.tokens", gguf.T_STRING, vocab["tokens"])
        w.add_array("tokenizer.ggml.token_type", gguf.T_INT32, vocab["types"])
        w.add_array("tokenizer.ggml.merges", gguf.T_STRING, vocab["merges"])
        w.add_u32("tokenizer.ggml.bos_token_id", vocab["bos"])
        w.add_u32("tokenizer.ggml.eos_token_id", vocab["eos"])
        w.add_u32("tokenizer.ggml.eot_token_id", vocab["eot"])
    w.add_bool("tokenizer.ggml.add_bos_token", arch != "gpt2")
    types = tensor_types(cfg)
    shapes = tensor_shapes(cfg)
    if types_override:
        types.update(types_override)
    for name in types:
        w.add_tensor(name, types[name], shapes[name])

    if header_only:
        return np.frombuffer(w.header_bytes()[0], np.uint8).copy()
    P = _init_params(cfg)

    def fill(name, t, shape, view):
        rng = _rng(seed, name)
        if name in ("token_embd.weight", "output.weight"):
            _fill_structured(cfg, seed, name, t, view, P)
            return
        if name == "rope_freqs.weight":
            # every pair, the fast ones included, gets a factor well away from 1 (not Llama-3.1's
            # 1 .. 8 ramp): dropping or mis-indexing the factors then moves every angle
            v = view.view(np.float32)
            v[:] = rng.uniform(0.5, 4.0, v.size).astype(np.float32)
        elif name.endswith("norm.weight"):
            v = view.view(np.float32)
            v[:] = rng.uniform(0.8, 1.2, v.size).astype(np.float32)
        elif name.endswith(".bias"):
            v = view.view(np.float32)
            v[:] = (rng.standard_normal(v.size) * 0.02).astype(np.float32)
        elif name == "position_embd.weight":
            fill_quant(view, t, rng, std=0.1)
        elif name.endswith("ffn_gate_inp.weight"):
            fill_quant(view, t, rng, std=0.05)
        else:
            fill_quant(view, t, rng, std=_init_std(P, name))

    return w.to_bytes(fill=fill)


def small_config(name: str, **kw) -> LlamaConfig:
    return replace(CONFIGS[name], **kw)


def write_cvec_gguf(path, directions) -> None:
    """A control-vector GGUF as llama.cpp's cvector-generator writes it: one tensor direction.N per
    steered layer N >= 1.  directions: {N: vector} or a list of (N or tensor name, array) pairs (a
    list can repeat a layer or carry a malformed entry for the loader's error tests); float32
    arrays are stored as F32, float16 ones as F16, in the array's own shape."""
    w = gguf.GGUFWriter()
    w.add_str("general.architecture", "controlvector")
    w.add_str("controlvector.model_hint", "llama")
    items = directions.items() if isinstance(directions, dict) else directions
    for key, v in items:
        a = np.asarray(v)
        if a.dtype != np.float16:
            a = a.astype(np.float32)
        name = key if isinstance(key, str) else f"direction.{int(key)}"
        w.add_tensor(name, 1 if a.dtype == np.float16 else 0, a.shape[::-1], a)
    with open(path, "wb") as f:
        f.write(w.to_bytes().tobytes())


LORA_TARGETS = ("attn_q", "attn_k", "attn_v", "attn_output", "ffn_gate", "ffn_up", "ffn_down")


def lora_tensors(cfg: LlamaConfig, targets, rank: int, dtype, seed: int, layers=None, std: float = 0.05) -> dict:
    """The pairs of a synthetic adapter: {"blk.L.T.weight": (A [rank][K], B [rows][rank])} of `dtype`
    (float16 or float32), normal(0, std) entries, each tensor from its own generator."""
    shapes = tensor_shapes(cfg)
    out = {}
    for l in (range(cfg.n_layer) if layers is None else layers):
        for t in targets:
            name = f"blk.{l}.{t}.weight"
            K, rows = shapes[name][0], shapes[name][1]
            a = _rng(seed, name + ".lora_a").standard_normal((rank, K)).astype(np.float32) * np.float32(std)
            b = _rng(seed, name + ".lora_b").standard_normal((rows, rank)).astype(np.float32) * np.float32(std)
            out[name] = (a.astype(dtype), b.astype(dtype))
    return out


def write_lora_gguf(dst, cfg: LlamaConfig, targets=LORA_TARGETS, rank: int = 4, alpha: float = 8.0, dtype=np.float16,
                    seed: int = 0, layers=None, std: float = 0.05) -> np.ndarray:
    """A LoRA adapter GGUF as llama.cpp's convert_lora_to_gguf.py writes it (general.type "adapter",
    adapter.type "lora", adapter.lora.alpha, pairs <base tensor>.lora_a ne [K, r] / .lora_b ne
    [r, rows]) over `targets` of `layers` (None: all).  Returns the image as a uint8 array and,
    when dst is a path, writes it there."""
    w = gguf.GGUFWriter()
    w.add_str("general.architecture", cfg.arch)
    w.add_str("general.type", "adapter")
    w.add_str("adapter.type", "lora")
    w.add_f32("adapter.lora.alpha", alpha)
    for name, (a, b) in lora_tensors(cfg, targets, rank, dtype, seed, layers, std).items():
        gt = 1 if a.dtype == np.float16 else 0
        w.add_tensor(name + ".lora_a", gt, a.shape[::-1], a)
        w.add_tensor(name + ".lora_b", gt, b.shape[::-1], b)
    img = w.to_bytes()
    if dst is not None:
        with open(dst, "wb") as f:
            f.write(img.tobytes())
    return img


# ---- BERT encoder models (llm_build_bert: the bge family's shape, F16) ----

@dataclass(frozen=True)
class BertConfig:
    name: str
    n_vocab: int
    n_embd: int
    n_layer: int
    n_head: int
    n_ff: int
    n_ctx_train: int
    eps: float = 1e-12
    pooling_type: int = -1            # >= 0: written as bert.pooling_type (bge: 2, CLS)
    n_token_types: int = 2

    @property
    def head_dim(self):
        return self.n_embd // self.n_head


BERT_CONFIGS = {
    # bge-small-en-v1.5's widths (384 / 12 heads of 32 / 1536) at 2 layers, CLS pooling as bge
    "bert-s": BertConfig("bert-s", 512, 384, 2, 12, 1536, 128, pooling_type=2),
    # head_dim 64, an n_ff that is no multiple of 128 (a partial workgroup of row tiles), no pooling key
    "bert-w": BertConfig("bert-w", 300, 128, 3, 2, 320, 64),
}

BERT_SPECIALS = ("[PAD]", "[UNK]", "[CLS]", "[SEP]")


def bert_vocab(n_vocab: int, words=()) -> dict:
    """A WordPiece vocabulary as convert_hf_to_gguf.py writes BERT's: [PAD] [UNK] [CLS] [SEP], then
    word starts (U+2581 + piece) and bare continuations -- `words` first (a "##x" entry is the
    continuation x, anything else a word start), then punctuation, letters, digits and syllables
    until n_vocab entries."""
    toks = list(BERT_SPECIALS)
    seen = set(toks)

    def put(t):
        if t not in seen and len(toks) < n_vocab:
            seen.add(t)
            toks.append(t)

    for w in words:
        put(w[2:] if w.startswith("##") else "▁" + w)
    for c in ".,!?-'\"()$+":
        put("▁" + c)
    letters = "abcdefghijklmnopqrstuvwxyz"
    for c in letters + "0123456789":
        put("▁" + c)
        put(c)
    put("▁中")
    put("▁文")
    cons, vows = "bcdfghjklmnprstvw", "aeiou"
    for a in cons:
        for b in vows:
            put("▁" + a + b)
            put(a + b)
    for a in cons:
        for b in vows:
            for c in "nrst":
                put("▁" + a + b + c)
                put(a + b + c)
    assert len(toks) == n_vocab, (len(toks), n_vocab)
    types = [3] * len(BERT_SPECIALS) + [1] * (n_vocab - len(BERT_SPECIALS))
    return dict(tokens=toks, types=types, pad=0, unk=1, cls=2, sep=3)


def bert_tensor_shapes(cfg: BertConfig) -> dict:
    d, f = cfg.n_embd, cfg.n_ff
    s = {"token_embd.weight": (d, cfg.n_vocab), "token_types.weight": (d, cfg.n_token_types),
         "position_embd.weight": (d, cfg.n_ctx_train), "token_embd_norm.weight": (d,), "token_embd_norm.bias": (d,)}
    for i in range(cfg.n_layer):
        p = f"blk.{i}."
        for n in ("attn_q", "attn_k", "attn_v", "attn_output"):
            s[p + n + ".weight"] = (d, d)
            s[p + n + ".bias"] = (d,)
        s[p + "attn_output_norm.weight"] = (d,)
        s[p + "attn_output_norm.bias"] = (d,)
        s[p + "ffn_up.weight"] = (d, f)
        s[p + "ffn_up.bias"] = (f,)
        s[p + "ffn_down.weight"] = (f, d)
        s[p + "ffn_down.bias"] = (d,)
        s[p + "layer_output_norm.weight"] = (d,)
        s[p + "layer_output_norm.bias"] = (d,)
    return s


def _bert_std(cfg: BertConfig, name: str) -> float:
    """Scales that keep every LayerNorm input well away from zero variance and no softmax one-hot:
    the LayerNorm'd stream has unit variance, so q and k rows get std 0.6 (scores of std 0.36 after
    the 1 / sqrt(head_dim) scale, as the attention op tests draw them), v, attn_output and ffn_up
    unit-variance outputs, ffn_down an output of the size of its GELU input."""
    d, f = cfg.n_embd, cfg.n_ff
    if name == "token_embd.weight":
        return 0.5
    if name == "token_types.weight":
        return 0.1
    if name == "position_embd.weight":
        return 0.2
    if name.endswith(("attn_q.weight", "attn_k.weight")):
        return 0.6 / np.sqrt(d)
    if name.endswith("ffn_down.weight"):
        return 1.0 / np.sqrt(f)
    return 1.0 / np.sqrt(d)


def build_bert_gguf(cfg: BertConfig, seed: int = 0, vocab: dict | None = None, header_only: bool = False,
                    types: dict | None = None, drop=(), causal=None) -> np.ndarray:
    """A synthetic BERT encoder GGUF (general.architecture "bert", llama.cpp b5187's keys and tensor
    names): F16 matrices and tables, F32 biases and LayerNorms, the WordPiece vocabulary of
    bert_vocab() unless one is given.  types: {tensor name: ggml type} overrides (F32 only, for the
    loader's refusals); drop: tensor names left out; causal: written as bert.attention.causal."""
    vocab = bert_vocab(cfg.n_vocab) if vocab is None else vocab
    assert len(vocab["tokens"]) == cfg.n_vocab
    w = gguf.GGUFWriter()
    w.add_str("general.architecture", "bert")
    w.add_str("general.name", f"synthetic {cfg.name} F16")
    w.add_u32("general.file_type", 1)
    w.add_u32("bert.context_length", cfg.n_ctx_train)
    w.add_u32("bert.embedding_length", cfg.n_embd)
    w.add_u32("bert.block_count", cfg.n_layer)
    w.add_u32("bert.feed_forward_length", cfg.n_ff)
    w.add_u32("bert.attention.head_count", cfg.n_head)
    w.add_f32("bert.attention.layer_norm_epsilon", cfg.eps)
    if causal is not None:
        w.add_bool("bert.attention.causal", causal)
    if cfg.pooling_type >= 0:
        w.add_u32("bert.pooling_type", cfg.pooling_type)
    w.add_str("tokenizer.ggml.model", "bert")
    w.add_array("tokenizer.ggml.tokens", gguf.T_STRING, vocab["tokens"])
    w.add_array("tokenizer.ggml.token_type", gguf.T_INT32, vocab["types"])
    w.add_u32("tokenizer.ggml.token_type_count", cfg.n_token_types)
    w.add_u32("tokenizer.ggml.cls_token_id", vocab["cls"])
    w.add_u32("tokenizer.ggml.seperator_token_id", vocab["sep"])
    w.add_u32("tokenizer.ggml.unknown_token_id", vocab["unk"])
    w.add_u32("tokenizer.ggml.padding_token_id", vocab["pad"])
    shapes = bert_tensor_shapes(cfg)
    ttypes = {n: (F16 if len(s) == 2 else F32) for n, s in shapes.items()}
    ttypes.update(types or {})
    for name, shape in shapes.items():
        if name not in drop:
            w.add_tensor(name, ttypes[name], shape)
    if header_only:
        return np.frombuffer(w.header_bytes()[0], np.uint8).copy()

    def fill(name, t, shape, view):
        rng = _rng(seed, name)
        n = int(np.prod(shape))
        if name.endswith("norm.weight"):
            v = rng.uniform(0.8, 1.2, n)
        elif name.endswith("norm.bias"):
            v = rng.standard_normal(n) * 0.05
        elif name.endswith(".bias"):
            v = rng.standard_normal(n) * 0.05
        else:
            v = rng.standard_normal(n) * _bert_std(cfg, name)
        view[:] = v.astype(np.float16 if t == F16 else np.float32).view(np.uint8)

    return w.to_bytes(fill=fill)
