"""ctypes binding of the C ABI in include/mi_engine.h.

This is the Python-side view of the drop-in boundary (the same entry points a
cgo/JNI/ctypes binding in a host application would declare).  It loads the
in-tree ``blama_amd/libmi_engine.so`` and fails loudly if it is missing: there
is no CPU fallback anywhere in the product path.
"""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# MI_ENGINE_LIB=<name> loads libmi_engine_<name>.so instead: "stamps" is the diagnostic build
# (per-workgroup timestamps), other names are A/B builds of an earlier revision (scripts/ab_build.sh)
_VARIANT = os.environ.get("MI_ENGINE_LIB")
LIB_PATH = os.path.join(_HERE, f"libmi_engine_{_VARIANT}.so" if _VARIANT else "libmi_engine.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "mi_engine.h")

_lib = None


class EngineError(RuntimeError):
    pass


class ModelParams(C.Structure):
    _fields_ = [("device_ordinal", C.c_int32), ("cpu_only", C.c_int32),
                ("vocab_only", C.c_int32), ("no_upload", C.c_int32)]


# llama_pooling_type (mi_engine.h MI_POOLING_*)
POOLING_UNSPECIFIED, POOLING_NONE, POOLING_MEAN, POOLING_CLS, POOLING_LAST, POOLING_RANK = -1, 0, 1, 2, 3, 4

_P = C.c_void_p
_SIGS = {
    "mi_last_error": (C.c_char_p, []),
    "mi_model_load": (_P, [C.c_char_p, C.POINTER(ModelParams)]),
    "mi_model_load_from_memory": (_P, [_P, C.c_size_t, C.POINTER(ModelParams)]),
    "mi_model_free": (None, [_P]),
    "mi_model_n_vocab": (C.c_int32, [_P]),
    "mi_model_n_ctx_train": (C.c_int32, [_P]),
    "mi_model_n_embd": (C.c_int32, [_P]),
    "mi_model_n_layer": (C.c_int32, [_P]),
    "mi_model_n_head": (C.c_int32, [_P]),
    "mi_model_n_head_kv": (C.c_int32, [_P]),
    "mi_model_n_ff": (C.c_int32, [_P]),
    "mi_model_n_expert": (C.c_int32, [_P]),
    "mi_model_rope_freq_scale": (C.c_float, [_P]),
    "mi_model_token_bos": (C.c_int32, [_P]),
    "mi_model_token_eos": (C.c_int32, [_P]),
    "mi_model_add_bos": (C.c_int32, [_P]),
    "mi_model_token_is_eog": (C.c_int32, [_P, C.c_int32]),
    "mi_model_token_text": (C.c_int32, [_P, C.c_int32, C.c_char_p, C.c_int32]),
    "mi_model_n_tokens": (C.c_int32, [_P]),
    "mi_model_token_score": (C.c_float, [_P, C.c_int32]),
    "mi_model_token_type": (C.c_int32, [_P, C.c_int32]),
    "mi_model_tokenizer": (C.c_int32, [_P, C.c_char_p, C.c_int32]),
    "mi_model_meta_str": (C.c_int32, [_P, C.c_char_p, C.c_char_p, C.c_int32]),
    "mi_model_n_merges": (C.c_int32, [_P]),
    "mi_model_merge": (C.c_int32, [_P, C.c_int32, C.c_char_p, C.c_int32]),
    "mi_model_weight_bytes": (C.c_int64, [_P]),
    "mi_model_arena": (C.c_int32, [_P, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    "mi_model_type_histogram": (C.c_int32, [_P, C.POINTER(C.c_int64), C.c_int32]),
    "mi_model_replicate": (C.c_int32, [C.POINTER(_P), C.c_int32]),
    "mi_ctx_create": (_P, [_P, C.c_uint32, C.c_uint32, C.c_uint32]),
    "mi_ctx_free": (None, [_P]),
    "mi_n_ctx": (C.c_uint32, [_P]),
    "mi_n_batch": (C.c_uint32, [_P]),
    "mi_decode": (C.c_int32, [_P, C.POINTER(C.c_int32), C.c_int32, C.c_int32]),
    "mi_topk": (C.c_int32, [_P, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_float)]),
    "mi_gather": (C.c_int32, [_P, C.c_int32, C.POINTER(C.c_int32), C.c_int32, C.POINTER(C.c_float)]),
    "mi_logits": (C.POINTER(C.c_float), [_P, C.c_int32]),
    "mi_gather_rows": (C.c_int32, [_P, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.c_int32, C.POINTER(C.c_float)]),
    "mi_synchronize": (None, [_P]),
    "mi_kv_clear": (None, [_P]),
    "mi_kv_seq_rm": (C.c_int32, [_P, C.c_int32, C.c_int32]),
    "mi_kv_seq_add": (C.c_int32, [_P, C.c_int32, C.c_int32, C.c_int32]),
    "mi_kv_seq_div": (C.c_int32, [_P, C.c_int32, C.c_int32, C.c_int32]),
    "mi_kv_pos_max": (C.c_int32, [_P]),
    "mi_kv_n_cells": (C.c_int32, [_P]),
    "mi_state_size": (C.c_size_t, [_P]),
    "mi_state_get": (C.c_size_t, [_P, _P, C.c_size_t]),
    "mi_state_set": (C.c_size_t, [_P, _P, C.c_size_t]),
    "mi_ctx_apply_cvec": (C.c_int32, [_P, C.POINTER(C.c_float), C.c_size_t, C.c_int32, C.c_int32, C.c_int32]),
    "mi_cvec_load": (C.c_int64, [C.c_char_p, C.c_float, C.POINTER(C.c_float), C.c_size_t, C.POINTER(C.c_int32)]),
    "mi_lora_load": (_P, [_P, C.c_char_p]),
    "mi_lora_load_from_memory": (_P, [_P, C.c_void_p, C.c_size_t]),
    "mi_lora_free": (None, [_P]),
    "mi_lora_alpha": (C.c_float, [_P]),
    "mi_lora_n_pairs": (C.c_int32, [_P]),
    "mi_ctx_set_lora": (C.c_int32, [_P, _P, C.c_float]),
    "mi_ctx_rm_lora": (C.c_int32, [_P, _P]),
    "mi_ctx_clear_lora": (None, [_P]),
    "mi_model_pooling_type": (C.c_int32, [_P]),
    "mi_model_causal_attn": (C.c_int32, [_P]),
    "mi_ctx_set_embeddings": (C.c_int32, [_P, C.c_int32, C.c_int32]),
    "mi_ctx_pooling": (C.c_int32, [_P]),
    "mi_embeddings": (C.POINTER(C.c_float), [_P, C.c_int32]),
    "mi_prof_enable": (C.c_int32, [_P, C.c_int32]),
    "mi_prof_read": (C.c_int32, [_P, C.POINTER(C.c_float), C.c_int32]),
    "mi_prof_ffn_bytes": (C.c_int64, [_P]),
    "mi_decode_path": (C.c_int32, [_P]),
    "mi_batch_path": (C.c_int32, [_P]),
    "mi_op_dgemv": (C.c_int32, [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mi_op_fgemv": (C.c_int32, [C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32,
                                C.c_void_p, C.c_void_p, C.c_void_p]),
    "mi_op_fgemv_bench": (C.c_int32, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_float),
                                      C.POINTER(C.c_int64)]),
    "mi_prof_bytes": (C.c_int64, [_P]),
    "mi_debug_stamps": (C.c_int32, [_P, _P, C.c_int32]),
    "mi_debug_down_quant": (C.c_int32, [_P, C.c_int32]),
    "mi_op_gemv": (C.c_int32, [C.c_int32, C.c_int32, _P, C.c_int32, C.c_int32, _P, _P]),
    "mi_op_dequant": (C.c_int32, [C.c_int32, C.c_int32, _P, C.c_int32, C.c_int32, _P]),
    "mi_op_quantize_q8_K": (C.c_int32, [C.c_int32, _P, C.c_int32, _P, _P, _P]),
    "mi_op_topk": (C.c_int32, [C.c_int32, _P, C.c_int32, C.c_int32, _P, _P]),
    "mi_op_attention": (C.c_int32, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P,
                                    C.c_int32, _P]),
    "mi_op_attn_plan": (C.c_int32, [C.c_int32] * 7 + [_P]),
    "mi_op_mmq_plan": (C.c_int32, [C.c_int32] * 3 + [_P] + [C.c_int32] * 9 + [_P]),
    "mi_op_attention_decode": (C.c_int32, [C.c_int32] * 8 + [_P, _P, _P, _P, C.c_int32, C.c_int32] + [_P] * 6),
    "mi_op_attention_short": (C.c_int32, [C.c_int32] * 6 + [_P] * 6 + [C.c_int32] + [_P] * 4),
    "mi_op_gemv_bench": (C.c_int32, [C.c_int32, C.c_int32, _P, C.c_int32, C.c_int32, C.c_int32,
                                     C.POINTER(C.c_float)]),
    "mi_op_gemm": (C.c_int32, [C.c_int32, C.c_int32, _P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P]),
    "mi_op_attention_batch": (C.c_int32, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                          _P, _P, _P, _P, _P, _P, _P]),
    "mi_op_gemm_bias": (C.c_int32, [C.c_int32, C.c_int32, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, C.c_float,
                                    _P, _P, C.c_int32, _P, _P, _P]),
    "mi_op_router": (C.c_int32, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int32, _P, C.c_float, _P, _P,
                                 _P, _P, _P]),
    "mi_op_moe_group": (C.c_int32, [C.c_int32, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P]),
    "mi_op_moe_gemm": (C.c_int32, [C.c_int32, C.c_int32, C.c_int32, _P, _P, C.c_int32, C.c_int32, C.c_int32,
                                   C.c_int32, _P, C.c_int32, _P, _P]),
    "mi_op_gemm_f16": (C.c_int32, [C.c_int32, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, C.c_int32, _P]),
    "mi_op_attention_enc": (C.c_int32, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P]),
    "mi_op_moe_decode": (C.c_int32, [C.c_int32, C.c_int32, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P,
                                     C.c_float, _P, _P, _P, _P, _P]),
}


def header_symbols(path: str = HEADER_PATH) -> list[str]:
    """Names of the functions include/mi_engine.h declares."""
    txt = open(path).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(mi_[A-Za-z0-9_]+)\s*\(", txt)))


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise EngineError(f"{LIB_PATH} is missing: run __graft_entry__.build() (no CPU fallback exists)")
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGS.items():
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
        _lib = L
    return _lib


def last_error() -> str:
    return (lib().mi_last_error() or b"").decode()


def _check(rc, what):
    if rc is None or (isinstance(rc, int) and rc < 0):
        raise EngineError(f"{what}: {last_error()}")
    return rc


def _ptr(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


class Model:
    """Owns an mi_model (llama_model_load_from_file + llama_model_free)."""

    def __init__(self, source, device: int = 0, vocab_only: bool = False, no_upload: bool = False):
        L = lib()
        p = ModelParams(device, 0, int(vocab_only), int(no_upload))
        if isinstance(source, (str, os.PathLike)):
            h = L.mi_model_load(os.fspath(source).encode(), C.byref(p))
        else:
            if isinstance(source, (bytes, bytearray, memoryview)):
                buf = np.frombuffer(source, np.uint8)
            else:
                buf = np.ascontiguousarray(source, dtype=np.uint8)
            h = L.mi_model_load_from_memory(_ptr(buf), buf.size, C.byref(p))
        if not h:
            raise EngineError(f"model load failed: {last_error()}")
        self.h = h
        self.n_vocab = L.mi_model_n_vocab(h)
        self.n_embd = L.mi_model_n_embd(h)
        self.n_layer = L.mi_model_n_layer(h)
        self.n_ctx_train = L.mi_model_n_ctx_train(h)
        self.n_head = L.mi_model_n_head(h)
        self.n_head_kv = L.mi_model_n_head_kv(h)
        self.n_ff = L.mi_model_n_ff(h)
        self.n_expert = L.mi_model_n_expert(h)
        self.rope_freq_scale = float(L.mi_model_rope_freq_scale(h))

    def close(self):
        if getattr(self, "h", None):
            lib().mi_model_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def weight_bytes(self) -> int:
        return lib().mi_model_weight_bytes(self.h)

    @property
    def arena(self):
        """(device pointer, bytes) of the weight arena (replica broadcast)."""
        p = C.c_void_p()
        n = C.c_size_t()
        _check(lib().mi_model_arena(self.h, C.byref(p), C.byref(n)), "arena")
        return p.value, n.value

    def type_histogram(self) -> dict:
        a = (C.c_int64 * 32)()
        lib().mi_model_type_histogram(self.h, a, 32)
        return {i: int(a[i]) for i in range(32) if a[i]}

    def token_text(self, tok: int) -> str:
        n = lib().mi_model_token_text(self.h, tok, None, 0)
        _check(n, "token_text")
        b = C.create_string_buffer(n + 1)
        lib().mi_model_token_text(self.h, tok, b, n + 1)
        return b.raw[:n].decode("utf-8", errors="replace")

    @property
    def bos(self):
        return lib().mi_model_token_bos(self.h)

    @property
    def eos(self):
        return lib().mi_model_token_eos(self.h)

    def is_eog(self, tok: int) -> bool:
        return lib().mi_model_token_is_eog(self.h, tok) == 1

    @property
    def pooling_type(self) -> int:
        """The GGUF's {arch}.pooling_type (llama_pooling_type), or -1 when it has none."""
        return int(lib().mi_model_pooling_type(self.h))

    @property
    def causal_attn(self) -> int:
        """1: a causal decoder (llama, gpt2); 0: a bidirectional encoder (bert)."""
        return int(lib().mi_model_causal_attn(self.h))

    @property
    def tokenizer(self) -> str:
        """tokenizer.ggml.model of the GGUF ("llama", "gpt2", "bert")."""
        n = lib().mi_model_tokenizer(self.h, None, 0)
        b = C.create_string_buffer(n + 1)
        lib().mi_model_tokenizer(self.h, b, n + 1)
        return b.raw[:n].decode()


class Lora:
    """Owns an mi_lora (llama_adapter_lora_init + llama_adapter_lora_free): a LoRA adapter GGUF
    (a path or an in-memory image) validated against `model`.  A context that was given the
    adapter keeps it alive, so close() while it is still set is safe."""

    def __init__(self, model: Model, source):
        L = lib()
        if isinstance(source, (str, os.PathLike)):
            h = L.mi_lora_load(model.h, os.fspath(source).encode())
        else:
            if isinstance(source, (bytes, bytearray, memoryview)):
                buf = np.frombuffer(source, np.uint8)
            else:
                buf = np.ascontiguousarray(source, dtype=np.uint8)
            h = L.mi_lora_load_from_memory(model.h, _ptr(buf), buf.size)
        if not h:
            raise EngineError(f"lora load failed: {last_error()}")
        self.h = h
        self.model = model
        self.alpha = float(L.mi_lora_alpha(h))
        self.n_pairs = int(L.mi_lora_n_pairs(h))

    def close(self):
        if getattr(self, "h", None):
            lib().mi_lora_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Context:
    """Owns an mi_ctx (llama_init_from_model + llama_free)."""

    def __init__(self, model: Model, n_ctx: int = 0, n_batch: int = 2048, n_ubatch: int = 512):
        h = lib().mi_ctx_create(model.h, n_ctx, n_batch, n_ubatch)
        if not h:
            raise EngineError(f"context creation failed: {last_error()}")
        self.h = h
        self.model = model
        self.n_ctx = lib().mi_n_ctx(h)
        self.n_batch = lib().mi_n_batch(h)

    def close(self):
        if getattr(self, "h", None):
            lib().mi_ctx_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def decode(self, tokens, all_logits: bool = False) -> int:
        """mi_decode; all_logits=True is MI_OUT_ALL (output row i = the distribution after token i)."""
        t = np.ascontiguousarray(tokens, dtype=np.int32)
        rc = lib().mi_decode(self.h, t.ctypes.data_as(C.POINTER(C.c_int32)), t.size, 1 if all_logits else 0)
        _check(rc, "decode")
        return rc

    def topk(self, k: int = 10, row: int = -1):
        ids = np.empty(k, np.int32)
        vals = np.empty(k, np.float32)
        _check(lib().mi_topk(self.h, row, k, ids.ctypes.data_as(C.POINTER(C.c_int32)),
                             vals.ctypes.data_as(C.POINTER(C.c_float))), "topk")
        return ids, vals

    def gather(self, ids, row: int = -1):
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        out = np.empty(ids.size, np.float32)
        _check(lib().mi_gather(self.h, row, ids.ctypes.data_as(C.POINTER(C.c_int32)), ids.size,
                               out.ctypes.data_as(C.POINTER(C.c_float))), "gather")
        return out

    def gather_rows(self, row0: int, ids) -> np.ndarray:
        """ids [n_rows][k] -> logits of rows row0.. at those ids (mi_gather_rows)."""
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        out = np.empty(ids.shape, np.float32)
        _check(lib().mi_gather_rows(self.h, row0, ids.shape[0], ids.ctypes.data_as(C.POINTER(C.c_int32)),
                                    ids.shape[1], out.ctypes.data_as(C.POINTER(C.c_float))), "gather_rows")
        return out

    def logits(self, row: int = -1) -> np.ndarray:
        p = lib().mi_logits(self.h, row)
        if not p:
            raise EngineError(f"logits: {last_error()}")
        return np.ctypeslib.as_array(p, shape=(self.model.n_vocab,)).copy()

    def synchronize(self):
        lib().mi_synchronize(self.h)

    def kv_clear(self):
        lib().mi_kv_clear(self.h)

    def kv_seq_rm(self, p0, p1):
        return _check(lib().mi_kv_seq_rm(self.h, p0, p1), "kv_seq_rm")

    def kv_seq_add(self, p0, p1, delta):
        return _check(lib().mi_kv_seq_add(self.h, p0, p1, delta), "kv_seq_add")

    def kv_seq_div(self, p0, p1, d):
        return _check(lib().mi_kv_seq_div(self.h, p0, p1, d), "kv_seq_div")

    @property
    def pos_max(self):
        return lib().mi_kv_pos_max(self.h)

    @property
    def n_cells(self):
        return lib().mi_kv_n_cells(self.h)

    def state_get(self) -> bytes:
        n = lib().mi_state_size(self.h)
        buf = np.empty(n, np.uint8)
        got = lib().mi_state_get(self.h, _ptr(buf), n)
        if got != n:
            raise EngineError(f"state_get: {last_error()}")
        return buf.tobytes()

    def state_set(self, data: bytes):
        buf = np.frombuffer(data, np.uint8).copy()
        got = lib().mi_state_set(self.h, _ptr(buf), buf.size)
        if got == 0:
            raise EngineError(f"state_set: {last_error()}")

    def apply_cvec(self, data, il_start: int, il_end: int, n_embd: int | None = None):
        """mi_ctx_apply_cvec (llama_apply_adapter_cvec): data holds the directions of layers 1, 2, ...
        back to back; layers il_start..il_end (and no layer past the data, never layer 0) carry theirs
        from the next decode on.  n_embd: the vectors' length (default: the model's)."""
        d = np.ascontiguousarray(data, dtype=np.float32).reshape(-1)
        _check(lib().mi_ctx_apply_cvec(self.h, d.ctypes.data_as(C.POINTER(C.c_float)), d.size,
                                       self.model.n_embd if n_embd is None else n_embd, il_start, il_end), "apply_cvec")

    def clear_cvec(self):
        _check(lib().mi_ctx_apply_cvec(self.h, None, 0, self.model.n_embd, 0, 0), "clear_cvec")

    def set_lora(self, lora: "Lora", scale: float = 1.0):
        """mi_ctx_set_lora (llama_set_adapter_lora): adds the adapter or updates its scale."""
        _check(lib().mi_ctx_set_lora(self.h, lora.h if lora is not None else None, scale), "set_lora")

    def rm_lora(self, lora: "Lora"):
        _check(lib().mi_ctx_rm_lora(self.h, lora.h if lora is not None else None), "rm_lora")

    def clear_lora(self):
        lib().mi_ctx_clear_lora(self.h)

    def set_embeddings(self, on: bool = True, pooling: int = POOLING_UNSPECIFIED):
        """mi_ctx_set_embeddings: from the next decode every pass ends in the embedding rows (no
        logits); pooling -1 resolves to the model's key, else NONE."""
        _check(lib().mi_ctx_set_embeddings(self.h, 1 if on else 0, pooling), "set_embeddings")

    @property
    def pooling(self) -> int:
        """The resolved pooling type (llama_pooling_type(ctx))."""
        return int(lib().mi_ctx_pooling(self.h))

    def embeddings(self, row: int = -1) -> np.ndarray:
        """mi_embeddings: n_embd floats -- pooling NONE: the row of an output token (as logits());
        pooled: the sequence embedding of the last decode call (row 0 or -1)."""
        p = lib().mi_embeddings(self.h, row)
        if not p:
            raise EngineError(f"embeddings: {last_error()}")
        return np.ctypeslib.as_array(p, shape=(self.model.n_embd,)).copy()

    def prof_enable(self, stride: int):
        lib().mi_prof_enable(self.h, stride)

    def prof_read(self, n: int = 64) -> np.ndarray:
        a = np.zeros(n, np.float32)
        k = _check(lib().mi_prof_read(self.h, a.ctypes.data_as(C.POINTER(C.c_float)), n), "prof_read")
        return a[:k]

    @property
    def ffn_bytes(self) -> int:
        return lib().mi_prof_ffn_bytes(self.h)

    def debug_down_quant(self, form: int):
        """Who quantises h for the FFN down launch of the streaming decode step, every layer: 0 a
        dv_quant launch, 1 the down workgroups of 8 waves, 2 those of 16 waves (same bits)."""
        _check(lib().mi_debug_down_quant(self.h, form), "debug_down_quant")

    def decode_path(self) -> int:
        """1: decode steps within 512 cells run on the streaming GEMV (dgemv.hip); 0: gemv_kernel;
        2: an encoder context (bert)."""
        return int(lib().mi_decode_path(self.h))

    def batch_path(self) -> int:
        """The form the most recent decode call took (its first physical batch's): 0 one decode step
        per token, 1 the v_dot4 GEMM, 2 the tiled int8-MFMA GEMM, 3 the short split-K GEMM, 4 the F16
        MFMA GEMM, 5 an encoder pass; -1 before the first call."""
        return int(lib().mi_batch_path(self.h))

    @property
    def prof_bytes(self) -> int:
        """Algorithmic bytes of the launch prof_read last timed (the FFN gate/up GEMV)."""
        return lib().mi_prof_bytes(self.h)


def cvec_load(path, strength: float = 1.0):
    """mi_cvec_load: the direction.N tensors of a control-vector GGUF times strength, as
    (data [max N * n_embd] f32, layer 1 first; n_embd).  Raises EngineError for an invalid file."""
    p = os.fspath(path).encode()
    ne = C.c_int32(0)
    need = lib().mi_cvec_load(p, strength, None, 0, C.byref(ne))
    if need < 0:
        raise EngineError(f"cvec_load: {last_error()}")
    data = np.zeros(need, np.float32)
    got = lib().mi_cvec_load(p, strength, data.ctypes.data_as(C.POINTER(C.c_float)), data.size, C.byref(ne))
    if got != need:
        raise EngineError(f"cvec_load: {last_error()}")
    return data, int(ne.value)


# ---- op-level entry points (parity tests / micro-benchmarks) ----

def op_gemv(type_: int, raw: np.ndarray, rows: int, K: int, x: np.ndarray, device: int = 0) -> np.ndarray:
    raw = np.ascontiguousarray(raw, np.uint8)
    x = np.ascontiguousarray(x, np.float32)
    y = np.empty(rows, np.float32)
    _check(lib().mi_op_gemv(device, type_, _ptr(raw), rows, K, _ptr(x), _ptr(y)), "op_gemv")
    return y


def op_dgemv(role: int, type_: int, raw: np.ndarray, rows: int, K: int, x: np.ndarray, type2: int = -1,
             raw2=None, rows2: int = 0, resid=None, device: int = 0) -> np.ndarray:
    """mi_op_dgemv: the decode step's streaming GEMV launch of `role` (0 Q/K/V without RoPE, 1 residual
    add, 2 SwiGLU pair, 3 store, 4 residual add with x quantised inside the launch, 5 the same in
    16-wave workgroups)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    out_rows = rows + (rows2 if role == 0 and raw2 is not None else 0)
    y = np.empty(out_rows, np.float32)
    r = None if resid is None else np.ascontiguousarray(resid, dtype=np.float32)
    raw = np.ascontiguousarray(raw)
    raw2 = None if raw2 is None else np.ascontiguousarray(raw2)
    rc = lib().mi_op_dgemv(device, role, type_, raw.ctypes.data, rows, K, type2,
                           raw2.ctypes.data if raw2 is not None else None, rows2 if raw2 is not None else 0,
                           _ptr(x), _ptr(r) if r is not None else None, _ptr(y))
    _check(rc, "op_dgemv")
    return y


def op_fgemv(role: int, w: np.ndarray, x: np.ndarray, w2=None, resid=None, device: int = 0) -> np.ndarray:
    """mi_op_fgemv: the F16 decode step's streaming GEMV launch of `role` (0 Q/K/V rows without RoPE,
    1 residual add, 2 SwiGLU pair, 3 store) over float16 matrices w [rows][K] (and w2)."""
    w = np.ascontiguousarray(w, dtype=np.float16)
    rows, K = w.shape
    x = np.ascontiguousarray(x, dtype=np.float32)
    w2 = None if w2 is None else np.ascontiguousarray(w2, dtype=np.float16)
    rows2 = 0 if w2 is None else w2.shape[0]
    y = np.empty(rows + (rows2 if role == 0 else 0), np.float32)
    r = None if resid is None else np.ascontiguousarray(resid, dtype=np.float32)
    rc = lib().mi_op_fgemv(device, role, w.ctypes.data, rows, K, w2.ctypes.data if w2 is not None else None, rows2,
                           _ptr(x), _ptr(r) if r is not None else None, _ptr(y))
    _check(rc, "op_fgemv")
    return y


def op_fgemv_bench(role: int, rows: int, K: int, iters: int = 100, device: int = 0):
    """(median microseconds, matrix bytes) of one fgemv launch of `role` over rows x K F16 matrices."""
    us, nb = C.c_float(), C.c_int64()
    _check(lib().mi_op_fgemv_bench(device, role, rows, K, iters, C.byref(us), C.byref(nb)), "op_fgemv_bench")
    return us.value, nb.value


def op_gemv_bench(type_: int, raw: np.ndarray, rows: int, K: int, iters: int = 100, device: int = 0) -> float:
    raw = np.ascontiguousarray(raw, np.uint8)
    us = C.c_float()
    _check(lib().mi_op_gemv_bench(device, type_, _ptr(raw), rows, K, iters, C.byref(us)), "op_gemv_bench")
    return us.value


def op_dequant(type_: int, raw: np.ndarray, rows: int, K: int, device: int = 0) -> np.ndarray:
    raw = np.ascontiguousarray(raw, np.uint8)
    out = np.empty(rows * K, np.float32)
    _check(lib().mi_op_dequant(device, type_, _ptr(raw), rows, K, _ptr(out)), "op_dequant")
    return out


def op_quantize_q8_K(x: np.ndarray, device: int = 0):
    x = np.ascontiguousarray(x, np.float32)
    K = x.size
    qs = np.empty(K, np.int8)
    d = np.empty(K // 256, np.float32)
    bs = np.empty((K // 256) * 16, np.int32)
    _check(lib().mi_op_quantize_q8_K(device, _ptr(x), K, _ptr(qs), _ptr(d), _ptr(bs)), "op_quantize_q8_K")
    return qs, d, bs


def op_topk(logits: np.ndarray, k: int, device: int = 0):
    logits = np.ascontiguousarray(logits, np.float32)
    ids = np.empty(k, np.int32)
    vals = np.empty(k, np.float32)
    _check(lib().mi_op_topk(device, _ptr(logits), logits.size, k, _ptr(ids), _ptr(vals)), "op_topk")
    return ids, vals


def op_attention(q: np.ndarray, k16: np.ndarray, v16: np.ndarray, n_head_kv: int, cell_pos=None, pos=None,
                 device: int = 0) -> np.ndarray:
    """q: (n_head, hd) f32; k16/v16: (n_cells, n_head_kv*hd) f16 -> (n_head, hd) f32."""
    q = np.ascontiguousarray(q, np.float32)
    n_head, hd = q.shape
    k16 = np.ascontiguousarray(k16, np.float16)
    v16 = np.ascontiguousarray(v16, np.float16)
    n = k16.shape[0]
    cp = np.ascontiguousarray(np.arange(n) if cell_pos is None else cell_pos, np.int32)
    pos = n - 1 if pos is None else pos
    out = np.empty(n_head * hd, np.float32)
    _check(lib().mi_op_attention(device, n_head, n_head_kv, hd, n, _ptr(q), _ptr(k16), _ptr(v16), _ptr(cp), pos,
                                 _ptr(out)), "op_attention")
    return out.reshape(n_head, hd)


ATTN_PLAN_FIELDS = ("kernel", "R", "LPC", "HG", "NWV", "grid_x", "grid_y", "block", "lds", "qsplit")


def op_attn_plan(mode: int, n_head: int, n_head_kv: int, hd: int, n_ctx: int = 512, ntok: int = 1,
                 long_ok: bool = False) -> dict:
    """mi_op_attn_plan: the kernel, template arguments and launch shape a cache-attention launch of
    this mode and head geometry would use, by ATTN_PLAN_FIELDS (needs no GPU)."""
    out = np.zeros(len(ATTN_PLAN_FIELDS), np.int32)
    _check(lib().mi_op_attn_plan(mode, n_head, n_head_kv, hd, n_ctx, ntok, int(long_ok), _ptr(out)), "op_attn_plan")
    return dict(zip(ATTN_PLAN_FIELDS, (int(v) for v in out)))


MMQ_PLAN_FIELDS = ("kernel", "T", "pair", "pre", "gx", "grouped", "nst", "nt", "nrb", "ntb", "kp", "grid_x", "grid_y",
                   "grid_z", "block", "lds")
MMQ_TILED, MMQ_SHORT = 0, 1                                                    # MmqForm
MK_NONE, MK_TILED, MK_SHORT, MK_SHORT1, MK_SHORT1_LEAN = range(5)              # MmqKernel


def op_mmq_plan(form: int, type_: int, rows, npad: int, K: int, pair: bool = False, grp_n: int = 0, grp_max: int = 0,
                ksplit: int = 0, pre: bool = False, gx: bool = False, n_cu: int = 256) -> dict:
    """mi_op_mmq_plan: the kernel, template arguments and launch shape a batch GEMM launch of this
    shape would use, by MMQ_PLAN_FIELDS (needs no GPU).  rows: the rows of each matrix of the launch.
    A shape no kernel serves has kernel MK_NONE and, under "why", the launcher's message."""
    r = np.asarray(list(rows), np.int32)
    out = np.zeros(len(MMQ_PLAN_FIELDS), np.int32)
    _check(lib().mi_op_mmq_plan(form, type_, int(pair), _ptr(r), len(r), npad, K, grp_n, grp_max, ksplit, int(pre), int(gx),
                                n_cu, _ptr(out)), "op_mmq_plan")
    plan = dict(zip(MMQ_PLAN_FIELDS, (int(v) for v in out)))
    if plan["kernel"] == MK_NONE:
        plan["why"] = last_error()
    return plan


ATTN_DECODE_QUANT, ATTN_DECODE_FUSED, ATTN_DECODE_SPLIT, ATTN_BATCH_QUANT, ATTN_BATCH_FUSED = range(5)   # AttnMode
AK_NONE, AK_DEC, AK_FUSED, AK_LONG, AK_SCORES_PV = range(5)                                              # AttnKernel
ATTN_FMT_Q8K, ATTN_FMT_Q80 = 1, 2


def op_attention_decode(mode: int, q: np.ndarray, k16: np.ndarray, v16: np.ndarray, n_head_kv: int, cell: int,
                        cell_pos=None, pos=None, fmt: int = 0, want_f32: bool = True, device: int = 0) -> dict:
    """mi_op_attention_decode: one decode step's attention in `mode` (ATTN_DECODE_*).  q (n_head, hd)
    f32; k16 / v16 (n_ctx, n_head_kv * hd) f16, cells 0 .. cell the context; fmt: ATTN_FMT_Q8K |
    ATTN_FMT_Q80.  Returns a dict: kernel (AK_*), out (n_head * hd,) f32 or None (want_f32 false on a
    quantising mode), and per format asked for q8k (K // 256, 256) int8, bsums (K // 256, 16) int32,
    dk (K // 256,) f32; q80 (K // 32, 32) int8, d0 (K // 32,) f32."""
    q = np.ascontiguousarray(q, np.float32)
    n_head, hd = q.shape
    k16 = np.ascontiguousarray(k16, np.float16)
    v16 = np.ascontiguousarray(v16, np.float16)
    n_ctx, K = k16.shape[0], n_head * hd
    cp = np.ascontiguousarray(np.arange(n_ctx) if cell_pos is None else cell_pos, np.int32)
    if k16.shape != (n_ctx, n_head_kv * hd) or v16.shape != k16.shape or cp.shape != (n_ctx,):
        raise ValueError("op_attention_decode: cache shapes")
    pos = cell if pos is None else pos
    r = {"out": np.empty(K, np.float32) if want_f32 or not fmt else None}
    if fmt & ATTN_FMT_Q8K:
        r.update(q8k=np.empty((K // 256, 256), np.int8), bsums=np.empty((K // 256, 16), np.int32),
                 dk=np.empty(K // 256, np.float32))
    if fmt & ATTN_FMT_Q80:
        r.update(q80=np.empty((K // 32, 32), np.int8), d0=np.empty(K // 32, np.float32))
    ptr = lambda name: None if r.get(name) is None else _ptr(r[name])
    r["kernel"] = _check(lib().mi_op_attention_decode(
        device, mode, n_head, n_head_kv, hd, n_ctx, cell, pos, _ptr(q), _ptr(k16), _ptr(v16), _ptr(cp), fmt,
        int(bool(want_f32)), ptr("out"), ptr("q8k"), ptr("bsums"), ptr("dk"), ptr("q80"), ptr("d0")), "op_attention_decode")
    return r


def op_attention_short(q: np.ndarray, k16: np.ndarray, v16: np.ndarray, n_head_kv: int, tok_cell, tok_pos=None,
                       cell_pos=None, quant: int = 0, device: int = 0) -> dict:
    """mi_op_attention_short: a short batch's attention, op_attention_batch's arguments on the decode
    step's kernels; quant 0 none, 1 Q8_K, 2 Q8_0.  Returns a dict: kernel (AK_*), out (ntok, n_head * hd)
    f32, and with quant q (ntok, K) int8, d (ntok, K // 256 or K // 32) f32 and, for Q8_K, bsums
    (ntok, K // 256, 8) int32 (32-element sums), all in token order."""
    q = np.ascontiguousarray(q, np.float32)
    ntok, n_head, hd = q.shape
    k16 = np.ascontiguousarray(k16, np.float16)
    v16 = np.ascontiguousarray(v16, np.float16)
    n, K = k16.shape[0], n_head * hd
    cp = np.ascontiguousarray(np.arange(n) if cell_pos is None else cell_pos, np.int32)
    tc = np.ascontiguousarray(tok_cell, np.int32)
    tpos = np.ascontiguousarray(tc if tok_pos is None else tok_pos, np.int32)
    if k16.shape != (n, n_head_kv * hd) or v16.shape != k16.shape or cp.shape != (n,) or tc.shape != (ntok,) \
            or tpos.shape != (ntok,):
        raise ValueError("op_attention_short: shapes")
    r = {"out": np.empty((ntok, K), np.float32)}
    if quant:
        r.update(q=np.empty((ntok, K), np.int8), d=np.empty((ntok, K // (256 if quant == 1 else 32)), np.float32))
    if quant == 1:
        r["bsums"] = np.empty((ntok, K // 256, 8), np.int32)
    ptr = lambda name: None if r.get(name) is None else _ptr(r[name])
    r["kernel"] = _check(lib().mi_op_attention_short(
        device, n_head, n_head_kv, hd, n, ntok, _ptr(q), _ptr(k16), _ptr(v16), _ptr(cp), _ptr(tc), _ptr(tpos), quant,
        ptr("out"), ptr("q"), ptr("d"), ptr("bsums")), "op_attention_short")
    return r


def op_gemm(type_: int, raw: np.ndarray, rows: int, K: int, x: np.ndarray, raw_up=None,
            device: int = 0) -> np.ndarray:
    """Prompt-batch GEMM (mmqs up to MI_MMQS_MAX tokens, mmq32 above) of x (ntok, K) f32 ->
    (ntok, rows); with raw_up the gate/up
    SwiGLU pair silu(gate . x) * (up . x)."""
    raw = np.ascontiguousarray(raw, np.uint8)
    x = np.ascontiguousarray(x, np.float32)
    ntok = x.shape[0]
    up = None if raw_up is None else np.ascontiguousarray(raw_up, np.uint8)
    y = np.empty((ntok, rows), np.float32)
    _check(lib().mi_op_gemm(device, type_, _ptr(raw), None if up is None else _ptr(up), rows, K, ntok, _ptr(x),
                            _ptr(y)), "op_gemm")
    return y


GEMM_BIAS_PLAIN, GEMM_BIAS_ADD, GEMM_BIAS_GELU = 0, 1, 2


def op_gemm_bias(type_: int, raw: np.ndarray, rows: int, K: int, x: np.ndarray, bias=None, resid=None,
                 epilogue: int = GEMM_BIAS_PLAIN, norm_w=None, norm_b=None, eps: float = 1e-5, device: int = 0):
    """mi_op_gemm_bias: a GPT-2 prompt-batch projection on the tiled int8-MFMA GEMM.  x (ntok, K) f32
    [layer-normed with norm_w / norm_b] quantised by the batch path, times the rows x K matrix, + bias,
    then the epilogue (0 store, 1 + resid, 2 GELU).  Returns (y (ntok, rows) f32, q (ntok, K) int8,
    d (ntok, K / 256 or K / 32) f32): the output and the quantised activation in token order."""
    raw = np.ascontiguousarray(raw, np.uint8)
    x = np.ascontiguousarray(x, np.float32)
    ntok = x.shape[0]
    opt = lambda a: None if a is None else np.ascontiguousarray(a, np.float32)
    bias, resid, norm_w, norm_b = opt(bias), opt(resid), opt(norm_w), opt(norm_b)
    ptr = lambda a: None if a is None else _ptr(a)
    y = np.empty((ntok, rows), np.float32)
    q = np.empty((ntok, K), np.int8)
    d = np.empty((ntok, K // (32 if type_ in (8, 2, 6) else 256)), np.float32)   # Q8_0 / Q4_0 / Q5_0: per 32
    _check(lib().mi_op_gemm_bias(device, type_, _ptr(raw), rows, K, ntok, _ptr(x), ptr(norm_w), ptr(norm_b), eps,
                                 ptr(bias), ptr(resid), epilogue, _ptr(y), _ptr(q), _ptr(d)), "op_gemm_bias")
    return y, q, d


def op_attention_batch(q: np.ndarray, k16: np.ndarray, v16: np.ndarray, n_head_kv: int, tok_cell, tok_pos=None,
                       cell_pos=None, device: int = 0) -> np.ndarray:
    """q: (ntok, n_head, hd) f32; k16/v16: (n_cells, n_head_kv*hd) f16; token t in cell tok_cell[t] at
    position tok_pos[t] (default: its cell) -> (ntok, n_head, hd) f32 (attn_mfma)."""
    q = np.ascontiguousarray(q, np.float32)
    ntok, n_head, hd = q.shape
    k16 = np.ascontiguousarray(k16, np.float16)
    v16 = np.ascontiguousarray(v16, np.float16)
    n = k16.shape[0]
    cp = np.ascontiguousarray(np.arange(n) if cell_pos is None else cell_pos, np.int32)
    tc = np.ascontiguousarray(tok_cell, np.int32)
    tpos = np.ascontiguousarray(tc if tok_pos is None else tok_pos, np.int32)
    out = np.empty((ntok, n_head, hd), np.float32)
    _check(lib().mi_op_attention_batch(device, n_head, n_head_kv, hd, n, ntok, _ptr(q), _ptr(k16), _ptr(v16),
                                       _ptr(cp), _ptr(tc), _ptr(tpos), _ptr(out)), "op_attention_batch")
    return out


def moe_rows_cap(n: int, E: int) -> int:
    """Rows of the grouped picks' buffers (kernels.h moe_rows_cap): every expert's rows padded to 32."""
    return (n + E * 31 + 31) // 32 * 32


def op_router(x: np.ndarray, norm_w: np.ndarray, w: np.ndarray, eps: float = 1e-5, n_embd: int | None = None,
              part=None, device: int = 0):
    """mi_op_router: x (ntok, x_stride) f32 rows whose first n_embd (default: norm_w's length)
    elements are the token, w (n_expert, n_embd) f32 -> (sel (ntok, 2) i32, selw (ntok, 2) f32,
    x after the call (ntok, x_stride)); part (2, ntok, n_embd): the split-K halves added to x first."""
    x = np.ascontiguousarray(x, np.float32)
    norm_w = np.ascontiguousarray(norm_w, np.float32)
    w = np.ascontiguousarray(w, np.float32)
    ntok, x_stride = x.shape
    n_embd = norm_w.size if n_embd is None else n_embd
    n_expert = w.shape[0]
    p = None if part is None else np.ascontiguousarray(part, np.float32)
    sel = np.empty((ntok, 2), np.int32)
    selw = np.empty((ntok, 2), np.float32)
    x_out = np.empty_like(x)
    _check(lib().mi_op_router(device, n_embd, n_expert, ntok, _ptr(x), x_stride, _ptr(norm_w), eps, _ptr(w),
                              None if p is None else _ptr(p), _ptr(sel), _ptr(selw), _ptr(x_out)), "op_router")
    return sel, selw, x_out


def op_moe_group(sel: np.ndarray, U: int, E: int, cap: int | None = None, device: int = 0):
    """mi_op_moe_group: the picks sel (n,) grouped by expert -> (grp (2E+1,), rows (cap,), rowsel
    (cap,), pos (n,)); cap defaults to moe_rows_cap(n, E).  Unwritten entries hold -2139062144."""
    sel = np.ascontiguousarray(sel, np.int32).reshape(-1)
    n = sel.size
    cap = moe_rows_cap(n, E) if cap is None else cap
    grp = np.empty(2 * max(E, 0) + 1, np.int32)
    rows = np.empty(max(cap, 1), np.int32)
    rowsel = np.empty(max(cap, 1), np.int32)
    pos = np.empty(n, np.int32)
    _check(lib().mi_op_moe_group(device, _ptr(sel), n, U, E, cap, _ptr(grp), _ptr(rows), _ptr(rowsel), _ptr(pos)),
           "op_moe_group")
    return grp, rows, rowsel, pos


def op_moe_gemm(mode: int, type_: int, raw: np.ndarray, n_expert: int, rows: int, K: int, x: np.ndarray,
                sel: np.ndarray, raw_up=None, per_pick: bool = False, device: int = 0) -> np.ndarray:
    """mi_op_moe_gemm: the grouped expert GEMM (mode 0 tiled, 1 short) of sel (ntok, 2) picks over
    raw = n_expert matrices of rows x K; x (ntok, K), or (2 ntok, K) with per_pick -> (2 ntok, rows),
    row i = pick i; with raw_up the gate/up SwiGLU pair."""
    raw = np.ascontiguousarray(raw, np.uint8)
    up = None if raw_up is None else np.ascontiguousarray(raw_up, np.uint8)
    x = np.ascontiguousarray(x, np.float32)
    sel = np.ascontiguousarray(sel, np.int32).reshape(-1, 2)
    ntok = sel.shape[0]
    if x.shape != ((2 * ntok if per_pick else ntok), K):
        raise EngineError(f"op_moe_gemm: x has shape {x.shape}")
    y = np.empty((2 * ntok, rows), np.float32)
    _check(lib().mi_op_moe_gemm(device, mode, type_, _ptr(raw), None if up is None else _ptr(up), n_expert, rows, K,
                                ntok, _ptr(x), 1 if per_pick else 0, _ptr(sel), _ptr(y)), "op_moe_gemm")
    return y


def op_moe_decode(type_: int, gate: np.ndarray, up: np.ndarray, down: np.ndarray, n_expert: int, n_embd: int,
                  n_ff: int, x: np.ndarray, norm_w: np.ndarray, sel, selw, eps: float = 1e-5, addend=None,
                  device: int = 0):
    """mi_op_moe_decode: the decode step's gate/up and down launches for the picks sel (2,) with
    weights selw (2,) -> (h (2, n_ff), x_out (n_embd,))."""
    gate = np.ascontiguousarray(gate, np.uint8)
    up = np.ascontiguousarray(up, np.uint8)
    down = np.ascontiguousarray(down, np.uint8)
    x = np.ascontiguousarray(x, np.float32)
    norm_w = np.ascontiguousarray(norm_w, np.float32)
    sel = np.ascontiguousarray(sel, np.int32)
    selw = np.ascontiguousarray(selw, np.float32)
    a = None if addend is None else np.ascontiguousarray(addend, np.float32)
    h = np.empty((2, n_ff), np.float32)
    x_out = np.empty(n_embd, np.float32)
    _check(lib().mi_op_moe_decode(device, type_, _ptr(gate), _ptr(up), _ptr(down), n_expert, n_embd, n_ff, _ptr(x),
                                  _ptr(norm_w), eps, _ptr(sel), _ptr(selw), None if a is None else _ptr(a), _ptr(h),
                                  _ptr(x_out)), "op_moe_decode")
    return h, x_out


GEMM_F16_NONE, GEMM_F16_BIAS, GEMM_F16_GELU, GEMM_F16_RESID = 0, 1, 2, 3


def op_gemm_f16(w16: np.ndarray, x: np.ndarray, bias=None, resid=None, epilogue: int = GEMM_F16_NONE,
                device: int = 0) -> np.ndarray:
    """mi_op_gemm_f16: w16 (rows, K) float16, x (ntok, K) f32 -> (ntok, rows) f32 after the epilogue
    (0 none, 1 + bias, 2 gelu(. + bias), 3 (. + bias) + resid)."""
    w16 = np.ascontiguousarray(w16, np.float16)
    x = np.ascontiguousarray(x, np.float32)
    rows, K = w16.shape
    ntok = x.shape[0]
    b = None if bias is None else np.ascontiguousarray(bias, np.float32)
    r = None if resid is None else np.ascontiguousarray(resid, np.float32)
    y = np.empty((ntok, rows), np.float32)
    _check(lib().mi_op_gemm_f16(device, _ptr(w16), rows, K, ntok, _ptr(x), None if b is None else _ptr(b),
                                None if r is None else _ptr(r), epilogue, _ptr(y)), "op_gemm_f16")
    return y


def op_attention_enc(q: np.ndarray, k16: np.ndarray, v16: np.ndarray, device: int = 0) -> np.ndarray:
    """mi_op_attention_enc: q (ntok, n_head, hd) f32, k16 / v16 (ntok, n_head * hd) f16 -> (ntok, n_head,
    hd) f32: every token over all ntok tokens."""
    q = np.ascontiguousarray(q, np.float32)
    ntok, n_head, hd = q.shape
    k16 = np.ascontiguousarray(k16, np.float16)
    v16 = np.ascontiguousarray(v16, np.float16)
    out = np.empty((ntok, n_head, hd), np.float32)
    _check(lib().mi_op_attention_enc(device, n_head, hd, ntok, _ptr(q), _ptr(k16), _ptr(v16), _ptr(out)),
           "op_attention_enc")
    return out
