"""Unquantised F16 LLaMA GGUFs at the loader (vocab_only: no GPU): the all-F16 dense file parses
with its hparams, type histogram and weight bytes; every file the F16 path does not serve is
refused with a message naming the tensor and the reason; a truncated header is refused."""
from dataclasses import replace

import ctypes as C

import numpy as np
import pytest

from blama_amd import engine, synthetic

F32, F16, Q8_0, BF16 = 0, 1, 8, 30


def _header(cfg, **kw):
    return synthetic.build_gguf(cfg, header_only=True, **kw)


def _expected_bytes(cfg):
    types, shapes = synthetic.tensor_types(cfg), synthetic.tensor_shapes(cfg)
    by_type, streamed = {}, 0
    for n, t in types.items():
        nb = int(np.prod(shapes[n])) * (2 if t == F16 else 4)
        by_type[t] = by_type.get(t, 0) + nb
        if n != "token_embd.weight" or cfg.tied_head:
            streamed += nb
    return by_type, streamed


@pytest.mark.parametrize("name", ["tiny-f16", "tiny-f16-hd128", "tiny-rf-f16"])
def test_f16_image_parses(name):
    cfg = synthetic.F16_CONFIGS[name]
    m = engine.Model(_header(cfg), vocab_only=True)
    try:
        assert (m.n_vocab, m.n_embd, m.n_layer, m.n_head, m.n_head_kv, m.n_ff, m.n_ctx_train, m.n_expert) == \
            (cfg.n_vocab, cfg.n_embd, cfg.n_layer, cfg.n_head, cfg.n_head_kv, cfg.n_ff, cfg.n_ctx_train, 0)
        by_type, streamed = _expected_bytes(cfg)
        hist = (C.c_int64 * 32)()
        assert engine.lib().mi_model_type_histogram(m.h, hist, 32) >= 0
        assert {t: int(hist[t]) for t in range(32) if hist[t]} == by_type
        assert set(by_type) == {F32, F16}
        assert engine.lib().mi_model_weight_bytes(m.h) == streamed
    finally:
        m.close()


def _refused(buf, *words):
    with pytest.raises(engine.EngineError) as e:
        engine.Model(buf, vocab_only=True)
    for w in words:
        assert w in str(e.value), (w, str(e.value))


def test_bf16_matrices_are_refused():
    cfg = synthetic.F16_CONFIGS["tiny-f16"]
    _refused(_header(cfg, types_override={n: BF16 for n, t in synthetic.tensor_types(cfg).items() if t == F16}), "BF16", ".weight")
    _refused(_header(cfg, types_override={"blk.1.ffn_up.weight": BF16}), "blk.1.ffn_up.weight", "BF16")


def test_f32_matrices_are_refused():
    cfg = synthetic.F16_CONFIGS["tiny-f16"]
    _refused(_header(cfg, types_override={"blk.0.attn_q.weight": F32}), "blk.0.attn_q.weight", "F32")
    _refused(_header(cfg, types_override={n: F32 for n in synthetic.tensor_types(cfg)}), "F32")


def test_mixed_f16_and_quantised_is_refused():
    cfg = synthetic.F16_CONFIGS["tiny-f16"]
    _refused(_header(cfg, types_override={"blk.1.attn_v.weight": Q8_0}), "blk.1.attn_v.weight", "mixes F16")
    # a quantised file with one F16 layer matrix, and one with an F16 head
    q = synthetic.CONFIGS["tiny-q8_0"]
    _refused(_header(q, types_override={"blk.0.ffn_down.weight": F16}), "mixes F16")
    _refused(_header(q, types_override={"output.weight": F16}), "mixes F16")


def test_f16_moe_is_refused():
    cfg = replace(synthetic.F16_CONFIGS["tiny-f16"], n_expert=4, n_expert_used=2)
    _refused(_header(cfg), "MoE", ".weight")


def test_f16_gpt2_is_refused():
    cfg = replace(synthetic.CONFIGS["tiny-gpt2-q6_k"], ftype="F16")
    _refused(_header(cfg), "GPT-2", ".weight")


def test_shape_outside_the_rules_is_refused():
    cfg = synthetic.F16_CONFIGS["tiny-f16"]
    _refused(_header(replace(cfg, n_ff=776)), "feed_forward_length", "776")
    _refused(_header(replace(cfg, n_vocab=500)), "vocabulary", "500")


def test_lora_on_an_f16_model_is_refused(tmp_path):
    cfg = synthetic.F16_CONFIGS["tiny-f16"]
    m = engine.Model(_header(cfg), vocab_only=True)
    try:
        path = tmp_path / "a.gguf"
        synthetic.write_lora_gguf(path, cfg, rank=4)
        h = engine.lib().mi_lora_load(m.h, str(path).encode())
        assert not h
        assert "F16" in engine.last_error()
    finally:
        m.close()


def test_truncated_image_is_refused():
    buf = _header(synthetic.F16_CONFIGS["tiny-f16"])
    for n in (0, 3, 23, 24, 100, len(buf) // 2, len(buf) - 9):
        with pytest.raises(engine.EngineError):
            engine.Model(buf[:n].copy(), vocab_only=True)
