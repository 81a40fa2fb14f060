"""Q4_0 / Q5_0 LLaMA GGUFs at the loader (vocab_only: no GPU): llama-quantize's two classic files
parse with their hparams, type histogram and weight bytes; a k-quant file with one Q5_0 matrix
loads; the types and models that stay unserved are refused with the tensor and the type by name;
every truncation of a good header is refused."""
import ctypes as C
from dataclasses import replace

import numpy as np
import pytest

from blama_amd import engine, gguf, synthetic

F32, Q4_0, Q4_1, Q5_0, Q5_1, Q6_K = 0, 2, 3, 6, 7, 14


def _header(cfg, **kw):
    return synthetic.build_gguf(cfg, header_only=True, **kw)


def _expected_bytes(cfg, override=None):
    types, shapes = synthetic.tensor_types(cfg), synthetic.tensor_shapes(cfg)
    types.update(override or {})
    by_type, streamed = {}, 0
    for n, t in types.items():
        nb = gguf.tensor_nbytes(t, shapes[n])
        by_type[t] = by_type.get(t, 0) + nb
        if n != "token_embd.weight":
            streamed += nb
    return by_type, streamed


def _histogram(m):
    hist = (C.c_int64 * 32)()
    assert engine.lib().mi_model_type_histogram(m.h, hist, 32) >= 0
    return {t: int(hist[t]) for t in range(32) if hist[t]}


@pytest.mark.parametrize("name,base,ftype", [("tiny-q4_0", Q4_0, 2), ("tiny-q5_0", Q5_0, 8),
                                             ("tiny-hd32-q4_0", Q4_0, 2), ("tiny-hd32-q5_0", Q5_0, 8)])
def test_legacy_image_parses(name, base, ftype):
    cfg = synthetic.LEGACY_CONFIGS[name]
    buf = _header(cfg)
    assert int(gguf.GGUFReader(synthetic.build_gguf(cfg)).kv["general.file_type"]) == ftype
    m = engine.Model(buf, vocab_only=True)
    try:
        assert (m.n_vocab, m.n_embd, m.n_layer, m.n_head, m.n_head_kv, m.n_ff, m.n_ctx_train, m.n_expert) == \
            (cfg.n_vocab, cfg.n_embd, cfg.n_layer, cfg.n_head, cfg.n_head_kv, cfg.n_ff, cfg.n_ctx_train, 0)
        by_type, streamed = _expected_bytes(cfg)
        assert set(by_type) == {F32, base, Q6_K}
        # every matrix of the file type, the head Q6_K
        types = synthetic.tensor_types(cfg)
        assert types["output.weight"] == Q6_K
        assert all(t == base for n, t in types.items() if n != "output.weight" and not n.endswith("norm.weight"))
        assert _histogram(m) == by_type
        assert engine.lib().mi_model_weight_bytes(m.h) == streamed
    finally:
        m.close()


def test_q5_0_matrix_inside_a_k_quant_file_loads():
    cfg = synthetic.CONFIGS["tiny-q4_k_m"]
    ov = {"blk.1.ffn_down.weight": Q5_0}
    m = engine.Model(_header(cfg, types_override=ov), vocab_only=True)
    try:
        by_type, streamed = _expected_bytes(cfg, ov)
        assert by_type[Q5_0] == cfg.n_ff * cfg.n_embd // 32 * 22
        assert _histogram(m) == by_type
        assert engine.lib().mi_model_weight_bytes(m.h) == streamed
    finally:
        m.close()


def _refused(buf, *words):
    with pytest.raises(engine.EngineError) as e:
        engine.Model(buf, vocab_only=True)
    for w in words:
        assert w in str(e.value), (w, str(e.value))


@pytest.mark.parametrize("t,tname", [(Q4_1, "Q4_1"), (Q5_1, "Q5_1")])
def test_q4_1_and_q5_1_are_refused(t, tname):
    _refused(_header(synthetic.CONFIGS["tiny-q4_k_m"], types_override={"blk.1.ffn_down.weight": t}),
             "blk.1.ffn_down.weight", tname)
    _refused(_header(synthetic.LEGACY_CONFIGS["tiny-q4_0"], types_override={"blk.0.attn_v.weight": t}),
             "blk.0.attn_v.weight", tname)


def test_legacy_experts_are_refused():
    cfg = replace(synthetic.CONFIGS["tiny-moe-q5_k_m"], ftype="Q4_0")
    _refused(_header(cfg), "_exps.weight", "Q4_0", "MoE")
    moe = synthetic.CONFIGS["tiny-moe-q5_k_m"]
    _refused(_header(moe, types_override={"blk.1.ffn_up_exps.weight": Q5_0}), "blk.1.ffn_up_exps.weight", "Q5_0", "MoE")


def test_legacy_gpt2_is_refused():
    cfg = replace(synthetic.CONFIGS["tiny-gpt2-q6_k"], ftype="Q4_0")
    _refused(_header(cfg), ".weight", "Q4_0", "GPT-2")


def test_legacy_bert_is_refused():
    cfg = synthetic.BERT_CONFIGS["bert-w"]
    buf = synthetic.build_bert_gguf(cfg, header_only=True, types={"blk.1.attn_q.weight": Q5_0})
    _refused(buf, "blk.1.attn_q.weight", "Q5_0", "BERT")


@pytest.mark.parametrize("name", ["tiny-q4_0", "tiny-q5_0"])
def test_every_truncation_is_refused(name):
    buf = _header(synthetic.LEGACY_CONFIGS[name])
    assert engine.Model(buf, vocab_only=True).close() is None
    end = gguf.GGUFReader(buf).pos   # the last byte of the tensor table (what follows is alignment padding)
    assert len(buf) - 32 < end <= len(buf)
    for n in range(end):
        with pytest.raises(engine.EngineError):
            engine.Model(buf[:n].copy(), vocab_only=True)
