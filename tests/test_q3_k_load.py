"""Q3_K LLaMA GGUFs at the loader (vocab_only: no GPU): the Q3_K_S and Q3_K_M files parse with their
hparams, type histogram and weight bytes at 110 B per superblock; a k-quant file with one Q3_K matrix
loads; Q3_K in MoE, GPT-2 and BERT models and Q2_K stay refused with the tensor and the type by name."""
from dataclasses import replace

import pytest

from blama_amd import engine, gguf, synthetic
from test_legacy_quant_load import _expected_bytes, _header, _histogram, _refused

F32, Q2_K, Q3_K, Q4_K, Q5_K, Q6_K = 0, 10, 11, 12, 13, 14


@pytest.mark.parametrize("name,ftype,kinds", [("tiny-q3_k_s", 11, {F32, Q3_K, Q6_K}),
                                              ("tiny-q3_k_m", 12, {F32, Q3_K, Q4_K, Q5_K, Q6_K})])
def test_q3_k_image_parses(name, ftype, kinds):
    cfg = synthetic.Q3K_CONFIGS[name]
    buf = _header(cfg)
    assert int(gguf.GGUFReader(buf).kv["general.file_type"]) == ftype
    m = engine.Model(buf, vocab_only=True)
    try:
        assert (m.n_vocab, m.n_embd, m.n_layer, m.n_head, m.n_head_kv, m.n_ff, m.n_expert) == \
            (cfg.n_vocab, cfg.n_embd, cfg.n_layer, cfg.n_head, cfg.n_head_kv, cfg.n_ff, 0)
        by_type, streamed = _expected_bytes(cfg)
        assert set(by_type) == kinds
        q3 = [t for t in gguf.GGUFReader(buf).tensors.values() if t.type == Q3_K]
        assert by_type[Q3_K] == sum(t.shape[0] * t.shape[1] for t in q3) // 256 * 110
        assert _histogram(m) == by_type
        assert engine.lib().mi_model_weight_bytes(m.h) == streamed
    finally:
        m.close()


def test_q3_k_matrix_inside_a_k_quant_file_loads():
    cfg = synthetic.CONFIGS["tiny-q4_k_m"]
    ov = {"blk.1.ffn_down.weight": Q3_K}
    m = engine.Model(_header(cfg, types_override=ov), vocab_only=True)
    try:
        by_type, streamed = _expected_bytes(cfg, ov)
        assert by_type[Q3_K] == cfg.n_ff * cfg.n_embd // 256 * 110
        assert _histogram(m) == by_type
        assert engine.lib().mi_model_weight_bytes(m.h) == streamed
    finally:
        m.close()


def test_q3_k_experts_gpt2_and_bert_are_refused():
    moe = synthetic.CONFIGS["tiny-moe-q5_k_m"]
    _refused(_header(moe, types_override={"blk.1.ffn_up_exps.weight": Q3_K}), "blk.1.ffn_up_exps.weight", "Q3_K", "MoE")
    _refused(_header(replace(synthetic.CONFIGS["tiny-gpt2-q6_k"], ftype="Q3_K_S")), ".weight", "Q3_K", "GPT-2")
    bert = synthetic.build_bert_gguf(synthetic.BERT_CONFIGS["bert-w"], header_only=True, types={"blk.1.attn_q.weight": Q3_K})
    _refused(bert, "blk.1.attn_q.weight", "Q3_K", "BERT")


def test_q2_k_is_still_refused():
    _refused(_header(synthetic.CONFIGS["tiny-q4_k_m"], types_override={"blk.1.ffn_down.weight": Q2_K}),
             "blk.1.ffn_down.weight", "Q2_K", "Q3_K")
    _refused(_header(synthetic.Q3K_CONFIGS["tiny-q3_k_s"], types_override={"blk.0.attn_v.weight": Q2_K}),
             "blk.0.attn_v.weight", "Q2_K")
