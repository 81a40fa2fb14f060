"""IQ4_XS / IQ4_NL LLaMA GGUFs at the loader (vocab_only: no GPU): llama-quantize's two files parse
with their hparams, type histogram and weight bytes (136 B per superblock / 18 B per block); a k-quant
file with one such matrix loads; the types in MoE, GPT-2 and BERT models stay refused with the tensor
and the type by name."""
from dataclasses import replace

import pytest

from blama_amd import engine, gguf, synthetic
from test_legacy_quant_load import _expected_bytes, _header, _histogram, _refused

F32, Q5_K, Q6_K, IQ4_NL, IQ4_XS = 0, 13, 14, 20, 23
PER_256 = {IQ4_NL: 8 * 18, IQ4_XS: 136}


@pytest.mark.parametrize("name,t,ftype", [("tiny-iq4_xs", IQ4_XS, 30), ("tiny-iq4_nl", IQ4_NL, 25)])
def test_iq4_image_parses(name, t, ftype):
    cfg = synthetic.IQ4_CONFIGS[name]
    buf = _header(cfg)
    rd = gguf.GGUFReader(buf)
    assert int(rd.kv["general.file_type"]) == ftype
    # llama-quantize's mix: V (GQA 4) and the first layer's ffn_down Q5_K, head Q6_K, the table of the type
    types = {n: x.type for n, x in rd.tensors.items()}
    assert types["blk.1.attn_v.weight"] == types["blk.0.ffn_down.weight"] == Q5_K
    assert types["blk.1.ffn_down.weight"] == types["token_embd.weight"] == types["blk.0.attn_q.weight"] == t
    m = engine.Model(buf, vocab_only=True)
    try:
        assert (m.n_vocab, m.n_embd, m.n_layer, m.n_head, m.n_head_kv, m.n_ff, m.n_expert) == \
            (cfg.n_vocab, cfg.n_embd, cfg.n_layer, cfg.n_head, cfg.n_head_kv, cfg.n_ff, 0)
        by_type, streamed = _expected_bytes(cfg)
        assert set(by_type) == {F32, t, Q5_K, Q6_K}
        assert by_type[t] == sum(x.shape[0] * x.shape[1] for x in rd.tensors.values() if x.type == t) // 256 * PER_256[t]
        assert _histogram(m) == by_type
        assert engine.lib().mi_model_weight_bytes(m.h) == streamed
    finally:
        m.close()


@pytest.mark.parametrize("t", [IQ4_XS, IQ4_NL])
def test_iq4_matrix_inside_a_k_quant_file_loads(t):
    cfg = synthetic.CONFIGS["tiny-q4_k_m"]
    ov = {"blk.1.ffn_down.weight": t}
    m = engine.Model(_header(cfg, types_override=ov), vocab_only=True)
    try:
        by_type, streamed = _expected_bytes(cfg, ov)
        assert by_type[t] == cfg.n_ff * cfg.n_embd // 256 * PER_256[t]
        assert _histogram(m) == by_type
        assert engine.lib().mi_model_weight_bytes(m.h) == streamed
    finally:
        m.close()


@pytest.mark.parametrize("t,tname", [(IQ4_XS, "IQ4_XS"), (IQ4_NL, "IQ4_NL")])
def test_iq4_experts_gpt2_and_bert_are_refused(t, tname):
    moe = synthetic.CONFIGS["tiny-moe-q5_k_m"]
    _refused(_header(moe, types_override={"blk.1.ffn_up_exps.weight": t}), "blk.1.ffn_up_exps.weight", tname, "MoE")
    _refused(_header(replace(synthetic.CONFIGS["tiny-gpt2-q6_k"], ftype=tname)), ".weight", tname, "GPT-2")
    bert = synthetic.build_bert_gguf(synthetic.BERT_CONFIGS["bert-w"], header_only=True, types={"blk.1.attn_q.weight": t})
    _refused(bert, "blk.1.attn_q.weight", tname, "BERT")
