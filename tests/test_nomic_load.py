"""nomic-bert GGUFs load (vocab_only: no GPU): the hparams, pooling, causal flag and tokenizer of both
synthetic configs, and the loader's refusals, each naming the tensor or the key."""
from dataclasses import replace

import pytest

from blama_amd import engine, synthetic

F16, F32 = synthetic.F16, synthetic.F32


@pytest.mark.parametrize("name,pooling", [("nomic-s", 1), ("nomic-h32", -1)])
def test_vocab_only_load(name, pooling):
    cfg = synthetic.NOMIC_CONFIGS[name]
    m = engine.Model(synthetic.build_nomic_gguf(cfg, header_only=True), vocab_only=True)
    try:
        assert (m.n_vocab, m.n_embd, m.n_layer, m.n_head, m.n_ff, m.n_ctx_train) == \
            (cfg.n_vocab, cfg.n_embd, cfg.n_layer, cfg.n_head, cfg.n_ff, cfg.n_ctx_train)
        assert m.n_head_kv == cfg.n_head and m.n_expert == 0
        assert m.pooling_type == pooling
        assert m.causal_attn == 0
        assert m.tokenizer == "bert"
        assert m.token_text(2) == "[CLS]" and m.token_text(3) == "[SEP]"
    finally:
        m.close()


@pytest.mark.parametrize("kw,msg", [
    (dict(types={"blk.1.attn_qkv.weight": F32}), r"blk\.1\.attn_qkv\.weight.*F16"),
    (dict(types={"blk.0.ffn_gate.weight": F32}), r"blk\.0\.ffn_gate\.weight.*F16"),
    (dict(drop=("blk.1.ffn_gate.weight",)), r"missing tensor blk\.1\.ffn_gate\.weight.*gated"),
    (dict(extra={"blk.0.attn_qkv.bias": (3 * 128,)}), r"blk\.0\.attn_qkv\.bias.*bias is not served"),
    (dict(extra={"blk.1.ffn_down.bias": (128,)}), r"blk\.1\.ffn_down\.bias.*bias is not served"),
    (dict(extra={"position_embd.weight": (128, 2048)}), r"position_embd\.weight.*no position table"),
    (dict(rope_scaling="yarn"), r"rope\.scaling\.type 'yarn'"),
])
def test_refusals_name_the_tensor(kw, msg):
    cfg = synthetic.NOMIC_CONFIGS["nomic-s"]
    with pytest.raises(engine.EngineError, match=msg):
        engine.Model(synthetic.build_nomic_gguf(cfg, header_only=True, **kw), vocab_only=True)


@pytest.mark.parametrize("bad,msg", [(dict(n_rot=66), "even and at most head_dim"), (dict(n_rot=24), "multiple of 16"),
                                     (dict(n_head=8), "head_dim"), (dict(n_ff=336), "feed_forward_length")])
def test_unserved_geometry_is_refused(bad, msg):
    cfg = replace(synthetic.NOMIC_CONFIGS["nomic-s"], **bad)
    with pytest.raises(engine.EngineError, match=msg):
        engine.Model(synthetic.build_nomic_gguf(cfg, header_only=True), vocab_only=True)
