"""jina-bert-v2 GGUFs load (vocab_only: no GPU): the hparams, pooling, causal flag and tokenizer of both
synthetic configs, and the loader's refusals, each naming the tensor or the key."""
from dataclasses import replace

import pytest

from blama_amd import engine, synthetic

F32, Q8_0 = synthetic.F32, 8


@pytest.mark.parametrize("name,pooling", [("jina-s", 1), ("jina-h3", -1)])
def test_vocab_only_load(name, pooling):
    cfg = synthetic.JINA_CONFIGS[name]
    m = engine.Model(synthetic.build_jina_gguf(cfg, header_only=True), vocab_only=True)
    try:
        assert (m.n_vocab, m.n_embd, m.n_layer, m.n_head, m.n_ff, m.n_ctx_train) == \
            (cfg.n_vocab, cfg.n_embd, cfg.n_layer, cfg.n_head, cfg.n_ff, 8192)
        assert m.n_head_kv == cfg.n_head and m.n_expert == 0
        assert m.pooling_type == pooling and m.causal_attn == 0 and m.tokenizer == "bert"
    finally:
        m.close()


@pytest.mark.parametrize("kw,msg", [
    (dict(extra={"blk.1.attn_q_norm.weight": (64,)}), r"blk\.1\.attn_q_norm\.weight.*not served"),
    (dict(extra={"blk.0.attn_k_norm.weight": (64,)}), r"blk\.0\.attn_k_norm\.weight.*not served"),
    (dict(extra={"blk.0.attn_norm_2.weight": (128,)}), r"blk\.0\.attn_norm_2\.weight.*not served"),
    (dict(extra={"position_embd.weight": (128, 8192)}), r"position_embd\.weight.*no position table"),
    (dict(drop=("blk.1.attn_k.bias",)), r"missing tensor blk\.1\.attn_k\.bias"),
    (dict(drop=("blk.0.ffn_down.bias",)), r"missing tensor blk\.0\.ffn_down\.bias"),
    (dict(drop=("blk.1.ffn_gate.weight",)), r"missing tensor blk\.1\.ffn_gate\.weight.*gated"),
    (dict(types={"blk.1.ffn_up.weight": F32}), r"blk\.1\.ffn_up\.weight.*F16"),
    (dict(types={"blk.0.attn_v.weight": Q8_0}), r"blk\.0\.attn_v\.weight.*F16"),
    (dict(causal=True), r"jina-bert-v2\.attention\.causal"),
])
def test_refusals_name_the_tensor(kw, msg):
    cfg = synthetic.JINA_CONFIGS["jina-s"]
    with pytest.raises(engine.EngineError, match=msg):
        engine.Model(synthetic.build_jina_gguf(cfg, header_only=True, **kw), vocab_only=True)


def test_head_dim_is_refused():
    cfg = replace(synthetic.JINA_CONFIGS["jina-s"], n_head=8)      # head_dim 16
    with pytest.raises(engine.EngineError, match="head_dim 16"):
        engine.Model(synthetic.build_jina_gguf(cfg, header_only=True), vocab_only=True)
