"""BERT encoder GGUFs load (vocab_only: no GPU): the hparams, the pooling key, the causal flag and
the tokenizer name of both synthetic configs; a causal BERT is refused."""
import pytest

from blama_amd import engine, synthetic


@pytest.mark.parametrize("name,pooling", [("bert-s", 2), ("bert-w", -1)])
def test_vocab_only_load(name, pooling):
    cfg = synthetic.BERT_CONFIGS[name]
    m = engine.Model(synthetic.build_bert_gguf(cfg, header_only=True), vocab_only=True)
    try:
        assert (m.n_vocab, m.n_embd, m.n_layer, m.n_head, m.n_ff, m.n_ctx_train) == \
            (cfg.n_vocab, cfg.n_embd, cfg.n_layer, cfg.n_head, cfg.n_ff, cfg.n_ctx_train)
        assert m.n_head_kv == cfg.n_head and m.n_expert == 0
        assert m.pooling_type == pooling
        assert m.causal_attn == 0
        assert m.tokenizer == "bert"
        assert m.token_text(0) == "[PAD]" and m.token_text(2) == "[CLS]" and m.token_text(3) == "[SEP]"
    finally:
        m.close()


def test_causal_attn_of_the_decoders():
    for name in ("tiny-q8_0", "tiny-gpt2-q6_k"):
        m = engine.Model(synthetic.build_gguf(synthetic.CONFIGS[name], header_only=True), vocab_only=True)
        assert m.causal_attn == 1
        m.close()
    assert engine.lib().mi_model_causal_attn(None) == -1


def test_causal_bert_is_refused():
    cfg = synthetic.BERT_CONFIGS["bert-w"]
    with pytest.raises(engine.EngineError, match="attention.causal"):
        engine.Model(synthetic.build_bert_gguf(cfg, header_only=True, causal=True), vocab_only=True)
    m = engine.Model(synthetic.build_bert_gguf(cfg, header_only=True, causal=False), vocab_only=True)
    assert m.causal_attn == 0
    m.close()


def test_unserved_geometry_is_refused():
    from dataclasses import replace
    cfg = synthetic.BERT_CONFIGS["bert-w"]
    for bad, what in ((replace(cfg, n_embd=144, n_head=3), "embedding_length"),
                      (replace(cfg, n_ff=336), "feed_forward_length"),
                      (replace(cfg, n_head=8), "head_dim")):
        with pytest.raises(engine.EngineError, match=what):
            engine.Model(synthetic.build_bert_gguf(bad, header_only=True), vocab_only=True)
