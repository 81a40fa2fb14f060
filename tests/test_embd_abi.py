"""The embeddings entry points that need no GPU: the model's pooling_type key on a vocab_only
model, the synthetic writer's key, and the null-handle returns of mi_engine.h."""
import dataclasses

import numpy as np

from blama_amd import engine, gguf, synthetic


def _image(pooling_type):
    cfg = dataclasses.replace(synthetic.CONFIGS["tiny-q4_k_m"], pooling_type=pooling_type)
    return synthetic.build_gguf(cfg, seed=5, header_only=True)


def test_pooling_type_key_is_read():
    for pt in (0, 1, 2, 3, 4):
        m = engine.Model(_image(pt), vocab_only=True)
        assert m.pooling_type == pt
        m.close()


def test_absent_key_is_unspecified():
    img = _image(-1)
    assert "llama.pooling_type" not in gguf.GGUFReader(img).kv
    m = engine.Model(img, vocab_only=True)
    assert m.pooling_type == -1
    m.close()


def test_default_config_image_is_unchanged():
    """pooling_type = -1 writes no key: the image of an existing config is the one it always was."""
    cfg = synthetic.CONFIGS["tiny-q4_k_m"]
    assert cfg.pooling_type == -1
    a = synthetic.build_gguf(cfg, seed=5, header_only=True)
    b = _image(1)
    assert b.size > a.size and int(gguf.GGUFReader(b).kv["llama.pooling_type"]) == 1
    assert np.array_equal(a, _image(-1))


def test_gpt2_key_is_read_too():
    cfg = dataclasses.replace(synthetic.CONFIGS["tiny-gpt2-q6_k"], pooling_type=3)
    m = engine.Model(synthetic.build_gguf(cfg, seed=5, header_only=True), vocab_only=True)
    assert m.pooling_type == 3
    m.close()


def test_null_handles():
    L = engine.lib()
    assert L.mi_model_pooling_type(None) == -1
    assert L.mi_ctx_pooling(None) == -1
    assert L.mi_ctx_set_embeddings(None, 1, 0) < 0
    assert engine.last_error()
    assert not L.mi_embeddings(None, -1)
    assert engine.last_error()
