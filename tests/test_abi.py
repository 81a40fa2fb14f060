"""The C-ABI library loads on a CPU-only host and exports every symbol the
public header declares (no compute is called without a GPU)."""
import ctypes
import os

from blama_amd import engine


def test_library_exists_and_loads():
    assert os.path.exists(engine.LIB_PATH), "run __graft_entry__.build() first"
    L = engine.lib()
    assert L is not None


def test_header_symbols_exported():
    syms = engine.header_symbols()
    assert len(syms) >= 40
    L = ctypes.CDLL(engine.LIB_PATH)
    missing = [s for s in syms if not hasattr(L, s)]
    assert not missing, missing


def test_binding_covers_header():
    assert set(engine.header_symbols()) == set(engine._SIGS)


def test_vocab_only_load_needs_no_gpu():
    """Model::Params{.vocabOnly=true} parses metadata + vocab only (t-integration.cpp:25-43)."""
    from blama_amd import synthetic
    buf = synthetic.build_gguf(synthetic.CONFIGS["tiny-q8_0"])
    m = engine.Model(buf, vocab_only=True)
    assert m.n_vocab == 384 and m.n_embd == 256 and m.n_ctx_train == 256
    assert m.token_text(1) == "<s>" and m.token_text(2) == "</s>"
    assert m.bos == 1 and m.eos == 2 and m.is_eog(2) and not m.is_eog(5)


def _header(**kw):
    from blama_amd import synthetic
    return synthetic.build_gguf(synthetic.small_config("tiny-q4_k_m", **kw), header_only=True)


def test_rope_scaling_keys():
    """freq_scale as llama.cpp b5187 derives it: rope.scaling.factor, else rope.scale_linear,
    1 / factor; rope.scaling.type absent or "linear" uses it, "none" runs unscaled."""
    def scale(**kw):
        m = engine.Model(_header(**kw), vocab_only=True)
        try:
            return m.rope_freq_scale
        finally:
            m.close()
    assert scale() == 1.0
    assert scale(rope_scale=4.0) == 0.25
    assert scale(rope_scale=4.0, rope_scale_legacy=True) == 0.25
    assert scale(rope_scale=8.0, rope_scaling_type="none") == 1.0


def test_unimplemented_rope_scaling_type_is_a_load_error():
    """YaRN / LongRoPE need an ext_factor / per-layer factors the kernels do not implement: the
    load names the type instead of running the model as linear."""
    import pytest
    for typ in ("yarn", "longrope"):
        with pytest.raises(engine.EngineError, match=f"rope.scaling.type '{typ}'"):
            engine.Model(_header(rope_scale=4.0, rope_scaling_type=typ), vocab_only=True)


def test_oracles_follow_the_same_rope_scaling_rule():
    """tests/util.oracle_from_gguf reads the keys as the engine does; the C oracle, whose rope()
    knows neither a scale nor frequency factors, refuses such an image instead of ignoring them."""
    import pytest
    import ggml_cpu
    from blama_amd import synthetic
    from util import oracle_from_gguf
    hp = lambda **kw: oracle_from_gguf(_header(**kw)).hp   # noqa: E731
    assert hp().freq_scale == 1.0
    assert hp(rope_scale=4.0).freq_scale == 0.25
    assert hp(rope_scale=4.0, rope_scale_legacy=True).freq_scale == 0.25
    assert hp(rope_scale=8.0, rope_scaling_type="none").freq_scale == 1.0
    with pytest.raises(NotImplementedError, match="yarn"):
        hp(rope_scale=4.0, rope_scaling_type="yarn")
    for name, what in (("tiny-rf-q4_k_m", "rope_freqs"), ("tiny-prot-q4_k_m", "freq_scale")):
        with pytest.raises(NotImplementedError, match=what):
            ggml_cpu.Model(synthetic.build_gguf(synthetic.CONFIGS[name], seed=5), n_ctx=8)


def test_errors_are_reported_not_thrown():
    import pytest
    with pytest.raises(engine.EngineError, match="not a GGUF"):
        engine.Model(b"NOPE" + bytes(64), vocab_only=True)
    with pytest.raises(engine.EngineError, match="cannot open"):
        engine.Model("/nonexistent/model.gguf")
