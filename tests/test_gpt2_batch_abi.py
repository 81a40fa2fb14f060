"""CPU: the header and the binding declare the GPT-2 batch work's entry points, and a vocab-only
GPT-2 model still loads (no MFMA-order copy, no context)."""
import ctypes

from blama_amd import engine, synthetic


def test_header_and_binding_declare_the_entry_points():
    syms = engine.header_symbols()
    for name in ("mi_batch_path", "mi_op_gemm_bias"):
        assert name in syms
        assert name in engine._SIGS
        assert hasattr(ctypes.CDLL(engine.LIB_PATH), name)
    assert len(engine._SIGS["mi_op_gemm_bias"][1]) == 16
    assert engine.lib().mi_batch_path(None) == -1   # a null context
    assert callable(engine.Context.batch_path) and callable(engine.op_gemm_bias)


def test_vocab_only_gpt2_model_loads():
    cfg = synthetic.CONFIGS["tiny-gpt2-q6_k"]
    m = engine.Model(synthetic.build_gguf(cfg), vocab_only=True)
    try:
        assert m.n_vocab == cfg.n_vocab and m.n_embd == cfg.n_embd and m.n_ctx_train == cfg.n_ctx_train
    finally:
        m.close()
