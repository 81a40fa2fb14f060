"""mi_lora_load / mi_lora_load_from_memory (llama_adapter_lora_init, LoraAdapter.cpp:12-19) on
vocab_only models, which parse and validate an adapter without a GPU: a good file reports alpha and
its pairs, and every check of llama-adapter.cpp plus the scope limits refuses its file with a
message naming the tensor or the reason."""
import numpy as np
import pytest

from blama_amd import engine, gguf, synthetic

CFG = "tiny-q4_k_m"


@pytest.fixture(scope="module")
def model():
    m = engine.Model(synthetic.build_gguf(synthetic.CONFIGS[CFG], seed=1, header_only=True), vocab_only=True)
    yield m
    m.close()


def _image(pairs, general_type="adapter", adapter_type="lora", arch="llama", alpha=8.0):
    """An adapter GGUF from (tensor name, array) pairs, as given (malformed on purpose)."""
    w = gguf.GGUFWriter()
    w.add_str("general.architecture", arch)
    if general_type is not None:
        w.add_str("general.type", general_type)
    if adapter_type is not None:
        w.add_str("adapter.type", adapter_type)
    w.add_f32("adapter.lora.alpha", alpha)
    for name, a in pairs:
        a = np.asarray(a)
        gt = {np.dtype(np.float32): 0, np.dtype(np.float16): 1, np.dtype(np.uint16): 30}[a.dtype]   # uint16: stored as BF16
        w.add_tensor(name, gt, a.shape[::-1], a)
    return w.to_bytes()


def _ab(base="blk.1.attn_q.weight", r=4, K=256, rows=256, dt=np.float16, rb=None):
    rng = np.random.default_rng(0)
    return [(base + ".lora_a", rng.standard_normal((r, K)).astype(dt)),
            (base + ".lora_b", rng.standard_normal((rows, r if rb is None else rb)).astype(dt))]


def test_good_file_reports_alpha_and_pairs(model, tmp_path):
    cfg = synthetic.CONFIGS[CFG]
    path = str(tmp_path / "a.gguf")
    img = synthetic.write_lora_gguf(path, cfg, ("attn_q", "ffn_down"), 4, 8.0, np.float16, 1, layers=(0, 2))
    for src in (img, path):
        a = engine.Lora(model, src)
        assert a.alpha == 8.0 and a.n_pairs == 4
        a.close()
    full = engine.Lora(model, synthetic.write_lora_gguf(None, cfg, rank=12, alpha=0.0, dtype=np.float32, seed=2))
    assert full.alpha == 0.0 and full.n_pairs == 7 * cfg.n_layer
    full.close()
    full.close()   # idempotent


def test_images_parse_with_the_gguf_reader():
    cfg = synthetic.CONFIGS[CFG]
    img = synthetic.write_lora_gguf(None, cfg, ("attn_k", "ffn_gate"), 6, 3.0, np.float32, 4, layers=(1,))
    rd = gguf.GGUFReader(img)
    assert rd.kv["general.type"] == "adapter" and rd.kv["adapter.type"] == "lora"
    assert rd.kv["general.architecture"] == "llama" and float(rd.kv["adapter.lora.alpha"]) == 3.0
    kv_dim = cfg.n_head_kv * cfg.head_dim
    assert {k: tuple(v.shape) for k, v in rd.tensors.items()} == {
        "blk.1.attn_k.weight.lora_a": (cfg.n_embd, 6), "blk.1.attn_k.weight.lora_b": (6, kv_dim),
        "blk.1.ffn_gate.weight.lora_a": (cfg.n_embd, 6), "blk.1.ffn_gate.weight.lora_b": (6, cfg.n_ff)}
    assert all(t.type == 0 for t in rd.tensors.values())
    again = synthetic.write_lora_gguf(None, cfg, ("attn_k", "ffn_gate"), 6, 3.0, np.float32, 4, layers=(1,))
    assert np.array_equal(img, again)


@pytest.mark.parametrize("what,img,fragment", [
    ("general.type", lambda: _image(_ab(), general_type="model"), "general.type"),
    ("no general.type", lambda: _image(_ab(), general_type=None), "general.type"),
    ("adapter.type", lambda: _image(_ab(), adapter_type="control_vector"), "adapter.type"),
    ("architecture", lambda: _image(_ab(), arch="gpt2"), "architecture"),
    ("suffix", lambda: _image(_ab() + [("blk.1.attn_q.weight.lora_c", np.zeros((4, 256), np.float16))]), "lora_c"),
    ("missing b", lambda: _image(_ab()[:1]), "missing its lora_b"),
    ("missing a", lambda: _image(_ab()[1:]), "missing its lora_a"),
    ("unknown base", lambda: _image(_ab("blk.9.attn_q.weight")), "does not exist"),
    ("token_embd", lambda: _image(_ab("token_embd.weight", rows=512)), "token_embd.weight' is not supported"),
    ("output", lambda: _image(_ab("output.weight", rows=512)), "output.weight' is not supported"),
    ("a norm", lambda: _image(_ab("blk.1.attn_norm.weight", rows=1)), "is not supported"),
    ("A width", lambda: _image(_ab(K=128)), "invalid shape"),
    ("B rows", lambda: _image(_ab("blk.1.attn_k.weight", rows=256)), "invalid shape"),
    ("rank mismatch", lambda: _image(_ab(rb=8)), "not transposed"),
    ("type", lambda: _image([(n, a.view(np.uint16)) for n, a in _ab()]), "neither F16 nor F32"),
    ("rank 129", lambda: _image(_ab(r=129)), "rank 129"),
])
def test_rejections(model, what, img, fragment):
    with pytest.raises(engine.EngineError, match="lora load failed") as e:
        engine.Lora(model, img())
    assert fragment in str(e.value), what


def test_rank_128_is_accepted_and_truncation_refused(model, tmp_path):
    good = _image(_ab(r=128))
    a = engine.Lora(model, good)
    assert a.n_pairs == 1
    a.close()
    with pytest.raises(engine.EngineError, match="truncated"):
        engine.Lora(model, good[:good.size - 64])
    with pytest.raises(engine.EngineError, match="lora load failed"):
        engine.Lora(model, good[:40])
    with pytest.raises(engine.EngineError, match="cannot open"):
        engine.Lora(model, str(tmp_path / "missing.gguf"))
    L = engine.lib()
    assert not L.mi_lora_load_from_memory(None, good.ctypes.data, good.size) and "null model" in engine.last_error()
    assert L.mi_lora_n_pairs(None) == -1
    L.mi_lora_free(None)


@pytest.mark.parametrize("cfg_name,fragment", [("tiny-moe-q5_k_m", "MoE"), ("tiny-gpt2-q6_k", "GPT-2")])
def test_other_base_models_are_refused(cfg_name, fragment):
    cfg = synthetic.CONFIGS[cfg_name]
    m = engine.Model(synthetic.build_gguf(cfg, seed=1, header_only=True), vocab_only=True)
    name = "blk.0.attn_output.weight"
    img = _image(_ab(name, K=cfg.n_embd, rows=cfg.n_embd), arch=cfg.arch)
    with pytest.raises(engine.EngineError, match=fragment):
        engine.Lora(m, img)
    m.close()
