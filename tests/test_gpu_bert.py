"""The encoder pass end to end on both synthetic BERT configs (bert-s: bge-small's widths, head_dim 32,
CLS pooling; bert-w: head_dim 64, no pooling key) against the numpy reference of bert_ref_util.py.

Row rule: the project's embedding rule, max|d| <= LOGIT_TOL x rms of the reference row -- or, where
that fails, within twice the reference's own rounding floor (the float64-accumulating reference
against the same reference accumulating in f32 in index order).  Measured on MI355X: worst
max|d| / rms 1.11e-3 (bert-s) and 1.53e-3 (bert-w); the floor fallback was never needed."""
import os
import subprocess

import numpy as np
import pytest

from bert_ref_util import LOGIT_TOL, BertRef, rms
from blama_amd import engine, synthetic

pytestmark = pytest.mark.gpu

NAMES = ("bert-s", "bert-w")


class Bert:
    def __init__(self, name):
        self.cfg = synthetic.BERT_CONFIGS[name]
        self.buf = synthetic.build_bert_gguf(self.cfg, seed=3)
        self.ref = BertRef(self.buf)
        self.model = engine.Model(self.buf, device=0)
        self._rows = {}

    def tokens(self, n, seed=0):
        rng = np.random.default_rng(1000 * seed + n)
        return rng.integers(0, self.cfg.n_vocab, n).astype(np.int32)

    def ref_rows(self, tokens):
        key = tuple(int(t) for t in tokens)
        if key not in self._rows:
            self._rows[key] = self.ref.forward(tokens)
        return self._rows[key]

    def ctx(self, pooling=engine.POOLING_NONE):
        c = engine.Context(self.model, n_ctx=0, n_batch=512)
        c.set_embeddings(True, pooling)
        return c

    def rows(self, c, tokens):
        c.decode(tokens, all_logits=True)
        return np.stack([c.embeddings(i) for i in range(len(tokens))])


@pytest.fixture(scope="module")
def berts(gpu_lib):
    return {n: Bert(n) for n in NAMES}


def _check_rows(B, got, tokens):
    ref = B.ref_rows(tokens)
    worst, floor = 0.0, None
    for i in range(len(tokens)):
        d = float(np.abs(got[i].astype(np.float64) - ref[i]).max())
        worst = max(worst, d / rms(ref[i]))
        if d <= LOGIT_TOL * rms(ref[i]):
            continue
        if floor is None:
            floor = np.abs(B.ref.forward(tokens, acc="f32").astype(np.float64) - ref).max(axis=1)
        assert d <= 2 * floor[i], (B.cfg.name, len(tokens), i, d, rms(ref[i]), float(floor[i]))
    return worst, floor is not None


@pytest.mark.parametrize("name", NAMES)
def test_rows_match_reference(berts, name):
    B = berts[name]
    c = B.ctx()
    assert c.pooling == engine.POOLING_NONE and c.decode_path() == 2
    worst, fell_back = 0.0, False
    for n in (1, 2, 31, 33, 70, B.cfg.n_ctx_train):
        # bert-w's position table ends at 64: its n = 70 case is refused by design (test_refusals) and
        # runs at 64; bert-s covers 70 end to end, the GEMM op test covers 70 token rows
        n = min(n, B.cfg.n_ctx_train)
        t = B.tokens(n)
        w, f = _check_rows(B, B.rows(c, t), t)
        worst, fell_back = max(worst, w), fell_back or f
        assert c.pos_max == -1 and c.n_cells == 0
        # MI_OUT_LAST: the last token's row
        c.decode(t)
        assert np.array_equal(c.embeddings(-1), c.embeddings(0))
        assert np.array_equal(c.embeddings(-1), B.rows(c, t)[-1])
    print(f"{name}: worst max|d|/rms {worst:.3g}, floor fallback needed: {fell_back}")
    c.close()


@pytest.mark.parametrize("name", NAMES)
def test_default_pooling_is_the_models(berts, name):
    B = berts[name]
    c = engine.Context(B.model, n_batch=512)
    assert c.pooling == (engine.POOLING_CLS if name == "bert-s" else engine.POOLING_NONE)
    c.decode(B.tokens(5))          # in embeddings mode from the start
    assert c.embeddings(-1).shape == (B.cfg.n_embd,)
    c.close()


@pytest.mark.parametrize("name", NAMES)
def test_pooling(berts, name):
    B = berts[name]
    n = 33
    t = B.tokens(n, seed=2)
    c = B.ctx()
    rows = B.rows(c, t)
    for pooling, want in ((engine.POOLING_CLS, rows[0]), (engine.POOLING_LAST, rows[-1])):
        c.set_embeddings(True, pooling)
        c.decode(t)
        assert np.array_equal(c.embeddings(0).view(np.uint32), want.view(np.uint32))
    c.set_embeddings(True, engine.POOLING_MEAN)
    c.decode(t)
    got = c.embeddings(0).astype(np.float64)
    mean = rows.astype(np.float64).mean(axis=0)
    bound = n * 2.0 ** -24 * np.abs(rows.astype(np.float64)).mean(axis=0)
    assert np.all(np.abs(got - mean) <= bound)
    c.close()


@pytest.mark.parametrize("name", NAMES)
def test_bidirectional(berts, name):
    """Row 0 sees the tokens after it: changing the last token moves it."""
    B = berts[name]
    c = B.ctx()
    a, b = [7, 19, 40], [7, 19, 41]
    ra, rb = B.rows(c, a), B.rows(c, b)
    _check_rows(B, ra, a)
    _check_rows(B, rb, b)
    assert np.abs(ra[0] - rb[0]).max() > 10 * LOGIT_TOL * rms(B.ref_rows(a)[0])
    c.close()


@pytest.mark.parametrize("name", NAMES)
def test_stateless(berts, name):
    B = berts[name]
    c = B.ctx()
    ta, tb = B.tokens(31, seed=5), B.tokens(20, seed=6)
    a0 = B.rows(c, ta)
    assert c.pos_max == -1
    B.rows(c, tb)
    assert c.pos_max == -1
    c.kv_clear()
    a1 = B.rows(c, ta)
    assert c.pos_max == -1 and c.n_cells == 0
    assert np.array_equal(a0.view(np.uint32), a1.view(np.uint32))
    assert c.state_get() == b""
    c.close()


def test_refusals(berts, tmp_path):
    B = berts["bert-w"]
    cfg = B.cfg
    c = B.ctx()
    with pytest.raises(engine.EngineError, match="at most 64 tokens"):
        c.decode(B.tokens(cfg.n_ctx_train).tolist() + [1])
    with pytest.raises(engine.EngineError, match="token id out of range"):
        c.decode([1, cfg.n_vocab])
    with pytest.raises(engine.EngineError, match="no output head"):
        c.set_embeddings(False)
    c.decode([1, 2, 3])
    with pytest.raises(engine.EngineError, match="embeddings mode"):
        c.topk(5)
    with pytest.raises(engine.EngineError, match="embeddings mode"):
        c.logits()
    with pytest.raises(engine.EngineError, match="no control vector"):
        c.apply_cvec(np.zeros(2 * cfg.n_embd, np.float32), 1, 2)
    with pytest.raises(engine.EngineError, match="no KV cache"):
        c.kv_seq_rm(0, 1)
    c.close()
    # a LoRA file is refused for any non-LLaMA base
    from dataclasses import replace
    lcfg = replace(synthetic.CONFIGS["tiny-q4_k_m"], arch="bert")
    with pytest.raises(engine.EngineError, match="LLaMA-architecture base models only"):
        engine.Lora(B.model, synthetic.write_lora_gguf(None, lcfg, targets=("attn_q",), rank=2))
    # matrices must be F16, every bias present
    with pytest.raises(engine.EngineError, match=r"blk\.1\.attn_q\.weight.*F16"):
        engine.Model(synthetic.build_bert_gguf(cfg, types={"blk.1.attn_q.weight": synthetic.F32}), device=0)
    with pytest.raises(engine.EngineError, match=r"missing tensor blk\.0\.ffn_up\.bias"):
        engine.Model(synthetic.build_bert_gguf(cfg, drop=("blk.0.ffn_up.bias",)), device=0)


def test_host_instance_embedding(berts, tmp_path):
    """bl::llama on a BERT model (tests/cpp/t_bert.cpp): the WordPiece tokens of a sentence through
    InstanceEmbedding::getEmbeddingVector equal the ABI's CLS-pooled row, bit for bit, put through the
    host's Euclidean rule as tests/test_host_embd.py forms it."""
    B = berts["bert-s"]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    binary = os.path.join(root, "tests", "cpp", "build", "t_bert")
    if not os.path.exists(binary):
        subprocess.run(["make", "-C", os.path.join(root, "blama_amd", "host")], check=True, capture_output=True)
    model_path, out = str(tmp_path / "bert.gguf"), str(tmp_path / "e.bin")
    B.buf.tofile(model_path)
    text = "Banana de la Luna, 7 kits! \u4e2d qzx\u00fe"
    r = subprocess.run([binary, "--embd", f"--model={model_path}", f"--text={text}", f"--out={out}"],
                       capture_output=True, text=True, timeout=120)
    print(r.stdout[-4000:], r.stderr[-2000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    raw_file = np.fromfile(out, np.uint8)
    n = int(raw_file[:4].view(np.uint32)[0])
    toks = raw_file[4:4 + 4 * n].view(np.int32)
    e2, raw = raw_file[4 + 4 * n:].view(np.float32).reshape(2, B.cfg.n_embd)
    assert toks[0] == 2 and toks[-1] == 3 and 8 < n < 40 and 1 in toks   # [CLS] ... [UNK] ... [SEP]
    assert abs(float(np.sqrt(np.sum(e2.astype(np.float64) ** 2))) - 1.0) <= 1e-6

    c = engine.Context(B.model, n_batch=512)      # the model's pooling: CLS
    assert c.pooling == engine.POOLING_CLS
    c.decode(toks)
    own = c.embeddings()
    c.close()
    assert np.array_equal(own.view(np.uint32), raw.view(np.uint32))
    s = 0.0
    for v in own:   # the f32 squares summed in double in index order
        s += float(np.float32(v * v))
    norm = np.float32(1.0 / np.sqrt(s))
    assert np.array_equal((own * norm).astype(np.float32).view(np.uint32), e2.view(np.uint32))
