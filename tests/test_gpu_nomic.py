"""The nomic-bert pass end to end on both synthetic configs (nomic-s: nomic-embed-text's head geometry,
head_dim 64, MEAN pooling, freq_base 1000; nomic-h32: head_dim 32, three heads, n_rot 16) against the
numpy reference of nomic_ref_util.py, at the row rule of test_gpu_bert.py unchanged: max|d| <=
LOGIT_TOL x rms of the reference row, else within twice the reference's own f32-accumulation floor.
n = 513 and 1100 run the long-sequence attention kernel."""
import os
import subprocess

import numpy as np
import pytest

from bert_ref_util import LOGIT_TOL, rms
from blama_amd import engine, synthetic
from nomic_ref_util import NomicRef

pytestmark = pytest.mark.gpu

NAMES = ("nomic-s", "nomic-h32")


class Nomic:
    def __init__(self, name):
        self.cfg = synthetic.NOMIC_CONFIGS[name]
        self.buf = synthetic.build_nomic_gguf(self.cfg, seed=3)
        self.ref = NomicRef(self.buf)
        self.model = engine.Model(self.buf, device=0)

    def tokens(self, n, seed=0):
        return np.random.default_rng(1000 * seed + n).integers(0, self.cfg.n_vocab, n).astype(np.int32)

    def ctx(self, pooling=engine.POOLING_NONE, n_batch=2048):
        c = engine.Context(self.model, n_ctx=0, n_batch=n_batch)
        c.set_embeddings(True, pooling)
        return c

    def rows(self, c, tokens):
        c.decode(tokens, all_logits=True)
        return np.stack([c.embeddings(i) for i in range(len(tokens))])


@pytest.fixture(scope="module")
def nomics(gpu_lib):
    return {n: Nomic(n) for n in NAMES}


def _check_rows(B, got, tokens):
    ref = B.ref.forward(tokens)
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


@pytest.mark.parametrize("n", [1, 33, 70, 513, 1100])
@pytest.mark.parametrize("name", NAMES)
def test_rows_match_reference(nomics, name, n):
    B = nomics[name]
    c = B.ctx()
    assert c.decode_path() == 2
    t = B.tokens(n)
    worst, fell_back = _check_rows(B, B.rows(c, t), t)
    assert c.pos_max == -1 and c.n_cells == 0
    print(f"{name} n {n}: worst max|d|/rms {worst:.3g}, floor fallback needed: {fell_back}")
    c.close()


@pytest.mark.parametrize("name", NAMES)
def test_pooling(nomics, name):
    B = nomics[name]
    c = engine.Context(B.model, n_batch=512)
    assert c.pooling == (engine.POOLING_MEAN if name == "nomic-s" else engine.POOLING_NONE)
    c.close()
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
    mean = rows.astype(np.float64).mean(axis=0)
    bound = n * 2.0 ** -24 * np.abs(rows.astype(np.float64)).mean(axis=0)
    assert np.all(np.abs(c.embeddings(0).astype(np.float64) - mean) <= bound)
    c.close()


@pytest.mark.parametrize("name", NAMES)
def test_encode_seqs_has_each_sequences_bits(nomics, name):
    """(5, 600, 64) in one call: the rows of each sequence alone, through either attention kernel."""
    B = nomics[name]
    c = B.ctx()
    seqs = [B.tokens(n, seed=7) for n in (5, 600, 64)]
    c.encode(seqs)
    assert c.batch_path() == 6
    batch = np.stack([c.embeddings(i) for i in range(669)])
    for a, s in zip((0, 5, 605), seqs):
        c.encode([s])
        alone = np.stack([c.embeddings(i) for i in range(s.size)])
        assert np.array_equal(alone.view(np.uint32), batch[a:a + s.size].view(np.uint32)), s.size
    _check_rows(B, batch[5:605], seqs[1])
    c.close()


def test_refusals(nomics):
    B = nomics["nomic-s"]
    c = B.ctx(n_batch=4096)
    with pytest.raises(engine.EngineError, match="at most 2048 tokens"):
        c.decode(np.ones(2049, np.int32))
    with pytest.raises(engine.EngineError, match="sequence 1 has 2049 tokens"):
        c.encode([np.ones(3, np.int32), np.ones(2049, np.int32)])
    c.close()
    c = B.ctx(n_batch=700)
    with pytest.raises(engine.EngineError, match="more than 700 tokens"):
        c.encode([np.ones(600, np.int32), np.ones(101, np.int32)])
    c.close()
    from dataclasses import replace
    lcfg = replace(synthetic.CONFIGS["tiny-q4_k_m"], arch="nomic-bert")
    with pytest.raises(engine.EngineError, match="LLaMA-architecture base models only"):
        engine.Lora(B.model, synthetic.write_lora_gguf(None, lcfg, targets=("attn_q",), rank=2))


def test_host_instance_embedding(nomics, tmp_path):
    """bl::llama on the nomic model (tests/cpp/t_bert.cpp --embd): InstanceEmbedding's raw vector equals
    the ABI's MEAN-pooled row bit for bit, as test_gpu_bert.py checks for bge."""
    B = nomics["nomic-s"]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    binary = os.path.join(root, "tests", "cpp", "build", "t_bert")
    if not os.path.exists(binary):
        subprocess.run(["make", "-C", os.path.join(root, "blama_amd", "host")], check=True, capture_output=True)
    model_path, out = str(tmp_path / "nomic.gguf"), str(tmp_path / "e.bin")
    B.buf.tofile(model_path)
    r = subprocess.run([binary, "--embd", f"--model={model_path}", "--text=Banana de la Luna, 7 kits!", f"--out={out}"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    raw_file = np.fromfile(out, np.uint8)
    n = int(raw_file[:4].view(np.uint32)[0])
    toks = raw_file[4:4 + 4 * n].view(np.int32)
    raw = raw_file[4 + 4 * n:].view(np.float32).reshape(2, B.cfg.n_embd)[1]
    c = engine.Context(B.model, n_batch=512)      # the model's pooling: MEAN
    c.decode(toks)
    own = c.embeddings()
    c.close()
    assert 4 < n < 40 and np.array_equal(own.view(np.uint32), raw.view(np.uint32))
