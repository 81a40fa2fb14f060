"""The jina-bert-v2 pass end to end on both synthetic configs (jina-s: jina-embeddings-v2's head geometry, head_dim
64, MEAN pooling; jina-h3: head_dim 32, three heads, so head 2's slope is the m1 branch's) against the numpy
reference of jina_ref_util.py, at the row rule of test_gpu_bert.py unchanged: max|d| <= LOGIT_TOL x rms of the
reference row, else within twice the reference's own f32-accumulation floor.  n = 513 runs the long-sequence
attention kernel, n = 2100 the 128-query kernel past 2048 tokens."""
import os
import subprocess
from dataclasses import replace

import numpy as np
import pytest

from blama_amd import engine, synthetic
from jina_ref_util import JinaRef
from test_gpu_nomic import Nomic, _check_rows

pytestmark = pytest.mark.gpu

NAMES = ("jina-s", "jina-h3")


class Jina(Nomic):      # test_gpu_nomic.py's helper (tokens, ctx, rows) on a jina model
    def __init__(self, name):
        self.cfg = synthetic.JINA_CONFIGS[name]
        self.buf = synthetic.build_jina_gguf(self.cfg, seed=3)
        self.ref = JinaRef(self.buf)
        self.model = engine.Model(self.buf, device=0)


@pytest.fixture(scope="module")
def jinas(gpu_lib):
    return {n: Jina(n) for n in NAMES}


@pytest.mark.parametrize("n", [1, 33, 513, 2100])
@pytest.mark.parametrize("name", NAMES)
def test_rows_match_reference(jinas, name, n):
    B = jinas[name]
    c = B.ctx(n_batch=4096)
    assert c.decode_path() == 2
    t = B.tokens(n)
    _check_rows(B, B.rows(c, t), t)
    assert c.batch_path() == 5 and c.pos_max == -1 and c.n_cells == 0
    c.close()


@pytest.mark.parametrize("name", NAMES)
def test_pooling(jinas, name):
    B = jinas[name]
    c = engine.Context(B.model, n_batch=512)
    assert c.pooling == (engine.POOLING_MEAN if name == "jina-s" else engine.POOLING_NONE)
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
def test_encode_seqs_has_each_sequences_bits(jinas, name):
    """(5, 2100, 64) in one call: the rows of each sequence alone, through the short and the 128-query kernel."""
    B = jinas[name]
    c = B.ctx(n_batch=4096)
    seqs = [B.tokens(n, seed=7) for n in (5, 2100, 64)]
    c.encode(seqs)
    assert c.batch_path() == 6
    batch = np.stack([c.embeddings(i) for i in range(2169)])
    for a, s in zip((0, 5, 2105), seqs):
        c.encode([s])
        alone = np.stack([c.embeddings(i) for i in range(s.size)])
        assert np.array_equal(alone.view(np.uint32), batch[a:a + s.size].view(np.uint32)), s.size
    c.close()


def test_refusals(jinas):
    B = jinas["jina-s"]
    c = B.ctx(n_batch=8192)
    with pytest.raises(engine.EngineError, match="at most 8192 tokens"):
        c.decode(np.ones(8193, np.int32))
    with pytest.raises(engine.EngineError, match="sequence 1 has 8193 tokens"):
        c.encode([np.ones(3, np.int32), np.ones(8193, np.int32)])
    with pytest.raises(engine.EngineError, match="no output head"):
        c.set_embeddings(False)
    c.close()
    c = B.ctx(n_batch=700)
    with pytest.raises(engine.EngineError, match="more than 700 tokens"):
        c.encode([np.ones(600, np.int32), np.ones(101, np.int32)])
    c.close()
    lcfg = replace(synthetic.CONFIGS["tiny-q4_k_m"], arch="jina-bert-v2")
    with pytest.raises(engine.EngineError, match="LLaMA-architecture base models only"):
        engine.Lora(B.model, synthetic.write_lora_gguf(None, lcfg, targets=("attn_q",), rank=2))


def test_host_instance_embedding(jinas, tmp_path):
    """bl::llama on the jina model (tests/cpp/t_bert.cpp --embd): InstanceEmbedding's raw vector equals the ABI's
    MEAN-pooled row bit for bit, as test_gpu_nomic.py checks for nomic-bert."""
    B = jinas["jina-s"]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    binary = os.path.join(root, "tests", "cpp", "build", "t_bert")
    if not os.path.exists(binary):
        subprocess.run(["make", "-C", os.path.join(root, "blama_amd", "host")], check=True, capture_output=True)
    model_path, out = str(tmp_path / "jina.gguf"), str(tmp_path / "e.bin")
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
