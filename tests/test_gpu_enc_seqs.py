"""Several sequences per encoder call (mi_encode_seqs) end to end on both synthetic BERT configs, against
BertRef.forward of each sequence alone.  Row rule: test_gpu_bert.py's -- max|d| <= LOGIT_TOL x rms of
the reference row, or else within twice the reference's own f32-order floor."""
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
        self.none = {}      # lengths -> (sequences, token rows of the pooling-NONE call)

    def seqs(self, lens):
        rng = np.random.default_rng(sum(lens) + len(lens))
        return [rng.integers(0, self.cfg.n_vocab, n).astype(np.int32) for n in lens]

    def ctx(self, pooling=engine.POOLING_NONE, n_batch=512):
        c = engine.Context(self.model, n_ctx=n_batch, n_batch=n_batch)   # n_ctx bounds n_batch and nothing else here
        c.set_embeddings(True, pooling)
        return c

    def none_rows(self, lens, n_batch=512):
        if lens not in self.none:
            seqs, c = self.seqs(lens), self.ctx(n_batch=n_batch)
            c.encode(seqs)
            assert c.batch_path() == 6
            rows = np.stack([c.embeddings(i) for i in range(sum(lens))])
            assert np.array_equal(c.embeddings(-1), rows[-1])
            c.close()
            self.none[lens] = (seqs, rows)
        return self.none[lens]


@pytest.fixture(scope="module")
def berts(gpu_lib):
    return {n: Bert(n) for n in NAMES}


def _check_rows(B, got, tokens):
    ref, floor = B.ref.forward(tokens), None
    for i in range(len(got)):
        d = float(np.abs(got[i].astype(np.float64) - ref[i]).max())
        if d <= LOGIT_TOL * rms(ref[i]):
            continue
        if floor is None:
            floor = np.abs(B.ref.forward(tokens, acc="f32").astype(np.float64) - ref).max(axis=1)
        assert d <= 2 * floor[i], (B.cfg.name, len(tokens), i, d, rms(ref[i]), float(floor[i]))


def _lens(B):
    return (1, 33, 5, B.cfg.n_ctx_train, 31)


@pytest.mark.parametrize("name,wide", [("bert-s", False), ("bert-w", False), ("bert-s", True)])
def test_rows_match_reference(berts, name, wide):
    B = berts[name]
    lens = (128,) * 5 if wide else _lens(B)     # wide: 640 rows, past one sequence's 512
    seqs, rows = B.none_rows(lens, n_batch=1024 if wide else 512)
    for a, t in zip(np.cumsum((0,) + lens), seqs):
        _check_rows(B, rows[a:a + len(t)], t)


@pytest.mark.parametrize("name", NAMES)
def test_pooled(berts, name):
    B = berts[name]
    lens = _lens(B)
    seqs, rows = B.none_rows(lens)
    starts = np.cumsum((0,) + lens)
    c = B.ctx()
    for pooling in (engine.POOLING_CLS, engine.POOLING_LAST, engine.POOLING_MEAN):
        c.set_embeddings(True, pooling)
        c.encode(seqs)
        got = [c.embeddings_seq(i) for i in range(len(seqs))]
        for i, (a, n) in enumerate(zip(starts, lens)):
            r = rows[a:a + n]
            if pooling == engine.POOLING_MEAN:
                bound = n * 2.0 ** -24 * np.abs(r.astype(np.float64)).mean(axis=0)
                assert np.all(np.abs(got[i].astype(np.float64) - r.astype(np.float64).mean(axis=0)) <= bound), i
            else:
                want = r[0] if pooling == engine.POOLING_CLS else r[-1]
                assert np.array_equal(got[i].view(np.uint32), want.view(np.uint32)), (pooling, i)
            c.encode([seqs[i]])       # the same sequence alone: the same bits
            assert np.array_equal(c.embeddings_seq(0).view(np.uint32), got[i].view(np.uint32)), (pooling, i)
            c.encode(seqs)
        c.decode(seqs[1])             # after mi_decode the call is sequence 0
        assert np.array_equal(c.embeddings_seq(0), c.embeddings(0))
    c.close()


def test_refusals(berts):
    B = berts["bert-w"]
    cfg, ok = B.cfg, [np.array([1, 2, 3], np.int32), np.array([4], np.int32)]
    c = B.ctx(n_batch=100)
    for seqs, msg in (([ok[0], []], "sequence 1 has 0 tokens"),
                      ([np.ones(cfg.n_ctx_train + 1, np.int32)], f"sequence 0 has {cfg.n_ctx_train + 1} tokens"),
                      ([np.ones(60, np.int32), np.ones(41, np.int32)], "more than 100 tokens"),
                      ([], "n_seq must be at least 1"),
                      ([ok[0], [1, cfg.n_vocab]], "token id out of range in sequence 1")):
        with pytest.raises(engine.EngineError, match=msg):
            c.encode(seqs)
    c.encode(ok)
    with pytest.raises(engine.EngineError, match="pooling NONE"):
        c.embeddings_seq(0)
    assert np.isfinite(c.embeddings(3)).all()          # the context still serves
    c.close()
    llama = engine.Model(synthetic.build_gguf(synthetic.CONFIGS["tiny-q4_k_m"], seed=1), device=0)
    lc = engine.Context(llama, n_ctx=64)
    with pytest.raises(engine.EngineError, match="not an encoder"):
        lc.encode(ok)
    lc.close()


@pytest.mark.parametrize("n_batch", [512, 64])
def test_host_embedding_vectors(berts, tmp_path, n_batch):
    """getEmbeddingVectors of four prompts (tests/cpp/t_enc_seqs.cpp): the bits of one call per prompt
    (checked in the binary), getEmbeddingVector within the row rule, normalised as it normalises; at
    n_batch 64 the 100 tokens take two calls."""
    B = berts["bert-s"]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    binary = os.path.join(root, "tests", "cpp", "build", "t_enc_seqs")
    if not os.path.exists(binary):
        subprocess.run(["make", "-C", os.path.join(root, "blama_amd", "host")], check=True, capture_output=True)
    prompts = B.seqs((30, 20, 40, 10))
    model_path, src, out = str(tmp_path / "bert.gguf"), str(tmp_path / "in.bin"), str(tmp_path / "e.bin")
    B.buf.tofile(model_path)
    with open(src, "wb") as f:
        for p in prompts:
            f.write(np.uint32(p.size).tobytes() + p.tobytes())
    r = subprocess.run([binary, f"--model={model_path}", f"--in={src}", f"--out={out}", f"--batch={n_batch}"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    raw, e2, single = np.fromfile(out, np.float32).reshape(3, len(prompts), B.cfg.n_embd)
    for i, p in enumerate(prompts):         # bert-s pools CLS: the vector is the first token's row
        _check_rows(B, raw[i][None], p)
        assert np.abs(raw[i].astype(np.float64) - single[i]).max() <= LOGIT_TOL * rms(single[i])
        s = 0.0
        for v in raw[i]:   # the f32 squares summed in double in index order
            s += float(np.float32(v * v))
        assert np.array_equal((raw[i] * np.float32(1.0 / np.sqrt(s))).astype(np.float32).view(np.uint32), e2[i].view(np.uint32))
