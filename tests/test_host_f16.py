"""The host mirror (blama_amd/host: Model, Instance, Session, InstanceEmbedding over libbl_llama) on
an unquantised F16 model, through tests/cpp/t_f16.cpp: 8 greedy tokens, Session verification of them
(serial: bit-identical; batched: the LogitComparer gate) and one InstanceEmbedding call; the
embedding is compared with the Python binding's through the C ABI."""
import os
import subprocess

import numpy as np
import pytest

from blama_amd import engine, synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "build", "t_f16")
PROMPT = [1, 300, 301, 302, 303, 400, 77, 5]


def _binary():
    if not os.path.exists(BIN):   # host-only g++ build (no HIP compile); build() normally did it
        subprocess.run(["make", "-C", os.path.join(ROOT, "blama_amd", "host")], check=True, capture_output=True)
    return BIN


@pytest.mark.gpu
def test_host_mirror_on_an_f16_model(tmp_path):
    cfg = synthetic.F16_CONFIGS["tiny-f16"]
    buf = synthetic.build_gguf(cfg, seed=11)
    model_path, out = str(tmp_path / "model.gguf"), str(tmp_path / "out.bin")
    buf.tofile(model_path)
    r = subprocess.run([_binary(), f"--model={model_path}", "--prompt=" + ",".join(map(str, PROMPT)), f"--out={out}"],
                       capture_output=True, text=True, timeout=120)
    print(r.stdout[-4000:], r.stderr[-2000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    raw = np.fromfile(out, np.uint8)
    n = int(raw[:4].view(np.uint32)[0])
    toks = [int(t) for t in raw[4:4 + 4 * n].view(np.int32)]
    embd = raw[4 + 4 * n:].view(np.float32)
    assert n == 8 and embd.size == cfg.n_embd

    m = engine.Model(buf)
    try:
        assert all(0 <= t < cfg.n_vocab for t in toks)
        ctx = engine.Context(m, n_ctx=64)
        ctx.set_embeddings(True)
        ctx.decode(PROMPT)
        assert np.array_equal(ctx.embeddings().view(np.uint32), embd.view(np.uint32))
        ctx.close()
    finally:
        m.close()
