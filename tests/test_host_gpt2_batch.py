"""The host mirror (blama_amd/host: Model, Instance, Session over libbl_llama) on a GPT-2 model,
through tests/cpp/t_gpt2_batch.cpp: 20 greedy tokens, then Session::fillCtx of the 20 claimed tokens
serially (one decode per token, the server's BLAMA_SERIAL_VERIFY=1 loop) and with batchedVerify (one
MI_OUT_ALL call on the GPT-2 batch path); the batched result passes the LogitComparer gate against
the serial one.  The tokens are the Python binding's greedy ones."""
import os
import subprocess

import numpy as np
import pytest

from blama_amd import engine, synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "build", "t_gpt2_batch")
PROMPT = [1, 300, 301, 302, 303, 400, 77, 5]


def _binary():
    if not os.path.exists(BIN):   # host-only g++ build (no HIP compile); build() normally did it
        subprocess.run(["make", "-C", os.path.join(ROOT, "blama_amd", "host")], check=True, capture_output=True)
    return BIN


@pytest.mark.gpu
def test_batched_verify_on_a_gpt2_model(tmp_path):
    cfg = synthetic.CONFIGS["tiny-gpt2-q6_k"]
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
    assert n == 20

    m = engine.Model(buf)
    try:
        ctx = engine.Context(m, n_ctx=64)
        ctx.decode(PROMPT)
        mine = []
        for _ in range(n):
            t = int(ctx.topk(1)[0][0])
            mine.append(t)
            ctx.decode([t])
        ctx.close()
        assert toks == mine
    finally:
        m.close()
