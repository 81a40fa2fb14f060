"""bl::llama::LoraAdapter and Instance::addLora / clearLoraState (blama_amd/host) through
tests/cpp/t_lora.cpp: on a synthetic model an adapter changes the next token's top-10 -- through
mi_decode and through a Session -- to exactly the values the Python binding obtains through the C
ABI, setting it again updates its scale, clearing restores the base values, a refused file and an
adapter of another Model throw."""
import os
import subprocess

import numpy as np
import pytest

from blama_amd import engine, synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "build", "t_lora")
PROMPT = [1, 300, 301, 302, 303, 400, 77, 5]     # kPrompt in t_lora.cpp


def _binary():
    if not os.path.exists(BIN):   # host-only g++ build (no HIP compile); build() normally did it
        subprocess.run(["make", "-C", os.path.join(ROOT, "blama_amd", "host")], check=True, capture_output=True)
    return BIN


def _top(ctx):
    ctx.kv_clear()
    ctx.decode(PROMPT)
    ids, vals = ctx.topk(10)
    return [int(i) for i in ids], [float(np.float32(v)) for v in vals]


@pytest.mark.gpu
def test_host_lora_matches_the_abi(tmp_path):
    cfg = synthetic.CONFIGS["tiny-q4_k_m"]
    buf = synthetic.build_gguf(cfg, seed=11)
    paths = {k: str(tmp_path / f"{k}.gguf") for k in ("model", "lora", "bad")}
    buf.tofile(paths["model"])
    synthetic.write_lora_gguf(paths["lora"], cfg, rank=8, alpha=16.0, dtype=np.float16, seed=5, std=0.07)
    synthetic.write_cvec_gguf(paths["bad"], {1: np.zeros(cfg.n_embd, np.float32)})   # no general.type "adapter"
    out = str(tmp_path / "top.txt")
    r = subprocess.run([_binary()] + [f"--{k}={p}" for k, p in paths.items()] + [f"--out={out}"],
                       capture_output=True, text=True, timeout=120)
    print(r.stdout[-4000:], r.stderr[-2000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    host = {}
    for line in open(out):
        f = line.split()
        host[f[0]] = ([int(t.split(":")[0]) for t in f[1:]], [float(np.float32(t.split(":")[1])) for t in f[1:]])
    assert host["cleared"] == host["base"] and host["adapted"] != host["base"] != host["rescaled"]

    m = engine.Model(buf)
    ctx = engine.Context(m, n_ctx=64)
    lora = engine.Lora(m, paths["lora"])
    assert _top(ctx) == host["base"]
    ctx.set_lora(lora, 0.75)
    assert _top(ctx) == host["adapted"]
    ctx.set_lora(lora, 0.25)
    assert _top(ctx) == host["rescaled"]
    ctx.clear_lora()
    assert _top(ctx) == host["base"]
