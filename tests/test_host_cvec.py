"""bl::llama::ControlVector and Instance::addControlVector / clearControlVector (blama_amd/host)
through tests/cpp/t_cvec.cpp: on a synthetic model, two control-vector files summed with their
strengths change the next token's top-10 to exactly the values the Python binding obtains through
the C ABI, clearing restores the unsteered ones, and a vector of another n_embd throws."""
import os
import subprocess

import numpy as np
import pytest

from blama_amd import engine, synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "build", "t_cvec")
PROMPT = [1, 300, 301, 302, 303, 400, 77, 5]     # kPrompt in t_cvec.cpp


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
def test_host_control_vector_matches_the_abi(tmp_path):
    cfg = synthetic.CONFIGS["tiny-q4_k_m"]
    buf = synthetic.build_gguf(cfg, seed=11)
    rng = np.random.default_rng(4)
    d = cfg.n_embd
    vec = lambda: (0.5 * rng.standard_normal(d)).astype(np.float32)   # noqa: E731
    paths = {k: str(tmp_path / f"{k}.gguf") for k in ("model", "a", "b", "other")}
    buf.tofile(paths["model"])
    synthetic.write_cvec_gguf(paths["a"], {1: vec(), 2: vec()})
    synthetic.write_cvec_gguf(paths["b"], {2: vec(), 3: vec()})
    synthetic.write_cvec_gguf(paths["other"], {1: vec()[:d // 2]})
    out = str(tmp_path / "top.txt")
    r = subprocess.run([_binary()] + [f"--{k}={p}" for k, p in paths.items()] + [f"--out={out}"],
                       capture_output=True, text=True, timeout=120)
    print(r.stdout[-4000:], r.stderr[-2000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    host = {}
    for line in open(out):
        f = line.split()
        host[f[0]] = ([int(t.split(":")[0]) for t in f[1:]], [float(np.float32(t.split(":")[1])) for t in f[1:]])
    assert host["cleared"] == host["base"] and host["steered"] != host["base"]

    # the same through the C ABI from Python: the files summed as ControlVector sums them
    da, na = engine.cvec_load(paths["a"], 0.5)
    db, nb = engine.cvec_load(paths["b"], -2.0)
    assert na == nb == d
    data = np.zeros(max(da.size, db.size), np.float32)
    data[:da.size] += da
    data[:db.size] += db
    m = engine.Model(buf)
    ctx = engine.Context(m, n_ctx=64)
    assert _top(ctx) == host["base"]
    ctx.apply_cvec(data, 1, cfg.n_layer)
    assert _top(ctx) == host["steered"]
    ctx.clear_cvec()
    assert _top(ctx) == host["base"]
