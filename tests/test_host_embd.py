"""bl::llama::InstanceEmbedding (blama_amd/host) through tests/cpp/t_embd.cpp: the normalisation on
the CPU against the same formulas in numpy float64, and on the GPU getEmbeddingVector against the
Python binding's embeddings of the same prompt through the C ABI."""
import os
import subprocess

import numpy as np
import pytest

from blama_amd import engine, synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "build", "t_embd")
PROMPT = [1, 300, 301, 302, 303, 400, 77, 5]
NORMS = (-1, 0, 1, 2, 3)


def _binary():
    if not os.path.exists(BIN):   # host-only g++ build (no HIP compile); build() normally did it
        subprocess.run(["make", "-C", os.path.join(ROOT, "blama_amd", "host")], check=True, capture_output=True)
    return BIN


def _normalize64(x, norm):
    """normalizeEmbedding (InstanceEmbedding.cpp:59-93) in numpy float64."""
    x64 = x.astype(np.float64)
    if norm == -1:
        s = 1.0
    elif norm == 0:
        s = float(np.max(np.abs(x64))) / 32760.0 if x.size else 0.0
    elif norm == 2:
        s = float(np.sqrt(np.sum(x64 * x64)))
    else:
        s = float(np.sum(np.abs(x64) ** norm) ** (1.0 / norm))
    return x * (np.float32(1.0 / s) if s > 0 else np.float32(0.0))


def _ulps(a, b):
    """Distance in f32 ulps between same-sign floats (or both zero)."""
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    return np.abs(ia - ib)


def test_normalize_matches_numpy(tmp_path):
    """-1, 0, 1, 2, 3 on a fixed 256-float vector and on the zero vector, within 2 f32 ulp: the
    double sums differ only in order, which can move float(1 / sum) by one ulp."""
    x = (np.random.default_rng(9).standard_normal(256) * 1.7).astype(np.float32)
    src, out = str(tmp_path / "x.f32"), str(tmp_path / "y.f32")
    x.tofile(src)
    r = subprocess.run([_binary(), "--norm-only", f"--in={src}", f"--out={out}"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.fromfile(out, np.float32).reshape(2, len(NORMS), x.size)
    for k, norm in enumerate(NORMS):
        ref = _normalize64(x, norm).astype(np.float32)
        assert np.all(np.signbit(got[0, k]) == np.signbit(ref))
        assert int(np.max(_ulps(got[0, k], ref))) <= 2, (norm, int(np.max(_ulps(got[0, k], ref))))
        if norm == -1:
            assert np.array_equal(got[0, k].view(np.uint32), x.view(np.uint32))
        # the zero vector: norm 0 for every rule but "none", the output all zero either way
        assert not np.any(got[1, k]), norm
    assert abs(float(np.sqrt(np.sum(got[0, 3].astype(np.float64) ** 2))) - 1.0) <= 1e-6
    assert abs(float(np.sum(np.abs(got[0, 2].astype(np.float64)))) - 1.0) <= 1e-5
    assert abs(float(np.max(np.abs(got[0, 1]))) - 32760.0) <= 0.01


@pytest.mark.gpu
def test_host_embedding_matches_the_abi(tmp_path):
    cfg = synthetic.CONFIGS["tiny-q4_k_m"]
    buf = synthetic.build_gguf(cfg, seed=11)
    model_path, out = str(tmp_path / "model.gguf"), str(tmp_path / "e.f32")
    buf.tofile(model_path)
    r = subprocess.run([_binary(), f"--model={model_path}", "--prompt=" + ",".join(map(str, PROMPT)), f"--out={out}"],
                       capture_output=True, text=True, timeout=120)
    print(r.stdout[-4000:], r.stderr[-2000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    e2, raw = np.fromfile(out, np.float32).reshape(2, cfg.n_embd)
    assert abs(float(np.sqrt(np.sum(e2.astype(np.float64) ** 2))) - 1.0) <= 1e-6

    m = engine.Model(buf)
    ctx = engine.Context(m, n_ctx=64)
    ctx.set_embeddings(True)
    ctx.decode(PROMPT)
    own = ctx.embeddings()
    ctx.close()
    m.close()
    assert np.array_equal(own.view(np.uint32), raw.view(np.uint32))
    # the Euclidean rule as the host forms it: the f32 squares summed in double in index order
    s = 0.0
    for v in own:
        s += float(np.float32(v * v))
    norm = np.float32(1.0 / np.sqrt(s))
    assert np.array_equal((own * norm).astype(np.float32).view(np.uint32), e2.view(np.uint32))
