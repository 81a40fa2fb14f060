"""bench.py's command line on a tiny synthetic model: a plain run times exactly --steps steps,
reports ms_per_step, leaves the --full legs out of the result line, and --dump-outputs writes
the last timed step's outputs, identical from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("roofline", "prefill", "cpu_baseline", "logit_comparer_vs_cpu")
N_VOCAB = 512   # tiny-q4_k_m


def _bench(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "tiny-q4_k_m",
                        *args], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_command_line_has_full_and_dump_outputs():
    """Argument parsing needs no GPU: both options exist, and a run with no timed step is refused."""
    bench = os.path.join(ROOT, "bench.py")
    r = subprocess.run([sys.executable, bench, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--full" in r.stdout and "--dump-outputs DIR" in r.stdout
    r = subprocess.run([sys.executable, bench, "--steps", "0"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--steps" in r.stderr


@pytest.mark.gpu
def test_plain_run_result_line_and_dumped_outputs(gpu_lib, tmp_path):
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    out = _bench("--steps", "5", "--warmup", "2", "--dump-outputs", a)
    assert out["steps"] == 5 and out["warmup"] == 2 and out["unit"] == "tokens/s" and out["higher_is_better"]
    assert out["ms_per_step"] > 0
    # value and ms_per_step are the same measurement; the line rounds ms_per_step to 1e-4 ms,
    # which at a step of >= 0.02 ms moves 1000 / ms_per_step by <= 2.5e-3
    assert out["ms_per_step"] >= 0.02
    assert out["value"] == pytest.approx(1000.0 / out["ms_per_step"], rel=5e-3)
    assert out["config"]["seq_len"] == 32 + 2 + 5
    assert not [k for k in FULL_ONLY if k in out]

    shapes = {"top40_ids": (40,), "top40_logits": (40,), "token": (1,), "logits": (N_VOCAB,),
              "next_top40_ids": (40,), "next_top40_logits": (40,)}
    got = {f[:-4]: np.load(os.path.join(a, f)) for f in sorted(os.listdir(a))}
    assert set(got) == set(shapes)
    for name, x in got.items():
        assert x.shape == shapes[name] and x.dtype in (np.float32, np.float64), name
        assert np.all(np.isfinite(x)), name
    # the step sampled its token from the top-40 it read; the row its decode left is consistent
    # with that row's own top-40 (descending, the row's largest values at those ids)
    assert got["token"][0] in got["top40_ids"]
    ids = got["next_top40_ids"].astype(np.int64)
    assert np.array_equal(got["logits"][ids], got["next_top40_logits"])
    assert np.all(np.diff(got["next_top40_logits"]) <= 0)
    assert got["next_top40_logits"][-1] >= np.sort(got["logits"])[-40]

    _bench("--steps", "5", "--warmup", "2", "--dump-outputs", b)
    for name, x in got.items():
        assert np.array_equal(x, np.load(os.path.join(b, name + ".npy"))), name
