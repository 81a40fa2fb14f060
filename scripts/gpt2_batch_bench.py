#!/usr/bin/env python3
"""GPT-2 prompt batches and batched verification: this build against another tree (the parent
commit, built) and against this build's own per-token loop (MI_NO_BATCH=1).

Model: synthetic gpt2-117m-q6_k.  Calls timed (wall time around decode + synchronize, after
warm-up, median of --iters calls):
  prompt512   a 512-token prompt into an empty cache (MI_OUT_LAST)
  verify20 / verify64 / verify256   an MI_OUT_ALL call of 20 / 64 / 256 tokens after a 32-token
              prefix (cache cleared and the prefix decoded again, untimed, before every call)

    python scripts/gpt2_batch_bench.py --parent DIR [--rounds 3] [--iters 20] [--out profiles/gpt2_batch_bench.json]

DIR is a checkout of the commit to compare with, built (its own blama_amd package and library).
The three builds' workers -- parent, this tree, this tree with MI_NO_BATCH=1 -- run in turn, one
fresh process each under its own timeout, --rounds times over: the figures of one build come from
several processes spread over the session, and their spread is reported beside the medians.

    python scripts/gpt2_batch_bench.py --worker ROOT     (one build, one JSON line; used by the above)
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["prompt512", "verify20", "verify64", "verify256"]


def worker(root, iters, warmup):
    sys.path.insert(0, root)
    import numpy as np
    from blama_amd import engine, synthetic
    cfg = synthetic.CONFIGS["gpt2-117m-q6_k"]
    model = engine.Model(synthetic.build_gguf(cfg, seed=5))
    ctx = engine.Context(model, n_ctx=1024)
    rng = np.random.default_rng(1)
    toks = [int(t) for t in rng.integers(0, cfg.n_vocab, 1024)]
    out = {}

    def timed(prefix, n, all_logits):
        ctx.kv_clear()
        if prefix:
            ctx.decode(toks[:prefix])
        ctx.synchronize()
        t0 = time.perf_counter()
        ctx.decode(toks[prefix:prefix + n], all_logits=all_logits)
        ctx.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for name, prefix, n, all_logits in [("prompt512", 0, 512, False), ("verify20", 32, 20, True),
                                        ("verify64", 32, 64, True), ("verify256", 32, 256, True)]:
        for _ in range(warmup):
            timed(prefix, n, all_logits)
        ts = [timed(prefix, n, all_logits) for _ in range(iters)]
        out[name] = {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts)}
    path = getattr(ctx, "batch_path", None)
    out["batch_path"] = path() if path else None   # (of the last call; a tree without the symbol: null)
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker")
    ap.add_argument("--parent")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=240, help="seconds, per worker process")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "gpt2_batch_bench.json"))
    a = ap.parse_args()
    if a.worker:
        worker(a.worker, a.iters, a.warmup)
        return 0
    if not a.parent:
        ap.error("--parent DIR: a built checkout of the commit to compare with")
    builds = [("parent", a.parent, {}), ("batch", HERE, {}), ("loop", HERE, {"MI_NO_BATCH": "1"})]
    runs = {b[0]: [] for b in builds}
    for r in range(a.rounds):
        for name, root, env in builds:
            e = dict(os.environ, **env)
            e.pop("PYTHONPATH", None)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", root, "--iters", str(a.iters),
                                "--warmup", str(a.warmup)], env=e, capture_output=True, text=True, timeout=a.timeout)
            line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
            if p.returncode != 0 or not line:   # a fault ends the session: nothing more is started on the card
                print(p.stdout[-2000:], p.stderr[-2000:])
                print(f"{name} worker failed (exit {p.returncode}); stopping")
                return 1
            runs[name].append(json.loads(line[0][7:]))
            print(f"round {r} {name}: " + ", ".join(f"{c} {runs[name][-1][c]['median_ms']:.3f} ms" for c in CASES), flush=True)
    res = {"model": "gpt2-117m-q6_k (synthetic)", "rounds": a.rounds, "iters": a.iters, "unit": "ms (wall, decode + synchronize)",
           "builds": {"parent": "the parent commit", "batch": "this change", "loop": "this change, MI_NO_BATCH=1"},
           "cases": {}, "batch_path": {n: runs[n][-1]["batch_path"] for n in runs}}
    for c in CASES:
        res["cases"][c] = {}
        for name in runs:
            med = [x[c]["median_ms"] for x in runs[name]]
            res["cases"][c][name] = {"median_ms": statistics.median(med), "process_medians_ms": med,
                                     "spread_ms": max(med) - min(med)}
        par, new = res["cases"][c]["parent"], res["cases"][c]["batch"]
        res["cases"][c]["speedup_vs_parent"] = par["median_ms"] / new["median_ms"]
        res["cases"][c]["faster_by_more_than_parent_spread"] = (par["median_ms"] - new["median_ms"]) > par["spread_ms"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res["cases"], indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
