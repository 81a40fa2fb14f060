#!/usr/bin/env python3
"""Time of one encoder call, from mi_decode to the mi_embeddings that synchronises, on two 12-layer
synthetic BERT models -- bge-small's widths (384 / 12 heads of 32 / 1536) and bge-base's (768 / 12
heads of 64 / 3072) -- at n = 16, 128 and 512 tokens, CLS pooling.  Reported: every repeat's median
over --iters calls, and their median and spread; the launch count and the f16 FLOPs of a call.

    python scripts/bert_bench.py [--iters 10] [--repeat 5] [--out profiles/bert_bench.json]
Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"bge-small-12l": (384, 12, 1536), "bge-base-12l": (768, 12, 3072)}
NS = (16, 128, 512)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from blama_amd import engine, synthetic

    out = {"iters": args.iters, "models": {}}
    for name, (d, heads, ff) in SHAPES.items():
        cfg = synthetic.BertConfig(name, 512, d, 12, heads, ff, 512, pooling_type=2)
        model = engine.Model(synthetic.build_bert_gguf(cfg, seed=0))
        ctx = engine.Context(model, n_batch=512)
        rng = np.random.default_rng(0)
        res = {}
        for n in NS:
            toks = rng.integers(0, cfg.n_vocab, n).astype(np.int32)
            reps = []
            for rep in range(args.repeat + 1):   # the first repeat warms the shape up and is dropped
                ts = []
                for _ in range(args.iters):
                    ctx.synchronize()
                    t0 = time.perf_counter()
                    ctx.decode(toks)
                    ctx.embeddings(0)
                    ts.append((time.perf_counter() - t0) * 1e3)
                if rep:
                    reps.append(round(statistics.median(ts), 4))
            flops = n * cfg.n_layer * (8 * d * d + 4 * d * ff) + 4 * n * n * d * cfg.n_layer
            res[str(n)] = {"ms": reps, "median_ms": round(statistics.median(reps), 4),
                           "spread_ms": round(max(reps) - min(reps), 4), "f16_flops": flops}
        out["models"][name] = {"n_embd": d, "n_head": heads, "n_ff": ff, "n_layer": cfg.n_layer,
                               "launches_per_call": 7 * cfg.n_layer + 3, "calls": res}
        ctx.close()
        model.close()
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
