#!/usr/bin/env python3
"""Cost of an embeddings call against the plain call of the same tokens, on a Llama-2-7B-shaped
Q4_K_M synthetic model: a 512-token MEAN-pooled embedding call against a 512-token prefill, and a
1-token LAST call on a 128-cell cache against a decode step there.  Each leg is timed from the call
to the read that synchronises (embeddings() / logits()), the legs alternated within a repeat;
reported: every repeat's median over --iters calls, and their median and spread.

    python scripts/embd_bench.py [--iters 20] [--repeat 5] [--out profiles/embd_bench.json]
    python scripts/embd_bench.py --plain-only --engine-root DIR    # the mode-off legs on another checkout
Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def timed(ctx, prep, call, read, iters):
    """Median ms of call() + read() over iters runs, prep() (untimed, synchronised) before each."""
    ts = []
    for _ in range(iters):
        prep()
        ctx.synchronize()
        t0 = time.perf_counter()
        call()
        read()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="llama2-7b-q4_k_m")
    ap.add_argument("--prompt", type=int, default=512)
    ap.add_argument("--cells", type=int, default=128)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--plain-only", action="store_true", help="time the mode-off legs only (a build without embeddings)")
    ap.add_argument("--engine-root", default=ROOT, help="the checkout whose blama_amd package and library are loaded")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.engine_root))
    from blama_amd import engine, synthetic

    cfg = synthetic.CONFIGS[args.config]
    model = engine.Model(synthetic.build_gguf(cfg, seed=0))
    ctx = engine.Context(model, n_ctx=1024)
    toks = [int(t) for t in np.random.default_rng(0).integers(0, cfg.n_vocab, args.prompt + 1)]
    prompt, fill, one = toks[:args.prompt], toks[:args.cells], toks[args.prompt:]

    def refill():
        ctx.kv_clear()
        ctx.decode(fill)

    def mode(on, pooling=0):
        if not args.plain_only:
            ctx.set_embeddings(on, pooling)

    legs = {"prefill_plain": [], "step_plain": []}
    if not args.plain_only:
        legs.update({"prefill_embd_mean": [], "step_embd_last": []})
    for rep in range(args.repeat + 1):   # the first repeat warms every shape up and is dropped
        r = {}
        mode(False)
        r["prefill_plain"] = timed(ctx, ctx.kv_clear, lambda: ctx.decode(prompt), ctx.logits, args.iters)
        r["step_plain"] = timed(ctx, refill, lambda: ctx.decode(one), ctx.logits, args.iters)
        if not args.plain_only:
            mode(True, engine.POOLING_MEAN)
            r["prefill_embd_mean"] = timed(ctx, ctx.kv_clear, lambda: ctx.decode(prompt), ctx.embeddings, args.iters)
            mode(True, engine.POOLING_LAST)
            r["step_embd_last"] = timed(ctx, refill, lambda: ctx.decode(one), ctx.embeddings, args.iters)
        if rep:
            for k, v in r.items():
                legs[k].append(round(v, 4))
    out = {
        "config": args.config, "prompt_tokens": args.prompt, "step_cells": args.cells, "iters": args.iters,
        "engine_root": os.path.relpath(os.path.abspath(args.engine_root), ROOT),
        "head_bytes_skipped": int(cfg.n_vocab * cfg.n_embd * 210 // 256),   # output.weight, Q6_K in a Q4_K_M file
        "ms": legs,
        "median_ms": {k: round(statistics.median(v), 4) for k, v in legs.items()},
        "spread_ms": {k: round(max(v) - min(v), 4) for k, v in legs.items()},
    }
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
