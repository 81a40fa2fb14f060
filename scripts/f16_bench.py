#!/usr/bin/env python3
"""Measurements of the unquantised F16 path.

Per launch (mi_op_fgemv_bench: the kernel's own start and end events, median of --iters launches
after a warm-up, every launch reading another copy of the weights so that it streams from HBM): each
role of fgemv.hip on the TinyLlama-1.1B and Llama-2-7B layer shapes and on both output heads
(32000 x 4096, 128256 x 4096), with the achieved matrix bytes/s as a fraction of the 6.29 TB/s
measured copy rate.

End to end, on synthetic F16 models (TinyLlama-1.1B, 2.2 GB; --big adds Llama-2-7B, 13.5 GB): decode
tokens/s over --steps graph-replayed steps after a 32-token prompt, with the whole-step fraction of
HBM (streamed weight bytes x tok/s / 6.29 TB/s); a 512-token prefill; a 20-token MI_OUT_ALL.  Every
figure is the median of --repeat timings, all of them listed.

    python scripts/f16_bench.py [--iters 100] [--steps 128] [--repeat 5] [--big] [--out profiles/f16_bench.json]
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

HBM_COPY = 6.29e12   # measured copy rate, bytes/s
# role: 0 Q/K/V (rows = Q + K + V), 1 residual add, 2 SwiGLU pair, 3 store
LAUNCHES = {
    "tinyllama-1.1b": [("qkv", 0, 2048 + 2 * 256, 2048), ("wo", 1, 2048, 2048), ("gate_up", 2, 5632, 2048),
                       ("down", 1, 2048, 5632), ("head_32000", 3, 32000, 2048)],
    "llama2-7b": [("qkv", 0, 3 * 4096, 4096), ("wo", 1, 4096, 4096), ("gate_up", 2, 11008, 4096),
                  ("down", 1, 4096, 11008), ("head_32000", 3, 32000, 4096)],
    "llama3-8b-head": [("head_128256", 3, 128256, 4096)],
}


def timed(f, repeat):
    ts = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        f()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def end_to_end(name, args, engine, synthetic):
    cfg = synthetic.F16_CONFIGS[name]
    model = engine.Model(synthetic.build_gguf(cfg, seed=0))
    wb = int(engine.lib().mi_model_weight_bytes(model.h))
    rng = np.random.default_rng(0)
    res = {"weight_bytes": wb}
    ctx = engine.Context(model, n_ctx=1024)
    assert ctx.decode_path() == 3
    toks = [int(t) for t in rng.integers(0, cfg.n_vocab, args.steps + 8)]

    def decode_run():
        ctx.kv_clear()
        ctx.decode(toks[:32] if len(toks) >= 32 else toks)
        for t in toks[:8]:
            ctx.decode([t])
        ctx.synchronize()
        t0 = time.perf_counter()
        for t in toks[8:8 + args.steps]:
            ctx.decode([t])
        ctx.synchronize()
        return args.steps / (time.perf_counter() - t0)

    decode_run()
    tps = [round(decode_run(), 2) for _ in range(args.repeat)]
    med = statistics.median(tps)
    res["decode"] = {"tok_s": tps, "median_tok_s": med, "whole_step_hbm_frac": round(med * wb / HBM_COPY, 4)}
    for key, n, all_rows in (("prefill_512", 512, False), ("out_all_20", 20, True)):
        p = [int(t) for t in rng.integers(0, cfg.n_vocab, n)]

        def call():
            ctx.kv_clear()
            ctx.decode(p, all_logits=all_rows)
            ctx.synchronize()

        call()
        ms = [round(t, 4) for t in timed(call, args.repeat)]
        res[key] = {"ms": ms, "median_ms": round(statistics.median(ms), 4)}
    ctx.close()
    model.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--big", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from blama_amd import engine, synthetic

    out = {"iters": args.iters, "hbm_copy_bytes_s": HBM_COPY, "launches": {}, "models": {}}
    for model, launches in LAUNCHES.items():
        rows_out = {}
        for tag, role, rows, K in launches:
            us, nbytes = engine.op_fgemv_bench(role, rows, K, args.iters)
            rows_out[tag] = {"role": role, "rows": rows, "K": K, "matrix_bytes": nbytes, "median_us": round(us, 3),
                             "bytes_s": round(nbytes / (us * 1e-6), 0), "frac_of_copy_rate": round(nbytes / (us * 1e-6) / HBM_COPY, 4)}
        out["launches"][model] = rows_out
    for name in ["tinyllama-1.1b-f16"] + (["llama2-7b-f16"] if args.big else []):
        out["models"][name] = end_to_end(name, args, engine, synthetic)
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
