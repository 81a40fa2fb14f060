#!/usr/bin/env python3
"""Measurements of the Q4_0 / Q5_0 path, each beside Q8_0 at the same shape on the same machine.

Per launch (mi_op_gemv_bench: gemv_kernel's store form between two events, median of --iters
launches after a warm-up, every launch reading another copy of the weights so that it streams from
HBM): the Q/K/V, WO, gate/up (both matrices' rows), down and head shapes of TinyLlama-1.1B and
Llama-2-7B for Q4_0, Q5_0 and Q8_0, with the GGUF matrix bytes/s as a fraction of the 6.29 TB/s
measured copy rate and the time relative to Q8_0 (which reads 34 bytes where Q4_0 reads 18 and Q5_0
22).  The streaming dgemv_kernel roles of the decode step are not timed one by one (no op entry
point times them); they are in the end-to-end figure.

End to end, on synthetic TinyLlama-1.1B models (Q4_0, Q5_0, and Q8_0 for comparison): decode
tokens/s over --steps graph-replayed steps after a 32-token prompt; a 512-token prefill; a 20-token
MI_OUT_ALL.  Every figure is the median of --repeat timings, all of them listed.

    python scripts/legacy_quant_bench.py [--iters 100] [--steps 128] [--repeat 5] [--out profiles/legacy_quant_bench.json]
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
Q4_0, Q5_0, Q8_0 = 2, 6, 8
TYPES = {"Q4_0": Q4_0, "Q5_0": Q5_0, "Q8_0": Q8_0}
LAUNCHES = {
    "tinyllama-1.1b": [("qkv", 2048 + 2 * 256, 2048), ("wo", 2048, 2048), ("gate_up", 2 * 5632, 2048),
                       ("down", 2048, 5632), ("head_32000", 32000, 2048)],
    "llama2-7b": [("qkv", 3 * 4096, 4096), ("wo", 4096, 4096), ("gate_up", 2 * 11008, 4096),
                  ("down", 4096, 11008), ("head_32000", 32000, 4096)],
}


def timed(f, repeat):
    ts = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        f()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def end_to_end(cfg, args, engine, synthetic):
    model = engine.Model(synthetic.build_gguf(cfg, seed=0))
    wb = int(engine.lib().mi_model_weight_bytes(model.h))
    rng = np.random.default_rng(0)
    res = {"weight_bytes": wb}
    ctx = engine.Context(model, n_ctx=1024)
    res["decode_path"] = ctx.decode_path()
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
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from blama_amd import engine, gguf, synthetic

    out = {"iters": args.iters, "hbm_copy_bytes_s": HBM_COPY, "launches": {}, "models": {}}
    for model, launches in LAUNCHES.items():
        rows_out = {}
        for tag, rows, K in launches:
            per = {}
            for tname, t in TYPES.items():
                nbytes = gguf.tensor_nbytes(t, (K, rows))
                raw = np.empty(nbytes, np.uint8)
                synthetic.fill_quant(raw, t, np.random.default_rng(rows + K + t))
                us = engine.op_gemv_bench(t, raw, rows, K, args.iters)
                per[tname] = {"matrix_bytes": nbytes, "median_us": round(us, 3),
                              "frac_of_copy_rate": round(nbytes / (us * 1e-6) / HBM_COPY, 4)}
            for tname in ("Q4_0", "Q5_0"):
                per[tname]["time_vs_q8_0"] = round(per[tname]["median_us"] / per["Q8_0"]["median_us"], 4)
                per[tname]["bytes_vs_q8_0"] = round(per[tname]["matrix_bytes"] / per["Q8_0"]["matrix_bytes"], 4)
            rows_out[tag] = {"rows": rows, "K": K, **per}
        out["launches"][model] = rows_out
    cfgs = [("tinyllama-1.1b-q4_0", synthetic.LEGACY_CONFIGS["tinyllama-1.1b-q4_0"]),
            ("tinyllama-1.1b-q5_0", synthetic.LEGACY_CONFIGS["tinyllama-1.1b-q5_0"]),
            ("tinyllama-1.1b-q8_0", synthetic.CONFIGS["tinyllama-1.1b-q8_0"])]
    for name, cfg in cfgs:
        out["models"][name] = end_to_end(cfg, args, engine, synthetic)
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
