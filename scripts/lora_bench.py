#!/usr/bin/env python3
"""Decode cost of a LoRA adapter: ms/step of batch-1 decode on a Llama-2-7B-shaped Q4_K_M synthetic
model with and without a rank-16 F16 adapter on all seven per-layer targets, on the same build and
context, and the adapter's bytes per step over 8 TB/s as the floor the difference is compared with.

    python scripts/lora_bench.py [--steps 128] [--warmup 16] [--rank 16] [--out profiles/lora_bench.json]
Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from blama_amd import engine, synthetic  # noqa: E402

HBM_BYTES_PER_S = 8e12


def ms_per_step(ctx, tokens, warmup, steps):
    ctx.kv_clear()
    ctx.decode(tokens[:32])
    for t in tokens[32:32 + warmup]:
        ctx.decode([t])
    ctx.logits()
    t0 = time.perf_counter()
    for t in tokens[32 + warmup:32 + warmup + steps]:
        ctx.decode([t])
    ctx.logits()   # synchronises
    return (time.perf_counter() - t0) * 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="llama2-7b-q4_k_m")
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--rank", type=int, default=16)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    cfg = synthetic.CONFIGS[args.config]
    model = engine.Model(synthetic.build_gguf(cfg, seed=0))
    img = synthetic.write_lora_gguf(None, cfg, synthetic.LORA_TARGETS, args.rank, 2.0 * args.rank, np.float16, 1, std=0.01)
    lora = engine.Lora(model, img)
    ctx = engine.Context(model, n_ctx=512)
    tokens = [int(t) for t in np.random.default_rng(0).integers(0, cfg.n_vocab, 32 + args.warmup + args.steps)]
    base, on = [], []
    for _ in range(args.repeat):   # alternated: both legs see the same drift
        ctx.clear_lora()
        base.append(ms_per_step(ctx, tokens, args.warmup, args.steps))
        ctx.set_lora(lora, 1.0)
        on.append(ms_per_step(ctx, tokens, args.warmup, args.steps))
    kv_dim = cfg.n_head_kv * cfg.head_dim
    shapes = [(cfg.n_embd, cfg.n_embd), (cfg.n_embd, kv_dim), (cfg.n_embd, kv_dim), (cfg.n_embd, cfg.n_embd),
              (cfg.n_embd, cfg.n_ff), (cfg.n_embd, cfg.n_ff), (cfg.n_ff, cfg.n_embd)]
    adapter_bytes = cfg.n_layer * sum((k + rows) * args.rank * 2 for k, rows in shapes)
    out = {
        "config": args.config, "rank": args.rank, "dtype": "f16", "targets": list(synthetic.LORA_TARGETS),
        "steps": args.steps, "decode_path": int(engine.lib().mi_decode_path(ctx.h)),
        "ms_per_step_base": [round(v, 4) for v in base], "ms_per_step_lora": [round(v, 4) for v in on],
        "added_ms_per_step": round(min(on) - min(base), 4),
        "added_launches_per_layer": 4,
        "added_us_per_launch": round((min(on) - min(base)) * 1e3 / (4 * cfg.n_layer), 3),
        "adapter_bytes_per_step": adapter_bytes,
        "floor_ms_at_8TBps": round(adapter_bytes / HBM_BYTES_PER_S * 1e3, 4),
        "weight_bytes_per_step": int(model.weight_bytes),
    }
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
