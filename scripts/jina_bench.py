#!/usr/bin/env python3
"""Measurements for the jina-bert-v2 work, written to profiles/jina_bench.json.

  python scripts/jina_bench.py [--out FILE]
      call times at jina-embeddings-v2-small-en's and -base-en's full-depth shapes (4 layers x 512 x 8 heads and
      12 layers x 768 x 12 heads, head_dim 64, synthetic weights): one mi_decode at n = 512, 2048, 8192 (the short,
      the long and the 128-query attention kernel).  Host clock around a call that ends in a read of the pooled row
      (a synchronise); each shape is repeated until its timed window is --window seconds; median, min, max.
  rocprofv3 --kernel-trace --output-format csv -d DIR -o run -- python scripts/jina_bench.py --ops
      the attention kernels alone, through mi_op_attention_enc_alibi at 12 heads x 64: OP_CASES below, each with
      max_bias 8 (the ALiBi variant) and 0 (the kernel without it), --op-reps launches per case after --op-warmup.
      A run of its own, no counters.
  python scripts/jina_bench.py --merge-trace DIR [--out FILE]
      the device time of every launch of that run from DIR's kernel trace (End - Start), assigned to the cases by
      launch order: median, min and max in us, and ps per (query, key) pair of one head = time / (12 x sum len^2)
  python scripts/jina_bench.py --merge-bench DIR [--out FILE]
      bench.py's tokens/s from DIR/bench_{new,parent}_*.log (alternating runs of this tree and of the parent commit)"""
import argparse
import csv
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from blama_amd import engine, synthetic  # noqa: E402

SHAPES = {"small": synthetic.JinaConfig("jina-v2-small", 512, 512, 4, 8, 2048, 8192, pooling_type=1),
          "base": synthetic.JinaConfig("jina-v2-base", 512, 768, 12, 12, 3072, 8192, pooling_type=1)}
N_HEAD, HD = 12, 64
# (label, sequence lengths, kernel): the issue's three ALiBi shapes, and the new kernel at 4096 and 8192 tokens
OP_CASES = [("64x64", (64,) * 64, "enc_attn_seq_kernel"), ("16x512", (512,) * 16, "enc_attn_seq_kernel"),
            ("1x2048", (2048,), "enc_attn_long_kernel"), ("1x4096", (4096,), "enc_attn_xlong_kernel"),
            ("1x8192", (8192,), "enc_attn_xlong_kernel")]
BIASES = (("alibi", 8.0), ("plain", 0.0))


def stats(t):
    return {"median": float(np.median(t)), "min": float(min(t)), "max": float(max(t)), "n": len(t)}


def timed_ms(fn, window):
    for _ in range(3):
        fn()
    t0 = time.perf_counter()
    fn()
    reps = max(15, int(window / max(time.perf_counter() - t0, 1e-5)))
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return {k + ("_ms" if k != "n" else ""): v for k, v in stats(t).items()}


def calls(kind, args):
    cfg = SHAPES[kind]
    model = engine.Model(synthetic.build_jina_gguf(cfg, seed=3), device=0)
    ctx = engine.Context(model, n_ctx=8192, n_batch=8192)
    rng = np.random.default_rng(0)
    res = {}
    for n in (512, 2048, 8192):
        t = rng.integers(0, cfg.n_vocab, n).astype(np.int32)
        res[f"decode_{n}"] = timed_ms(lambda: ctx.decode(t) or ctx.embeddings(), args.window)
    ctx.close()
    model.close()
    return res


def ops(args):
    rng = np.random.default_rng(0)
    for _, lens, _ in OP_CASES:
        n = sum(lens)
        q = (rng.standard_normal((n, N_HEAD, HD)) * 0.6).astype(np.float32)
        k16 = (rng.standard_normal((n, N_HEAD * HD)) * 0.6).astype(np.float16)
        v16 = rng.standard_normal((n, N_HEAD * HD)).astype(np.float16)
        for _, bias in BIASES:
            for _ in range(args.op_warmup + args.op_reps):
                engine.op_attention_enc_alibi(q, k16, v16, lens, bias)


def merge_trace(d, args, res):
    paths = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    rows = [r for p in paths for r in csv.DictReader(open(p)) if "enc_attn" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    per = args.op_warmup + args.op_reps
    if len(rows) != per * len(OP_CASES) * len(BIASES):
        raise SystemExit(f"{len(rows)} attention launches in the trace, expected {per * len(OP_CASES) * len(BIASES)}")
    out, i = {}, 0
    for label, lens, kernel in OP_CASES:
        pairs = N_HEAD * sum(n * n for n in lens)
        for bname, _ in BIASES:
            chunk = rows[i + args.op_warmup:i + per]
            i += per
            if not all(kernel in r["Kernel_Name"] for r in chunk):
                raise SystemExit(f"{label} {bname}: expected {kernel}, the trace has {chunk[0]['Kernel_Name']}")
            us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in chunk]
            s = stats(us)
            out[f"{label}_{bname}"] = {"kernel": kernel, "median_us": s["median"], "min_us": s["min"], "max_us": s["max"],
                                       "n": s["n"], "ps_per_query_key_pair": s["median"] * 1e6 / pairs}
    res["attention_kernels"] = {"shape": f"{N_HEAD} heads x {HD}, device time per launch from a rocprofv3 kernel trace", "cases": out}


def merge_bench(d, res):
    out = {}
    for who in ("new", "parent"):
        vals = []
        for p in sorted(glob.glob(os.path.join(d, f"bench_{who}_*.log"))):
            line = [x for x in open(p).read().splitlines() if x.startswith("{")][-1]
            vals.append(float(json.loads(line)["value"]))
        out[who] = {"tokens_per_s": vals, "median": float(np.median(vals)), "min": min(vals), "max": max(vals)}
    res["bench_py"] = {"what": "bench.py --gpus 1 --steps 64 --warmup 8, this tree and the parent commit alternating", **out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jina_bench.json"))
    ap.add_argument("--window", type=float, default=2.0)
    ap.add_argument("--op-warmup", type=int, default=5)
    ap.add_argument("--op-reps", type=int, default=40)
    ap.add_argument("--ops", action="store_true")
    ap.add_argument("--merge-trace")
    ap.add_argument("--merge-bench")
    args = ap.parse_args()
    if args.ops:
        return ops(args)
    res = json.load(open(args.out)) if os.path.exists(args.out) else {}
    if args.merge_trace:
        merge_trace(args.merge_trace, args, res)
    elif args.merge_bench:
        merge_bench(args.merge_bench, res)
    else:
        res["shapes"] = {k: f"{c.n_embd} / {c.n_head} heads of 64 / {c.n_ff}, {c.n_layer} layers, F16, synthetic weights"
                         for k, c in SHAPES.items()}
        res["calls"] = {k: calls(k, args) for k in SHAPES}
    json.dump(res, open(args.out, "w"), indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "shapes"}, indent=1)[-3000:])


if __name__ == "__main__":
    main()
