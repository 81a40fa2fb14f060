#!/usr/bin/env python3
"""Several sequences per encoder call against one mi_decode per sequence, on synthetic full-depth
BERT shapes (bge-small: 384 / 12 heads of 32 / 1536, 12 layers; bge-large: 1024 / 16 heads of 64 /
4096, 24 layers).  A caller wants one pooled (CLS) vector per sequence, so both forms read every
vector back: the loop is decode + embeddings() per sequence, the batch is one encode() and
embeddings_seq(i) per sequence.  Host clock around work that ends in a synchronise; median of
--reps after --warmup.

  python scripts/enc_seqs_bench.py [--large] [--out profiles/enc_seqs_bench.json]
  rocprofv3 --kernel-trace --stats -d DIR -o enc -- python scripts/enc_seqs_bench.py --trace batch --workload 64x64
      two passes of one workload in one form (batch | loop), or (--trace attn) one 512-token sequence
      through each attention kernel, for the per-kernel device times (DIR/enc_kernel_stats.csv)
  python scripts/enc_seqs_bench.py --merge-stats DIR/enc_kernel_stats.csv --out FILE
      adds the trace's per-kernel figures to FILE

On a build without mi_encode_seqs only the loop is timed (the same script times the parent)."""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from blama_amd import engine, synthetic  # noqa: E402

SHAPES = {
    "bge-small": synthetic.BertConfig("bge-small", 512, 384, 12, 12, 1536, 512, pooling_type=2),
    "bge-large": synthetic.BertConfig("bge-large", 512, 1024, 24, 16, 4096, 512, pooling_type=2),
}
WORKLOADS = [(64, 64), (16, 512)]      # sequences x tokens


def median_ms(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": float(np.median(t)), "min_ms": float(min(t)), "max_ms": float(max(t))}


def run(name, args):
    cfg = SHAPES[name]
    model = engine.Model(synthetic.build_bert_gguf(cfg, seed=3), device=0)
    has_batch = hasattr(engine.Context, "encode")
    res = {}
    for n_seq, n_tok in WORKLOADS:
        if args.workload not in (None, f"{n_seq}x{n_tok}"):
            continue
        rng = np.random.default_rng(n_seq)
        seqs = [rng.integers(0, cfg.n_vocab, n_tok).astype(np.int32) for _ in range(n_seq)]
        ctx = engine.Context(model, n_ctx=n_seq * n_tok, n_batch=n_seq * n_tok)

        def loop():
            return [ctx.decode(s) or ctx.embeddings() for s in seqs]

        def batch():
            ctx.encode(seqs)
            return [ctx.embeddings_seq(i) for i in range(n_seq)]

        if args.trace == "attn":
            ctx.close()
            continue
        if args.trace:
            for _ in range(2):
                (batch if args.trace == "batch" else loop)()
            ctx.close()
            continue
        r = {"loop": median_ms(loop, args.warmup, args.reps)}
        if has_batch:
            r["batch"] = median_ms(batch, args.warmup, args.reps)
            r["loop_over_batch"] = r["loop"]["median_ms"] / r["batch"]["median_ms"]
            d = max(float(np.abs(a - b).max()) for a, b in zip(loop(), batch()))
            r["max_abs_diff_loop_vs_batch"] = d
        res[f"{n_seq}x{n_tok}"] = r
        print(name, f"{n_seq}x{n_tok}", json.dumps(r), flush=True)
        ctx.close()
    if args.trace == "attn":           # kernel against kernel: one 512-token sequence
        hd, nh = cfg.n_embd // cfg.n_head, cfg.n_head
        rng = np.random.default_rng(5)
        q = rng.standard_normal((512, nh, hd)).astype(np.float32)
        k16 = rng.standard_normal((512, nh * hd)).astype(np.float16)
        for _ in range(3):
            engine.op_attention_enc(q, k16, k16)
            engine.op_attention_enc_seqs(q, k16, k16, (512,))
    return res


def merge_stats(path, out):
    doc = json.load(open(out)) if os.path.exists(out) else {}
    rows = list(csv.DictReader(open(path)))
    doc["kernel_stats"] = [{"kernel": r["Name"][:90], "calls": int(r["Calls"]), "avg_us": float(r["AverageNs"]) / 1e3,
                            "total_ms": float(r["TotalDurationNs"]) / 1e6} for r in rows if "enc_" in r["Name"] or "embd_" in r["Name"]]
    json.dump(doc, open(out, "w"), indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--large", action="store_true", help="also the bge-large shape")
    ap.add_argument("--only-large", action="store_true")
    ap.add_argument("--trace", choices=("batch", "loop", "attn"), default=None)
    ap.add_argument("--workload", default=None, help="64x64 or 16x512 (default: both)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "enc_seqs_bench.json"))
    ap.add_argument("--merge-stats", default=None)
    args = ap.parse_args()
    if args.merge_stats:
        return merge_stats(args.merge_stats, args.out)
    names = ["bge-large"] if args.only_large else ["bge-small"] + (["bge-large"] if args.large else [])
    doc = {"device": "MI355X", "timing": "host clock around decode/encode + every vector read back (synchronises)",
           "results": {n: run(n, args) for n in names}}
    if not args.trace:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        json.dump(doc, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
