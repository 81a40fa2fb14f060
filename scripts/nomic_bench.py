#!/usr/bin/env python3
"""The nomic-bert encoder pass at nomic-embed-text's full-depth shape (768 / 12 heads of 64 / 3072, 12
layers, synthetic weights) and a synthetic BERT model of the same widths.  Host clock around a call
that ends in a read of the pooled row (a synchronise); median, min and max of --reps after --warmup.

  python scripts/nomic_bench.py [--out profiles/nomic_bench.json]
      call times: one mi_decode at n = 128, 512, 2048 (BERT: 128, 512), mi_encode_seqs of 16 x 512 and 4 x 2048
  rocprofv3 --kernel-trace --stats -d DIR -o nomic -- python scripts/nomic_bench.py --trace nomic:2048
      three passes of one workload (nomic:N or bert:N, one mi_decode of N tokens; nomic:N:seqs: one
      mi_encode_seqs call of one N-token sequence, the segmented attention) for the per-kernel
      device times (DIR/nomic_kernel_stats.csv); a run of its own, no counters
  python scripts/nomic_bench.py --merge-stats nomic:2048=DIR/nomic_kernel_stats.csv --out FILE
      adds the trace's encoder kernels to FILE; for the attention kernels also the time per (query, key)
      pair of one head: average ns / (heads x N x N)"""
import argparse
import csv
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from blama_amd import engine, synthetic  # noqa: E402

N_LAYER, N_HEAD = 12, 12
NOMIC = synthetic.NomicConfig("nomic-embed", 512, 768, N_LAYER, N_HEAD, 3072, 2048, pooling_type=1)
BERT = synthetic.BertConfig("bert-768", 512, 768, N_LAYER, N_HEAD, 3072, 512, pooling_type=1)


def load(kind):
    if kind == "nomic":
        return NOMIC, engine.Model(synthetic.build_nomic_gguf(NOMIC, seed=3), device=0)
    return BERT, engine.Model(synthetic.build_bert_gguf(BERT, seed=3), device=0)


def median_ms(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": float(np.median(t)), "min_ms": float(min(t)), "max_ms": float(max(t))}


def calls(kind, args):
    cfg, model = load(kind)
    ctx = engine.Context(model, n_ctx=8192, n_batch=8192)
    rng = np.random.default_rng(0)
    res = {}
    for n in (128, 512, 2048):
        if n > cfg.n_ctx_train:
            continue
        t = rng.integers(0, cfg.n_vocab, n).astype(np.int32)
        res[f"decode_{n}"] = median_ms(lambda: ctx.decode(t) or ctx.embeddings(), args.warmup, args.reps)
    for n_seq, n in ((16, 512), (4, 2048)):
        if n > cfg.n_ctx_train:
            continue
        seqs = [rng.integers(0, cfg.n_vocab, n).astype(np.int32) for _ in range(n_seq)]
        res[f"encode_{n_seq}x{n}"] = median_ms(lambda: ctx.encode(seqs) or ctx.embeddings_seq(n_seq - 1), args.warmup, args.reps)
    ctx.close()
    model.close()
    return res


def trace(spec):
    kind, n = spec.split(":")[:2]
    cfg, model = load(kind)
    ctx = engine.Context(model, n_ctx=2048, n_batch=2048)
    t = np.random.default_rng(0).integers(0, cfg.n_vocab, int(n)).astype(np.int32)
    for _ in range(3):
        if spec.endswith(":seqs"):      # the same tokens as a one-sequence mi_encode_seqs call: the segmented kernels
            ctx.encode([t])
            ctx.embeddings_seq(0)
        else:
            ctx.decode(t)
            ctx.embeddings()
    ctx.close()


def merge(spec, out):
    key, path = spec.split("=")
    n = int(key.split(":")[1])
    res = json.load(open(out)) if os.path.exists(out) else {}
    ks = {}
    for r in csv.DictReader(open(path)):
        name = r["Name"]
        if "enc_" not in name and "embd_" not in name:
            continue
        short = re.search(r"(\w+_kernel(<[^>]*>)?)", name).group(1)
        ks[short] = {"calls": int(r["Calls"]), "avg_us": float(r["AverageNs"]) / 1e3, "min_us": float(r["MinNs"]) / 1e3,
                     "max_us": float(r["MaxNs"]) / 1e3}
        if "attn" in short:
            ks[short]["ps_per_query_key_pair"] = float(r["AverageNs"]) * 1e3 / (N_HEAD * n * n)
    res.setdefault("kernels", {})[key] = ks
    json.dump(res, open(out, "w"), indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nomic_bench.json"))
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--trace")
    ap.add_argument("--merge-stats")
    args = ap.parse_args()
    if args.trace:
        return trace(args.trace)
    if args.merge_stats:
        return merge(args.merge_stats, args.out)
    res = json.load(open(args.out)) if os.path.exists(args.out) else {}
    res["shape"] = "768 / 12 heads of 64 / 3072, 12 layers, F16, synthetic weights"
    res["calls"] = {"nomic": calls("nomic", args), "bert": calls("bert", args)}
    json.dump(res, open(args.out, "w"), indent=1)
    print(json.dumps(res["calls"], indent=1))


if __name__ == "__main__":
    main()
