#!/usr/bin/env python3
"""Measurements of the IQ4_XS / IQ4_NL paths, each beside Q4_K at the same shape, in one process.

Per launch, at the shapes of Llama-2-7B (Q/K/V as one matrix of 3 x 4096 rows, WO, gate/up, down, the
32000-row head), as IQ4_XS, IQ4_NL and Q4_K, --repeat times each, the types alternating; a timing is
the median device time between two events of --iters launches after a warm-up, every launch reading
another copy of the weights so that it streams from HBM; the median of the repeats and their spread
(max - min) are written next to each other.  IQ4_XS streams 136 bytes where Q4_K streams 144 (IQ4_NL:
144).
  dgemv:   the decode step's streaming dgemv_kernel (mi_op_dgemv_bench) in the role the step gives
           the shape: Q/K/V, WO + residual, gate/up SwiGLU, down + residual quantising in the launch
           (16-wave workgroups), head store
  gemv:    gemv_kernel's store form (mi_op_gemv_bench), the r04 step's launch
  gemm:    mi_op_gemm_bench over 512 tokens (the tiled MFMA GEMM) and 20 tokens (the short split-K
           GEMM with its part sum); gate/up as the pair launch; the head at 20 tokens only

End to end, on synthetic TinyLlama-1.1B models (llama-quantize's IQ4_XS mix, and Q4_K throughout as the
yardstick): decode tokens/s over --steps steps after a 32-token prompt; a 512-token prefill; a 20-token
MI_OUT_ALL; host clock around calls that end in a device synchronise, every repeat listed.

    python scripts/iq4_bench.py [--iters 100] [--steps 128] [--repeat 15] [--out profiles/iq4_bench.json] [--models-only]
Prints one JSON line."""
import argparse
import json
import os
import re
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from legacy_quant_bench import HBM_COPY, end_to_end  # noqa: E402

TYPES = {"IQ4_XS": 23, "IQ4_NL": 20, "Q4_K": 12}
# tag, rows (of each matrix of a pair), K, pair, mi_op_dgemv role
LAUNCHES = [("qkv", 3 * 4096, 4096, False, 0), ("wo", 4096, 4096, False, 1), ("gate_up", 11008, 4096, True, 2),
            ("down", 4096, 11008, False, 5), ("head_32000", 32000, 4096, False, 3)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--repeat", type=int, default=15)
    ap.add_argument("--out", default=None)
    ap.add_argument("--models-only", action="store_true", help="re-measure the end-to-end legs into the existing --out file")
    args = ap.parse_args()
    from blama_amd import engine, gguf, synthetic

    out = {"iters": args.iters, "repeat": args.repeat, "hbm_copy_bytes_s": HBM_COPY, "dgemv": {}, "gemv": {}, "gemm": {},
           "models": {}}
    if args.models_only:
        with open(args.out) as f:
            out = json.load(f)

    def record(section, tag, info, nbytes, run):
        """run(type name) -> us, --repeat times, the types alternating."""
        us = {n: [] for n in TYPES}
        for _ in range(args.repeat):
            for tname in TYPES:
                us[tname].append(round(run(tname), 3))
        per = {}
        for tname in TYPES:
            med = statistics.median(us[tname])
            per[tname] = {"matrix_bytes": nbytes[tname], "us": us[tname], "median_us": med,
                          "spread_us": round(max(us[tname]) - min(us[tname]), 3),
                          "frac_of_copy_rate": round(nbytes[tname] / (med * 1e-6) / HBM_COPY, 4)}
        for tname in ("IQ4_XS", "IQ4_NL"):
            per[f"{tname.lower()}_time_vs_q4_k"] = round(per[tname]["median_us"] / per["Q4_K"]["median_us"], 4)
        out[section][tag] = {**info, **per}
        print(section, tag, {n: (per[n]["median_us"], per[n]["spread_us"]) for n in TYPES}, file=sys.stderr, flush=True)

    for tag, rows, K, pair, role in ([] if args.models_only else LAUNCHES):
        raw, up, t, nbytes = {}, {}, TYPES, {}
        for tname in TYPES:
            mats = []
            for i in range(2 if pair else 1):
                mats.append(np.empty(gguf.tensor_nbytes(t[tname], (K, rows)), np.uint8))
                synthetic.fill_quant(mats[-1], t[tname], np.random.default_rng(rows + K + t[tname] + i))
            raw[tname], up[tname] = mats[0], mats[1] if pair else None
            nbytes[tname] = int(sum(m.size for m in mats))
        info = {"rows": rows, "K": K, "pair": pair}
        record("dgemv", tag, {**info, "role": role}, nbytes, lambda n: engine.op_dgemv_bench(
            role, t[n], raw[n], rows, K, type2=t[n], raw2=up[n], rows2=rows, iters=args.iters))
        both = {n: raw[n] if not pair else np.concatenate([raw[n], up[n]]) for n in TYPES}
        record("gemv", tag, info, nbytes, lambda n: engine.op_gemv_bench(t[n], both[n], rows * (2 if pair else 1), K, args.iters))
        for ntok in (512, 20):
            if ntok == 20 or not tag.startswith("head"):
                record("gemm", f"{tag}_x{ntok}", {**info, "ntok": ntok}, nbytes, lambda n: engine.op_gemm_bench(
                    t[n], raw[n], rows, K, ntok, raw_up=up[n], iters=args.iters))
    args.repeat = min(args.repeat, 5)   # the end-to-end legs: five timings each
    for name, table in (("tinyllama-1.1b-iq4_xs", synthetic.IQ4_CONFIGS), ("tinyllama-1.1b-q4_k", synthetic.Q3K_CONFIGS)):
        out["models"][name] = end_to_end(table[name], args, engine, synthetic)
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            text = json.dumps(out, indent=1)   # the lists of timings on one line each
            f.write(re.sub(r"\[\s+([-\d.,\s]+?)\s+\]", lambda m: "[" + " ".join(m.group(1).split()) + "]", text) + "\n")


if __name__ == "__main__":
    main()
