#!/usr/bin/env python3
"""Builds tests/cpp/t_legacy_quant_parse.cpp with the engine's GGUF parser and model loader
(model.cpp, with Model::check_types) under -fsanitize=address,undefined -- host code only, the rest
of the engine comes from the built libmi_engine.so -- and runs it over the headers of the Q4_0 /
Q5_0 configs, a k-quant file with a Q5_0 matrix, the files the loader must refuse
(tests/test_legacy_quant_load.py's) and every truncation of each.  No GPU is used.

    python scripts/legacy_quant_parse_sanitize.py [--keep DIR]"""
import argparse
import os
import subprocess
import sys
import tempfile
from dataclasses import replace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
from blama_amd import synthetic  # noqa: E402

Q4_0, Q4_1, Q5_0, Q5_1 = 2, 3, 6, 7


def images():
    S = synthetic
    hdr = lambda c, **kw: S.build_gguf(c, header_only=True, **kw)   # noqa: E731
    for name in ("tiny-q4_0", "tiny-q5_0", "tiny-hd32-q4_0", "tiny-hd32-q5_0"):
        yield "ok", hdr(S.LEGACY_CONFIGS[name])
    q4km = S.CONFIGS["tiny-q4_k_m"]
    yield "ok", hdr(q4km, types_override={"blk.1.ffn_down.weight": Q5_0})
    yield "bad=blk.1.ffn_down.weight,Q4_1", hdr(q4km, types_override={"blk.1.ffn_down.weight": Q4_1})
    yield "bad=blk.0.attn_v.weight,Q5_1", hdr(S.LEGACY_CONFIGS["tiny-q4_0"], types_override={"blk.0.attn_v.weight": Q5_1})
    yield "bad=_exps.weight,Q4_0,MoE", hdr(replace(S.CONFIGS["tiny-moe-q5_k_m"], ftype="Q4_0"))
    yield "bad=blk.1.ffn_up_exps.weight,Q5_0,MoE", hdr(S.CONFIGS["tiny-moe-q5_k_m"],
                                                        types_override={"blk.1.ffn_up_exps.weight": Q5_0})
    yield "bad=.weight,Q4_0,GPT-2", hdr(replace(S.CONFIGS["tiny-gpt2-q6_k"], ftype="Q4_0"))
    yield "bad=blk.1.attn_q.weight,Q5_0,BERT", S.build_bert_gguf(S.BERT_CONFIGS["bert-w"], header_only=True,
                                                                 types={"blk.1.attn_q.weight": Q5_0})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keep", default=None)
    args = ap.parse_args()
    d = args.keep or tempfile.mkdtemp(prefix="legacy_parse_")
    os.makedirs(d, exist_ok=True)
    files = []
    for i, (kind, img) in enumerate(images()):
        p = os.path.join(d, f"img{i:02d}.gguf")
        img.tofile(p)
        files.append(f"{kind}:{p}")
    exe = os.path.join(d, "t_legacy_quant_parse")
    csrc = os.path.join(ROOT, "blama_amd", "csrc")
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-x", "hip", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer",
           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(ROOT, "include"), "-I", csrc,
           os.path.join(ROOT, "tests", "cpp", "t_legacy_quant_parse.cpp"), os.path.join(csrc, "model.cpp"),
           "-fsanitize=address,undefined", "-L", os.path.join(ROOT, "blama_amd"), "-lmi_engine",
           "-Wl,-rpath," + os.path.join(ROOT, "blama_amd"), "-o", exe]
    subprocess.run(cmd, check=True)
    r = subprocess.run([exe] + files, capture_output=True, text=True)
    print(r.stdout[-6000:])
    print(r.stderr[-6000:], file=sys.stderr)
    print(f"exit status {r.returncode}; {len(files)} images")
    return r.returncode


if __name__ == "__main__":
    sys.exit(main())
