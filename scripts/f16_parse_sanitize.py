#!/usr/bin/env python3
"""Builds tests/cpp/t_f16_parse.cpp with the engine's GGUF parser and model loader (model.cpp, with
Model::check_f16) under -fsanitize=address,undefined -- host code only, the rest of the engine comes
from the built libmi_engine.so -- and runs it over the headers of the F16 configs, the files the F16
path must refuse (tests/test_f16_load.py's) and every truncation of each.  No GPU is used.

    python scripts/f16_parse_sanitize.py [--keep DIR]"""
import argparse
import os
import subprocess
import sys
import tempfile
from dataclasses import replace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
from blama_amd import synthetic  # noqa: E402

F32, F16, Q8_0, BF16 = 0, 1, 8, 30


def images():
    S = synthetic
    cfg = S.F16_CONFIGS["tiny-f16"]
    hdr = lambda c, **kw: S.build_gguf(c, header_only=True, **kw)   # noqa: E731
    for name in ("tiny-f16", "tiny-f16-hd128", "tiny-rf-f16"):
        yield "ok", hdr(S.F16_CONFIGS[name])
    yield "ok", hdr(S.CONFIGS["tiny-q4_k_m"])
    yield "bad", hdr(cfg, types_override={n: BF16 for n, t in S.tensor_types(cfg).items() if t == F16})
    yield "bad", hdr(cfg, types_override={"blk.0.attn_q.weight": F32})
    yield "bad", hdr(cfg, types_override={"blk.1.attn_v.weight": Q8_0})
    yield "bad", hdr(S.CONFIGS["tiny-q8_0"], types_override={"output.weight": F16})
    yield "bad", hdr(replace(cfg, n_expert=4, n_expert_used=2))
    yield "bad", hdr(replace(S.CONFIGS["tiny-gpt2-q6_k"], ftype="F16"))
    yield "bad", hdr(replace(cfg, n_ff=776))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keep", default=None)
    args = ap.parse_args()
    d = args.keep or tempfile.mkdtemp(prefix="f16_parse_")
    os.makedirs(d, exist_ok=True)
    files = []
    for i, (kind, img) in enumerate(images()):
        p = os.path.join(d, f"{kind}{i:02d}.gguf")
        img.tofile(p)
        files.append(f"{kind}:{p}")
    exe = os.path.join(d, "t_f16_parse")
    csrc = os.path.join(ROOT, "blama_amd", "csrc")
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-x", "hip", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer",
           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(ROOT, "include"), "-I", csrc,
           os.path.join(ROOT, "tests", "cpp", "t_f16_parse.cpp"), os.path.join(csrc, "model.cpp"),
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
