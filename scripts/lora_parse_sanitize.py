#!/usr/bin/env python3
"""Builds tests/cpp/t_lora_parse.cpp with the engine's GGUF parser and adapter loader (model.cpp,
lora.cpp) under -fsanitize=address,undefined -- host code only, the rest of the engine comes from
the built libmi_engine.so -- and runs it over a good adapter, the malformed images of
tests/test_lora_load.py and their truncations, on a vocab_only model.  No GPU is used.

    python scripts/lora_parse_sanitize.py [--keep DIR]"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]
from blama_amd import synthetic  # noqa: E402
import test_lora_load as T  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keep", default=None)
    args = ap.parse_args()
    d = args.keep or tempfile.mkdtemp(prefix="lora_parse_")
    os.makedirs(d, exist_ok=True)
    cfg = synthetic.CONFIGS[T.CFG]
    model = os.path.join(d, "model.gguf")
    synthetic.build_gguf(cfg, seed=1, header_only=True).tofile(model)
    files = []
    good = os.path.join(d, "good.gguf")
    synthetic.write_lora_gguf(good, cfg, rank=12, alpha=8.0, dtype=np.float16, seed=2)
    files.append("ok:" + good)
    r128 = os.path.join(d, "r128.gguf")
    T._image(T._ab(r=128)).tofile(r128)
    files.append("ok:" + r128)
    cases = T.test_rejections.pytestmark[0].args[1]
    for i, (what, img, _) in enumerate(cases):
        p = os.path.join(d, f"bad{i:02d}.gguf")
        img().tofile(p)
        files.append("bad:" + p)
    exe = os.path.join(d, "t_lora_parse")
    csrc = os.path.join(ROOT, "blama_amd", "csrc")
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-x", "hip", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer",
           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(ROOT, "include"), "-I", csrc,
           os.path.join(ROOT, "tests", "cpp", "t_lora_parse.cpp"), os.path.join(csrc, "lora.cpp"), os.path.join(csrc, "model.cpp"),
           "-fsanitize=address,undefined", "-L", os.path.join(ROOT, "blama_amd"), "-lmi_engine",
           "-Wl,-rpath," + os.path.join(ROOT, "blama_amd"), "-o", exe]
    subprocess.run(cmd, check=True)
    r = subprocess.run([exe, model] + files, capture_output=True, text=True)
    print(r.stdout[-6000:])
    print(r.stderr[-6000:], file=sys.stderr)
    print(f"exit status {r.returncode}; {len(files)} images")
    return r.returncode


if __name__ == "__main__":
    sys.exit(main())
