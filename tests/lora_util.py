"""LoRA reference for the tests: the CPU oracle with llama-graph.cpp's build_lora_mm (llama.cpp
b5187) on every mul_mat of a targeted tensor, y = W cur + s * (B (A cur)) for each adapter set, with
s = scale * alpha / r (alpha 0: s = scale).  An F16 matrix has its f32 operand rounded to f16
first (ggml's mul_mat with an F16 src0); the sums are taken in f64.  llama.cpp itself is not
available to these tests: parity with its LoRA arithmetic is pinned to this restatement."""
import numpy as np

import ggml_ref as R
import util
from blama_amd import gguf
from cvec_util import CvecOracle
from util import oracle_from_gguf


class Adapter:
    """One adapter as the oracle reads it: {base tensor name: (A [r][K], B [rows][r])}, alpha."""

    def __init__(self, pairs, alpha):
        self.pairs = dict(pairs)
        self.alpha = float(alpha)

    @classmethod
    def from_gguf(cls, img):
        rd = gguf.GGUFReader(img)
        pairs = {}
        for name, t in rd.tensors.items():
            if not name.endswith(".lora_a"):
                continue
            base = name[:-7]
            b = rd.tensors[base + ".lora_b"]

            def arr(x):
                dt = np.float16 if x.type == R.F16 else np.float32
                return np.ascontiguousarray(x.data).view(dt).reshape(x.shape[1], x.shape[0])
            pairs[base] = (arr(t), arr(b))
        return cls(pairs, rd.kv["adapter.lora.alpha"])


def _mat_vec(M, x):
    """ggml_mul_mat(M, x) of an F16 / F32 matrix: an F16 M rounds x to f16 first; f64 sums."""
    x = np.asarray(x, np.float32)
    if M.dtype == np.float16:
        x = R.f32_to_f16(x).astype(np.float32)
    return (M.astype(np.float64) @ x.astype(np.float64)).astype(np.float32)


class LoraOracle(CvecOracle):
    """LlamaOracle (through CvecOracle, so that a control vector can be carried too; with none it is
    the plain oracle) whose _mm adds the low-rank term of every adapter in `loras` that holds the
    tensor.  loras: list of (Adapter, scale).  drop_rank: s = scale * alpha (the wrong rule a power
    check wants rejected)."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.loras = []
        self.drop_rank = False

    def _mm(self, name, x):
        y = super()._mm(name, x)
        for ad, scale in self.loras:
            p = ad.pairs.get(name)
            if p is None:
                continue
            A, B = p
            r = A.shape[0]
            s = scale if ad.alpha == 0.0 else (scale * ad.alpha if self.drop_rank else scale * ad.alpha / r)
            d = _mat_vec(B, _mat_vec(A, x))
            y = (y + (d * np.float32(s)).astype(np.float32)).astype(np.float32)
        return y


def lora_oracle(buf, n_ctx, loras=(), vec=None, drop_rank=False) -> LoraOracle:
    o = oracle_from_gguf(buf, n_ctx=n_ctx)
    c = LoraOracle(o.hp, o.tensors, n_ctx=n_ctx)
    c.loras = list(loras)
    c.vec = dict(vec or {})
    c.drop_rank = drop_rank
    return c


def lora_ulp_floor(buf, n_ctx, prompt, tokens, loras, vec=None, runs=4):
    """util.oracle_ulp_floor with the adapted oracle (as cvec_util.cvec_ulp_floor): its perturbed
    re-runs build their oracle through util.oracle_from_gguf, which for the length of the call
    returns a LoraOracle."""
    orig = util.oracle_from_gguf
    util.oracle_from_gguf = lambda b, n_ctx=0: lora_oracle(b, n_ctx, loras, vec)
    try:
        return util.oracle_ulp_floor(buf, n_ctx, prompt, tokens, runs=runs)
    finally:
        util.oracle_from_gguf = orig
