"""The synthetic GGUF images are the fixtures of the whole suite and of the benchmark: a change to
blama_amd/synthetic.py must leave every existing config's image byte for byte as it was."""
import hashlib

import numpy as np
import pytest

from blama_amd import gguf, synthetic

# sha256(build_gguf(cfg, seed=5)), recorded before LlamaConfig grew its RoPE-variant fields
PINNED = {
    "tiny-q4_k_m": "8d017568c266e3f51caad44c6e74419764b0a21c9eb11e17a01010c65f368fe5",
    "tiny-q5_k_m": "9524166b82c73bb15673e09fc7d1c3b6e7643ee235d076ca6a22258af90767ef",
    "tiny-q6_k": "47401d500a16316ab612c943ea7ad718d98e730a6fdb786e4c6af6712f3efc13",
    "tiny-q8_0": "cd587962eedf43b1989fb0bff647b197c5d5b35e30e2c1c943ff5bf20f459546",
    "tiny1-q4_k_m": "56fa8135fc147f0f26b25d10a777cc81b94dbd6ab193e17d886d5ae16dc2e114",
    "tiny-moe-q5_k_m": "c110549262178e7119a34450df0efcc01f4c1e9116a973197dae90bc2148ca32",
    "tiny-gqa16-q4_k_m": "e37a73dffb906e6edac906aecd76ceb01973d79f79d0051c9f2959f273f3018c",
    "tiny-gpt2-q6_k": "b1eebc739ecb814b9ab49d239685c47b11997569e5c5fa37ae62c8b493cdb955",
    "tiny-gpt2-q8_0": "bde628d8d927d5906b4dc04cafafbccebc1b07c68c07bf0c55dc990be2932b61",
}
# the same for the header_only image (metadata + tensor table) of the full-size configs
PINNED_HEADER = {
    "tinyllama-1.1b-q8_0": "88aadd36b8d63d0b5b08e51d7bcf1cfac7d694e01300273ecae888bd5891bce6",
    "llama2-7b-q4_k_m": "b334100669d67f4939be3db7d6a686965af8eae88c6197701f9de5be8182a337",
    "llama3-8b-q6_k": "5514c9908411bf6bb04d95d06b6a08e2bb42308e08cff01cb7a4fcf357177f12",
    "mixtral-8x7b-q5_k_m": "0e0e74518aa0eb73f36c12119d41efee71c1b74dec8d844504c5deae5f90327e",
    "gpt2-117m-q6_k": "457ed20fbd47e2087165df3ec0c39f75fd3653a7a9bfbee5e1dfebb0ac9869dd",
}
ROPE_VARIANTS = ["tiny-rf-q4_k_m", "tiny-prot-q4_k_m", "tiny-rf-q8_0", "tiny-rf-moe-q5_k_m"]


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@pytest.mark.parametrize("name", sorted(PINNED))
def test_existing_tiny_images_are_byte_identical(name):
    assert _sha(synthetic.build_gguf(synthetic.CONFIGS[name], seed=5)) == PINNED[name]


@pytest.mark.parametrize("name", sorted(PINNED_HEADER))
def test_existing_full_size_headers_are_byte_identical(name):
    assert _sha(synthetic.build_gguf(synthetic.CONFIGS[name], seed=5, header_only=True)) == PINNED_HEADER[name]


def test_every_other_config_is_a_rope_variant():
    """A config is either pinned above or one of the RoPE variants (a new one gets a pin)."""
    assert sorted(set(synthetic.CONFIGS) - set(PINNED) - set(PINNED_HEADER)) == sorted(ROPE_VARIANTS)


def test_rope_variant_metadata_and_factors():
    """What each variant writes: the rotated width, the scaling keys under the spelling asked for,
    and an F32 rope_freqs.weight of n_rot/2 factors in [0.5, 4] (seeded; neither quant blocks nor
    a norm weight's 0.8 .. 1.2)."""
    want = {"tiny-rf-q4_k_m": (64, 4.0, False, 32), "tiny-prot-q4_k_m": (32, 2.0, True, 0),
            "tiny-rf-q8_0": (16, 4.0, False, 8), "tiny-rf-moe-q5_k_m": (64, 2.0, False, 32)}
    for name, (n_rot, scale, legacy, nff) in want.items():
        cfg = synthetic.CONFIGS[name]
        assert (cfg.n_layer, cfg.n_vocab, cfg.n_embd) == (2, 512, 256)
        buf = synthetic.build_gguf(cfg, seed=5)
        rd = gguf.GGUFReader(buf)
        kv = rd.kv
        assert int(kv["llama.rope.dimension_count"]) == n_rot
        if legacy:
            assert float(kv["llama.rope.scale_linear"]) == scale
            assert "llama.rope.scaling.type" not in kv and "llama.rope.scaling.factor" not in kv
        else:
            assert kv["llama.rope.scaling.type"] == "linear" and float(kv["llama.rope.scaling.factor"]) == scale
            assert "llama.rope.scale_linear" not in kv
        assert ("rope_freqs.weight" in rd.tensors) == (nff > 0)
        if nff:
            t = rd.tensors["rope_freqs.weight"]
            assert t.type == synthetic.F32 and tuple(t.shape) == (nff,)
            ff = np.ascontiguousarray(t.data).view(np.float32)
            assert ff.size == nff and ff.min() >= 0.5 and ff.max() <= 4.0
            assert np.ptp(ff) > 1.0 and ff[0] != 1.0      # spread over the range, pair 0 included
            again = gguf.GGUFReader(synthetic.build_gguf(cfg, seed=5)).tensors["rope_freqs.weight"]
            assert np.array_equal(ff, np.ascontiguousarray(again.data).view(np.float32))
