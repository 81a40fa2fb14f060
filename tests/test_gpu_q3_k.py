"""Q3_K_S / Q3_K_M LLaMA models end to end on the HIP engine against the CPU oracle run on the Q6_K
re-encoding of the same image (q3_k_util.transcode_gguf), under the gates of
tests/test_gpu_legacy_quant.py.  Token seeds: DESIGN.md §13, "Test inputs"."""
import contextlib
import functools

import numpy as np
import pytest

import embd_util
import q3_k_util as U
from blama_amd import engine, synthetic
from lora_util import Adapter, lora_oracle, lora_ulp_floor
from test_gpu_decode import LOGIT_TOL
from test_gpu_legacy_quant import PROMPT, _gate, _rms, _tokens
from util import oracle_from_gguf

pytestmark = pytest.mark.gpu

NAMES = ["tiny-q3_k_s", "tiny-q3_k_m"]


@functools.lru_cache(maxsize=None)
def _images(name):
    buf = synthetic.build_gguf(synthetic.Q3K_CONFIGS[name], seed=5)
    ref = U.transcode_gguf(buf)
    buf.setflags(write=False)
    ref.setflags(write=False)
    return buf, ref


@contextlib.contextmanager
def _run(name, n_ctx=64):
    """(config, engine context, model, the re-encoded image) of one test."""
    buf, ref = _images(name)
    m = engine.Model(buf)
    ctx = engine.Context(m, n_ctx=n_ctx)
    try:
        yield synthetic.Q3K_CONFIGS[name], ctx, m, ref
    finally:
        ctx.close()
        m.close()


@pytest.mark.parametrize("name", NAMES)
def test_decode_matches_oracle(gpu_lib, name):
    with _run(name) as (cfg, ctx, _, ref):
        orc = oracle_from_gguf(ref, n_ctx=64)
        assert ctx.decode_path() == 1   # the streaming step, as tiny-q4_k_m
        assert ctx.decode(PROMPT) == 0
        outs = [(ctx.logits(), orc.decode(PROMPT), ctx.topk(10))]
        for t in _tokens(cfg, 6, seed=1):
            assert ctx.decode([t]) == 0
            outs.append((ctx.logits(), orc.decode_one(t), ctx.topk(10)))
        _gate(name, outs)


# 40 tokens: the short split-K GEMM (mi_batch_path 3); 70: the tiled MFMA GEMM (2)
@pytest.mark.parametrize("n,path", [(40, 3), (70, 2)])
@pytest.mark.parametrize("name", NAMES)
def test_prompt_batch(gpu_lib, name, n, path):
    with _run(name, 128) as (cfg, ctx, _, ref):
        prompt = _tokens(cfg, n, seed=3)
        orc = oracle_from_gguf(ref, n_ctx=128)
        assert ctx.decode(prompt) == 0
        assert ctx.batch_path() == path
        outs = [(ctx.logits(), orc.decode(prompt), ctx.topk(10))]
        ctx.decode([9])
        outs.append((ctx.logits(), orc.decode_one(9), ctx.topk(10)))
        _gate(f"{name} {n} tokens", outs)


@pytest.mark.parametrize("name", NAMES)
def test_out_all_rows(gpu_lib, name):
    with _run(name) as (cfg, ctx, _, ref):
        toks = _tokens(cfg, 20, seed=16)
        assert ctx.decode(toks, all_logits=True) == 0
        orc = oracle_from_gguf(ref, n_ctx=64)
        refs = [orc.decode_one(t) for t in toks]
        _gate(f"{name} out_all", [(ctx.logits(i), refs[i], ctx.topk(10, row=i)) for i in range(len(toks))])


@pytest.mark.parametrize("name", NAMES)
def test_embeddings_mean_pooling(gpu_lib, name):
    with _run(name) as (cfg, ctx, _, ref):
        toks = _tokens(cfg, 9, seed=13)
        rows, _, _ = embd_util.oracle_rows(oracle_from_gguf(ref, n_ctx=64), toks)
        want = embd_util.pool(rows, engine.POOLING_MEAN)
        ctx.set_embeddings(True, engine.POOLING_MEAN)
        assert ctx.decode(toks) == 0
        assert float(np.max(np.abs(ctx.embeddings().astype(np.float64) - want))) <= LOGIT_TOL * _rms(want)


@pytest.mark.parametrize("name", NAMES)
def test_lora_set_and_cleared(gpu_lib, name):
    """test_gpu_legacy_quant's adapter and rule (within the bar, or twice the adapted oracle's own 1-ulp
    floor); the adapter moves the logits by more than 50 x the bar; cleared, the unadapted bits return."""
    with _run(name) as (cfg, ctx, m, ref):
        img = synthetic.write_lora_gguf(None, cfg, synthetic.LORA_TARGETS, 4, 8.0, np.float16, 4, std=0.1)
        loras = [(Adapter.from_gguf(img), 0.75)]
        toks = _tokens(cfg, 3, seed=19)
        ad = engine.Lora(m, img)
        try:
            ctx.decode(PROMPT)
            plain = ctx.logits()
            ctx.kv_clear()
            ctx.set_lora(ad, 0.75)
            orc = lora_oracle(ref, 64, loras)
            for i, step in enumerate([PROMPT] + [[t] for t in toks]):
                ctx.decode(step)
                got, want = ctx.logits(), orc.decode(step) if i == 0 else orc.decode_one(step[0])
                assert i or np.max(np.abs(got - plain)) > 50 * LOGIT_TOL * _rms(plain)
                err = float(np.max(np.abs(got - want)))
                if err > LOGIT_TOL * _rms(want):
                    assert err <= 2 * lora_ulp_floor(ref, 64, PROMPT, toks, loras)[1][i], (name, i, err / _rms(want))
            ctx.clear_lora()
            ctx.kv_clear()
            ctx.decode(PROMPT)
            assert np.array_equal(ctx.logits().view(np.uint32), plain.view(np.uint32))
        finally:
            ad.close()
