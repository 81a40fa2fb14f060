"""IQ4_XS / IQ4_NL LLaMA models (llama-quantize's mix: Q5_K V and first ffn_down, Q6_K head) end to
end on the HIP engine against the CPU oracle of iq4_util.iq4_oracle, under the gates of
tests/test_gpu_legacy_quant.py: logits within LOGIT_TOL x rms, identical top-10, the LogitComparer
gate."""
import contextlib
import functools

import numpy as np
import pytest

import iq4_util as U
from blama_amd import engine, synthetic
from cvec_util import layer_vectors
from embd_util import oracle_rows
from lora_util import Adapter
from test_gpu_decode import LOGIT_TOL
from test_gpu_legacy_quant import PROMPT, _gate, _rms, _tokens

pytestmark = pytest.mark.gpu

NAMES = ["tiny-iq4_xs", "tiny-iq4_nl"]


@functools.lru_cache(maxsize=None)
def _image(name):
    buf = synthetic.build_gguf(synthetic.IQ4_CONFIGS[name], seed=5)
    buf.setflags(write=False)
    return buf


@contextlib.contextmanager
def _run(name, n_ctx=64):
    """(config, engine context, model, the image) of one test."""
    m = engine.Model(_image(name))
    ctx = engine.Context(m, n_ctx=n_ctx)
    try:
        yield synthetic.IQ4_CONFIGS[name], ctx, m, _image(name)
    finally:
        ctx.close()
        m.close()


@pytest.mark.parametrize("name", NAMES)
def test_decode_matches_oracle(gpu_lib, name):
    with _run(name) as (cfg, ctx, _, img):
        orc = U.iq4_oracle(img, 64)
        if name == "tiny-iq4_xs":
            assert ctx.decode_path() == 1   # the streaming step, as tiny-q4_k_m
        assert ctx.decode(PROMPT) == 0
        outs = [(ctx.logits(), orc.decode(PROMPT), ctx.topk(10))]
        for t in _tokens(cfg, 6, seed=1):
            assert ctx.decode([t]) == 0
            outs.append((ctx.logits(), orc.decode_one(t), ctx.topk(10)))
        _gate(name, outs)


# 20 tokens: the short split-K GEMM (mi_batch_path 3); 130: the tiled MFMA GEMM (2).  Token seeds:
# DESIGN.md §14, "Test inputs"
@pytest.mark.parametrize("n,path,seed", [(20, 3, 16), (130, 2, 4)])
@pytest.mark.parametrize("name", NAMES)
def test_out_all_rows(gpu_lib, name, n, path, seed):
    """Every row of an MI_OUT_ALL batch against per-token oracle decode."""
    with _run(name, 160) as (cfg, ctx, _, img):
        toks = _tokens(cfg, n, seed=seed)
        assert ctx.decode(toks, all_logits=True) == 0
        assert ctx.batch_path() == path
        orc = U.iq4_oracle(img, 160)
        refs = [orc.decode_one(t) for t in toks]
        _gate(f"{name} {n} tokens", [(ctx.logits(i), refs[i], ctx.topk(10, row=i)) for i in range(n)])


def test_kv_edit_and_embedding(gpu_lib, name="tiny-iq4_xs"):
    """mi_kv_seq_rm [2, 5) + mi_kv_seq_add(5, 12, -3) (a context shift with its K-shift), then two steps
    against the oracle's kv_seq_*, and a third in embeddings mode against the oracle's embedding row."""
    with _run(name) as (cfg, ctx, _, img):
        orc = U.iq4_oracle(img, 64)
        prompt = _tokens(cfg, 12, seed=8)
        ctx.decode(prompt)
        orc.decode(prompt)
        ctx.kv_seq_rm(2, 5)
        orc.kv_seq_rm(2, 5)
        ctx.kv_seq_add(5, 12, -3)
        orc.kv_seq_shift(5, 12, delta=-3)
        assert ctx.pos_max == 8 and ctx.n_cells == 9
        outs = []
        for t in (40, 41):
            ctx.decode([t])
            outs.append((ctx.logits(), orc.decode_one(t), ctx.topk(10)))
        _gate(f"{name} context shift", outs)
        ctx.set_embeddings(True, 0)
        ctx.decode([42])
        want = oracle_rows(orc, [42])[0][0]
        err = float(np.max(np.abs(ctx.embeddings().astype(np.float64) - want)))
        assert err <= LOGIT_TOL * _rms(want), err / _rms(want)


def test_state_cvec_and_lora(gpu_lib, name="tiny-iq4_xs"):
    """A state round trip returns the same bits; a control vector on layer 1 and a LoRA adapter on every
    target, set together, agree with the oracle carrying both; cleared, the plain bits return."""
    with _run(name) as (cfg, ctx, m, img):
        toks = _tokens(cfg, 3, seed=19)
        ctx.decode(PROMPT)
        plain = ctx.logits()
        st = ctx.state_get()
        ctx.decode([toks[0]])
        nxt = ctx.logits()
        ctx.kv_clear()
        ctx.state_set(st)
        ctx.decode([toks[0]])
        assert np.array_equal(ctx.logits().view(np.uint32), nxt.view(np.uint32))

        data = (np.random.default_rng(7).standard_normal(cfg.n_embd) * 0.5).astype(np.float32)
        lora = synthetic.write_lora_gguf(None, cfg, synthetic.LORA_TARGETS, 4, 8.0, np.float16, 4, std=0.1)
        ad = engine.Lora(m, lora)
        try:
            ctx.kv_clear()
            ctx.apply_cvec(data, 1, 1)
            ctx.set_lora(ad, 0.75)
            orc = U.iq4_oracle(img, 64, [(Adapter.from_gguf(lora), 0.75)], layer_vectors(data, cfg.n_embd, cfg.n_layer, 1, 1))
            for i, step in enumerate([PROMPT] + [[t] for t in toks]):
                ctx.decode(step)
                got, want = ctx.logits(), orc.decode(step) if i == 0 else orc.decode_one(step[0])
                assert i or np.max(np.abs(got - plain)) > 50 * LOGIT_TOL * _rms(plain)
                assert float(np.max(np.abs(got - want))) <= LOGIT_TOL * _rms(want), (i, float(np.max(np.abs(got - want))) / _rms(want))
            ctx.clear_lora()
            ctx.clear_cvec()
            ctx.kv_clear()
            ctx.decode(PROMPT)
            assert np.array_equal(ctx.logits().view(np.uint32), plain.view(np.uint32))
        finally:
            ad.close()
