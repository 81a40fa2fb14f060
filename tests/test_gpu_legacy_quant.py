"""Q4_0 / Q5_0 LLaMA models end to end on the HIP engine against the CPU oracle run on the Q8_0
re-encoding of the same image (legacy_quant_util.transcode_gguf: every Q4_0 / Q5_0 block is the
Q8_0 block with the same d and the signed weights, and ggml computes both the same way).

Bar: tests/test_gpu_decode.py::test_decode_matches_oracle's -- logits within LOGIT_TOL x rms
element-wise, identical top-10, top-1 match and the reference's LogitComparer gate (score >= 0.95,
mean similarity >= 0.98)."""
import functools

import numpy as np
import pytest

import embd_util
import ggml_ref as R
import legacy_quant_util as U
from blama_amd import engine, synthetic
from lora_util import Adapter, lora_oracle, lora_ulp_floor
from test_gpu_decode import LOGIT_TOL
from util import oracle_from_gguf

pytestmark = pytest.mark.gpu

PROMPT = [1, 17, 42, 99, 7]
OVERRIDE = "tiny-q4_k_m+q5_0"   # Q4_K_M with blk.1.ffn_down.weight as Q5_0
PATHS = {"tiny-q4_0": 1, "tiny-q5_0": 1, "tiny-hd32-q4_0": 0, "tiny-hd32-q5_0": 0, OVERRIDE: 1}


def _cfg(name):
    return synthetic.CONFIGS["tiny-q4_k_m"] if name == OVERRIDE else synthetic.LEGACY_CONFIGS[name]


@functools.lru_cache(maxsize=None)
def _images(name):
    """(the image, its Q8_0 re-encoding), built once and shared read-only."""
    ov = {"blk.1.ffn_down.weight": U.Q5_0} if name == OVERRIDE else None
    buf = synthetic.build_gguf(_cfg(name), seed=5, types_override=ov)
    ref = U.transcode_gguf(buf)
    buf.setflags(write=False)
    ref.setflags(write=False)
    return buf, ref


def _rms(a):
    return float(np.sqrt(np.mean(np.asarray(a, np.float64) ** 2)))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _tokens(cfg, n, seed):
    return [int(t) for t in np.random.default_rng(seed).integers(0, cfg.n_vocab, n)]


def _gate(tag, outs):
    """test_decode_matches_oracle's checks over outs = [(logits, reference, (top-k ids, vals))]."""
    agg = R.MetricsAggregator()
    sims = []
    score = 1.0
    for s, (got, ref, (ids, vals)) in enumerate(outs):
        rms = _rms(ref)
        err = float(np.max(np.abs(got - ref)))
        print(f"{tag} output {s}: max|dlogit|/rms = {err / rms:.2e}")
        assert err <= LOGIT_TOL * rms, (tag, s, err / rms)
        assert [int(i) for i in ids] == [i for i, _ in R.topk(ref, 10)], (tag, s)
        a = [(int(i), float(v)) for i, v in zip(ids, vals)]
        b = R.gather(ref, [i for i, _ in a])
        cm = R.compare(a, b)
        assert cm.top1Match == 1.0, (tag, s)
        score = agg.push_and_verify([cm])
        sims.append(R.logit_similarity(a, b))
    assert score >= 0.95 and np.mean(sims) >= 0.98, (tag, score, float(np.mean(sims)))


def test_transcoded_image_is_q8_0():
    buf, ref = _images("tiny-q5_0")
    from blama_amd import gguf
    a, b = gguf.GGUFReader(buf), gguf.GGUFReader(ref)
    assert list(a.tensors) == list(b.tensors)
    assert {t.type for t in a.tensors.values()} == {0, U.Q5_0, 14}
    assert {t.type for t in b.tensors.values()} == {0, R.Q8_0, 14}
    t = "blk.1.ffn_up.weight"
    assert np.array_equal(R.dequantize(np.asarray(b.tensors[t].data), R.Q8_0),
                          R.dequantize(U.to_q8_0(np.asarray(a.tensors[t].data), U.Q5_0), R.Q8_0))


@pytest.mark.parametrize("name", sorted(PATHS))
def test_decode_matches_oracle(gpu_lib, name):
    """A 5-token prompt, then 6 steps; mi_decode_path by today's rules (heads of 64: the streaming
    step; heads of 32: gemv_kernel)."""
    cfg = _cfg(name)
    buf, ref = _images(name)
    m = engine.Model(buf)
    ctx = engine.Context(m, n_ctx=64)
    orc = oracle_from_gguf(ref, n_ctx=64)
    try:
        assert ctx.decode_path() == PATHS[name]
        assert ctx.decode(PROMPT) == 0
        outs = [(ctx.logits(), orc.decode(PROMPT), ctx.topk(10))]
        for t in _tokens(cfg, 6, seed=1):
            assert ctx.decode([t]) == 0
            outs.append((ctx.logits(), orc.decode_one(t), ctx.topk(10)))
        _gate(name, outs)
    finally:
        ctx.close()
        m.close()


@pytest.mark.parametrize("name", ["tiny-q4_0", "tiny-q5_0", "tiny-hd32-q4_0"])
def test_long_prompt_on_the_tiled_batch(gpu_lib, name):
    """70 tokens in one call: the tiled MFMA GEMMs and the Q6_K head, then one step."""
    cfg = _cfg(name)
    buf, ref = _images(name)
    prompt = _tokens(cfg, 70, seed=3)
    m = engine.Model(buf)
    ctx = engine.Context(m, n_ctx=128)
    orc = oracle_from_gguf(ref, n_ctx=128)
    try:
        assert ctx.decode(prompt) == 0
        outs = [(ctx.logits(), orc.decode(prompt), ctx.topk(10))]
        ctx.decode([9])
        outs.append((ctx.logits(), orc.decode_one(9), ctx.topk(10)))
        _gate(f"{name} 70 tokens", outs)
    finally:
        ctx.close()
        m.close()


@pytest.mark.parametrize("name", ["tiny-q4_0", "tiny-q5_0"])
def test_out_all_rows(gpu_lib, name):
    """MI_OUT_ALL of 20 tokens (the short-batch form): every row against the oracle's."""
    cfg = _cfg(name)
    buf, ref = _images(name)
    toks = _tokens(cfg, 20, seed=6)
    m = engine.Model(buf)
    ctx = engine.Context(m, n_ctx=64)
    try:
        assert ctx.decode(toks, all_logits=True) == 0
        orc = oracle_from_gguf(ref, n_ctx=64)
        refs = [orc.decode_one(t) for t in toks]
        _gate(f"{name} out_all", [(ctx.logits(i), refs[i], ctx.topk(10, row=i)) for i in range(len(toks))])
    finally:
        ctx.close()
        m.close()


@pytest.mark.parametrize("name", ["tiny-q4_0", "tiny-q5_0", "tiny-hd32-q5_0"])
def test_bit_deterministic(gpu_lib, name):
    cfg = _cfg(name)
    m = engine.Model(_images(name)[0])
    res = []
    try:
        for _ in range(2):
            ctx = engine.Context(m, n_ctx=64)
            ctx.decode(PROMPT)
            out = [ctx.logits()]
            for t in _tokens(cfg, 5, seed=2):
                ctx.decode([t])
                out.append(ctx.logits())
            ctx.decode(_tokens(cfg, 20, seed=4), all_logits=True)
            out += [ctx.logits(i) for i in range(20)]
            res.append(np.stack(out))
            ctx.close()
        assert np.array_equal(_bits(res[0]), _bits(res[1]))
    finally:
        m.close()


@pytest.mark.parametrize("name", ["tiny-q4_0", "tiny-q5_0"])
def test_kv_edits_then_decode(gpu_lib, name):
    """mi_kv_seq_rm [2, 5) + mi_kv_seq_add(5, 12, -3) (a context shift with its K-shift), then 3 steps
    against the oracle's kv_seq_*."""
    cfg = _cfg(name)
    buf, ref = _images(name)
    prompt = _tokens(cfg, 12, seed=8)
    m = engine.Model(buf)
    ctx = engine.Context(m, n_ctx=64)
    orc = oracle_from_gguf(ref, n_ctx=64)
    try:
        ctx.decode(prompt)
        orc.decode(prompt)
        ctx.kv_seq_rm(2, 5)
        orc.kv_seq_rm(2, 5)
        ctx.kv_seq_add(5, 12, -3)
        orc.kv_seq_shift(5, 12, delta=-3)
        assert ctx.pos_max == 8 and ctx.n_cells == 9
        outs = []
        for t in (40, 41, 42):
            ctx.decode([t])
            outs.append((ctx.logits(), orc.decode_one(t), ctx.topk(10)))
        _gate(f"{name} context shift", outs)
    finally:
        ctx.close()
        m.close()


@pytest.mark.parametrize("name", ["tiny-q4_0", "tiny-q5_0"])
def test_state_round_trip(gpu_lib, name):
    m = engine.Model(_images(name)[0])
    try:
        a = engine.Context(m, n_ctx=64)
        a.decode(PROMPT)
        st = a.state_get()
        a.decode([77])
        want = a.logits()
        b = engine.Context(m, n_ctx=64)
        b.state_set(st)
        assert b.state_get() == st
        assert b.pos_max == len(PROMPT) - 1 and b.n_cells == len(PROMPT)
        b.decode([77])
        assert np.array_equal(_bits(b.logits()), _bits(want))
        a.close()
        b.close()
    finally:
        m.close()


@pytest.mark.parametrize("name", ["tiny-q4_0", "tiny-q5_0"])
def test_lora_changes_the_logits_and_matches(gpu_lib, name):
    """An F16 adapter on all seven targets (rank 4, alpha 8, scale 0.75; entries normal(0, 0.1): on the
    CPU oracle it moves the prompt's logits by 84 / 82 x LOGIT_TOL x rms on tiny-q4_0 / tiny-q5_0, 28 /
    32 x at the 0.07 of tests/test_gpu_lora.py's all-target adapters): the steps and a batch match
    lora_util's oracle on the re-encoded image -- within LOGIT_TOL x rms or, at an output on a rounding
    boundary, twice the adapted oracle's own 1-ulp floor (tests/test_gpu_lora.py's rule) -- and differ
    from the unadapted model's by more than 50 x the bar (test_gpu_lora.py's MOVE)."""
    cfg = _cfg(name)
    buf, ref = _images(name)
    img = synthetic.write_lora_gguf(None, cfg, synthetic.LORA_TARGETS, 4, 8.0, np.float16, 4, std=0.1)
    loras = [(Adapter.from_gguf(img), 0.75)]
    toks = _tokens(cfg, 3, seed=9)
    more = _tokens(cfg, 6, seed=10)
    m = engine.Model(buf)
    ctx = engine.Context(m, n_ctx=64)
    ad = engine.Lora(m, img)
    try:
        ctx.decode(PROMPT)
        plain = ctx.logits()
        ctx.kv_clear()
        ctx.set_lora(ad, 0.75)
        orc = lora_oracle(ref, 64, loras)
        ctx.decode(PROMPT)
        pairs = [(ctx.logits(), orc.decode(PROMPT))]
        for t in toks:
            ctx.decode([t])
            pairs.append((ctx.logits(), orc.decode_one(t)))
        ctx.decode(more)
        for t in more:
            last = orc.decode_one(t)
        pairs.append((ctx.logits(), last))
        assert np.max(np.abs(pairs[0][0] - plain)) > 50 * LOGIT_TOL * _rms(plain)
        floor = None
        for i, (got, want) in enumerate(pairs):
            err = float(np.max(np.abs(got - want)))
            print(f"{name} lora output {i}: max|dlogit|/rms = {err / _rms(want):.2e}")
            if err <= LOGIT_TOL * _rms(want):
                continue
            if floor is None:
                floor = lora_ulp_floor(ref, 64, PROMPT, toks + more, loras)[1]
            k = i if i <= len(toks) else len(floor) - 1
            assert err <= 2 * floor[k], (name, i, err / _rms(want), floor[k] / _rms(want))
    finally:
        ad.close()
        ctx.close()
        m.close()


@pytest.mark.parametrize("name", ["tiny-q4_0", "tiny-q5_0"])
def test_embeddings_mean_pooling(gpu_lib, name):
    cfg = _cfg(name)
    buf, ref = _images(name)
    toks = _tokens(cfg, 9, seed=13)
    rows, _, _ = embd_util.oracle_rows(oracle_from_gguf(ref, n_ctx=64), toks)
    want = embd_util.pool(rows, engine.POOLING_MEAN)
    m = engine.Model(buf)
    ctx = engine.Context(m, n_ctx=64)
    try:
        ctx.set_embeddings(True, engine.POOLING_MEAN)
        assert ctx.decode(toks) == 0
        err = float(np.max(np.abs(ctx.embeddings().astype(np.float64) - want))) / _rms(want)
        print(f"{name} MEAN embedding: max|d|/rms = {err:.2e}")
        assert err <= LOGIT_TOL
    finally:
        ctx.close()
        m.close()
