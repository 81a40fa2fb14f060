"""Unquantised F16 LLaMA models end to end on the HIP engine vs the CPU oracle (oracle/ggml_ref
LlamaOracle runs an F16 GGUF as any other): the decode step on fgemv.hip, prompt batches and
MI_OUT_ALL on the F16 MFMA GEMM, and everything that hangs off a context.

Bar: tests/test_gpu_gpt2.py's rule -- max|dlogit| <= 2e-3 x rms with identical top-10, or, at a step
where it is not, within twice the oracle's own 1-ulp floor there (util.oracle_ulp_floor) -- and the
reference's LogitComparer gate (score >= 0.95, mean similarity >= 0.98)."""
import numpy as np
import pytest

import cvec_util
import embd_util
import ggml_ref as R
from blama_amd import engine, synthetic
from util import oracle_from_gguf, oracle_ulp_floor

pytestmark = pytest.mark.gpu

LOGIT_TOL = 2e-3
CFGS = ["tiny-f16", "tiny-f16-hd128", "tiny-rf-f16"]
PROMPT = [3, 50, 7, 199, 12]
_BUF = {}


def _buf(name, seed=5):
    if (name, seed) not in _BUF:
        _BUF[(name, seed)] = synthetic.build_gguf(synthetic.F16_CONFIGS[name], seed=seed)
    return _BUF[(name, seed)]


def _rms(a):
    return float(np.sqrt(np.mean(np.asarray(a, np.float64) ** 2)))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _steps(cfg, n, seed=2):
    return [int(t) for t in np.random.default_rng(seed).integers(0, cfg.n_vocab, n)]


def _compare(tag, outs, floor_of):
    """outs: [(logits, reference, (top-k ids, vals))]; floor_of(): the per-output 1-ulp floor."""
    floor = None
    agg = R.MetricsAggregator()
    sims = []
    score = 1.0
    for s, (got, ref, (ids, vals)) in enumerate(outs):
        rms = _rms(ref)
        err = float(np.max(np.abs(got - ref)))
        print(f"{tag} output {s}: max|dlogit|/rms = {err / rms:.2e}")
        if err <= LOGIT_TOL * rms:
            assert [int(i) for i in ids] == [i for i, _ in R.topk(ref, 10)], (tag, s)
        else:
            if floor is None:
                floor = floor_of()
            print(f"  oracle 1-ulp floor at output {s}: {floor[s] / rms:.2e} x rms")
            assert err <= 2 * floor[s], (tag, s, err / rms, floor[s] / rms)
            ref_sorted = np.sort(ref)[::-1][:10]
            assert np.all(np.abs(ref[np.asarray(ids, np.int64)] - ref_sorted) <= 2 * err + 1e-6)
        a = [(int(i), float(v)) for i, v in zip(ids, vals)]
        cm = R.compare(a, R.gather(ref, [i for i, _ in a]))
        assert cm.top1Match == 1.0, (tag, s)
        score = agg.push_and_verify([cm])
        sims.append(R.logit_similarity(a, R.gather(ref, [i for i, _ in a])))
    assert score >= 0.95 and np.mean(sims) >= 0.98, (tag, score, float(np.mean(sims)))


def _run(name, prompt, steps, n_ctx=64, oracle=None):
    """The prompt in one call, then `steps` one at a time, on the engine and the oracle."""
    buf = _buf(name)
    m = engine.Model(buf)
    ctx = engine.Context(m, n_ctx=n_ctx)
    orc = oracle or oracle_from_gguf(buf, n_ctx=n_ctx)
    assert ctx.decode(prompt) == 0
    outs = [(ctx.logits(), orc.decode(prompt), ctx.topk(10))]
    for t in steps:
        assert ctx.decode([t]) == 0
        outs.append((ctx.logits(), orc.decode_one(t), ctx.topk(10)))
    return m, ctx, outs


@pytest.mark.parametrize("name", CFGS)
def test_decode_matches_oracle(gpu_lib, name):
    cfg = synthetic.F16_CONFIGS[name]
    steps = _steps(cfg, 8)
    m, ctx, outs = _run(name, PROMPT, steps)
    try:
        assert ctx.decode_path() == 3
        _compare(name, outs, lambda: oracle_ulp_floor(_buf(name), 64, PROMPT, steps)[1])
    finally:
        ctx.close()
        m.close()


@pytest.mark.parametrize("name", CFGS)
def test_loaded_model_accounting(gpu_lib, name):
    """mi_model_weight_bytes and mi_model_type_histogram of the loaded model: the F16 and F32 bytes of
    the file, token_embd streamed only where it is also the head."""
    import ctypes as C
    cfg = synthetic.F16_CONFIGS[name]
    types, shapes = synthetic.tensor_types(cfg), synthetic.tensor_shapes(cfg)
    by_type, streamed = {}, 0
    for n, t in types.items():
        nb = int(np.prod(shapes[n])) * (2 if t == 1 else 4)
        by_type[t] = by_type.get(t, 0) + nb
        if n != "token_embd.weight" or cfg.tied_head:
            streamed += nb
    m = engine.Model(_buf(name))
    try:
        hist = (C.c_int64 * 32)()
        assert engine.lib().mi_model_type_histogram(m.h, hist, 32) >= 0
        assert {t: int(hist[t]) for t in range(32) if hist[t]} == by_type
        assert engine.lib().mi_model_weight_bytes(m.h) == streamed
    finally:
        m.close()


def test_past_512_cells(gpu_lib):
    """A 520-token prompt (two physical batches) at n_ctx 600, then 4 steps on the split attention."""
    cfg = synthetic.F16_CONFIGS["tiny-f16"]
    prompt = _steps(cfg, 520, seed=4)
    steps = _steps(cfg, 4)
    m, ctx, outs = _run("tiny-f16", prompt, steps, n_ctx=600)
    try:
        assert ctx.n_cells == 524
        _compare("520 cells", outs, lambda: oracle_ulp_floor(_buf("tiny-f16"), 600, prompt, steps)[1])
    finally:
        ctx.close()
        m.close()


@pytest.mark.parametrize("n", [20, 64])
def test_out_all_rows(gpu_lib, n):
    """MI_OUT_ALL: every row against the oracle's per-token outputs; gather_rows = the rows of logits."""
    cfg = synthetic.F16_CONFIGS["tiny-f16"]
    buf = _buf("tiny-f16")
    toks = _steps(cfg, n, seed=6)
    m = engine.Model(buf)
    ctx = engine.Context(m, n_ctx=128)
    try:
        assert ctx.decode(toks, all_logits=True) == 0
        orc = oracle_from_gguf(buf, n_ctx=128)
        refs = [orc.decode_one(t) for t in toks]
        outs = [(ctx.logits(i), refs[i], ctx.topk(10, row=i)) for i in range(n)]
        # (the floor run's outputs are the prompt's last token, then each further one: token 0 alone is the prompt)
        _compare(f"out_all {n}", outs, lambda: oracle_ulp_floor(buf, 128, toks[:1], toks[1:])[1])
        ids = np.stack([np.asarray(ctx.topk(10, row=i)[0], np.int32) for i in range(n)])
        got = ctx.gather_rows(0, ids)
        want = np.stack([ctx.logits(i)[ids[i]] for i in range(n)])
        assert np.array_equal(_bits(got), _bits(want))
        assert np.array_equal(_bits(ctx.logits(-1)), _bits(ctx.logits(n - 1)))
    finally:
        ctx.close()
        m.close()


def test_bit_deterministic(gpu_lib):
    """Two contexts, the same prompt and steps: bit-identical logits (t-integration.cpp:219-248); a
    serial per-token push of the sequence gives the bits generating it gave."""
    cfg = synthetic.F16_CONFIGS["tiny-f16"]
    m = engine.Model(_buf("tiny-f16"))
    steps = _steps(cfg, 6)
    res = []
    try:
        for _ in range(2):
            ctx = engine.Context(m, n_ctx=64)
            ctx.decode(PROMPT)
            out = [ctx.logits()]
            for t in steps:
                ctx.decode([t])
                out.append(ctx.logits())
            res.append(out)
            ctx.close()
        for a, b in zip(*res):
            assert np.array_equal(_bits(a), _bits(b))
        # generate greedily from one token, then push the same sequence token by token
        gen, pushed = [], []
        ctx = engine.Context(m, n_ctx=64)
        t = PROMPT[0]
        seq = []
        for _ in range(6):
            seq.append(t)
            ctx.decode([t])
            gen.append(ctx.logits())
            t = int(ctx.topk(1)[0][0])
        ctx.close()
        ctx = engine.Context(m, n_ctx=64)
        for t in seq:
            ctx.decode([t])
            pushed.append(ctx.logits())
        ctx.close()
        for a, b in zip(gen, pushed):
            assert np.array_equal(_bits(a), _bits(b))
    finally:
        m.close()


class _WrongRope(R.LlamaOracle):
    """An oracle whose Q and K rotation ignores the frequency factors."""

    def _rope(self, x, pos, ffv, which):
        return super()._rope(x, pos, None, which)


def test_rope_fault_fails_the_bar(gpu_lib):
    """On tiny-rf-f16 (rope_freqs, linear scaling, partial rotary, O(1) scores) an oracle with the
    rotation deliberately wrong is far outside the bar the right one meets."""
    name = "tiny-rf-f16"
    cfg = synthetic.F16_CONFIGS[name]
    buf = _buf(name)
    base = oracle_from_gguf(buf, n_ctx=64)
    wrong = _WrongRope(base.hp, base.tensors, n_ctx=64)
    steps = _steps(cfg, 8)
    m, ctx, outs = _run(name, PROMPT, steps, oracle=wrong)
    try:
        worst = max(float(np.max(np.abs(g - r))) / _rms(r) for g, r, _ in outs)
        print(f"wrong rotation: max|dlogit|/rms = {worst:.2e}")
        assert worst > 10 * LOGIT_TOL
        with pytest.raises(AssertionError):
            _compare("wrong rope", outs, lambda: np.zeros(len(outs)))
    finally:
        ctx.close()
        m.close()


def test_kv_shift_then_steps(gpu_lib):
    """seq_rm [2, 5) + seq_add(5, 12, -3) (a context shift), then 3 steps against the oracle's kv_seq_*."""
    cfg = synthetic.F16_CONFIGS["tiny-rf-f16"]
    buf = _buf("tiny-rf-f16")
    prompt = _steps(cfg, 12, seed=8)
    m = engine.Model(buf)
    ctx = engine.Context(m, n_ctx=64)
    orc = oracle_from_gguf(buf, n_ctx=64)
    try:
        ctx.decode(prompt)
        orc.decode(prompt)
        ctx.kv_seq_rm(2, 5)
        orc.kv_seq_rm(2, 5)
        ctx.kv_seq_add(5, 12, -3)
        orc.kv_seq_shift(5, 12, delta=-3)
        assert ctx.pos_max == 8 and ctx.n_cells == 9
        for t in (40, 41, 42):
            ctx.decode([t])
            ref, got = orc.decode_one(t), ctx.logits()
            err = float(np.max(np.abs(got - ref))) / _rms(ref)
            print(f"context shift, token {t}: max|dlogit|/rms = {err:.2e}")
            assert err <= LOGIT_TOL
            assert [int(i) for i in ctx.topk(10)[0]] == [i for i, _ in R.topk(ref, 10)]
        ctx.kv_clear()
        assert ctx.n_cells == 0
    finally:
        ctx.close()
        m.close()


def test_state_round_trip(gpu_lib):
    cfg = synthetic.F16_CONFIGS["tiny-f16"]
    m = engine.Model(_buf("tiny-f16"))
    try:
        a = engine.Context(m, n_ctx=64)
        a.decode(PROMPT)
        st = a.state_get()
        a.decode([77])
        want = a.logits()
        b = engine.Context(m, n_ctx=64)
        b.state_set(st)
        assert b.state_get() == st
        b.decode([77])
        assert np.array_equal(_bits(b.logits()), _bits(want))
        a.close()
        b.close()
    finally:
        m.close()


def test_control_vector_mid_run(gpu_lib):
    """A control vector applied after the prompt: the steps (fgemv's addend) and a further batch (its
    own pass) match the oracle with the same add."""
    cfg = synthetic.F16_CONFIGS["tiny-f16"]
    buf = _buf("tiny-f16")
    data = (np.random.default_rng(11).standard_normal((cfg.n_layer - 1) * cfg.n_embd) * 2.0).astype(np.float32)
    vec = cvec_util.layer_vectors(data, cfg.n_embd, cfg.n_layer, 1, cfg.n_layer - 1)
    m = engine.Model(buf)
    ctx = engine.Context(m, n_ctx=64)
    orc = cvec_util.cvec_oracle(buf, 64)
    try:
        ctx.decode(PROMPT)
        orc.decode(PROMPT)
        plain = ctx.logits()
        ctx.apply_cvec(data, 1, cfg.n_layer - 1)
        orc.vec = vec
        outs = []
        steps = _steps(cfg, 3)
        for t in steps:
            ctx.decode([t])
            outs.append((ctx.logits(), orc.decode_one(t), ctx.topk(10)))
        more = _steps(cfg, 5, seed=12)
        ctx.decode(more)
        for t in more:
            ref = orc.decode_one(t)
        outs.append((ctx.logits(), ref, ctx.topk(10)))
        for got, ref, _ in outs:
            err = float(np.max(np.abs(got - ref))) / _rms(ref)
            print(f"control vector: max|dlogit|/rms = {err:.2e}")
            assert err <= LOGIT_TOL
        assert np.max(np.abs(outs[0][0] - plain)) > 50 * LOGIT_TOL * _rms(plain)   # the vector does steer
    finally:
        ctx.close()
        m.close()


@pytest.mark.parametrize("pooling", [engine.POOLING_NONE, engine.POOLING_MEAN, engine.POOLING_LAST])
def test_embeddings(gpu_lib, pooling):
    """Pooling NONE (every row), MEAN and LAST against the oracle's final-norm rows (embd_util)."""
    cfg = synthetic.F16_CONFIGS["tiny-f16"]
    buf = _buf("tiny-f16")
    toks = _steps(cfg, 9, seed=13)
    rows, _, _ = embd_util.oracle_rows(oracle_from_gguf(buf, n_ctx=64), toks)
    m = engine.Model(buf)
    ctx = engine.Context(m, n_ctx=64)
    try:
        ctx.set_embeddings(True, pooling)
        assert ctx.decode(toks, all_logits=(pooling == engine.POOLING_NONE)) == 0
        if pooling == engine.POOLING_NONE:
            pairs = [(ctx.embeddings(i), rows[i]) for i in range(len(toks))]
        else:
            pairs = [(ctx.embeddings(), embd_util.pool(rows, pooling))]
        for got, ref in pairs:
            err = float(np.max(np.abs(got.astype(np.float64) - ref))) / _rms(ref)
            print(f"embeddings pooling {pooling}: max|d|/rms = {err:.2e}")
            assert err <= LOGIT_TOL
        # one more token through the decode step's embedding tail
        ctx.decode([5])
        if pooling != engine.POOLING_MEAN:
            ref = embd_util.oracle_rows(_replay(buf, toks), [5])[0][0]
            err = float(np.max(np.abs(ctx.embeddings().astype(np.float64) - ref))) / _rms(ref)
            assert err <= LOGIT_TOL
    finally:
        ctx.close()
        m.close()


def _replay(buf, toks):
    orc = oracle_from_gguf(buf, n_ctx=64)
    for t in toks:
        orc.decode_one(t)
    return orc


def test_lora_is_refused(gpu_lib, tmp_path):
    cfg = synthetic.F16_CONFIGS["tiny-f16"]
    m = engine.Model(_buf("tiny-f16"))
    ctx = engine.Context(m, n_ctx=64)
    try:
        assert ctx.decode_path() == 3
        path = tmp_path / "a.gguf"
        synthetic.write_lora_gguf(path, cfg, rank=4)
        assert not engine.lib().mi_lora_load(m.h, str(path).encode())
        assert "F16" in engine.last_error()
        # an adapter of a quantised model of the same shapes cannot be set either
        q = engine.Model(synthetic.build_gguf(synthetic.small_config("tiny-q8_0"), header_only=True), vocab_only=True)
        qpath = tmp_path / "q.gguf"
        synthetic.write_lora_gguf(qpath, synthetic.CONFIGS["tiny-q8_0"], rank=4)
        h = engine.lib().mi_lora_load(q.h, str(qpath).encode())
        assert h
        assert engine.lib().mi_ctx_set_lora(ctx.h, h, 1.0) != 0
        engine.lib().mi_lora_free(h)
        q.close()
    finally:
        ctx.close()
        m.close()
