"""Embeddings mode (mi_ctx_set_embeddings / mi_embeddings = llama_context_params.embeddings +
llama_get_embeddings_ith / _seq, InstanceEmbedding.cpp) on every forward path: the decode step
(dgemv; gemv_kernel for MoE experts, GPT-2 and Q8_0), the short batches (mmqs), the tiled prompt
batches (mmq32) and the v_dot4 chunks, with pooling NONE / MEAN / CLS / LAST.

Reference: embd_util -- the CPU oracle's result_norm rows (the vector it hands to its output head)
and their pooled forms.  Comparison as tests/test_gpu_decode.py: element-wise within LOGIT_TOL x
rms(reference row) -- the logits the suite holds to that figure are this vector through one more
quantised matmul -- or, at an output on a rounding boundary, within twice the oracle's own 1-ulp
floor for that row (embd_util.embd_ulp_floor).  The models' norm weights are uniform(0.8, 1.2) and
their biases N(0, 0.02), so a tail that drops either is off by far more than that (asserted by the
power checks).

The engine cuts a decode call into physical batches of 512 tokens (UB_MAX), whatever n_ubatch says,
so the 170-token / n_ubatch = 80 case is one tiled batch here; the accumulation of the
pooled row from chunk to chunk is reached on the v_dot4 path (MI_NO_MMQ=1: chunks of 8 tokens,
test_pooling_accumulates_over_chunks)."""
import dataclasses
import functools

import numpy as np
import pytest

import embd_util
from blama_amd import engine, synthetic
from cvec_util import cvec_oracle, layer_vectors
from util import oracle_from_gguf

pytestmark = pytest.mark.gpu
LOGIT_TOL = 2e-3
N_CTX = 128
MODELS = ["tiny-q4_k_m", "tiny-q8_0", "tiny-moe-q5_k_m", "tiny-gpt2-q6_k"]
DECODE_PATH = {"tiny-q4_k_m": 1, "tiny-q8_0": 0, "tiny-moe-q5_k_m": 1, "tiny-gpt2-q6_k": 0}   # as test_gpu_decode.py
NONE, MEAN, CLS, LAST, RANK = 0, 1, 2, 3, 4


def _rms(a):
    return float(np.sqrt(np.mean(np.asarray(a, np.float64) ** 2)))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _model(cfg_name, pooling_type=-1):
    cfg = dataclasses.replace(synthetic.CONFIGS[cfg_name], pooling_type=pooling_type)
    buf = synthetic.build_gguf(cfg, seed=5)
    buf.setflags(write=False)
    return cfg, buf


@functools.lru_cache(maxsize=None)
def _seq(cfg_name):
    """The token sequence every test of a model reads prefixes of (172 for the model of the
    170-token pooling case, else 72)."""
    cfg, _ = _model(cfg_name)
    n = 172 if cfg_name == "tiny-q4_k_m" else 72
    return tuple(int(t) for t in np.random.default_rng(41).integers(0, cfg.n_vocab, n))


@functools.lru_cache(maxsize=None)
def _ref(cfg_name, n):
    """(rows, pre, plain) of the oracle over the first n tokens of _seq: row i depends on tokens
    0..i only, so one run serves every prefix.  Computed once, read-only."""
    _, buf = _model(cfg_name)
    out = embd_util.oracle_rows(oracle_from_gguf(buf, n_ctx=max(N_CTX, n)), _seq(cfg_name)[:n])
    for a in out:
        a.setflags(write=False)
    return out


def _ref_rows(cfg_name, n):
    return _ref(cfg_name, 72 if n <= 72 else 172)[0][:n]


def _within(got, ref, floor=None):
    """(ok, max err / rms): within LOGIT_TOL x rms(ref), or within twice the oracle's rounding floor."""
    err = float(np.max(np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64))))
    r = _rms(ref)
    return err <= LOGIT_TOL * r or (floor is not None and err <= 2 * floor), err / r


class _Floor:
    """The rounding floor of the rows of a token sequence, computed when a comparison first needs it."""

    def __init__(self, buf, tokens, n_ctx=N_CTX, **kw):
        self.args, self.kw, self.runs = (buf, n_ctx, list(tokens)), kw, None

    def rows(self, reduce=None):
        if self.runs is None:
            self.runs = embd_util.embd_ulp_floor(*self.args, **self.kw)
        return embd_util.floor_of(self.runs, reduce)


def _check(tag, got, ref, floor, i, reduce=None):
    ok, rel = _within(got, ref)
    print(f"{tag}: max|d|/rms = {rel:.2e}")
    if not ok:
        f = floor.rows(reduce)
        ok, rel = _within(got, ref, f[i if reduce is None else 0])
        print(f"{tag}: oracle floor / rms = {f[i if reduce is None else 0] / _rms(ref):.2e}")
    assert ok, (tag, rel)


def _ctx(cfg_name, pooling=NONE, n_ctx=N_CTX, pooling_type=-1, **kw):
    _, buf = _model(cfg_name, pooling_type)
    m = engine.Model(buf)
    ctx = engine.Context(m, n_ctx=n_ctx, **kw)
    ctx.set_embeddings(True, pooling)
    return m, ctx


# ---- 1. the last token's embedding on every path ----
@pytest.mark.parametrize("n", [1, 5, 70])
@pytest.mark.parametrize("cfg_name", MODELS)
def test_last_token_embedding(gpu_lib, cfg_name, n):
    """A prompt of n tokens -- the decode step (1), the short batch (5), the tiled batch (70; GPT-2:
    token by token on gemv_kernel) -- then two single-token steps on the filled cache."""
    _, buf = _model(cfg_name)
    toks = _seq(cfg_name)[:n + 2]
    rows = _ref_rows(cfg_name, n + 2)
    m, ctx = _ctx(cfg_name)
    assert ctx.decode_path() == DECODE_PATH[cfg_name]
    assert ctx.pooling == NONE
    floor = _Floor(buf, toks)
    ctx.decode(toks[:n])
    _check(f"{cfg_name} prompt {n}", ctx.embeddings(-1), rows[n - 1], floor, n - 1)
    assert np.array_equal(_bits(ctx.embeddings(0)), _bits(ctx.embeddings(-1)))   # MI_OUT_LAST: row 0 is the last token's
    for k in range(2):
        ctx.decode([toks[n + k]])
        _check(f"{cfg_name} prompt {n} step {k}", ctx.embeddings(), rows[n + k], floor, n + k)
    assert ctx.n_cells == n + 2   # KV written as usual
    ctx.close()
    m.close()


# ---- 2. every row ----
@pytest.mark.parametrize("n", [20, 70])
@pytest.mark.parametrize("cfg_name", ["tiny-q4_k_m", "tiny-gpt2-q6_k"])
def test_every_row(gpu_lib, cfg_name, n):
    """Pooling NONE after MI_OUT_ALL: a row per token (20: mmqs, 70: mmq32; GPT-2: the steps)."""
    _, buf = _model(cfg_name)
    toks = _seq(cfg_name)[:n]
    rows = _ref_rows(cfg_name, n)
    m, ctx = _ctx(cfg_name)
    ctx.decode(toks, all_logits=True)
    floor = _Floor(buf, toks)
    worst = 0.0
    for i in range(n):
        got = ctx.embeddings(i)
        ok, rel = _within(got, rows[i])
        if not ok:
            ok, rel = _within(got, rows[i], floor.rows()[i])
        assert ok, (cfg_name, n, i, rel)
        worst = max(worst, rel)
    print(f"{cfg_name} x {n}: worst max|d|/rms = {worst:.2e}")
    assert np.array_equal(_bits(ctx.embeddings(-1)), _bits(ctx.embeddings(n - 1)))
    with pytest.raises(engine.EngineError, match="out of range"):
        ctx.embeddings(n)
    ctx.close()
    m.close()


# ---- 3. pooling ----
def _pooled_against_rows(tag, got, pooling, own, n):
    """A pooled row against the engine's own NONE rows of the same tokens: CLS / LAST bit-equal to
    rows 0 / n - 1; MEAN within the sequential-sum bound n * 2^-24 * mean_t |row_t[j]| per column of
    the float64 mean of those rows."""
    if pooling == CLS:
        assert np.array_equal(_bits(got), _bits(own[0])), tag
    elif pooling == LAST:
        assert np.array_equal(_bits(got), _bits(own[n - 1])), tag
    else:
        o = own.astype(np.float64)
        bound = n * 2.0 ** -24 * np.mean(np.abs(o), axis=0)
        d = np.abs(got.astype(np.float64) - np.mean(o, axis=0))
        print(f"{tag}: max |mean - f64 mean| / bound = {float(np.max(d / bound)):.3f}")
        assert np.all(d <= bound), (tag, float(np.max(d / bound)))


@functools.lru_cache(maxsize=None)
def _own_rows(n, n_ctx, n_ubatch):
    """The engine's NONE rows of tiny-q4_k_m's first n tokens, read on a context of their own."""
    m, ctx = _ctx("tiny-q4_k_m", NONE, n_ctx=n_ctx, n_ubatch=n_ubatch)
    ctx.decode(_seq("tiny-q4_k_m")[:n], all_logits=True)
    own = np.stack([ctx.embeddings(i) for i in range(n)])
    ctx.close()
    m.close()
    own.setflags(write=False)
    return own


@pytest.mark.parametrize("pooling", [MEAN, CLS, LAST])
@pytest.mark.parametrize("n,n_ubatch", [(1, 512), (5, 512), (70, 512), (170, 80)])
def test_pooling(gpu_lib, n, n_ubatch, pooling):
    cfg_name = "tiny-q4_k_m"
    _, buf = _model(cfg_name)
    toks = _seq(cfg_name)[:n]
    n_ctx = 256 if n > N_CTX else N_CTX
    m, ctx = _ctx(cfg_name, pooling, n_ctx=n_ctx, n_ubatch=n_ubatch)
    assert ctx.pooling == pooling
    ctx.decode(toks)
    got = ctx.embeddings(0)
    assert np.array_equal(_bits(got), _bits(ctx.embeddings(-1)))
    with pytest.raises(engine.EngineError, match="one row"):
        ctx.embeddings(1)
    ref = embd_util.pool(_ref_rows(cfg_name, n), pooling)
    red = functools.partial(embd_util.pool, pooling=pooling)
    _check(f"pooling {pooling} x {n}", got, ref, _Floor(buf, toks, n_ctx), 0, reduce=red)
    _pooled_against_rows(f"pooling {pooling} x {n}", got, pooling, _own_rows(n, n_ctx, n_ubatch), n)
    # a pooled call yields its one row whatever out_mode says
    ctx.kv_clear()
    ctx.decode(toks, all_logits=True)
    assert np.array_equal(_bits(ctx.embeddings()), _bits(got))
    ctx.close()
    m.close()


@pytest.mark.parametrize("pooling", [MEAN, CLS, LAST])
def test_pooling_accumulates_over_chunks(gpu_lib, monkeypatch, pooling):
    """20 tokens on the v_dot4 path (MI_NO_MMQ=1): physical batches of 8, 8 and 4 tokens, the pooled
    row carried from one to the next; and on GPT-2, whose calls run token by token."""
    monkeypatch.setenv("MI_NO_MMQ", "1")
    for cfg_name in ("tiny-q4_k_m", "tiny-gpt2-q6_k"):
        n = 20
        _, buf = _model(cfg_name)
        toks = _seq(cfg_name)[:n]
        m, ctx = _ctx(cfg_name, pooling)
        ctx.decode(toks)
        got = ctx.embeddings()
        ref = embd_util.pool(_ref_rows(cfg_name, n), pooling)
        red = functools.partial(embd_util.pool, pooling=pooling)
        _check(f"{cfg_name} chunks pooling {pooling}", got, ref, _Floor(buf, toks), 0, reduce=red)
        ctx.set_embeddings(True, NONE)
        ctx.kv_clear()
        ctx.decode(toks, all_logits=True)
        own = np.stack([ctx.embeddings(i) for i in range(n)])
        _pooled_against_rows(f"{cfg_name} chunks pooling {pooling}", got, pooling, own, n)
        ctx.close()
        m.close()


def test_unspecified_pooling_reads_the_model_key(gpu_lib):
    n = 5
    toks = _seq("tiny-q4_k_m")[:n]
    m, ctx = _ctx("tiny-q4_k_m", engine.POOLING_UNSPECIFIED, pooling_type=MEAN)
    assert m.pooling_type == MEAN and ctx.pooling == MEAN
    ctx.decode(toks)
    ok, rel = _within(ctx.embeddings(), embd_util.pool_mean(_ref_rows("tiny-q4_k_m", n)))
    assert ok, rel
    ctx.set_embeddings(True, LAST)   # an explicit type overrides the key
    assert ctx.pooling == LAST
    ctx.close()
    m.close()
    m, ctx = _ctx("tiny-q4_k_m", engine.POOLING_UNSPECIFIED)
    assert m.pooling_type == -1 and ctx.pooling == NONE
    ctx.close()
    m.close()


# ---- 4. steering reaches the embedding ----
def _steer_data(cfg, buf):
    """Directions for layers 1 .. n_layer - 1 as test_gpu_cvec.py builds them."""
    o = cvec_oracle(buf, 8)
    o.decode_one(7)
    return (0.5 * o.x_rms * np.random.default_rng(11).standard_normal((cfg.n_layer - 1) * cfg.n_embd)).astype(np.float32)


def test_control_vector_reaches_the_embedding(gpu_lib):
    cfg_name, n = "tiny-q4_k_m", 8
    cfg, buf = _model(cfg_name)
    data = _steer_data(cfg, buf)
    vec = layer_vectors(data, cfg.n_embd, cfg.n_layer, 1, cfg.n_layer - 1)
    toks = _seq(cfg_name)[:n + 2]
    rows = embd_util.oracle_rows(cvec_oracle(buf, N_CTX, vec), toks)[0]
    plain = _ref_rows(cfg_name, n + 2)
    m, ctx = _ctx(cfg_name)
    ctx.apply_cvec(data, 1, cfg.n_layer - 1)
    floor = _Floor(buf, toks, vec=vec)
    ctx.decode(toks[:n])
    outs = [ctx.embeddings()]
    for t in toks[n:]:
        ctx.decode([t])
        outs.append(ctx.embeddings())
    for k, got in enumerate(outs):
        i = n - 1 + k
        _check(f"steered output {k}", got, rows[i], floor, i)
        assert np.max(np.abs(rows[i] - plain[i])) > 50 * LOGIT_TOL * _rms(plain[i]), k
    ctx.close()
    m.close()


def test_lora_reaches_the_embedding(gpu_lib):
    """One adapter over all seven targets (lora_util's reference yields the normed vector by the same
    wrapping: its head call is CvecOracle's)."""
    from lora_util import Adapter, lora_oracle
    cfg_name, n = "tiny-q4_k_m", 8
    cfg, buf = _model(cfg_name)
    img = synthetic.write_lora_gguf(None, cfg, synthetic.LORA_TARGETS, 8, 16.0, np.float16, 3, std=0.1)
    loras = [(Adapter.from_gguf(img), 1.0)]
    toks = _seq(cfg_name)[:n + 2]
    rows = embd_util.oracle_rows(lora_oracle(buf, N_CTX, loras), toks)[0]
    plain = _ref_rows(cfg_name, n + 2)
    m, ctx = _ctx(cfg_name)
    ad = engine.Lora(m, img)
    ctx.set_lora(ad, 1.0)
    floor = _Floor(buf, toks, loras=loras)
    ctx.decode(toks[:n])
    outs = [ctx.embeddings()]
    for t in toks[n:]:
        ctx.decode([t])
        outs.append(ctx.embeddings())
    for k, got in enumerate(outs):
        i = n - 1 + k
        _check(f"adapted output {k}", got, rows[i], floor, i)
        assert np.max(np.abs(rows[i] - plain[i])) > 50 * LOGIT_TOL * _rms(plain[i]), k
    ctx.close()
    ad.close()
    m.close()


# ---- 5. power ----
@pytest.mark.parametrize("cfg_name", ["tiny-q4_k_m", "tiny-gpt2-q6_k"])
def test_wrong_references_are_rejected(gpu_lib, cfg_name):
    """The comparison of test 1 fails at every output, by more than ten times the tolerance, against
    (a) the pre-norm residual, (b) the norm without its weight, (c) GPT-2: the norm without its
    bias; and (d) MEAN against the rows summed with 1 / (n + 1)."""
    cfg, buf = _model(cfg_name)
    n = 5
    toks = _seq(cfg_name)[:n + 2]
    rows, pre, plain = (a[:n + 2] for a in _ref(cfg_name, 72))
    o = oracle_from_gguf(buf, n_ctx=8)
    wrong = {"pre-norm": pre, "no weight": plain}
    if cfg.arch == "gpt2":
        wrong["no bias"] = (plain * o._w("output_norm.weight")).astype(np.float32)
    m, ctx = _ctx(cfg_name)
    ctx.decode(toks[:n])
    outs = [ctx.embeddings()]
    for t in toks[n:]:
        ctx.decode([t])
        outs.append(ctx.embeddings())
    for k, got in enumerate(outs):
        i = n - 1 + k
        for name, w in wrong.items():
            ok, rel = _within(got, w[i])
            print(f"{cfg_name} output {k} vs {name}: max|d|/rms = {rel:.2e}")
            assert not ok and rel > 10 * LOGIT_TOL, (name, k, rel)
    for nn in (5, 70):
        ctx.set_embeddings(True, MEAN)
        ctx.kv_clear()
        ctx.decode(_seq(cfg_name)[:nn])
        ok, rel = _within(ctx.embeddings(), embd_util.pool_mean(_ref_rows(cfg_name, nn), nn + 1))
        print(f"{cfg_name} MEAN x {nn} vs 1/(n+1): max|d|/rms = {rel:.2e}")
        assert not ok and rel > 10 * LOGIT_TOL, (nn, rel)
    ctx.close()
    m.close()


# ---- 6. mode rules ----
def test_mode_rules(gpu_lib):
    cfg_name = "tiny-q4_k_m"
    _, buf = _model(cfg_name)
    toks = list(_seq(cfg_name)[:12])
    m = engine.Model(buf)
    ctx = engine.Context(m, n_ctx=N_CTX)
    with pytest.raises(engine.EngineError, match="not in embeddings mode"):
        ctx.embeddings()
    ctx.decode(toks[:8])
    with pytest.raises(engine.EngineError, match="not in embeddings mode"):
        ctx.embeddings()
    ctx.set_embeddings(True, NONE)
    with pytest.raises(engine.EngineError, match="decode"):
        ctx.embeddings()              # no decode since the mode was set
    assert ctx.n_cells == 8           # the KV cache was left alone
    ctx.decode(toks[8:10])
    ctx.embeddings()
    for call in (ctx.logits, ctx.topk, lambda: ctx.gather([1, 2]), lambda: ctx.gather_rows(0, [[1, 2]])):
        with pytest.raises(engine.EngineError, match="embeddings mode"):
            call()
    assert not engine.lib().mi_logits(ctx.h, -1) and "embeddings mode" in engine.last_error()
    # refused pooling types leave the mode as it was
    for bad in (RANK, 5, -2):
        with pytest.raises(engine.EngineError):
            ctx.set_embeddings(True, bad)
    assert "RANK" in _err(ctx, RANK) and ctx.pooling == NONE
    # off again: the next decodes' logits are those of a context that never had the mode on
    # (batch and step: the step graphs were dropped with the mode change)
    ctx.set_embeddings(False)
    with pytest.raises(engine.EngineError, match="not in embeddings mode"):
        ctx.embeddings()
    with pytest.raises(engine.EngineError, match="no logits"):
        ctx.logits()
    ctx.decode(toks[10:11])
    a = [ctx.logits()]
    ctx.decode(toks[11:12])
    a.append(ctx.logits())
    other = engine.Context(m, n_ctx=N_CTX)
    other.decode(toks[:8])
    other.decode(toks[8:10])
    other.decode(toks[10:11])
    b = [other.logits()]
    other.decode(toks[11:12])
    b.append(other.logits())
    assert np.array_equal(_bits(np.stack(a)), _bits(np.stack(b)))
    ids_a, _ = ctx.topk(5)
    ids_b, _ = other.topk(5)
    assert list(ids_a) == list(ids_b)
    other.close()
    ctx.close()
    m.close()


def _err(ctx, pooling):
    assert engine.lib().mi_ctx_set_embeddings(ctx.h, 1, pooling) < 0
    return engine.last_error()


@pytest.mark.parametrize("cfg_name", ["tiny-q4_k_m", "tiny-moe-q5_k_m", "tiny-gpt2-q6_k"])
def test_two_runs_are_bit_identical(gpu_lib, cfg_name):
    def session():
        m, ctx = _ctx(cfg_name)
        s = _seq(cfg_name)
        out = []
        ctx.decode(s[:5])
        out.append(ctx.embeddings())
        ctx.decode(s[5:6])
        out.append(ctx.embeddings())
        ctx.decode(s[6:36], all_logits=True)
        out += [ctx.embeddings(i) for i in range(30)]
        ctx.set_embeddings(True, MEAN)
        ctx.decode(s[36:72])
        out.append(ctx.embeddings())
        ctx.close()
        m.close()
        return _bits(np.stack(out))
    assert np.array_equal(session(), session())
