"""Control vectors (mi_ctx_apply_cvec = llama_apply_adapter_cvec, Instance.cpp:73-84) on every
forward path: the streaming decode step (dgemv), gemv_kernel (MoE experts, GPT-2), the short
batches (mmqs) and the tiled prompt batches (mmq32 / mmq2).

Reference: cvec_util.CvecOracle, the CPU oracle with x = ((ffn + x) + v_il) and llama.cpp b5187's
layer rule.  Comparison as tests/test_gpu_decode.py: element-wise within LOGIT_TOL x rms(logits),
or -- at an output that sits on a rounding boundary -- within twice the steered oracle's own
1-ulp floor there (util.oracle_ulp_floor).  The vectors are 0.5 x rms(residual stream) x randn per
layer, so steering moves the logits by far more than the tolerance (asserted)."""
import functools

import numpy as np
import pytest

from blama_amd import engine, synthetic
from cvec_util import cvec_oracle, cvec_ulp_floor, layer_vectors
from util import parse_state

pytestmark = pytest.mark.gpu
LOGIT_TOL = 2e-3
N_CTX = 128


def _rms(a):
    return float(np.sqrt(np.mean(np.asarray(a, np.float64) ** 2)))


@functools.lru_cache(maxsize=None)
def _model(cfg_name):
    """(cfg, GGUF image, data): directions for layers 1 .. n_layer-1 back to back, each
    0.5 x rms(x) x randn with x the unsteered oracle's residual stream after one token."""
    cfg = synthetic.CONFIGS[cfg_name]
    buf = synthetic.build_gguf(cfg, seed=5)
    o = cvec_oracle(buf, 8)
    o.decode_one(7)
    rng = np.random.default_rng(11)
    data = (0.5 * o.x_rms * rng.standard_normal((cfg.n_layer - 1) * cfg.n_embd)).astype(np.float32)
    data.setflags(write=False)
    return cfg, buf, data


def _tokens(cfg, n, seed):
    return [int(t) for t in np.random.default_rng(seed).integers(0, cfg.n_vocab, n)]


def _within(got, ref, floor=None):
    """(ok, err / rms): within LOGIT_TOL x rms, or within twice the oracle's rounding floor."""
    err = float(np.max(np.abs(got.astype(np.float64) - ref)))
    r = _rms(ref)
    return err <= LOGIT_TOL * r or (floor is not None and err <= 2 * floor), err / r


def _decode_run(cfg_name, il_start, il_end, data, prompt_n=8, steps=6):
    """Engine outputs (the prompt's last token, then each single-token step) with the vector set
    before the first decode, and the tokens."""
    cfg, buf, _ = _model(cfg_name)
    m = engine.Model(buf)
    ctx = engine.Context(m, n_ctx=N_CTX)
    if data is not None:
        ctx.apply_cvec(data, il_start, il_end)
    prompt, toks = _tokens(cfg, prompt_n, 1), _tokens(cfg, steps, 2)
    ctx.decode(prompt)
    outs = [ctx.logits()]
    for t in toks:
        ctx.decode([t])
        outs.append(ctx.logits())
    ctx.close()
    m.close()
    return outs, prompt, toks


def _oracle_run(buf, vec, prompt, toks):
    o = cvec_oracle(buf, N_CTX, vec)
    return [o.decode(prompt)] + [o.decode_one(t) for t in toks]


def _check_outputs(cfg_name, outs, vec, prompt, toks):
    cfg, buf, _ = _model(cfg_name)
    refs = _oracle_run(buf, vec, prompt, toks)
    floor = None
    for i, (got, ref) in enumerate(zip(outs, refs)):
        ok, rel = _within(got, ref)
        print(f"{cfg_name} output {i}: max|dlogit|/rms = {rel:.2e}")
        if not ok:
            if floor is None:
                floor = cvec_ulp_floor(buf, N_CTX, prompt, toks, vec)[1]
            ok, rel = _within(got, ref, floor[i])
        assert ok, (cfg_name, i, rel)
    return refs


@pytest.mark.parametrize("cfg_name", ["tiny-q4_k_m", "tiny-moe-q5_k_m", "tiny-gpt2-q6_k"])
def test_decode_steps_match_steered_oracle(gpu_lib, cfg_name):
    """An 8-token prompt and 6 single-token steps with every layer from 1 up steered: the streaming
    step with its in-launch-quantising down launch (tiny-q4_k_m), gemv_kernel's MoE-down and
    GPT-2 residual epilogues."""
    cfg, buf, data = _model(cfg_name)
    outs, prompt, toks = _decode_run(cfg_name, 1, cfg.n_layer - 1, data)
    vec = layer_vectors(data, cfg.n_embd, cfg.n_layer, 1, cfg.n_layer - 1)
    assert sorted(vec) == list(range(1, cfg.n_layer))
    refs = _check_outputs(cfg_name, outs, vec, prompt, toks)
    # steering moved the logits by far more than the tolerance
    plain = _oracle_run(buf, {}, prompt, toks)
    for ref, p in zip(refs, plain):
        assert np.max(np.abs(ref - p)) > 50 * LOGIT_TOL * _rms(p)


def test_off_by_one_oracle_is_rejected(gpu_lib):
    """Power: an oracle that puts data[0:n_embd] on layer 0 (every slice one layer early) fails the
    same comparison at every output, by more than ten times the tolerance (far from anything a
    rounding floor could excuse)."""
    cfg, buf, data = _model("tiny-q4_k_m")
    outs, prompt, toks = _decode_run("tiny-q4_k_m", 1, cfg.n_layer - 1, data)
    wrong = layer_vectors(data, cfg.n_embd, cfg.n_layer, 1, cfg.n_layer - 1, shift=-1)
    assert sorted(wrong) == list(range(0, cfg.n_layer - 1))
    for i, (got, ref) in enumerate(zip(outs, _oracle_run(buf, wrong, prompt, toks))):
        ok, rel = _within(got, ref)
        assert not ok and rel > 10 * LOGIT_TOL, (i, rel)


@pytest.mark.parametrize("cfg_name,n", [("tiny-q4_k_m", 20), ("tiny-q4_k_m", 96), ("tiny-moe-q5_k_m", 20)])
def test_batch_rows_match_steered_oracle(gpu_lib, cfg_name, n):
    """Every row of an MI_OUT_ALL batch: 20 tokens on the short-batch GEMM (mmqs; MoE: the grouped
    form and moe_combine), 96 on the tiled one (split-K partials added by the next quant_act, the
    last layer by the GEMM's own residual epilogue)."""
    cfg, buf, data = _model(cfg_name)
    m = engine.Model(buf)
    ctx = engine.Context(m, n_ctx=N_CTX)
    ctx.apply_cvec(data, 1, cfg.n_layer - 1)
    toks = _tokens(cfg, n, 3)
    ctx.decode(toks, all_logits=True)
    vec = layer_vectors(data, cfg.n_embd, cfg.n_layer, 1, cfg.n_layer - 1)
    o = cvec_oracle(buf, N_CTX, vec)
    p = cvec_oracle(buf, N_CTX, {})
    floor = None
    worst = 0.0
    for i, t in enumerate(toks):
        ref, plain = o.decode_one(t), p.decode_one(t)
        assert np.max(np.abs(ref - plain)) > 50 * LOGIT_TOL * _rms(plain), i
        ok, rel = _within(ctx.logits(row=i), ref)
        if not ok:
            if floor is None:
                floor = cvec_ulp_floor(buf, N_CTX, toks[:1], toks[1:], vec, runs=16)[1]
            ok, rel = _within(ctx.logits(row=i), ref, floor[i])
        assert ok, (cfg_name, n, i, rel)
        worst = max(worst, rel)
    print(f"{cfg_name} x {n}: worst max|dlogit|/rms = {worst:.2e}")


@pytest.mark.parametrize("case", ["one_layer", "short_data", "start_zero"])
def test_range_rules(gpu_lib, case):
    """il_start = il_end = 2 steers layer 2 alone; data of one layer's length steers layer 1 alone;
    il_start = 0 still leaves layer 0 unsteered (its data cannot be expressed)."""
    cfg, buf, data = _model("tiny-q4_k_m")
    d, lo, hi = {"one_layer": (data, 2, 2), "short_data": (data[:cfg.n_embd], 1, 3), "start_zero": (data, 0, 3)}[case]
    vec = layer_vectors(d, cfg.n_embd, cfg.n_layer, lo, hi)
    assert sorted(vec) == {"one_layer": [2], "short_data": [1], "start_zero": [1, 2, 3]}[case]
    outs, prompt, toks = _decode_run("tiny-q4_k_m", lo, hi, d, prompt_n=4, steps=3)
    _check_outputs("tiny-q4_k_m", outs, vec, prompt, toks)
    if case == "start_zero":   # and bit for bit what il_start = 1 gives
        same, _, _ = _decode_run("tiny-q4_k_m", 1, 3, d, prompt_n=4, steps=3)
        assert np.array_equal(np.stack(outs).view(np.uint32), np.stack(same).view(np.uint32))
    else:   # the full range's oracle does not pass for this run
        full = layer_vectors(data, cfg.n_embd, cfg.n_layer, 1, 3)
        assert not _within(outs[-1], _oracle_run(buf, full, prompt, toks)[-1])[0]


def _session(ctx, cfg):
    """Logits of every path as one uint32 array: an 8-token prompt (mmqs), 4 streaming steps, a
    20-token MI_OUT_ALL batch (mmqs) and a 70-token one (tiled)."""
    rows = []
    ctx.decode(_tokens(cfg, 8, 21))
    rows.append(ctx.logits())
    for t in _tokens(cfg, 4, 22):
        ctx.decode([t])
        rows.append(ctx.logits())
    for n, seed in ((20, 23), (70, 24)):
        ctx.decode(_tokens(cfg, n, seed), all_logits=True)
        rows += [ctx.logits(row=i) for i in range(n)]
    return np.stack(rows).view(np.uint32)


@pytest.mark.parametrize("cfg_name", ["tiny-q4_k_m", "tiny-moe-q5_k_m"])
def test_bit_exactness(gpu_lib, cfg_name):
    """An all-zero vector changes no bit; clearing restores the unsteered bits; a steered run
    repeats bit for bit on a second context."""
    cfg, buf, data = _model(cfg_name)
    m = engine.Model(buf)
    ctx = engine.Context(m, n_ctx=N_CTX)
    base = _session(ctx, cfg)
    ctx.kv_clear()
    ctx.apply_cvec(np.zeros_like(data), 1, cfg.n_layer - 1)
    assert np.array_equal(_session(ctx, cfg), base)
    ctx.kv_clear()
    ctx.apply_cvec(data, 1, cfg.n_layer - 1)
    steered = _session(ctx, cfg)
    assert not np.array_equal(steered, base)
    ctx.kv_clear()
    ctx.clear_cvec()
    assert np.array_equal(_session(ctx, cfg), base)
    other = engine.Context(m, n_ctx=N_CTX)
    other.apply_cvec(data, 1, cfg.n_layer - 1)
    assert np.array_equal(_session(other, cfg), steered)


def test_set_mid_session(gpu_lib):
    """4 unsteered tokens, then the vector, then 4 more: the steps follow an oracle that does the
    same, and the first 4 cells' K and V stay as they were."""
    cfg, buf, data = _model("tiny-q4_k_m")
    m = engine.Model(buf)
    ctx = engine.Context(m, n_ctx=32)
    vec = layer_vectors(data, cfg.n_embd, cfg.n_layer, 1, 3)
    o = cvec_oracle(buf, 32, {})
    first, second = _tokens(cfg, 4, 31), _tokens(cfg, 4, 32)
    for t in first:
        ctx.decode([t])
        ref = o.decode_one(t)
    assert _within(ctx.logits(), ref)[0]
    kv_dim = cfg.n_head_kv * (cfg.n_embd // cfg.n_head)
    _, k0, v0 = parse_state(ctx.state_get(), cfg.n_layer, kv_dim)
    ctx.apply_cvec(data, 1, 3)
    o.vec = vec
    plain = cvec_oracle(buf, 32, {})
    plain.decode(first)
    for i, t in enumerate(second):
        ctx.decode([t])
        ref = o.decode_one(t)
        ok, rel = _within(ctx.logits(), ref)
        assert ok, (i, rel)
        assert not _within(ctx.logits(), plain.decode_one(t))[0], i
    _, k1, v1 = parse_state(ctx.state_get(), cfg.n_layer, kv_dim)
    assert k1.shape[1] == 8
    assert np.array_equal(k1[:, :4].view(np.uint16), k0.view(np.uint16))
    assert np.array_equal(v1[:, :4].view(np.uint16), v0.view(np.uint16))


def test_errors(gpu_lib):
    import ctypes as C
    cfg, buf, data = _model("tiny-q4_k_m")
    m = engine.Model(buf)
    ctx = engine.Context(m, n_ctx=16)
    with pytest.raises(engine.EngineError, match="n_embd"):
        ctx.apply_cvec(data, 1, 3, n_embd=cfg.n_embd + 1)
    p = data.ctypes.data_as(C.POINTER(C.c_float))
    assert engine.lib().mi_ctx_apply_cvec(ctx.h, p, data.size, cfg.n_embd // 2, 1, 3) < 0
    assert "n_embd" in engine.last_error()
    assert engine.lib().mi_ctx_apply_cvec(None, p, data.size, cfg.n_embd, 1, 3) < 0
    assert engine.last_error()
    # the failed calls left the context unsteered
    ctx.decode([1, 2, 3])
    ref = cvec_oracle(buf, 16, {}).decode([1, 2, 3])
    assert _within(ctx.logits(), ref)[0]
