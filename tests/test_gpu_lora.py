"""LoRA adapters (mi_lora_load / mi_ctx_set_lora / rm / clear = llama_adapter_lora_init,
llama_set_adapter_lora, llama_rm_adapter_lora, llama_clear_adapter_lora) on every dense LLaMA path:
the streaming decode step (dgemv, both the in-launch-quantising and the dv_quant form), the tiled
prompt batches (mmq2, which a context with an adapter also takes for its short batches) and the
v_dot4 GEMM (MI_NO_MMQ).

Reference: lora_util.LoraOracle, the CPU oracle with build_lora_mm on every targeted mul_mat.
Comparison as tests/test_gpu_cvec.py: element-wise within LOGIT_TOL x rms(logits), or -- at an
output on a rounding boundary -- within twice the adapted oracle's own 1-ulp floor there.

Where no activation quantum flips, the engine's outputs equal the oracle's to 0 - 4e-7 x rms: the
kernels sum the adapter's dots in double and add the terms in the oracle's order.  These 256-wide
synthetic models are touchy, though: a 1-ulp difference upstream (the fp32 order of the attention
sums) can move one Q8_K quantum of an activation, or one f16 rounding of an F16 adapter's operand,
which shifts the logits by a discrete 4e-3 - 6e-3 x rms; the oracle's sampled 1-ulp floor excuses
such an output only when one of its few runs hits the same quantum.  The adapter seeds and
magnitudes below are therefore the ones at which every compared output is free of such a flip on
both sides (found by measuring, recorded here): among seeds 4, 5, 6 and std 0.03 / 0.05 / 0.07 for
the all-target adapters, and std 0.2 / 0.3 / 0.4 for the single-target ones.

Adapter magnitude: A and B are normal(0, std) with std = STD[target] for the single-target adapters,
chosen on the CPU oracle (model seed 5, rank 4, alpha 8, scale 0.75, the 7 outputs of the
per-target run) so that the oracle's logits move by more than 50 x LOGIT_TOL x rms = 0.1 x rms at
every output.  Smallest movement over the outputs, in units of rms, on tiny-q4_k_m: attn_v 0.322,
attn_output 1.094, ffn_gate 0.363, ffn_up 0.350 (std 0.4), ffn_down 0.482 (std 0.3).  On that model
attn_q and attn_k cannot reach 0.1: an adapter on Q or K only re-weights the attention, whose
output projection is drawn small (synthetic "resid" = 0.03 / sqrt(2 n_layer)), and the movement
saturates (attn_q 0.018 / 0.038 / 0.062 / 0.066 at std 0.2 / 0.4 / 1.0 / 2.0).  Those two targets
therefore run on QK_MODEL, tiny-q4_k_m's geometry and quantisation mix with the layer outputs drawn
at resid = 0.12, where attention carries weight: smallest movement attn_q 0.212, attn_k 0.302 at std
0.4 (resid = 0.06: 0.115 / 0.157).  All seven assert the 50 x."""
import functools

import numpy as np
import pytest

from blama_amd import engine, synthetic
from cvec_util import layer_vectors
from lora_util import Adapter, lora_oracle, lora_ulp_floor
from util import parse_state

pytestmark = pytest.mark.gpu
LOGIT_TOL = 2e-3
N_CTX = 128
TARGETS = synthetic.LORA_TARGETS
STD = dict(attn_q=0.4, attn_k=0.4, attn_v=0.4, attn_output=0.4, ffn_gate=0.4, ffn_up=0.4, ffn_down=0.3)
MOVE = 50         # x LOGIT_TOL x rms: the movement of the oracle's logits every single-target adapter must exceed
QK_MODEL = "tiny-q4_k_m:resid=0.12"   # the model of the attn_q / attn_k cases (module docstring)
ALL_STD = 0.07   # all seven targets at once: each term 10-25 % of its base projection
BATCH_STD = 0.03  # the batch rows: 96 rows stay free of flips at this size only (module docstring)


def _rms(a):
    return float(np.sqrt(np.mean(np.asarray(a, np.float64) ** 2)))


@functools.lru_cache(maxsize=None)
def _model(cfg_name):
    name, _, init = cfg_name.partition(":")   # "config:init" draws the config with synthetic init overrides
    cfg = synthetic.small_config(name, init=init) if init else synthetic.CONFIGS[name]
    buf = synthetic.build_gguf(cfg, seed=5)
    buf.setflags(write=False)
    return cfg, buf


@functools.lru_cache(maxsize=None)
def _adapter(cfg_name, targets, rank, alpha, f16, seed, layers=None, std=ALL_STD):
    """(GGUF image, the oracle's view of it)."""
    cfg, _ = _model(cfg_name)
    img = synthetic.write_lora_gguf(None, cfg, targets, rank, alpha, np.float16 if f16 else np.float32, seed,
                                    layers=layers, std=std)
    return img, Adapter.from_gguf(img)


def _tokens(cfg, n, seed):
    return [int(t) for t in np.random.default_rng(seed).integers(0, cfg.n_vocab, n)]


def _within(got, ref, floor=None):
    err = float(np.max(np.abs(got.astype(np.float64) - ref)))
    r = _rms(ref)
    return err <= LOGIT_TOL * r or (floor is not None and err <= 2 * floor), err / r


def _engine_run(buf, loras, prompt, toks, n_ctx=N_CTX, before=None):
    """Engine outputs (the prompt's last token, then each single-token step) with the adapters
    (list of (image, scale)) set before the first decode."""
    m = engine.Model(buf)
    ctx = engine.Context(m, n_ctx=n_ctx)
    hs = [engine.Lora(m, img) for img, _ in loras]
    for h, (_, scale) in zip(hs, loras):
        ctx.set_lora(h, scale)
    if before:
        before(ctx, hs)
    path = engine.lib().mi_decode_path(ctx.h)
    ctx.decode(prompt)
    outs = [ctx.logits()]
    for t in toks:
        ctx.decode([t])
        outs.append(ctx.logits())
    ctx.close()
    for h in hs:
        h.close()
    m.close()
    return outs, path


def _oracle_run(buf, loras, prompt, toks, n_ctx=N_CTX, **kw):
    o = lora_oracle(buf, n_ctx, loras, **kw)
    return [o.decode(prompt)] + [o.decode_one(t) for t in toks]


def _check(tag, buf, outs, loras, prompt, toks, n_ctx=N_CTX, vec=None):
    refs = _oracle_run(buf, loras, prompt, toks, n_ctx, vec=vec)
    floor = None
    for i, (got, ref) in enumerate(zip(outs, refs)):
        ok, rel = _within(got, ref)
        print(f"{tag} output {i}: max|dlogit|/rms = {rel:.2e}")
        if not ok:
            if floor is None:
                floor = lora_ulp_floor(buf, n_ctx, prompt, toks, loras, vec)[1]
            ok, rel = _within(got, ref, floor[i])
        assert ok, (tag, i, rel)
    return refs


# ---- 1. per target ----
@pytest.mark.parametrize("target", TARGETS)
def test_single_target_matches_oracle(gpu_lib, target):
    """Rank 4, F16, alpha 8, scale 0.75 on one tensor of every layer: an 8-token prompt, then 6
    single-token steps (positions > 0: a Q/K term added after RoPE would show).  A site that is not
    wired leaves the engine at the base logits, which the movement assertion puts far outside the
    tolerance."""
    name = QK_MODEL if target in ("attn_q", "attn_k") else "tiny-q4_k_m"
    cfg, buf = _model(name)
    img, ad = _adapter(name, (target,), 4, 8.0, True, 3, std=STD[target])
    prompt, toks = _tokens(cfg, 8, 1), _tokens(cfg, 6, 2)
    outs, path = _engine_run(buf, [(img, 0.75)], prompt, toks)
    assert path == 1
    refs = _check(target, buf, outs, [(ad, 0.75)], prompt, toks)
    plain = _oracle_run(buf, [], prompt, toks)
    move = min(float(np.max(np.abs(r - p))) / _rms(p) for r, p in zip(refs, plain))
    print(f"{target}: smallest movement {move:.3f} x rms")
    assert move > MOVE * LOGIT_TOL, (target, move)


# ---- 2. all seven targets ----
@pytest.mark.parametrize("cfg_name,rank,f16,seed", [("tiny-q4_k_m", 16, True, 5), ("tiny-q4_k_m", 12, False, 5),
                                                     ("tiny-q8_0", 4, True, 4), ("tiny-gqa16-q4_k_m", 16, True, 4)])
def test_all_targets_match_oracle(gpu_lib, cfg_name, rank, f16, seed):
    """All seven tensors of every layer: rank 16 F16, rank 12 F32 (no power of two, the fp32 path),
    Q8_0 activations with n_head_kv 4, and the GQA geometry (n_embd 2048); the last two step on
    gemv_kernel, which takes the adapters' terms precomputed."""
    cfg, buf = _model(cfg_name)
    img, ad = _adapter(cfg_name, TARGETS, rank, 8.0, f16, seed)
    prompt, toks = _tokens(cfg, 8, 1), _tokens(cfg, 6, 2)
    outs, path = _engine_run(buf, [(img, 0.75)], prompt, toks)
    # tiny-q4_k_m steps on the streaming launches; head_dim 32 (tiny-q8_0) and the 16-kv-head GQA
    # geometry have no quantising attention kernel and step on gemv_kernel
    assert path == (1 if cfg_name == "tiny-q4_k_m" else 0)
    _check(f"{cfg_name} r{rank}", buf, outs, [(ad, 0.75)], prompt, toks)


def test_dv_quant_form(gpu_lib):
    """The step whose normed inputs exist only through dv_quant launches (n_ff * n_embd > 2^24): one
    7B-wide layer, 3 tokens."""
    cfg = synthetic.small_config("llama2-7b-q4_k_m", n_layer=1, n_ff=4352, n_vocab=512)
    assert cfg.n_ff * cfg.n_embd > 1 << 24
    buf = synthetic.build_gguf(cfg, seed=5)
    img = synthetic.write_lora_gguf(None, cfg, TARGETS, 16, 8.0, np.float16, 4, std=0.05)
    ad = Adapter.from_gguf(img)
    prompt, toks = [5], [9, 300]
    m = engine.Model(buf)
    ctx = engine.Context(m, n_ctx=16)
    lora = engine.Lora(m, img)
    ctx.set_lora(lora, 0.75)
    assert engine.lib().mi_decode_path(ctx.h) == 1
    outs = []
    for t in prompt + toks:
        ctx.decode([t])
        outs.append(ctx.logits())
    refs, plain = [], []
    o, p = lora_oracle(buf, 16, [(ad, 0.75)]), lora_oracle(buf, 16, [])
    for t in prompt + toks:
        refs.append(o.decode_one(t))
        plain.append(p.decode_one(t))
    floor = None
    for i, (got, ref, pl) in enumerate(zip(outs, refs, plain)):
        ok, rel = _within(got, ref)
        print(f"dv_quant form output {i}: {rel:.2e}")
        if not ok:
            if floor is None:
                floor = lora_ulp_floor(buf, 16, prompt, toks, [(ad, 0.75)], runs=8)[1]
            print(f"  oracle floor {floor[i] / _rms(ref):.2e}")
            ok, rel = _within(got, ref, floor[i])
        assert ok, (i, rel)
        assert not _within(got, pl)[0], i


# ---- 3. batches ----
@pytest.mark.parametrize("n,no_mmq", [(20, False), (96, False), (20, True)])
def test_batch_rows_match_oracle(gpu_lib, monkeypatch, n, no_mmq):
    """Every row of an MI_OUT_ALL batch on tiny-q4_k_m rank 16: 20 and 96 tokens on the tiled GEMM,
    20 on the v_dot4 one (MI_NO_MMQ=1: MI_OUT_ALL then runs the steps token by token, and a plain
    20-token prompt runs decode_batch -- both compared)."""
    if no_mmq:
        monkeypatch.setenv("MI_NO_MMQ", "1")
    cfg, buf = _model("tiny-q4_k_m")
    img, ad = _adapter("tiny-q4_k_m", TARGETS, 16, 8.0, True, 5, std=BATCH_STD)
    m = engine.Model(buf)
    ctx = engine.Context(m, n_ctx=N_CTX)
    lora = engine.Lora(m, img)
    ctx.set_lora(lora, 0.75)
    toks = _tokens(cfg, n, 3)
    ctx.decode(toks, all_logits=True)
    o = lora_oracle(buf, N_CTX, [(ad, 0.75)])
    p = lora_oracle(buf, N_CTX, [])
    floor, worst, ref = None, 0.0, None
    for i, t in enumerate(toks):
        ref, plain = o.decode_one(t), p.decode_one(t)
        # the adapter shows in every row (smallest movement measured 0.010 x rms; the engine's rows
        # differ from the oracle's by at most 7e-5 x rms)
        assert np.max(np.abs(ref - plain)) > 4 * LOGIT_TOL * _rms(plain), i
        ok, rel = _within(ctx.logits(row=i), ref)
        if not ok:
            if floor is None:
                floor = lora_ulp_floor(buf, N_CTX, toks[:1], toks[1:], [(ad, 0.75)], runs=16)[1]
            ok, rel = _within(ctx.logits(row=i), ref, floor[i])
        assert ok, (n, i, rel)
        worst = max(worst, rel)
    print(f"{n} tokens, no_mmq={no_mmq}: worst max|dlogit|/rms = {worst:.2e}")
    if no_mmq:   # the prompt form of the v_dot4 GEMM: the last token's logits
        ctx.kv_clear()
        ctx.decode(toks)
        ok, rel = _within(ctx.logits(), ref)
        print(f"decode_batch last row: {rel:.2e}")
        assert ok, rel


# ---- 4. rules ----
def test_alpha_zero_uses_scale(gpu_lib):
    cfg, buf = _model("tiny-q4_k_m")
    img, ad = _adapter("tiny-q4_k_m", TARGETS, 4, 0.0, True, 6)
    assert ad.alpha == 0.0
    prompt, toks = _tokens(cfg, 4, 1), _tokens(cfg, 3, 2)
    outs, _ = _engine_run(buf, [(img, 0.5)], prompt, toks)
    _check("alpha 0", buf, outs, [(ad, 0.5)], prompt, toks)
    assert not _within(outs[-1], _oracle_run(buf, [], prompt, toks)[-1])[0]


def test_oracle_without_rank_division_is_rejected(gpu_lib):
    """Power: an oracle with s = scale * alpha fails at every output by more than 10 x the tolerance."""
    cfg, buf = _model("tiny-q4_k_m")
    img, ad = _adapter("tiny-q4_k_m", TARGETS, 4, 8.0, True, 4)
    prompt, toks = _tokens(cfg, 8, 1), _tokens(cfg, 6, 2)
    outs, _ = _engine_run(buf, [(img, 0.75)], prompt, toks)
    for i, (got, ref) in enumerate(zip(outs, _oracle_run(buf, [(ad, 0.75)], prompt, toks, drop_rank=True))):
        ok, rel = _within(got, ref)
        assert not ok and rel > 10 * LOGIT_TOL, (i, rel)


def test_subset_of_layers_and_targets(gpu_lib):
    cfg, buf = _model("tiny-q4_k_m")
    img, ad = _adapter("tiny-q4_k_m", ("attn_v", "ffn_down"), 4, 8.0, True, 7, layers=(1, 3), std=0.4)
    assert sorted(ad.pairs) == [f"blk.{l}.{t}.weight" for l in (1, 3) for t in ("attn_v", "ffn_down")]
    prompt, toks = _tokens(cfg, 8, 1), _tokens(cfg, 4, 2)
    outs, _ = _engine_run(buf, [(img, 0.75)], prompt, toks)
    _check("layers 1,3", buf, outs, [(ad, 0.75)], prompt, toks)
    assert not _within(outs[-1], _oracle_run(buf, [], prompt, toks)[-1])[0]


def test_stack_rescale_and_remove(gpu_lib):
    """Two adapters (rank 4 F16 and rank 12 F32) equal the oracle's sum; set again with a new scale
    updates that adapter; rm_lora of one leaves the other."""
    cfg, buf = _model("tiny-q4_k_m")
    img1, ad1 = _adapter("tiny-q4_k_m", TARGETS, 4, 8.0, True, 4)
    img2, ad2 = _adapter("tiny-q4_k_m", TARGETS, 12, 6.0, False, 8)
    prompt, toks = _tokens(cfg, 8, 1), _tokens(cfg, 3, 2)
    outs, _ = _engine_run(buf, [(img1, 0.75), (img2, 0.5)], prompt, toks)
    _check("stacked", buf, outs, [(ad1, 0.75), (ad2, 0.5)], prompt, toks)
    assert not _within(outs[-1], _oracle_run(buf, [(ad1, 0.75)], prompt, toks)[-1])[0]
    outs, _ = _engine_run(buf, [(img1, 0.75), (img2, 0.5)], prompt, toks, before=lambda c, hs: c.set_lora(hs[0], -0.3))
    _check("rescaled", buf, outs, [(ad1, -0.3), (ad2, 0.5)], prompt, toks)
    outs, _ = _engine_run(buf, [(img1, 0.75), (img2, 0.5)], prompt, toks, before=lambda c, hs: c.rm_lora(hs[0]))
    _check("removed", buf, outs, [(ad2, 0.5)], prompt, toks)


def _session(ctx, cfg):
    rows = []
    ctx.decode(_tokens(cfg, 8, 21))
    rows.append(ctx.logits())
    for t in _tokens(cfg, 4, 22):
        ctx.decode([t])
        rows.append(ctx.logits())
    ctx.decode(_tokens(cfg, 20, 23), all_logits=True)
    rows += [ctx.logits(row=i) for i in range(20)]
    return np.stack(rows).view(np.uint32)


def test_clear_and_no_adapter_bit_exactness(gpu_lib):
    """clear_lora returns decode steps and a 20-token batch to the bits of a context that never had an
    adapter; so does set + clear before the first decode (and rm of the only adapter)."""
    cfg, buf = _model("tiny-q4_k_m")
    img, _ = _adapter("tiny-q4_k_m", TARGETS, 16, 8.0, True, 4)
    m = engine.Model(buf)
    fresh = engine.Context(m, n_ctx=N_CTX)
    base = _session(fresh, cfg)
    lora = engine.Lora(m, img)
    ctx = engine.Context(m, n_ctx=N_CTX)
    ctx.set_lora(lora, 0.75)
    ctx.clear_lora()
    assert np.array_equal(_session(ctx, cfg), base)
    ctx.kv_clear()
    ctx.set_lora(lora, 0.75)
    adapted = _session(ctx, cfg)
    assert not np.array_equal(adapted, base)
    ctx.kv_clear()
    ctx.clear_lora()
    assert np.array_equal(_session(ctx, cfg), base)
    ctx.kv_clear()
    ctx.set_lora(lora, 0.75)
    ctx.rm_lora(lora)
    assert np.array_equal(_session(ctx, cfg), base)


def test_set_mid_session_and_state(gpu_lib):
    """4 plain tokens, the adapter, 4 more: the steps follow an oracle that does the same, the first
    4 cells' K and V stay as they were; a state_get / state_set round trip into a second context that
    carries the adapter continues identically (the adapter is no part of the state)."""
    cfg, buf = _model("tiny-q4_k_m")
    img, ad = _adapter("tiny-q4_k_m", TARGETS, 16, 8.0, True, 4)
    m = engine.Model(buf)
    ctx = engine.Context(m, n_ctx=32)
    lora = engine.Lora(m, img)
    o = lora_oracle(buf, 32, [])
    first, second = _tokens(cfg, 4, 31), _tokens(cfg, 4, 32)
    for t in first:
        ctx.decode([t])
        ref = o.decode_one(t)
    assert _within(ctx.logits(), ref)[0]
    kv_dim = cfg.n_head_kv * (cfg.n_embd // cfg.n_head)
    _, k0, v0 = parse_state(ctx.state_get(), cfg.n_layer, kv_dim)
    ctx.set_lora(lora, 0.75)
    o.loras = [(ad, 0.75)]
    plain = lora_oracle(buf, 32, [])
    plain.decode(first)
    for i, t in enumerate(second[:2]):
        ctx.decode([t])
        ok, rel = _within(ctx.logits(), o.decode_one(t))
        assert ok, (i, rel)
        assert not _within(ctx.logits(), plain.decode_one(t))[0], i
    st = ctx.state_get()
    _, k1, v1 = parse_state(st, cfg.n_layer, kv_dim)
    assert k1.shape[1] == 6
    assert np.array_equal(k1[:, :4].view(np.uint16), k0.view(np.uint16))
    assert np.array_equal(v1[:, :4].view(np.uint16), v0.view(np.uint16))
    other = engine.Context(m, n_ctx=32)
    other.state_set(st)
    assert np.array_equal(np.frombuffer(other.state_get(), np.uint8), np.frombuffer(st, np.uint8))
    other.set_lora(lora, 0.75)
    for t in second[2:]:
        ctx.decode([t])
        other.decode([t])
        assert np.array_equal(ctx.logits().view(np.uint32), other.logits().view(np.uint32))
        assert _within(ctx.logits(), o.decode_one(t))[0]


def test_with_control_vector(gpu_lib):
    cfg, buf = _model("tiny-q4_k_m")
    img, ad = _adapter("tiny-q4_k_m", TARGETS, 4, 8.0, True, 4)
    o = lora_oracle(buf, 8, [])
    o.decode_one(7)
    data = (0.5 * o.x_rms * np.random.default_rng(11).standard_normal((cfg.n_layer - 1) * cfg.n_embd)).astype(np.float32)
    vec = layer_vectors(data, cfg.n_embd, cfg.n_layer, 1, cfg.n_layer - 1)
    prompt, toks = _tokens(cfg, 8, 1), _tokens(cfg, 3, 2)
    outs, _ = _engine_run(buf, [(img, 0.75)], prompt, toks, before=lambda c, hs: c.apply_cvec(data, 1, cfg.n_layer - 1))
    _check("cvec + lora", buf, outs, [(ad, 0.75)], prompt, toks, vec=vec)
    assert not _within(outs[-1], _oracle_run(buf, [(ad, 0.75)], prompt, toks)[-1])[0]
    assert not _within(outs[-1], _oracle_run(buf, [], prompt, toks, vec=vec)[-1])[0]


# ---- 6. errors ----
def test_errors_and_lifetime(gpu_lib):
    cfg, buf = _model("tiny-q4_k_m")
    img, ad = _adapter("tiny-q4_k_m", TARGETS, 4, 8.0, True, 4)
    m, m2 = engine.Model(buf), engine.Model(buf)
    ctx = engine.Context(m, n_ctx=32)
    foreign = engine.Lora(m2, img)
    with pytest.raises(engine.EngineError, match="another model"):
        ctx.set_lora(foreign, 1.0)
    with pytest.raises(engine.EngineError, match="another model"):
        ctx.rm_lora(foreign)
    lora = engine.Lora(m, img)
    with pytest.raises(engine.EngineError, match="not set"):
        ctx.rm_lora(lora)
    L = engine.lib()
    assert L.mi_ctx_set_lora(None, lora.h, 1.0) < 0 and "null" in engine.last_error()
    assert L.mi_ctx_set_lora(ctx.h, None, 1.0) < 0 and "null" in engine.last_error()
    assert L.mi_ctx_rm_lora(None, lora.h) < 0
    L.mi_ctx_clear_lora(None)
    # the failed calls left the context without an adapter
    prompt, toks = _tokens(cfg, 4, 1), _tokens(cfg, 2, 2)
    ctx.decode(prompt)
    assert _within(ctx.logits(), _oracle_run(buf, [], prompt, [])[0])[0]
    # mi_lora_free before mi_ctx_free: the context keeps the adapter alive
    ctx.kv_clear()
    ctx.set_lora(lora, 0.75)
    lora.close()
    ctx.decode(prompt)
    outs = [ctx.logits()]
    for t in toks:
        ctx.decode([t])
        outs.append(ctx.logits())
    _check("after free", buf, outs, [(ad, 0.75)], prompt, toks)
    ctx.close()
