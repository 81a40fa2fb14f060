"""RoPE variants -- frequency factors (rope_freqs.weight), linear scaling, partial rotary -- on
every device implementation of the rotation, against the numpy oracle.

The engine rotates in six places: the streaming decode step's Q/K/V epilogue (dgemv.hip), the
gemv_kernel step's LDS table + epilogue (gemv.hip), the v_dot4 GEMM's prologue table (kernels.hip
gemm_t, MI_NO_MMQ=1), the rope table kernel read by the tiled int8-MFMA GEMM's epilogue and by the
short batches' qkv_finish (mmq.hip), and the K-shift (kernels.hip kv_shift_kernel).  The
tiny-rf-* / tiny-prot-* configs turn on the three branches of each that no other model reaches.

What is compared
----------------
(b) Layer 0's K and V cache rows, element by element, after a 40-token prompt.  They depend only
on embed -> rms_norm -> Q8 quantisation -> GEMV -> RoPE -> f16, and the integer dots are exact, so
the bound is derived, not measured: for a rotated pair with the oracle's pre-rotation values
(k0, k1) and GEMV abs-sums (a0, a1)

    delta = GEMV_TOL (a0 + a1) + 2^-21 (|k0| + |k1|)

(the 2e-5 GEMV bar of test_gpu_ops.py / test_gpu_dgemv.py through a rotation, |cos|, |sin| <= 1;
cosf / sinf and the two products within a few fp32 ulps), and the f16 result may differ by
delta + ulp16(ref).  Elements from n_rot on, and V: GEMV_TOL a + ulp16(ref).  The one way the
reference itself leaves this bound -- a last-bit rms_norm difference flipping an int8 quantum of
the activation -- is removed by the choice of prompt: qualifying_tokens() takes the first 40
token ids whose layer-0 activation has no element within 1e-3 quanta of a rounding boundary.
(c) Logits and top-10 ids after the prompt and 4 further steps, the bar of test_gpu_decode.py:
this covers Q's rotation, which the state does not expose.  The prompt window is the first on which
the oracle's own logits hold still under a few-ulp change of its GEMV and attention sums (_stable):
on tiny-prot's first window they move by 7.7e-3 x rms at the prompt's last token (a quantum of a
later activation on its boundary), and so did the MFMA batch paths there, by the same 7.69e-3; on
its second, flipping the oracle's three quanta within 1e-4 of a boundary at step 2 moves its logits
by 3.6e-3 x rms, where the token-by-token paths differed by 3.44e-3 (every other output 4e-7).
(d) The K-shift on the engine's own cache (<= 1 f16 ulp on rotated elements, bits elsewhere) and
the logits after a Self-Extend / context-shift sequence.
(a) A CPU guard that (b) and (c) can fail: deliberately wrong oracles (factors dropped, shifted by
one pair, freq_scale 1, n_rot = head_dim, factors on Q only) must leave the K bound on at least a
quarter of the rotated elements and move the final logits by more than 10 x LOGIT_TOL x rms.
"""
import numpy as np
import pytest

import ggml_ref as R
from blama_amd import engine, synthetic
from test_gpu_decode import DECODE_PATH, LOGIT_TOL, _kshift_ref
from util import oracle_from_gguf, parse_state

GEMV_TOL = 2e-5
TRIG_TOL = 2.0 ** -21
NOISE = 16 * 2.0 ** -24  # _stable's relative perturbation: 16 fp32 ulps
BOUNDARY = 1e-3          # quanta: a prompt token's activation stays this far from every .5
SEED, N_CTX, N_PROMPT = 5, 64, 40
STEPS = [7, 99, 250, 33]

CFGS = ["tiny-rf-q4_k_m", "tiny-prot-q4_k_m", "tiny-rf-q8_0", "tiny-rf-moe-q5_k_m"]
# the deliberately wrong oracles that mean something for each config
MUTATIONS = {
    "tiny-rf-q4_k_m": ["drop", "shift", "scale1", "q_only"],
    "tiny-prot-q4_k_m": ["scale1", "nrot_full"],
    "tiny-rf-q8_0": ["drop", "shift", "scale1", "nrot_full", "q_only"],
    "tiny-rf-moe-q5_k_m": ["drop", "shift", "scale1", "q_only"],
}
# prompt ingestion paths: the environment each needs before the context is created
PATHS = {
    "single": {"MI_NO_BATCH": "1"},     # token by token: dgemv.hip DV_QKV or gemv.hip EPI_QKV
    "mmqs": {},                         # one short batch: rope_table_kernel + qkv_finish
    "mmq": {"MI_MMQS_MAX": "0"},        # the tiled int8-MFMA GEMM: rope_table_kernel + mmq_epilogue
    "gemm_t": {"MI_NO_MMQ": "1"},       # the v_dot4 GEMM (dense models; MoE decodes token by token)
}


class _Mutant(R.LlamaOracle):
    """The oracle with one RoPE fault of the kind a kernel could have."""
    mut = None

    def _rope(self, x, pos, ffv, which):
        hp = self.hp
        n_rot, fs = hp.n_rot, hp.freq_scale
        if self.mut == "drop":
            ffv = None
        elif self.mut == "shift":
            ffv = np.roll(ffv, 1)
        elif self.mut == "scale1":
            fs = 1.0
        elif self.mut == "nrot_full":
            n_rot = hp.head_dim
            if ffv is not None:
                ffv = np.concatenate([ffv, np.ones(n_rot // 2 - ffv.size, np.float32)])
        elif self.mut == "q_only":
            ffv = ffv if which == "q" else None
        else:
            raise ValueError(self.mut)
        return R.rope_norm(x, pos, n_rot, hp.rope_base, ffv, fs)


def _normed0(orc, tok):
    """Layer 0's attention input of one token: rms_norm(embedding) * attn_norm."""
    x = orc._row("token_embd.weight", tok)
    return (R.rms_norm(x, orc.hp.eps) * orc._w("blk.0.attn_norm.weight")).astype(np.float32)


def _quanta(cur, wtype):
    """The activation in units of its int8 quantum, as the quantiser of wtype's vec_dot_type
    forms it just before rounding (quantize_row_q8_K_ref / quantize_row_q8_0)."""
    if wtype == R.Q8_0:
        x = cur.reshape(-1, R.QK8_0)
        amax = np.abs(x).max(axis=1).astype(np.float32)
        return (x * (np.float32(127.0) / amax)[:, None]).astype(np.float32)
    x = cur.reshape(-1, R.QK_K)
    mx = x[np.arange(x.shape[0]), np.argmax(np.abs(x), axis=1)]
    return ((np.float32(-127.0) / mx).astype(np.float32)[:, None] * x).astype(np.float32)


def qualifying_tokens(orc, n):
    """The first n token ids, in id order, whose layer-0 normed activation has no element within
    BOUNDARY quanta of a rounding boundary of the format attn_k reads (Q8_K or Q8_0): the device's
    rms_norm differs from the oracle's in the last bit (~1e-4 quanta), which then cannot flip an
    int8 of the activation and move a whole K row by several times the GEMV bar."""
    wtype = orc.tensors["blk.0.attn_k.weight"].type
    out = []
    for tok in range(orc.hp.n_vocab):
        v = _quanta(_normed0(orc, tok), wtype).astype(np.float64)
        if np.min(np.abs(v - np.floor(v) - 0.5)) >= BOUNDARY:
            out.append(tok)
            if len(out) == n:
                break
    return out


def _outputs(orc, prompt):
    return [orc.decode(prompt)] + [orc.decode_one(t) for t in STEPS]


def _stable(buf, prompt, runs=4):
    """Whether the oracle's logits at the 5 checked outputs move by less than LOGIT_TOL / 10 x rms
    under util.oracle_ulp_floor's kind of perturbation: every GEMV output, attention score and head
    output moved by up to NOISE (relative) at random, the attention dots summed in f32 as ggml's
    AVX2 ggml_vec_dot_f16 does.  16 ulps, not 1: an f16 rounding of q or of a softmax weight that
    falls the other way moves the next activation by that much, and the int8 quantum it then
    crosses moves these models' logits by 3e-3 .. 8e-3 x rms (Q/K weights 30 x the default)."""
    base = _outputs(oracle_from_gguf(buf, n_ctx=N_CTX), prompt)
    orig, orig_attn = R.mul_mat_vec, R.attention_head
    try:
        for seed in range(runs):
            rng = np.random.default_rng(seed)

            def ulp(y):
                y = np.ascontiguousarray(y, np.float32)
                return (y * (1.0 + rng.uniform(-1.0, 1.0, y.shape) * NOISE)).astype(np.float32)

            def mm(raw, t, K, x):
                return ulp(orig(raw, t, K, x))

            def attn32(q, K16, V16, scale):
                q16 = R.f32_to_f16(q).astype(np.float32)
                s = ulp((K16.astype(np.float32) @ q16).astype(np.float32))
                p16 = R.f32_to_f16(R.soft_max(s, scale)).astype(np.float32)
                return ulp((p16 @ V16.astype(np.float32)).astype(np.float32))
            R.mul_mat_vec = mm
            R.attention_head = attn32
            for b, o in zip(base, _outputs(oracle_from_gguf(buf, n_ctx=N_CTX), prompt)):
                if float(np.max(np.abs(o - b))) > 0.1 * LOGIT_TOL * _rms(b):
                    return False
    finally:
        R.mul_mat_vec, R.attention_head = orig, orig_attn
    return True


def _ulp16(a16):
    return np.spacing(np.abs(a16)).astype(np.float64)


class _Ref:
    """One correct oracle run of a config: prompt, layer-0 cache, its element-wise bounds, logits."""

    def __init__(self, name):
        self.name = name
        self.buf = synthetic.build_gguf(synthetic.CONFIGS[name], seed=SEED)
        orc = oracle_from_gguf(self.buf, n_ctx=N_CTX)
        hp = self.hp = orc.hp
        self.kvd = hp.n_head_kv * hp.head_dim
        # the first window of 40 qualifying tokens on which the oracle's own logits are stable
        # under a last-bit change of every GEMV output (_stable): a later activation can sit on
        # a quantum boundary too, and the logit bar is for the kernels, not for that
        cand = qualifying_tokens(orc, N_PROMPT + 8)
        assert len(cand) == N_PROMPT + 8, f"{name}: {len(cand)} qualifying tokens"
        self.skipped = next(s for s in range(9) if _stable(self.buf, cand[s:s + N_PROMPT]))
        self.prompt = cand[self.skipped:self.skipped + N_PROMPT]
        self.logits = [orc.decode(self.prompt)]
        self.k0 = orc.kcache[0][:N_PROMPT].copy()
        self.v0 = orc.vcache[0][:N_PROMPT].copy()
        self.cell_pos = list(orc.cell_pos)
        self.logits += [orc.decode_one(t) for t in STEPS]
        # the bounds: pre-rotation K, V and their abs-sums per prompt token
        tk, tv = orc.tensors["blk.0.attn_k.weight"], orc.tensors["blk.0.attn_v.weight"]
        ff = orc.tensors.get("rope_freqs.weight")
        ffv = None if ff is None else R.dequantize(ff.data, ff.type)
        hd, nr = hp.head_dim, hp.n_rot
        self.rot = np.tile(np.arange(hd) < nr, hp.n_head_kv)         # (kvd,) rotated elements
        self.kbound = np.empty((N_PROMPT, self.kvd))
        self.vbound = np.empty((N_PROMPT, self.kvd))
        for c, tok in enumerate(self.prompt):
            cur = _normed0(orc, tok)
            k = R.mul_mat_vec(tk.data, tk.type, tk.shape[0], cur).astype(np.float64)
            a = R.mul_mat_vec_abs(tk.data, tk.type, tk.shape[0], cur)
            # the helper restates the oracle's own layer-0 K (a wrong helper would bound nothing)
            kr = R.rope_norm(k.astype(np.float32).reshape(hp.n_head_kv, hd), c, nr, hp.rope_base, ffv, hp.freq_scale)
            assert np.array_equal(R.f32_to_f16(kr.reshape(-1)), self.k0[c])
            pair = lambda z: np.repeat(z[0::2] + z[1::2], 2)   # noqa: E731  (x0 + x1 on both elements)
            d = np.where(self.rot, GEMV_TOL * pair(a) + TRIG_TOL * pair(np.abs(k)), GEMV_TOL * a)
            self.kbound[c] = d + _ulp16(self.k0[c])
            av = R.mul_mat_vec_abs(tv.data, tv.type, tv.shape[0], cur)
            self.vbound[c] = GEMV_TOL * av + _ulp16(self.v0[c])

    def k_ratio(self, k16):
        return np.abs(k16.astype(np.float64) - self.k0.astype(np.float64)) / self.kbound

    def mutant(self, mut):
        """(layer-0 K rows, final logits) of the oracle with the fault `mut`."""
        orc = oracle_from_gguf(self.buf, n_ctx=N_CTX)
        orc.__class__ = _Mutant
        orc.mut = mut
        orc.decode(self.prompt)
        k = orc.kcache[0][:N_PROMPT].copy()
        for t in STEPS:
            lg = orc.decode_one(t)
        return k, lg


_REFS = {}


def _ref(name) -> _Ref:
    if name not in _REFS:
        _REFS[name] = _Ref(name)
    return _REFS[name]


def _rms(x):
    return float(np.sqrt(np.mean(x.astype(np.float64) ** 2)))


# ---- CPU guards ---------------------------------------------------------------------------------

@pytest.mark.parametrize("name", CFGS)
def test_prompt_tokens_qualify(name):
    """40 qualifying tokens exist, roughly 60 % of the ids scanned (256 elements x 2e-3), and the
    oracle's run holds its own K bound trivially (ratio 0)."""
    r = _ref(name)
    assert len(r.prompt) == N_PROMPT and r.prompt == sorted(set(r.prompt))
    assert r.prompt[-1] < 3 * N_PROMPT, r.prompt[-1]
    assert r.cell_pos == list(range(N_PROMPT))
    assert float(r.k_ratio(r.k0).max()) == 0.0


@pytest.mark.parametrize("name,mut", [(n, m) for n in CFGS for m in MUTATIONS[n]])
def test_rope_fault_would_be_detected(name, mut):
    """Each fault leaves the K bound on >= 1/4 of the rotated elements and moves the final logits
    by more than 10 x LOGIT_TOL x rms: the GPU tests below fail on a kernel with that fault."""
    r = _ref(name)
    k, lg = r.mutant(mut)
    out = r.k_ratio(k)[:, r.rot] > 1.0
    ref = r.logits[-1]
    dl = float(np.max(np.abs(lg - ref))) / _rms(ref)
    print(f"{name} {mut}: K outside its bound on {out.mean():.2f} of the rotated elements, "
          f"max|dlogit|/rms = {dl:.2e}")
    assert out.mean() >= 0.25
    assert dl > 10 * LOGIT_TOL


# ---- GPU: the prompt paths -----------------------------------------------------------------------

_RUNS = {}


def _gpu_run(name, path, monkeypatch):
    """The prompt through `path` on a fresh context, then STEPS one token at a time: the state
    after the prompt and the logits / top-10 ids at each output.  One run per (config, path)."""
    key = (name, path)
    if key not in _RUNS:
        for k, v in PATHS[path].items():
            monkeypatch.setenv(k, v)
        r = _ref(name)
        try:
            m = engine.Model(r.buf)
            ctx = engine.Context(m, n_ctx=N_CTX)
            try:
                res = {"decode_path": ctx.decode_path()}
                assert ctx.decode(r.prompt) == 0
                res["state"] = parse_state(ctx.state_get(), r.hp.n_layer, r.kvd)
                res["out"] = [(ctx.logits(), [int(i) for i in ctx.topk(10)[0]])]
                for t in STEPS:
                    assert ctx.decode([t]) == 0
                    res["out"].append((ctx.logits(), [int(i) for i in ctx.topk(10)[0]]))
            finally:
                ctx.close()
                m.close()
            _RUNS[key] = res
        except Exception as e:   # the second test of this run reports the same failure, without a second run
            _RUNS[key] = e
    if isinstance(_RUNS[key], Exception):
        raise _RUNS[key]
    return _RUNS[key]


GPU_CASES = [(n, p) for n in CFGS for p in PATHS]


@pytest.mark.gpu
@pytest.mark.parametrize("name,path", GPU_CASES)
def test_layer0_kv_cache_matches_oracle(gpu_lib, monkeypatch, name, path):
    """Every element of layer 0's K and V rows within its derived bound (module docstring)."""
    r = _ref(name)
    run = _gpu_run(name, path, monkeypatch)
    if path == "single":   # which of the two decode-step implementations this was
        assert run["decode_path"] == DECODE_PATH[name]
    pos, k, v = run["state"]
    assert list(pos) == r.cell_pos
    kr = r.k_ratio(k[0])
    vr = np.abs(v[0].astype(np.float64) - r.v0.astype(np.float64)) / r.vbound
    print(f"{name} {path}: K max err/bound = {kr.max():.3f} (rotated {kr[:, r.rot].max():.3f}), "
          f"V max err/bound = {vr.max():.3f}")
    bad = np.argwhere(kr > 1.0)
    assert bad.size == 0, f"{len(bad)} K elements outside their bound, first (cell, element) {bad[0]}"
    assert vr.max() <= 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("name,path", GPU_CASES)
def test_logits_match_oracle(gpu_lib, monkeypatch, name, path):
    """Logits within LOGIT_TOL x rms and the same top-10 ids after the prompt and each of the 4
    following single-token steps (Q's rotation; the guard above shows the bar is sensitive)."""
    r = _ref(name)
    run = _gpu_run(name, path, monkeypatch)
    worst = 0.0
    for i, ((got, ids), ref) in enumerate(zip(run["out"], r.logits)):
        err = float(np.max(np.abs(got - ref))) / _rms(ref)
        worst = max(worst, err)
        assert err <= LOGIT_TOL, (name, path, i, err)
        assert ids == [t for t, _ in R.topk(ref, 10)], (name, path, i)
    print(f"{name} {path}: max|dlogit|/rms = {worst:.2e}")


# ---- GPU: the K-shift ----------------------------------------------------------------------------

def _ffv(orc):
    ff = orc.tensors.get("rope_freqs.weight")
    return None if ff is None else R.dequantize(ff.data, ff.type)


def _check_shift(k_before, k_after, v_before, v_after, deltas, orc):
    """The shifted cache against f16(rope(f32(K_before), delta)): <= 1 f16 ulp on rotated elements
    (cosf / sinf may differ by an ulp), the same bits from n_rot on and in V."""
    hp = orc.hp
    ref = _kshift_ref(k_before, deltas, hp, _ffv(orc))
    rot = np.tile(np.arange(hp.head_dim) < hp.n_rot, hp.n_head_kv)
    ulp = np.abs(k_after.view(np.int16).astype(np.int32) - ref.view(np.int16).astype(np.int32))
    assert ulp[..., rot].max() <= 1
    assert np.array_equal(k_after[..., ~rot].view(np.int16), k_before[..., ~rot].view(np.int16))
    assert np.array_equal(v_after.view(np.int16), v_before.view(np.int16))
    moved = np.array(deltas) != 0   # the shift did rotate: not a comparison of two untouched caches
    assert np.any(k_after[:, moved][..., rot] != k_before[:, moved][..., rot])


SHIFT_CFGS = ["tiny-rf-q4_k_m", "tiny-prot-q4_k_m", "tiny-rf-q8_0"]
SHIFT_TOKS = list(range(3, 15))


def _shift_setup(name):
    buf = synthetic.build_gguf(synthetic.CONFIGS[name], seed=SEED)
    m = engine.Model(buf)
    a = engine.Context(m, n_ctx=32)
    o = oracle_from_gguf(buf, n_ctx=32)
    a.decode(SHIFT_TOKS)
    o.decode(SHIFT_TOKS)
    return m, a, o, parse_state(a.state_get(), o.hp.n_layer, o.hp.n_head_kv * o.hp.head_dim)


@pytest.mark.gpu
@pytest.mark.parametrize("name", SHIFT_CFGS)
def test_self_extend_kshift(gpu_lib, name):
    """test_self_extend_div_matches_oracle's sequence with factors, scale and partial rotary."""
    m, a, o, (_, k_before, v_before) = _shift_setup(name)
    hp = o.hp
    try:
        a.kv_seq_add(0, 12, 0)
        a.kv_seq_div(0, 8, 2)
        a.kv_seq_add(8, 12, -4)
        o.kv_seq_shift(0, 8, div=2)
        o.kv_seq_shift(8, 12, delta=-4)
        pos, k_after, v_after = parse_state(a.state_get(), hp.n_layer, hp.n_head_kv * hp.head_dim)
        assert list(pos) == o.cell_pos and a.pos_max == max(o.cell_pos)
        _check_shift(k_before, k_after, v_before, v_after, [p // 2 - p for p in range(8)] + [-4] * 4, o)
        a.decode([40])
        ref, got = o.decode_one(40), a.logits()
        err = float(np.max(np.abs(got - ref))) / _rms(ref)
        print(f"{name} self-extend: max|dlogit|/rms = {err:.2e}")
        assert err <= 5e-2
        assert int(np.argmax(got)) == int(np.argmax(ref))
    finally:
        a.close()
        m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", SHIFT_CFGS)
def test_context_shift_kshift(gpu_lib, name):
    """test_context_shift_matches_oracle's sequence: seq_rm [2, 5) then seq_add(5, 12, -3)."""
    m, a, o, (_, k_before, v_before) = _shift_setup(name)
    hp = o.hp
    try:
        a.kv_seq_rm(2, 5)
        o.kv_seq_rm(2, 5)
        a.kv_seq_add(5, 12, -3)
        o.kv_seq_shift(5, 12, delta=-3)
        pos, k_after, v_after = parse_state(a.state_get(), hp.n_layer, hp.n_head_kv * hp.head_dim)
        assert list(pos) == o.cell_pos == [0, 1] + list(range(2, 9)) and a.pos_max == 8
        keep = [0, 1] + list(range(5, 12))
        _check_shift(k_before[:, keep], k_after, v_before[:, keep], v_after, [0, 0] + [-3] * 7, o)
        a.decode([40])
        ref, got = o.decode_one(40), a.logits()
        err = float(np.max(np.abs(got - ref))) / _rms(ref)
        print(f"{name} context shift: max|dlogit|/rms = {err:.2e}")
        assert err <= LOGIT_TOL
    finally:
        a.close()
        m.close()
