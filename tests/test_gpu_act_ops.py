"""Op-level tests of the kernels that run between the GEMMs, against the numpy reference of act_ref_util.py
(oracle/ggml_ref.py's rms_norm, layer_norm, quantize_q8_K, quantize_q8_0, silu and RoPE angles):

  mi_op_quant_act   quant_act_kernel in every mode: plain, RMSNorm, LayerNorm, rows, part (with the
                    write-back and an addend), swiglu; every instantiation (<16, 1|2|4|16>), the
                    gridDim.y > 1 spread of un-normed rows, padding rows, Q8_K and Q8_0
  mi_op_dgemv_norm  dv_quant_kernel with a norm at K within, at and past one request round, and the
                    DV_QKVN / DV_SWIGLUN launches bit-identical to DV_QKV / DV_SWIGLU over its output
  mi_op_qkv_finish  rope_table_kernel and qkv_finish_kernel at real head geometry, positions to 131071
  mi_op_part_sum    part_sum_kernel with resid, addend, aliasing, strides and swiglu

Bars (act_ref_util): quants equal the reference's but within BOUNDARY quanta of a .5 (either neighbour),
scales within 2 ulp, sums exactly those of the returned quants; f32-add-only paths bit-exact; rotated
elements TRIG_TOL (|v0| + |v1|) (+ one f16 ulp in the cache); silu(g) u within 4 f32 ulps.

The rope table against float64 cos / sin of the reference's float32 angle: the largest deviation measured
on an MI355X over QKV_CASES (positions 0, 1, 4095, 131071) is 5.977e-08 (ROPE_TABLE_MEASURED, per case
5.98e-8, 5.13e-8, 4.30e-8, 2.97e-8, 3.83e-8, 4.10e-8); the bar is twice that, 1.2e-7, no looser than
TRIG_TOL = 4.77e-7.

The CPU tests at the end hold the comparators to deliberately wrong references, and the listed inputs to
the conditions the comparators need."""
import functools

import numpy as np
import pytest

import act_ref_util as A
import ggml_ref as R
from blama_amd import engine
from gemm_ref_util import gemv_ref, gemv_swiglu_ref
from test_gpu_dgemv import GEMV_TOL, _check
from util import rand_matrix

gpu = pytest.mark.gpu

ROPE_TABLE_MEASURED = 6.0e-8                                 # (5.977e-08: half an f32 ulp at 1)
ROPE_TABLE_TOL = A.TRIG_TOL if ROPE_TABLE_MEASURED is None else min(2 * ROPE_TABLE_MEASURED, A.TRIG_TOL)

QA_IDS = [c["name"] for c in A.QA_CASES]


@functools.lru_cache(maxsize=None)
def _qa(i):
    case = A.QA_CASES[i]
    return A.qa_build(case, A.qa_seed(case))


# ---- quant_act -----------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("i", range(len(A.QA_CASES)), ids=QA_IDS)
def test_quant_act(gpu_lib, i):
    args, ref, zero, x_after = _qa(i)
    got = engine.op_quant_act(**args)
    A.check_quant_act(got, ref, zero, A.QA_CASES[i]["name"])
    if "x" in args:   # the rows after the call: the part mode's write-back bit for bit, else untouched
        want = args["x"] if x_after is None else x_after
        assert np.array_equal(got["x"].view(np.uint32), np.ascontiguousarray(want).view(np.uint32))


@gpu
def test_quant_act_refusals(gpu_lib):
    K, n = 512, 3
    x = np.ones((n, K), np.float32)
    w = np.ones(K, np.float32)
    part = np.ones((2, n, K), np.float32)
    pair = np.ones((2, n, 2 * K), np.float32)
    for kw, msg in [
        (dict(x=x, addend=w), "an addend goes with"),
        (dict(x=x, part=pair, swiglu=True, addend=w), "an addend goes with"),
        (dict(x=x, norm_b=w), "a LayerNorm bias goes with"),
        (dict(x=x, part=np.ones((65, n, K), np.float32)), "1..64 split-K partials"),
        (dict(x=x, swiglu=True), "swiglu takes a pair launch's parts"),
        (dict(part=pair, swiglu=True, norm_w=w), "swiglu takes a pair launch's parts"),
        (dict(), "no input rows"),
        (dict(x=np.ones((n, K + 4), np.float32), part=part), "split-K partials take a dense"),
        (dict(x=x, part=part, rows=np.arange(n)), "split-K partials take a dense"),
    ]:
        with pytest.raises(engine.EngineError, match=msg):
            engine.op_quant_act(K, n, **kw)
    with pytest.raises(engine.EngineError, match="K must be a multiple of 256"):
        engine.op_quant_act(384, n, x=np.ones((n, 384), np.float32))
    with pytest.raises(engine.EngineError, match="K past 65536"):
        engine.op_quant_act(65536 + 256, 1, x=np.ones((1, 65536 + 256), np.float32))
    with pytest.raises(engine.EngineError, match="row index outside x"):
        engine.op_quant_act(K, n, x=x, rows=np.array([0, 3, 1]))


# ---- dv_quant_kernel with a norm; the in-launch normed roles ----------------------------------------------

@functools.lru_cache(maxsize=None)
def _dvq(K):
    x, w = A.dvq_build(K, A.DVQ_SEEDS.get(K, 0))
    return (x, w) + A.dvq_ref(x, w)


@gpu
@pytest.mark.parametrize("fmt", [1, 2, 3], ids=["q8k", "q80", "both"])
@pytest.mark.parametrize("K", A.DVQ_KS)
def test_dv_quant_norm(gpu_lib, K, fmt):
    x, w, refk, ref0 = _dvq(K)
    got = engine.op_dgemv_norm(False, 0, 0, None, 0, K, x, w, eps=A.EPS, fmt=fmt)
    assert got["fmt"] == fmt and ("q8k" in got) == bool(fmt & 1) and ("q80" in got) == bool(fmt & 2)
    A.check_published(got, refk, ref0, f"K={K} fmt={fmt}")


def _dgemv_norm_case(K, seed):
    x, w = A.dvq_build(K, seed)
    return x, w, A.rms32(x, w)


@gpu
@pytest.mark.parametrize("role", [0, 2], ids=["qkv", "swiglu"])
@pytest.mark.parametrize("t", [R.Q4_K, R.Q6_K, R.Q8_0], ids=lambda t: R.TYPE_NAME[t])
@pytest.mark.parametrize("rows,K", [(64, 256), (256, 2048), (512, 4096)])
def test_dgemv_norm(gpu_lib, rows, K, t, role):
    x, w, xn = _dgemv_norm_case(K, 0)
    a = rand_matrix(t, rows, K, seed=rows + K + t)
    b = rand_matrix(t, rows, K, seed=rows + K + t + 1) if role == 2 else None
    kw = dict(type2=t, raw2=b, rows2=rows) if role == 2 else {}
    r0 = engine.op_dgemv_norm(False, role, t, a, rows, K, x, w, eps=A.EPS, want_act=True, **kw)
    r1 = engine.op_dgemv_norm(True, role, t, a, rows, K, x, w, eps=A.EPS, **kw)
    assert np.array_equal(r0["y"].view(np.uint32), r1["y"].view(np.uint32)), "the in-launch form differs from dv_quant + GEMV"
    A.check_published(r0, *A.dvq_ref(x, w), f"{rows}x{K}")
    g, ga = gemv_ref(t, a, K, xn)
    if role == 0:
        _check(r0["y"], g, ga, f"QKV {R.TYPE_NAME[t]} {rows}x{K}")
        return
    u, ua = gemv_ref(t, b, K, xn)
    ref, bound = gemv_swiglu_ref(g, ga, u, ua, GEMV_TOL)
    err = np.abs(r0["y"].astype(np.float64) - ref)
    assert np.all(err <= bound), (R.TYPE_NAME[t], rows, K, float((err / bound).max()))


@gpu
def test_dgemv_norm_mixed_qkv(gpu_lib):
    rows0, rows1, K = 256, 128, 2048
    x, w, xn = _dgemv_norm_case(K, 0)
    a, b = rand_matrix(R.Q4_K, rows0, K, seed=11), rand_matrix(R.Q6_K, rows1, K, seed=12)
    kw = dict(type2=R.Q6_K, raw2=b, rows2=rows1)
    r0 = engine.op_dgemv_norm(False, 0, R.Q4_K, a, rows0, K, x, w, eps=A.EPS, **kw)
    r1 = engine.op_dgemv_norm(True, 0, R.Q4_K, a, rows0, K, x, w, eps=A.EPS, **kw)
    assert np.array_equal(r0["y"].view(np.uint32), r1["y"].view(np.uint32))
    _check(r0["y"][:rows0], *gemv_ref(R.Q4_K, a, K, xn), "mixed seg 0")
    _check(r0["y"][rows0:], *gemv_ref(R.Q6_K, b, K, xn), "mixed seg 1")


@gpu
def test_dgemv_norm_refusals(gpu_lib):
    K = 5632   # 3 chunks: no Q/K/V or SwiGLU variant is compiled, in either form
    x, w = np.ones(K, np.float32), np.ones(K, np.float32)
    a = rand_matrix(R.Q4_K, 64, K, seed=1)
    for inl in (False, True):
        with pytest.raises(engine.EngineError, match="no compiled variant"):
            engine.op_dgemv_norm(inl, 0, R.Q4_K, a, 64, K, x, w)
    with pytest.raises(engine.EngineError, match="role 0 .* or 2"):
        engine.op_dgemv_norm(False, 1, R.Q4_K, a, 64, K, x, w)
    with pytest.raises(engine.EngineError, match="quantise only"):
        engine.op_dgemv_norm(False, 0, 0, None, 0, 256, x[:256], w[:256], fmt=0)


# ---- rope table, Q / K / V finish ------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _qkv(i):
    a = A.qkv_build(A.QKV_CASES[i])
    return a, A.qkv_ref(a)


@gpu
@pytest.mark.parametrize("i", range(len(A.QKV_CASES)))
def test_qkv_finish(gpu_lib, i):
    a, ref = _qkv(i)
    got = engine.op_qkv_finish(**a)
    dev = float(np.abs(got["rope"].astype(np.float64) - ref["rope"]).max())
    print(f"qkv case {i}: rope table max deviation {dev:.3e} (TRIG_TOL {A.TRIG_TOL:.3e})")
    A.check_qkv(got, ref, ROPE_TABLE_TOL, f"case {i}")


@gpu
def test_qkv_finish_refusals(gpu_lib):
    a = A.qkv_build(A.QKV_CASES[4])
    part = a.pop("part")
    with pytest.raises(engine.EngineError, match="qkv_finish: bad shape"):
        engine.op_qkv_finish(part, **{**a, "nq": 255})
    with pytest.raises(engine.EngineError, match="qkv_finish: bad shape"):
        engine.op_qkv_finish(part, **{**a, "n_rot": 34, "theta_scale": 0.5})


# ---- part_sum ------------------------------------------------------------------------------------------
PS_VARIANTS = ["bare", "resid", "resid_addend", "alias", "swiglu"]


@gpu
@pytest.mark.parametrize("variant", PS_VARIANTS)
@pytest.mark.parametrize("kp,ntok", [(1, 1), (4, 33)])
@pytest.mark.parametrize("rows", [1, 255, 257, 32000])
def test_part_sum(gpu_lib, rows, kp, ntok, variant):
    rng = np.random.default_rng(rows + kp)
    sw = rows + 3 if variant == "swiglu" else 0
    pstride = (2 * rows + 5) if sw else rows + 2
    part = rng.standard_normal((kp, ntok, pstride)).astype(np.float32)
    ostride = rows + 3
    resid = addend = None
    if variant in ("resid", "resid_addend", "alias"):
        resid = rng.standard_normal((ntok, ostride if variant == "alias" else rows + 1)).astype(np.float32)
    if variant == "resid_addend":
        addend = rng.standard_normal(rows).astype(np.float32)
    out = engine.op_part_sum(part, rows, resid=resid, alias=variant == "alias", ostride=ostride, swiglu=sw, addend=addend)
    ref, bound = A.part_sum_ref(part, rows, resid, addend, sw)
    A.check_part_sum(out, ref, bound, rows, resid[:, rows:] if variant == "alias" else None, variant)


@gpu
def test_part_sum_refusals(gpu_lib):
    part = np.ones((2, 3, 40), np.float32)
    res = np.ones((3, 16), np.float32)
    add = np.ones(16, np.float32)
    for kw, msg in [
        (dict(addend=add), "an addend goes with a residual"),
        (dict(addend=add, resid=res, swiglu=16), "an addend goes with a residual"),
        (dict(swiglu=30), "part_sum: bad shape"),      # rows + swiglu past pstride
        (dict(swiglu=8), "part_sum: bad shape"),       # the up rows inside the gate rows
        (dict(ostride=8), "a stride shorter than the rows"),
    ]:
        with pytest.raises(engine.EngineError, match=msg):
            engine.op_part_sum(part, 16, **kw)
    with pytest.raises(engine.EngineError, match="part_sum: bad shape"):
        engine.op_part_sum(part, 41)


# ---- CPU: the inputs meet the comparators' conditions; wrong references are caught -------------------------

@pytest.mark.parametrize("i", range(len(A.QA_CASES)), ids=QA_IDS)
def test_quant_act_inputs_meet_conditions(i):
    _, ref, zero, _ = _qa(i)
    share, ties = A.input_conditions(ref)
    assert share <= A.NEAR_SHARE and ties == 0, (share, ties)
    npad = (A.QA_CASES[i]["ntok"] + 31) // 32 * 32
    A.check_quant_act(A.qa_simulate(ref, zero, npad), ref, zero)   # the reference passes its own comparator
    assert (ref["d"] == 0).any() or (A.QA_CASES[i]["mode"] == "ln" and A.QA_CASES[i]["K"] < 512), "no all-zero block"


@pytest.mark.parametrize("K", A.DVQ_KS)
def test_dv_quant_inputs_meet_conditions(K):
    for ref in _dvq(K)[2:]:
        share, ties = A.input_conditions(ref)
        assert share <= A.NEAR_SHARE and ties == 0, (share, ties)
    for Kg in (256, 2048, 4096):
        x, w = A.dvq_build(Kg, 0)
        for ref in A.dvq_ref(x, w):
            assert A.input_conditions(ref)[0] <= A.NEAR_SHARE and A.input_conditions(ref)[1] == 0


def test_rope_args_restate_the_oracle():
    assert A.rope_consistent()


def _case(name):
    case = next(c for c in A.QA_CASES if c["name"] == name)
    return case, A.qa_build(case, A.qa_seed(case))


def _requant(case, args, ref, X=None, **norm):
    """quant_ref of the case's rows under another norm (the wrong references)."""
    X = args["x"][:, :case["K"]] if X is None else X
    Y32, Y64 = norm["fn"](X)
    out = A.quant_ref(Y32, Y64, case["q80"])
    out["live"] = ref["live"]
    return out


def test_quant_act_faults_would_be_detected():
    # the RMS scale over the first 8192 elements only
    case, (args, ref, zero, _) = _case("rms-16384")
    sim = A.qa_simulate(ref, zero, 32)
    w = args["norm_w"]

    def rms_8192(X):
        sc = [np.float32(1.0) / np.sqrt(np.float32(np.float32(np.sum((x[:8192] * x[:8192]).astype(np.float64)) / 8192) + np.float32(A.EPS)))
              for x in X]
        Y = np.stack([((x * s).astype(np.float32) * w).astype(np.float32) for x, s in zip(X, sc)])
        return Y, Y.astype(np.float64)
    with pytest.raises(AssertionError):
        A.check_quant_act(sim, _requant(case, args, ref, fn=rms_8192), zero)
    # eps dropped
    case, (args, ref, zero, _) = _case("rms-4096")
    sim = A.qa_simulate(ref, zero, 32)
    w = args["norm_w"]
    with pytest.raises(AssertionError):
        A.check_quant_act(sim, _requant(case, args, ref, fn=lambda X: A.normed_rows(X, "rms", w, eps=0.0)), zero)
    # a padding row non-zero
    bad = {k: v.copy() for k, v in sim.items()}
    bad["q"][17, 5] = 1
    with pytest.raises(AssertionError):
        A.check_quant_act(bad, ref, zero)
    bad = {k: v.copy() for k, v in sim.items()}
    bad["d"][31, 0] = np.float32(1e-3)
    with pytest.raises(AssertionError):
        A.check_quant_act(bad, ref, zero)
    # lo outside 0..63 (64 hi + lo still the sum)
    bad = {k: v.copy() for k, v in sim.items()}
    bad["hi"][1, 2, 3] -= 1
    bad["lo"][1, 2, 3] += 64
    with pytest.raises(AssertionError):
        A.check_quant_act(bad, ref, zero)
    # a row the launch never wrote: the fill pattern
    bad = {k: v.copy() for k, v in sim.items()}
    bad["q"][2] = -128
    with pytest.raises(AssertionError):
        A.check_quant_act(bad, ref, zero)
    bad = {k: v.copy() for k, v in sim.items()}
    bad["d"][0, 0] = np.float32(np.nan)   # (the reference's scale there is 0: one "ulp" from the NaN fill's bits)
    with pytest.raises(AssertionError):
        A.check_quant_act(bad, ref, zero)


def test_part_order_faults_would_be_detected():
    # the write-back: parts summed in reverse order; the addend before the residual
    case, (args, ref, zero, x_after) = _case("part-rms-k4-add")
    P, x, add = args["part"], args["x"], args["addend"]
    rev = A.add32(A.add32(A.sum_parts(P[::-1]), x), add)
    first = A.add32(A.add32(A.sum_parts(P), add), x)
    for wrong in (rev, first):
        assert not np.array_equal(wrong.view(np.uint32), x_after.view(np.uint32))
    # part_sum
    rng = np.random.default_rng(0)
    part = rng.standard_normal((4, 33, 259)).astype(np.float32)
    resid = rng.standard_normal((33, 258)).astype(np.float32)
    addend = rng.standard_normal(257).astype(np.float32)
    ref, bound = A.part_sum_ref(part, 257, resid, addend)
    sim = np.full((33, 260), np.nan, np.float32)
    sim.view(np.uint32)[:] = 0xFFFFFFFF
    sim[:, :257] = ref.astype(np.float32)
    A.check_part_sum(sim, ref, bound, 257)
    for kw in (dict(order="reverse"), dict(addend_first=True)):
        wrong, _ = A.part_sum_ref(part, 257, resid, addend, **kw)
        with pytest.raises(AssertionError):
            A.check_part_sum(sim, wrong, bound, 257)
    over = sim.copy()
    over[3, 257] = 0.0
    with pytest.raises(AssertionError):
        A.check_part_sum(over, ref, bound, 257)
    # swiglu: silu left out
    ref, bound = A.part_sum_ref(part[:, :, :259], 100, swiglu=128)
    sim = np.full((33, 100), 0, np.float32)
    sim[:] = ref.astype(np.float32)
    A.check_part_sum(sim, ref, bound, 100)
    with pytest.raises(AssertionError):
        A.check_part_sum((A.sum_parts(part[:, :, :100]) * A.sum_parts(part[:, :, 128:228])).astype(np.float32), ref, bound, 100)


@pytest.mark.parametrize("i", [1, 5])
@pytest.mark.parametrize("fault", ["neox", "pos", "rotate_v", "cell", "table"])
def test_qkv_faults_would_be_detected(i, fault):
    a, ref = _qkv(i)
    sim = A.qkv_simulate(ref)
    A.check_qkv(sim, ref, ROPE_TABLE_TOL)   # the reference passes its own comparator
    ntok = a["part"].shape[1]
    if fault == "table":                    # a table entry one TRIG_TOL and a bit off
        bad = dict(sim, rope=sim["rope"].copy())
        bad["rope"][0, 0, 1] += np.float32(3 * A.TRIG_TOL)
        with pytest.raises(AssertionError):
            A.check_qkv(bad, ref, ROPE_TABLE_TOL)
        return
    if fault == "cell" and ntok == 1:
        wrong = A.qkv_ref(a, cell_of=(a["tok_cell"] + 1) % a["n_ctx"])
    else:
        wrong = A.qkv_ref(a, **{"neox": dict(pairing="neox"), "pos": dict(pos_shift=1), "rotate_v": dict(rotate_v=True),
                                "cell": dict(cell_of=np.arange(ntok))}[fault])
    with pytest.raises(AssertionError):
        A.check_qkv(sim, wrong, ROPE_TABLE_TOL)
