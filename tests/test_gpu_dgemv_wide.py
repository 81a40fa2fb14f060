"""The wide form of the in-launch-quantising residual GEMV (blama_amd/csrc/dgemv.hip DV_ADDQW,
mi_op_dgemv role 5: 16-wave workgroups of 16 rows, wave w quantising blocks w, w + 16, ..) must
compute the bits of role 1 (a dv_quant launch, then DV_ADD) and of role 4 (the 8-wave form):
the same dv_quant_block arithmetic per 256-block, only another wave doing it.

Shapes: rows 16 / 24 / 40 (one full workgroup, a partial last one, several with an odd tail) x one
K per chunk instantiation -- 256 (C 1: one block, 15 idle quantising waves), 4096 (C 2: a block per
wave), 4352 (17 blocks: one wave takes two), 5632 (C 3), 11008 (C 6: 43 blocks, 3 / 2 per wave),
14336 (C 7: 56 blocks) -- x Q4_K, Q5_K, Q6_K, Q8_0, Q4_0, Q5_0; per type one input with an all-zero
block and a block whose largest |x| occurs twice (the tie rules of the quantiser); and 13 decode
steps of a tiny dense model with each of the three forms selected for the FFN down launch."""
import numpy as np
import pytest

import ggml_ref as R
import legacy_quant_util as U
from blama_amd import engine, synthetic
from gemm_ref_util import gemv_ref
from test_gpu_dgemv import GEMV_TOL, ROLE_ADD, ROLE_ADDQ
from util import rand_matrix, rand_x

pytestmark = pytest.mark.gpu

ROLE_ADDQW = 5
TYPES = [R.Q4_K, R.Q5_K, R.Q6_K, R.Q8_0, U.Q4_0, U.Q5_0]
IDS = ["Q4_K", "Q5_K", "Q6_K", "Q8_0", "Q4_0", "Q5_0"]
ROWS = (16, 24, 40)
KS = (256, 4096, 4352, 5632, 11008, 14336)


def _matrix(t, rows, K, seed):
    return (U.rand_matrix if t in (U.Q4_0, U.Q5_0) else rand_matrix)(t, rows, K, seed=seed)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _three(t, w, rows, K, x, res):
    y1 = engine.op_dgemv(ROLE_ADD, t, w, rows, K, x, resid=res)
    y4 = engine.op_dgemv(ROLE_ADDQ, t, w, rows, K, x, resid=res)
    y5 = engine.op_dgemv(ROLE_ADDQW, t, w, rows, K, x, resid=res)
    return y1, y4, y5


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("t", TYPES, ids=IDS)
def test_wide_inlaunch_quant_same_bits(gpu_lib, t, K):
    x = rand_x(K, seed=K + 5)
    for rows in ROWS:
        w = _matrix(t, rows, K, rows + K + t + 7)
        res = rand_x(rows, seed=rows + 2)
        y1, y4, y5 = _three(t, w, rows, K, x, res)
        assert np.array_equal(_bits(y5), _bits(y1)), ("wide vs dv_quant + ADD", rows, K)
        assert np.array_equal(_bits(y5), _bits(y4)), ("wide vs 8-wave", rows, K)


def test_wide_role_needs_resid(gpu_lib):
    rows, K = 16, 256
    w = rand_matrix(R.Q4_K, rows, K, seed=rows + K)
    with pytest.raises(engine.EngineError, match="op_dgemv: residual role needs resid"):
        engine.op_dgemv(ROLE_ADDQW, R.Q4_K, w, rows, K, rand_x(K, seed=K + 3), resid=None)


# 17 blocks (wave 0 quantises blocks 0 and 16).  Block 0 and block 16 all zeros; blocks 1 and 15: the
# largest |x| twice within one 32-element Q8_0 block, first negative then positive
TIE_K = 4352
TIE_M = np.float32(6.5)


def _tie_input():
    x = rand_x(TIE_K, seed=77)
    x[:256] = 0.0
    x[16 * 256:] = 0.0
    for b in (1, 15):
        x[b * 256 + 3] = -TIE_M
        x[b * 256 + 17] = TIE_M
    assert np.abs(x).max() == TIE_M
    return x


def test_tie_input_oracle_quantisation():
    """What ROLE_ADD has to reproduce for the tie input (CPU only): a zero block quantises to d = 0,
    q = 0; of two equal largest |x| the first decides the sign of Q8_K's scale (quantize_row_q8_K:
    iscale = -127 / max), so the first maps to -127 and the second, +127.0 exactly, stays 127."""
    x = _tie_input()
    a = R.quantize_q8_K(x)
    for b in (0, 16):
        assert a.d[b] == 0 and not a.qs[b].any() and not a.bsums[b].any()
    for b in (1, 15):
        assert a.d[b] == np.float32(1.0) / (np.float32(-127.0) / -TIE_M) and a.d[b] > 0
        assert a.qs[b][3] == -127 and a.qs[b][17] == 127
        assert np.abs(a.qs[b]).max() == 127
    z = R.quantize_q8_0(x)
    for b in list(range(8)) + list(range(16 * 8, 17 * 8)):
        assert z.d[b] == 0 and not z.qs[b].any()
    for b in (8, 15 * 8):
        assert z.d[b] == R.f32_to_f16(TIE_M / np.float32(127.0)).astype(np.float32)
        assert z.qs[b][3] == -127 and z.qs[b][17] == 127


@pytest.mark.parametrize("t", TYPES, ids=IDS)
def test_wide_tie_rules(gpu_lib, t):
    K, rows = TIE_K, 24
    x = _tie_input()
    w = _matrix(t, rows, K, 31 + t)
    res = rand_x(rows, seed=9)
    y1, y4, y5 = _three(t, w, rows, K, x, res)
    # ROLE_ADD reproduces the oracle's quantisation of this input (test_dgemv_residual_add's bound) ...
    legacy = t in (U.Q4_0, U.Q5_0)
    ref, absb = gemv_ref(R.Q8_0 if legacy else t, U.to_q8_0(w, t) if legacy else w, K, x)
    r = res.astype(np.float64)
    bound = absb * GEMV_TOL + (np.abs(ref) + np.abs(r)) * 1.2e-7 + 1e-30
    err = np.abs(y1.astype(np.float64) - (ref + r))
    print(f"tie input {t}: ROLE_ADD err / bound = {float((err / bound).max()):.3f}")
    assert np.all(err <= bound), float((err / bound).max())
    # ... and both in-launch forms reproduce ROLE_ADD
    assert np.array_equal(_bits(y5), _bits(y1))
    assert np.array_equal(_bits(y5), _bits(y4))


@pytest.mark.parametrize("cfg_name", ["tiny-q4_k_m", "tiny-q6_k"])
def test_decode_same_logits_whoever_quantises_h(gpu_lib, cfg_name):
    """13 decode steps with the FFN down launch fed by a dv_quant launch (form 0), quantising h in
    8-wave workgroups (1) and in 16-wave workgroups (2): bit-equal logits at every step."""
    m = engine.Model(synthetic.build_gguf(synthetic.CONFIGS[cfg_name], seed=6))
    toks = [1, 5, 9, 13, 4, 8, 15, 16, 23, 42, 101, 7, 250]
    out = []
    for form in (0, 1, 2):
        ctx = engine.Context(m, n_ctx=32)
        assert ctx.decode_path() == 1
        ctx.debug_down_quant(form)
        a = []
        for t in toks:
            ctx.decode([t])
            a.append(ctx.logits())
        out.append(np.stack(a))
        ctx.close()
    assert np.isfinite(out[0]).all()
    assert np.array_equal(out[2].view(np.uint32), out[0].view(np.uint32))
    assert np.array_equal(out[2].view(np.uint32), out[1].view(np.uint32))
