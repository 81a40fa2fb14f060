"""The reference of the Q4_0 / Q5_0 tests, checked on its own: hand-written blocks whose values are
worked out here from ggml's block definitions (ggml-common.h block_q4_0 / block_q5_0,
dequantize_row_q4_0 / _q5_0 of b5187) must come out of legacy_quant_util.to_q8_0 +
ggml_ref.dequantize exactly; synthetic.quantize_rows must land within half a quantum."""
import numpy as np
import pytest

import ggml_ref as R
import legacy_quant_util as U
from blama_amd import synthetic

Q4_0, Q5_0 = 2, 6
D = np.float16(0.25)   # exact in f16 and in every product below


def _q4_block(qs):
    """block_q4_0 {f16 d; u8 qs[16]} and its 32 values: j -> (qs[j] & 0xF) - 8, j + 16 -> (qs[j] >> 4) - 8."""
    qs = [int(b) for b in qs]
    raw = np.array(list(np.array([D]).view(np.uint8)) + qs, np.uint8)
    vals = [((b & 0xF) - 8) for b in qs] + [((b >> 4) - 8) for b in qs]
    return raw, np.array(vals, np.float32) * np.float32(D)


def _q5_block(qh, qs):
    """block_q5_0 {f16 d; u8 qh[4]; u8 qs[16]}: x0 = ((qs[j] & 0xF) | (((qh >> j) << 4) & 0x10)) - 16 is
    value j, x1 = ((qs[j] >> 4) | ((qh >> (j + 12)) & 0x10)) - 16 value j + 16 (qh little-endian)."""
    qs = [int(b) for b in qs]
    qh = int(qh)
    raw = np.array(list(np.array([D]).view(np.uint8)) + [(qh >> (8 * i)) & 0xFF for i in range(4)] + qs, np.uint8)
    x0 = [(((b & 0xF) | (((qh >> j) << 4) & 0x10)) - 16) for j, b in enumerate(qs)]
    x1 = [(((b >> 4) | ((qh >> (j + 12)) & 0x10)) - 16) for j, b in enumerate(qs)]
    return raw, np.array(x0 + x1, np.float32) * np.float32(D)


NIBBLES = {
    "zeros": [0x00] * 16,
    "fifteens": [0xFF] * 16,
    "ramp": [(j & 0xF) | (((15 - j) & 0xF) << 4) for j in range(16)],
}


def _dequant_through_q8_0(raw, t):
    return R.dequantize(U.to_q8_0(raw, t), R.Q8_0)


@pytest.mark.parametrize("nib", sorted(NIBBLES))
def test_q4_0_blocks(nib):
    raw, want = _q4_block(NIBBLES[nib])
    assert raw.size == 18
    got = _dequant_through_q8_0(raw, Q4_0)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (nib, got, want)
    if nib == "zeros":
        assert np.all(want == -8 * 0.25)
    if nib == "fifteens":
        assert np.all(want == 7 * 0.25)
    if nib == "ramp":   # the low nibbles are the first 16 values, the high ones the last 16
        assert list(want / 0.25) == [j - 8 for j in range(16)] + [7 - j for j in range(16)]


QH = [0, 0xFFFFFFFF] + [1 << b for b in (0, 11, 12, 15, 16, 31)]


@pytest.mark.parametrize("qh", QH)
@pytest.mark.parametrize("nib", sorted(NIBBLES))
def test_q5_0_blocks(nib, qh):
    raw, want = _q5_block(qh, NIBBLES[nib])
    assert raw.size == 22
    got = _dequant_through_q8_0(raw, Q5_0)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (nib, hex(qh), got, want)
    # bit b of qh is the fifth bit of value b, whatever the nibbles
    base = _q5_block(0, NIBBLES[nib])[1]
    hi = [b for b in range(32) if (qh >> b) & 1]
    diff = (want - base) / 0.25
    assert [int(i) for i in np.nonzero(diff)[0]] == hi and np.all(diff[hi] == 16)
    assert want.min() >= -16 * 0.25 and want.max() <= 15 * 0.25


def test_blocks_in_a_row_keep_their_order():
    """Several blocks back to back: to_q8_0 keeps block order and each block's d."""
    blocks = [_q4_block(NIBBLES[n]) for n in ("ramp", "zeros", "fifteens")] * 3
    raw = np.concatenate([b[0] for b in blocks])
    want = np.concatenate([b[1] for b in blocks])
    got = _dequant_through_q8_0(raw, Q4_0)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("t", [Q4_0, Q5_0])
def test_quantize_rows_within_half_a_quantum(t):
    rng = np.random.default_rng(t)
    X = (rng.standard_normal((64, 256)) * 0.05).astype(np.float32)
    X[3, :32] = 0.0                                    # an all-zero block: d = 0
    raw = synthetic.quantize_rows(X, t)
    assert raw.size == 64 * U.row_bytes(t, 256)
    back = _dequant_through_q8_0(raw, t).reshape(X.shape)
    d = R.f16_bits_to_f32(raw.reshape(-1, U.BLOCK_BYTES[t])[:, 0:2].copy().view(np.uint16).reshape(-1))
    err = np.abs(back - X).reshape(-1, 32)
    assert np.all(err <= 0.5 * d[:, None] * (1 + 1e-6) + 1e-12), float((err / (d[:, None] + 1e-30)).max())
    assert np.all(back.reshape(-1, 32)[3 * 8] == 0.0)
    # fill_quant's random blocks are valid too: every value within the type's range times d
    buf = U.rand_matrix(t, 4, 512, seed=1)
    v = _dequant_through_q8_0(buf, t).reshape(-1, 32)
    dd = R.f16_bits_to_f32(buf.reshape(-1, U.BLOCK_BYTES[t])[:, 0:2].copy().view(np.uint16).reshape(-1))
    lo = 8 if t == Q4_0 else 16
    assert np.all(v >= -lo * dd[:, None] - 1e-9) and np.all(v <= (lo - 1) * dd[:, None] + 1e-9)
