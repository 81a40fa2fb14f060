"""Op-level tests of the cache-attention launches that mi_op_attention does not reach: the decode
kernel and the fused kernel's quantising epilogue (decode step and short batch), the fused kernel's
R > 1 instantiations on a short batch, the scores + pv launches at head_dim 64 / 128 / 256, and the
combine-and-quantise launch -- through mi_op_attention_decode and mi_op_attention_short, which run
the engine's own launchers.

f32 output: against ggml_ref.attention_head per head (test_gpu_ops._attn_ref), within
test_attention_matches_oracle's two bounds (its docstring derives them): max error <= 2^-10 max|V|,
mean error <= 1e-5.  Quantised output: the kernels quantise the very floats they store, so
ggml_ref.quantize_q8_K / quantize_q8_0 of the f32 row THE SAME CALL returned must give the same bytes:
quants, sums and scales bit-identical (a batch's 32-element sums: pair sums of the 16-element ones).

The unmarked tests at the end need no GPU: they apply the faults these kernels could have to a
reference result and check that the compare functions used above reject each."""
import functools

import numpy as np
import pytest

import ggml_ref as R
from blama_amd import engine
from test_gpu_ops import _attn_ref

gpu = pytest.mark.gpu

DQ, DF, DS, BQ, BF = (engine.ATTN_DECODE_QUANT, engine.ATTN_DECODE_FUSED, engine.ATTN_DECODE_SPLIT,
                      engine.ATTN_BATCH_QUANT, engine.ATTN_BATCH_FUSED)
DEC, FUSED, SPV = engine.AK_DEC, engine.AK_FUSED, engine.AK_SCORES_PV
Q8K, Q80 = engine.ATTN_FMT_Q8K, engine.ATTN_FMT_Q80

# (n_head, n_head_kv, head_dim) -> the instantiation attn_plan gives it: (kernel, R, LPC, HG, NWV, qsplit)
QUANT_DEC = {(32, 32, 128): (DEC, 1, 16, 2, 8, 0), (32, 8, 128): (DEC, 1, 16, 2, 8, 4),
             (32, 4, 64): (DEC, 1, 8, 4, 4, 8), (4, 4, 64): (DEC, 1, 8, 4, 4, 0)}
QUANT_FUSED = {(32, 16, 128): (FUSED, 2, 16, 1, 4, 0), (64, 16, 64): (FUSED, 4, 8, 1, 4, 0),
               (16, 16, 256): (FUSED, 1, 32, 1, 4, 0)}
QUANT = {**QUANT_DEC, **QUANT_FUSED}
BATCH_FUSED = {(32, 16, 64): (FUSED, 2, 8, 1, 4, 0), (32, 8, 128): (FUSED, 4, 16, 1, 4, 0),
               (32, 4, 64): (FUSED, 8, 8, 1, 4, 0)}
SPLIT = {(32, 32, 128): (SPV, 1, 16, 1, 4, 0), (32, 8, 128): (SPV, 1, 16, 1, 4, 4), (32, 4, 64): (SPV, 1, 8, 1, 4, 8),
         (64, 16, 128): (SPV, 4, 16, 1, 4, 0), (16, 16, 256): (SPV, 1, 32, 1, 4, 0)}
# a decode step's non-quantising launch with R > 1 (mi_op_attention reaches R = 1 alone)
DECODE_FUSED = {(64, 16, 128): (FUSED, 4, 16, 1, 4, 0), (32, 16, 64): (FUSED, 2, 8, 1, 4, 0)}

DECODE_CELLS = [1, 2, 37, 128, 129, 512]   # 128 | 129: the decode kernel's prefetched steps end; 1, 2: under a wave step
SPLIT_CELLS = [513, 1100, 2048]            # 9, 9 and 16 splits
NTOKS = [1, 20, 33, 64]                    # 33: past one 32-token tile of the batch activation
STARTS = [0, 100]                          # a batch from cell 0, and appended to 100 cells of context
PAST = 70                                  # rows allocated past the count (within the fused kernel's entry prefetch)

gid = lambda g: "%d-%d-%d" % g
bits = lambda a: np.ascontiguousarray(a).view(np.uint32)


def inputs(geom, n_ctx, ntok=0, seed=0):
    """q (n_head, hd) [ntok > 0: (ntok, n_head, hd)], k16, v16 (n_ctx, n_head_kv * hd): every head its own."""
    n_head, n_head_kv, hd = geom
    rng = np.random.default_rng(n_ctx * 7 + hd + n_head_kv + 1000 * ntok + seed)
    q = (rng.standard_normal((ntok, n_head, hd) if ntok else (n_head, hd)) * 0.6).astype(np.float32)
    k16 = (rng.standard_normal((n_ctx, n_head_kv * hd)) * 0.6).astype(np.float16)
    v16 = rng.standard_normal((n_ctx, n_head_kv * hd)).astype(np.float16)
    return q, k16, v16


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def decode_case(geom, ncell):
    """A decode step over ncell cells in order, and its reference (computed once, read-only)."""
    q, k16, v16 = inputs(geom, ncell)
    ref = _attn_ref(q, k16, v16, geom[1], np.arange(ncell), ncell - 1).reshape(-1)
    return frozen(q, k16, v16, ref)


def batch_ref(geom, q, k16, v16, cell_pos, tok_cell, tok_pos):
    return np.stack([_attn_ref(q[t], k16[:c + 1], v16[:c + 1], geom[1], cell_pos[:c + 1], int(p)).reshape(-1)
                     for t, (c, p) in enumerate(zip(tok_cell, tok_pos))])


@functools.lru_cache(maxsize=None)
def batch_case(geom, ntok, start):
    """ntok tokens in cells start .. start + ntok - 1, positions to match: token t sees start + t + 1 cells."""
    n = start + ntok
    q, k16, v16 = inputs(geom, n, ntok)
    tc = np.arange(start, n, dtype=np.int32)
    ref = batch_ref(geom, q, k16, v16, np.arange(n), tc, tc)
    return frozen(q, k16, v16, tc, ref)


# ---- the compare functions ----
def check_f32(got, ref, v16):
    """test_attention_matches_oracle's bounds for one attention output (all heads of one token)."""
    err = np.abs(np.asarray(got, np.float32).reshape(-1) - np.asarray(ref, np.float32).reshape(-1))
    assert err.max() <= 2.0 ** -10 * np.abs(np.asarray(v16, np.float32)).max(), float(err.max())
    assert err.mean() <= 1e-5, float(err.mean())


def check_f32_rows(got, ref, v16):
    assert got.shape == ref.shape
    for t in range(ref.shape[0]):
        check_f32(got[t], ref[t], v16)


def check_q8k(row, q, sums, d, per=16):
    """Q8_K of `row` by quantize_row_q8_K_ref's rules, bit for bit; sums over `per` elements."""
    ref = R.quantize_q8_K(row)
    nb = ref.qs.shape[0]
    assert np.array_equal(np.asarray(q).reshape(nb, 256).astype(np.int32), ref.qs)
    assert np.array_equal(np.asarray(sums).reshape(nb, 256 // per), ref.bsums.reshape(nb, 256 // per, per // 16).sum(axis=2))
    assert np.array_equal(bits(d).reshape(-1), bits(ref.d))


def check_q80(row, q, d):
    """Q8_0 of `row` by quantize_row_q8_0's rules (d = f16(amax / 127)), bit for bit."""
    ref = R.quantize_q8_0(row)
    assert np.array_equal(np.asarray(q).reshape(-1, 32).astype(np.int32), ref.qs)
    assert np.array_equal(bits(d).reshape(-1), bits(ref.d))


def check_act(r, fmt):
    """The activation a decode call published against the f32 row the same call returned."""
    if fmt & Q8K:
        check_q8k(r["out"], r["q8k"], r["bsums"], r["dk"])
    if fmt & Q80:
        check_q80(r["out"], r["q80"], r["d0"])


def check_rows(r, quant):
    """A short batch's quantised rows, token by token, against the f32 rows of the same call."""
    for t in range(r["out"].shape[0]):
        if quant == 1:
            check_q8k(r["out"][t], r["q"][t], r["bsums"][t], r["d"][t], per=32)
        else:
            check_q80(r["out"][t], r["q"][t], r["d"][t])


ACT_KEYS = {Q8K: ("q8k", "bsums", "dk"), Q80: ("q80", "d0")}


def same_bytes(a, b, keys):
    for k in keys:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k


def act_keys(fmt):
    return sum((ACT_KEYS[f] for f in (Q8K, Q80) if fmt & f), ())


def plan_of(mode, geom, n_ctx=512, ntok=1):
    p = engine.op_attn_plan(mode, *geom, n_ctx=n_ctx, ntok=ntok)
    return tuple(p[f] for f in ("kernel", "R", "LPC", "HG", "NWV", "qsplit"))


def test_cases_reach_the_instantiations_they_name():
    """What attn_plan gives the geometries of this file (no GPU): the table in the summary of the
    kernels reached rests on this, not on assumption."""
    for mode, table in ((DQ, QUANT), (BQ, QUANT), (BF, BATCH_FUSED), (DS, SPLIT), (DF, DECODE_FUSED)):
        for geom, want in table.items():
            assert plan_of(mode, geom, n_ctx=2048, ntok=20 if mode in (BQ, BF) else 1) == want, (mode, geom)
    reached = set(QUANT.values()) | set(BATCH_FUSED.values()) | set(SPLIT.values()) | set(DECODE_FUSED.values())
    assert {(k, r, lpc) for k, r, lpc, _, _, _ in reached} == {
        (DEC, 1, 16), (DEC, 1, 8),
        (FUSED, 2, 16), (FUSED, 4, 8), (FUSED, 1, 32), (FUSED, 2, 8), (FUSED, 4, 16), (FUSED, 8, 8),
        (SPV, 1, 16), (SPV, 1, 8), (SPV, 4, 16), (SPV, 1, 32)}


# ---- a decode step within 512 cells, the output also quantised ----
@gpu
@pytest.mark.parametrize("ncell", DECODE_CELLS)
@pytest.mark.parametrize("geom", list(QUANT), ids=gid)
def test_decode_quant_matches_oracle(gpu_lib, geom, ncell):
    q, k16, v16, ref = decode_case(geom, ncell)
    r = engine.op_attention_decode(DQ, q, k16, v16, geom[1], ncell - 1, fmt=Q8K | Q80)
    assert r["kernel"] == QUANT[geom][0]
    check_f32(r["out"], ref, v16)
    check_act(r, Q8K | Q80)


@gpu
@pytest.mark.parametrize("ncell", [37, 129])
@pytest.mark.parametrize("geom", list(QUANT), ids=gid)
def test_decode_quant_formats_and_no_f32_row(gpu_lib, geom, ncell):
    """Both formats in one launch equal each format's own launch; and without the f32 row (the
    decode kernel's production path: out_f32 unset) the published bytes are the same."""
    q, k16, v16, _ = decode_case(geom, ncell)
    both = engine.op_attention_decode(DQ, q, k16, v16, geom[1], ncell - 1, fmt=Q8K | Q80)
    for fmt in (Q8K, Q80):
        one = engine.op_attention_decode(DQ, q, k16, v16, geom[1], ncell - 1, fmt=fmt)
        assert np.array_equal(bits(one["out"]), bits(both["out"]))
        same_bytes(one, both, act_keys(fmt))
    for fmt in (Q8K, Q80, Q8K | Q80):
        bare = engine.op_attention_decode(DQ, q, k16, v16, geom[1], ncell - 1, fmt=fmt, want_f32=False)
        assert bare["out"] is None
        same_bytes(bare, both, act_keys(fmt))


@gpu
@pytest.mark.parametrize("ncell", [37, 512])
@pytest.mark.parametrize("geom", list(DECODE_FUSED), ids=gid)
def test_decode_fused_gqa_matches_oracle(gpu_lib, geom, ncell):
    q, k16, v16, ref = decode_case(geom, ncell)
    r = engine.op_attention_decode(DF, q, k16, v16, geom[1], ncell - 1)
    assert r["kernel"] == FUSED
    check_f32(r["out"], ref, v16)


# ---- a decode step past 512 cells: scores + pv, then the two combine launches ----
@gpu
@pytest.mark.parametrize("ncell", SPLIT_CELLS)
@pytest.mark.parametrize("geom", list(SPLIT), ids=gid)
def test_decode_split_matches_oracle(gpu_lib, geom, ncell):
    q, k16, v16, ref = decode_case(geom, ncell)
    r = engine.op_attention_decode(DS, q, k16, v16, geom[1], ncell - 1, fmt=Q8K | Q80)
    assert r["kernel"] == SPV
    check_f32(r["out"], ref, v16)
    check_act(r, Q8K | Q80)
    for fmt in (Q8K, Q80):
        one = engine.op_attention_decode(DS, q, k16, v16, geom[1], ncell - 1, fmt=fmt)
        assert np.array_equal(bits(one["out"]), bits(r["out"]))
        same_bytes(one, r, act_keys(fmt))


# ---- short batches ----
@gpu
@pytest.mark.parametrize("start", STARTS)
@pytest.mark.parametrize("ntok", NTOKS)
@pytest.mark.parametrize("geom", list(QUANT), ids=gid)
def test_short_batch_quant_matches_oracle(gpu_lib, geom, ntok, start):
    q, k16, v16, tc, ref = batch_case(geom, ntok, start)
    rows = None
    for quant in (1, 2):
        r = engine.op_attention_short(q, k16, v16, geom[1], tc, quant=quant)
        assert r["kernel"] == QUANT[geom][0]
        check_f32_rows(r["out"], ref, v16)
        check_rows(r, quant)
        if rows is not None:   # the f32 rows do not depend on the format
            assert np.array_equal(bits(rows), bits(r["out"]))
        rows = r["out"]


@gpu
@pytest.mark.parametrize("start", STARTS)
@pytest.mark.parametrize("ntok", NTOKS)
@pytest.mark.parametrize("geom", list(BATCH_FUSED), ids=gid)
def test_short_batch_fused_matches_oracle(gpu_lib, geom, ntok, start):
    q, k16, v16, tc, ref = batch_case(geom, ntok, start)
    r = engine.op_attention_short(q, k16, v16, geom[1], tc)
    assert r["kernel"] == FUSED
    check_f32_rows(r["out"], ref, v16)


# ---- masking by cell position ----
def shuffled(n, seed):
    """Positions shuffled over the cells (a Self-Extend / seq_add shuffle); the last cell is the query's."""
    cp = np.random.default_rng(seed).permutation(n).astype(np.int32)
    return cp, int(cp[-1])


@gpu
@pytest.mark.parametrize("mode,geom,ncell", [(DQ, (32, 8, 128), 300), (DQ, (32, 4, 64), 300), (DQ, (32, 16, 128), 300),
                                             (DQ, (64, 16, 64), 300), (DQ, (16, 16, 256), 300),
                                             (DS, (32, 8, 128), 700), (DS, (64, 16, 128), 700), (DS, (32, 4, 64), 700)],
                         ids=lambda v: gid(v) if isinstance(v, tuple) else str(v))
def test_decode_masks_future_positions(gpu_lib, mode, geom, ncell):
    q, k16, v16 = inputs(geom, ncell, seed=5)
    cp, pos = shuffled(ncell, 5)
    assert 0 < pos < ncell - 1   # some cells masked, some not
    r = engine.op_attention_decode(mode, q, k16, v16, geom[1], ncell - 1, cell_pos=cp, pos=pos, fmt=Q8K | Q80)
    check_f32(r["out"], _attn_ref(q, k16, v16, geom[1], cp, pos), v16)
    check_act(r, Q8K | Q80)


@gpu
@pytest.mark.parametrize("geom,quant", [((32, 8, 128), 1), ((32, 4, 64), 2), ((32, 16, 128), 1), ((64, 16, 64), 2),
                                        ((32, 8, 128), 0), ((32, 4, 64), 0)],
                         ids=lambda v: gid(v) if isinstance(v, tuple) else str(v))
def test_short_batch_masks_future_positions(gpu_lib, geom, quant):
    """20 tokens appended to 100 cells whose positions are shuffled: every token its own mask."""
    start, ntok = 100, 20
    q, k16, v16 = inputs(geom, start + ntok, ntok, seed=6)
    cp = np.r_[np.random.default_rng(6).permutation(start) * 2, 200 + np.arange(ntok)].astype(np.int32)
    tc = np.arange(start, start + ntok, dtype=np.int32)
    tpos = np.r_[np.arange(30, 30 + 7 * (ntok - 1), 7), 300].astype(np.int32)   # most tokens before some context cells
    cp[tc] = tpos
    r = engine.op_attention_short(q, k16, v16, geom[1], tc, tok_pos=tpos, cell_pos=cp, quant=quant)
    check_f32_rows(r["out"], batch_ref(geom, q, k16, v16, cp, tc, tpos), v16)
    if quant:
        check_rows(r, quant)


# ---- cells past the count ----
def garbage_past(k16, v16, cp, first):
    """Rows from `first` on: f16 NaN, infinities and the largest finite value; positions that would be
    visible if read, and wild ones."""
    k, v, c = k16.copy(), v16.copy(), cp.copy()
    pat = np.array([0x7E00, 0x7C00, 0xFC00, 0x7BFF, 0xFE01], np.uint16).view(np.float16)
    n = k.shape[0] - first
    k[first:] = pat[(np.arange(n)[:, None] + np.arange(k.shape[1])[None, :]) % 5]
    v[first:] = pat[(np.arange(n)[:, None] + 2 * np.arange(k.shape[1])[None, :]) % 5]
    c[first:] = np.array([0, -1, 1 << 30, 3, -(1 << 31)], np.int64)[np.arange(n) % 5].astype(np.int32)
    return k, v, c


@gpu
@pytest.mark.parametrize("mode,geom,ncell", [(DQ, g, n) for g in QUANT for n in (1, 37, 129)] +
                         [(DS, g, 1100) for g in SPLIT] + [(DF, g, 37) for g in DECODE_FUSED],
                         ids=lambda v: gid(v) if isinstance(v, tuple) else str(v))
def test_decode_ignores_cells_past_the_count(gpu_lib, mode, geom, ncell):
    """The cache has more rows than the context has cells: what those rows hold (NaN bits, garbage
    positions) does not reach the output, bit for bit, and the output is the oracle's."""
    q, k16, v16, ref = decode_case(geom, ncell)
    fmt = 0 if mode == DF else Q8K | Q80
    pad = np.zeros((PAST, k16.shape[1]), np.float16)
    kz, vz, cz = np.vstack([k16, pad]), np.vstack([v16, pad]), np.r_[np.arange(ncell), np.zeros(PAST)].astype(np.int32)
    kg, vg, cg = garbage_past(kz, vz, cz, ncell)
    zero = engine.op_attention_decode(mode, q, kz, vz, geom[1], ncell - 1, cell_pos=cz, fmt=fmt)
    junk = engine.op_attention_decode(mode, q, kg, vg, geom[1], ncell - 1, cell_pos=cg, fmt=fmt)
    check_f32(zero["out"], ref, v16)
    same_bytes(junk, zero, ("out",) + act_keys(fmt))


@gpu
@pytest.mark.parametrize("geom,quant", [(g, 1) for g in QUANT] + [((32, 8, 128), 2), ((32, 16, 128), 2)] +
                         [(g, 0) for g in BATCH_FUSED], ids=lambda v: gid(v) if isinstance(v, tuple) else str(v))
def test_short_batch_ignores_cells_past_the_count(gpu_lib, geom, quant):
    q, k16, v16, tc, ref = batch_case(geom, 20, 100)
    n = k16.shape[0]
    pad = np.zeros((PAST, k16.shape[1]), np.float16)
    kz, vz, cz = np.vstack([k16, pad]), np.vstack([v16, pad]), np.r_[np.arange(n), np.zeros(PAST)].astype(np.int32)
    kg, vg, cg = garbage_past(kz, vz, cz, n)
    zero = engine.op_attention_short(q, kz, vz, geom[1], tc, cell_pos=cz, quant=quant)
    junk = engine.op_attention_short(q, kg, vg, geom[1], tc, cell_pos=cg, quant=quant)
    check_f32_rows(zero["out"], ref, v16)
    same_bytes(junk, zero, ("out",) + (() if not quant else ("q", "d", "bsums") if quant == 1 else ("q", "d")))


# ---- an all-zero block ----
def zero_block_v(geom, v16, block):
    """V zero for the kv heads that feed the q heads of output block `block`; the blocks that become zero."""
    n_head, n_head_kv, hd = geom
    r = n_head // n_head_kv
    nb = n_head * hd // 256
    block = min(block, nb - 1)   # (4, 4, 64) is a single block
    heads = range(256 * block // hd, (256 * block + 255) // hd + 1)
    v = v16.copy().reshape(v16.shape[0], n_head_kv, hd)
    kv = sorted({h // r for h in heads})
    v[:, kv] = 0
    zeroed = [b for b in range(nb) if all((h // r) in kv for h in range(256 * b // hd, (256 * b + 255) // hd + 1))]
    assert block in zeroed and (len(zeroed) < nb or nb == 1)
    return v.reshape(v16.shape), zeroed


@gpu
@pytest.mark.parametrize("mode,geom,ncell", [(DQ, g, 129) for g in QUANT] + [(DS, g, 1100) for g in SPLIT],
                         ids=lambda v: gid(v) if isinstance(v, tuple) else str(v))
def test_decode_zero_block(gpu_lib, mode, geom, ncell):
    """A 256-block of exact zeros: d = 0, every quant 0, every sum 0, on both formats; the rest as ever."""
    q, k16, v16, _ = decode_case(geom, ncell)
    vz, zeroed = zero_block_v(geom, v16, 1)
    r = engine.op_attention_decode(mode, q, k16, vz, geom[1], ncell - 1, fmt=Q8K | Q80)
    check_f32(r["out"], _attn_ref(q, k16, vz, geom[1], np.arange(ncell), ncell - 1), vz)
    check_act(r, Q8K | Q80)
    for b in zeroed:
        assert not r["out"].reshape(-1, 256)[b].any()
        assert not r["q8k"][b].any() and not r["bsums"][b].any() and bits(r["dk"])[b] == 0
        assert not r["q80"].reshape(-1, 256)[b].any() and not bits(r["d0"]).reshape(-1, 8)[b].any()
    assert r["q8k"].any(axis=1).sum() == r["q8k"].shape[0] - len(zeroed)


@gpu
@pytest.mark.parametrize("geom", list(QUANT), ids=gid)
def test_short_batch_zero_block(gpu_lib, geom):
    q, k16, v16, tc, _ = batch_case(geom, 33, 100)
    vz, zeroed = zero_block_v(geom, v16, 1)
    ref = batch_ref(geom, q, k16, vz, np.arange(k16.shape[0]), tc, tc)
    for quant in (1, 2):
        r = engine.op_attention_short(q, k16, vz, geom[1], tc, quant=quant)
        check_f32_rows(r["out"], ref, vz)
        check_rows(r, quant)
        nt = len(tc)
        for b in zeroed:
            assert not r["out"].reshape(nt, -1, 256)[:, b].any()
            assert not r["q"].reshape(nt, -1, 256)[:, b].any()
            if quant == 1:
                assert not r["bsums"][:, b].any() and not bits(r["d"])[:, b].any()
            else:
                assert not bits(r["d"]).reshape(nt, -1, 8)[:, b].any()


# ---- determinism: one case per kernel ----
@gpu
@pytest.mark.parametrize("mode,geom,ncell", [(DQ, (32, 32, 128), 300), (DQ, (32, 4, 64), 300), (DQ, (64, 16, 64), 300),
                                             (DS, (32, 8, 128), 1100), (DS, (64, 16, 128), 1100)],
                         ids=lambda v: gid(v) if isinstance(v, tuple) else str(v))
def test_decode_deterministic(gpu_lib, mode, geom, ncell):
    q, k16, v16 = inputs(geom, ncell, seed=9)
    a = engine.op_attention_decode(mode, q, k16, v16, geom[1], ncell - 1, fmt=Q8K | Q80)
    b = engine.op_attention_decode(mode, q, k16, v16, geom[1], ncell - 1, fmt=Q8K | Q80)
    same_bytes(a, b, ("out",) + act_keys(Q8K | Q80))


@gpu
@pytest.mark.parametrize("geom,quant", [((32, 8, 128), 1), ((32, 4, 64), 2), ((32, 16, 128), 1), ((32, 8, 128), 0)],
                         ids=lambda v: gid(v) if isinstance(v, tuple) else str(v))
def test_short_batch_deterministic(gpu_lib, geom, quant):
    q, k16, v16, tc, _ = batch_case(geom, 33, 100)
    a = engine.op_attention_short(q, k16, v16, geom[1], tc, quant=quant)
    b = engine.op_attention_short(q, k16, v16, geom[1], tc, quant=quant)
    same_bytes(a, b, ("out",) + (() if not quant else ("q", "d", "bsums") if quant == 1 else ("q", "d")))


# ---- refusals: an error to the caller before the device is touched (so: no GPU needed, nothing launched) ----
def test_refusals():
    from test_attn_plan import UNSERVED
    no_plan = "no kernel serves this head geometry"
    for geom in [(6, 6, 64), (32, 16, 64), (32, 8, 32)]:   # served, but not by a quantising kernel
        q, k16, v16 = inputs(geom, 40)
        with pytest.raises(engine.EngineError, match=no_plan):
            engine.op_attention_decode(DQ, q, k16, v16, geom[1], 39, fmt=Q8K)
        qb = np.stack([q, q])
        for quant in (1, 2):
            with pytest.raises(engine.EngineError, match=no_plan):
                engine.op_attention_short(qb, k16, v16, geom[1], [38, 39], quant=quant)
    for geom in UNSERVED:
        if geom[1] <= 0 or geom[0] % geom[1]:
            continue   # not a shape the arrays can take: refused as a bad shape (below)
        q, k16, v16 = inputs(geom, 600)
        for mode, cell, fmt in ((DQ, 39, Q8K), (DF, 39, 0), (DS, 599, 0)):
            with pytest.raises(engine.EngineError, match=no_plan):
                engine.op_attention_decode(mode, q, k16, v16, geom[1], cell, fmt=fmt)
        for quant in (0, 1):
            with pytest.raises(engine.EngineError, match=no_plan):
                engine.op_attention_short(np.stack([q, q]), k16, v16, geom[1], [38, 39], quant=quant)
    geom = (32, 8, 128)
    q, k16, v16 = inputs(geom, 600)
    for ntok in (0, 65):
        with pytest.raises(engine.EngineError, match="1..64 tokens"):
            engine.op_attention_short(np.zeros((ntok, 32, 128), np.float32), k16, v16, 8, np.arange(ntok), quant=1)
    for cells in ([511, 512], [512], [599]):
        with pytest.raises(engine.EngineError, match="token cell out of range"):
            engine.op_attention_short(np.stack([q] * len(cells)), k16, v16, 8, cells, quant=1)
    with pytest.raises(engine.EngineError, match="must ascend"):
        engine.op_attention_short(np.stack([q, q]), k16, v16, 8, [7, 7])
    # a mode on the wrong side of 512 cells, a format the mode does not take, a cell outside the cache
    for mode, cell, fmt, what in ((DQ, 512, Q8K, "512 cells"), (DF, 599, 0, "512 cells"), (DS, 511, Q8K, "512 cells"),
                                  (DQ, 39, 0, "fmt"), (DF, 39, Q8K, "fmt"), (DQ, 39, 4, "fmt"), (DS, 600, 0, "outside the cache"),
                                  (DQ, -1, Q8K, "outside the cache"), (BQ, 39, Q8K, "mode")):
        with pytest.raises(engine.EngineError, match=what):
            engine.op_attention_decode(mode, q, k16, v16, 8, cell, fmt=fmt)
    with pytest.raises(engine.EngineError, match="bad shape"):
        engine.op_attention_decode(DQ, np.zeros((10, 64), np.float32), np.zeros((40, 256), np.float16),
                                   np.zeros((40, 256), np.float16), 4, 39, fmt=Q8K)


# ---- no GPU: the faults these kernels could have are rejected by the compare functions above ----
GUARD_DECODE = [((32, 8, 128), 129), ((32, 4, 64), 37), ((64, 16, 64), 512), ((16, 16, 256), 2), ((32, 32, 128), 2048),
                ((64, 16, 128), 513)]
GUARD_BATCH = [((32, 8, 128), 33, 100), ((32, 4, 64), 20, 0), ((32, 16, 128), 33, 0)]


def rejects(check, *args, **kw):
    with pytest.raises(AssertionError):
        check(*args, **kw)


@pytest.mark.parametrize("geom,ncell", GUARD_DECODE, ids=lambda v: gid(v) if isinstance(v, tuple) else str(v))
def test_decode_faults_would_be_detected(geom, ncell):
    q, k16, v16, ref = decode_case(geom, ncell)
    n_head, n_head_kv, hd = geom
    check_f32(ref, ref, v16)
    k8, k0 = R.quantize_q8_K(ref), R.quantize_q8_0(ref)
    check_q8k(ref, k8.qs, k8.bsums, k8.d)
    check_q80(ref, k0.qs, k0.d)
    # two 256-blocks swapped: in the f32 row, and in the published activation alone
    sw = np.arange(n_head * hd // 256)
    sw[[0, 1]] = [1, 0]
    rejects(check_f32, ref.reshape(-1, 256)[sw], ref, v16)
    rejects(check_q8k, ref, k8.qs[sw], k8.bsums[sw], k8.d[sw])
    rejects(check_q8k, ref, k8.qs[sw], k8.bsums, k8.d)
    rejects(check_q8k, ref, k8.qs, k8.bsums[sw], k8.d)
    rejects(check_q8k, ref, k8.qs, k8.bsums, k8.d[sw])
    rejects(check_q80, ref, k0.qs.reshape(-1, 256)[sw], k0.d.reshape(-1, 8)[sw])
    rejects(check_q80, ref, k0.qs, k0.d.reshape(-1, 8)[sw])
    # the q heads of one kv group permuted (a workgroup per q head under qsplit)
    r = n_head // n_head_kv
    if r > 1:
        perm = np.arange(n_head)
        perm[r:2 * r] = np.roll(perm[r:2 * r], 1)
        rejects(check_f32, ref.reshape(n_head, hd)[perm], ref, v16)
    # a q head served with its neighbour's kv head
    grp = np.minimum(np.arange(n_head) // r + 1, n_head_kv - 1)
    wrong = np.stack([R.attention_head(q[h], k16.reshape(ncell, n_head_kv, hd)[:, grp[h]],
                                       v16.reshape(ncell, n_head_kv, hd)[:, grp[h]], np.float32(1.0 / np.sqrt(np.float32(hd))))
                      for h in range(n_head)])
    rejects(check_f32, wrong, ref, v16)
    # one cell too many, one too few
    if ncell > 1:
        rejects(check_f32, _attn_ref(q, k16[:-1], v16[:-1], n_head_kv, np.arange(ncell - 1), ncell - 2), ref, v16)
    q2, k2, v2 = inputs(geom, ncell + 1, seed=77)
    k2[:ncell], v2[:ncell] = k16, v16
    rejects(check_f32, _attn_ref(q, k2, v2, n_head_kv, np.arange(ncell + 1), ncell), ref, v16)


@pytest.mark.parametrize("geom,ntok,start", GUARD_BATCH, ids=lambda v: gid(v) if isinstance(v, tuple) else str(v))
def test_batch_faults_would_be_detected(geom, ntok, start):
    q, k16, v16, tc, ref = batch_case(geom, ntok, start)
    nb = ref.shape[1] // 256
    check_f32_rows(ref, ref, v16)
    qk = [R.quantize_q8_K(row) for row in ref]
    good = {"out": np.array(ref), "q": np.stack([x.qs.reshape(-1) for x in qk]).astype(np.int8),
            "d": np.stack([x.d for x in qk]), "bsums": np.stack([x.bsums.reshape(nb, 8, 2).sum(axis=2) for x in qk])}
    q0 = [R.quantize_q8_0(row) for row in ref]
    good0 = {"out": np.array(ref), "q": np.stack([x.qs.reshape(-1) for x in q0]).astype(np.int8),
             "d": np.stack([x.d for x in q0])}
    check_rows(good, 1)
    check_rows(good0, 2)
    # a token row written to its neighbour in the 32-token tile
    nbr = np.arange(ntok)
    nbr[[5, 6]] = [6, 5]
    rejects(check_f32_rows, ref[nbr], ref, v16)
    for key in ("q", "d", "bsums"):
        rejects(check_rows, {**good, key: good[key][nbr]}, 1)
    for key in ("q", "d"):
        rejects(check_rows, {**good0, key: good0[key][nbr]}, 2)
    # two 256-blocks of every row swapped
    sw = np.arange(nb)
    sw[[0, 1]] = [1, 0]
    rejects(check_f32_rows, ref.reshape(ntok, nb, 256)[:, sw].reshape(ntok, -1), ref, v16)
    rejects(check_rows, {**good, "q": good["q"].reshape(ntok, nb, 256)[:, sw].reshape(ntok, -1)}, 1)
    rejects(check_rows, {**good, "bsums": good["bsums"][:, sw]}, 1)
    rejects(check_rows, {**good, "d": good["d"][:, sw]}, 1)
    rejects(check_rows, {**good0, "d": good0["d"].reshape(ntok, nb, 8)[:, sw].reshape(ntok, -1)}, 2)
    # a 32-element sum taken over the wrong half: 16-element sums 2 j + 1 and 2 j + 2
    s16 = np.stack([x.bsums for x in qk])                                  # (ntok, nb, 16)
    shifted = np.roll(s16, -1, axis=2).reshape(ntok, nb, 8, 2).sum(axis=3)
    rejects(check_rows, {**good, "bsums": shifted}, 1)
    rejects(check_rows, {**good, "bsums": s16[:, :, 0::2] * 2}, 1)        # the first half twice
    # every token with one cell too many (its successor's count), and with its predecessor's query
    more = batch_ref(geom, q, np.vstack([k16, k16[:1]]), np.vstack([v16, v16[:1]]), np.arange(len(k16) + 1), tc + 1, tc + 1)
    rejects(check_f32_rows, more, ref, v16)
    for t in range(ntok):
        rejects(check_f32, more[t], ref[t], v16)
    if ntok > 1:
        rejects(check_f32_rows, batch_ref(geom, np.roll(q, 1, axis=0), k16, v16, np.arange(len(k16)), tc, tc), ref, v16)
    # the q heads of one kv group permuted
    n_head, n_head_kv, hd = geom
    r = n_head // n_head_kv
    perm = np.arange(n_head)
    perm[r:2 * r] = np.roll(perm[r:2 * r], 1)
    rejects(check_f32_rows, ref.reshape(ntok, n_head, hd)[:, perm].reshape(ntok, -1), ref, v16)
