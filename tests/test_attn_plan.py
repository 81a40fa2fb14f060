"""attn_plan (attn.hip), through mi_op_attn_plan: which cache-attention kernel a launch runs, with
which template arguments, grid, block, LDS size and qsplit, for every mode and head geometry the
launchers meet.  A pure host function: no GPU.

The expected plans are the choices the launchers made before the plan existed, written out as
literals; QUANT_SUPPORTED is what attn_quant_supported returned then, recorded once from that
library over the sweep of test_quant_supported_as_recorded."""
import pytest

from blama_amd import engine

DQ, DF, DS, BQ, BF = range(5)          # AttnMode
NONE, DEC, FUSED, LONG, SPV = range(5)  # AttnKernel
S = 16                                  # ATTN_SMAX
N_CTX = 4096                            # the long kernel's LDS: max(64, roundup64(ceil(n_ctx / S))) * 4
LDS = 1024


def plan(mode, geom, n_ctx=N_CTX, ntok=1, long_ok=False):
    p = engine.op_attn_plan(mode, *geom, n_ctx=n_ctx, ntok=ntok, long_ok=long_ok)
    return tuple(p[f] for f in engine.ATTN_PLAN_FIELDS)


# (n_head, n_head_kv, head_dim) -> the plans of a decode step: quantising, fused, past 512 cells
# in two launches, past 512 cells with the single launch allowed; then R, LPC, grid_x of a short
# batch's non-quantising launch.
# A plan: (kernel, R, LPC, HG, NWV, grid_x, grid_y, block, lds, qsplit)
TABLE = {
    (32, 32, 128): ((DEC, 1, 16, 2, 8, 16, 1, 1024, 0, 0), (FUSED, 1, 16, 1, 4, 32, 1, 256, 0, 0),
                    (SPV, 1, 16, 1, 4, 32, S, 256, 0, 0), (LONG, 1, 16, 1, 4, 32, S, 256, LDS, 0), (1, 16, 32)),
    (32, 8, 128): ((DEC, 1, 16, 2, 8, 16, 1, 1024, 0, 4), (FUSED, 1, 16, 1, 4, 32, 1, 256, 0, 4),
                   (SPV, 1, 16, 1, 4, 32, S, 256, 0, 4), (LONG, 1, 16, 1, 4, 32, S, 256, LDS, 0), (4, 16, 8)),
    (32, 4, 64): ((DEC, 1, 8, 4, 4, 8, 1, 1024, 0, 8), (FUSED, 1, 8, 1, 4, 32, 1, 256, 0, 8),
                  (SPV, 1, 8, 1, 4, 32, S, 256, 0, 8), (LONG, 1, 8, 1, 4, 32, S, 256, LDS, 0), (8, 8, 4)),
    (64, 16, 128): ((FUSED, 4, 16, 1, 4, 16, 1, 256, 0, 0), (FUSED, 4, 16, 1, 4, 16, 1, 256, 0, 0),
                    (SPV, 4, 16, 1, 4, 16, S, 256, 0, 0), (LONG, 1, 16, 1, 4, 64, S, 256, LDS, 0), (4, 16, 16)),
    (4, 4, 64): ((DEC, 1, 8, 4, 4, 1, 1, 1024, 0, 0), (FUSED, 1, 8, 1, 4, 4, 1, 256, 0, 0),
                 (SPV, 1, 8, 1, 4, 4, S, 256, 0, 0), (LONG, 1, 8, 1, 4, 4, S, 256, LDS, 0), (1, 8, 4)),
    (12, 12, 64): ((DEC, 1, 8, 4, 4, 3, 1, 1024, 0, 0), (FUSED, 1, 8, 1, 4, 12, 1, 256, 0, 0),
                   (SPV, 1, 8, 1, 4, 12, S, 256, 0, 0), (LONG, 1, 8, 1, 4, 12, S, 256, LDS, 0), (1, 8, 12)),
    # head_dim 256: no decode kernel and no long kernel
    (16, 16, 256): ((FUSED, 1, 32, 1, 4, 16, 1, 256, 0, 0), (FUSED, 1, 32, 1, 4, 16, 1, 256, 0, 0),
                    (SPV, 1, 32, 1, 4, 16, S, 256, 0, 0), (SPV, 1, 32, 1, 4, 16, S, 256, 0, 0), (1, 32, 16)),
    # no quantising kernel: 6 heads are not whole groups of 4; 2 x 64 is half a 256-block; head_dim 32
    (6, 6, 64): (None, (FUSED, 1, 8, 1, 4, 6, 1, 256, 0, 0),
                 (SPV, 1, 8, 1, 4, 6, S, 256, 0, 0), (LONG, 1, 8, 1, 4, 6, S, 256, LDS, 0), (1, 8, 6)),
    (32, 16, 64): (None, (FUSED, 2, 8, 1, 4, 16, 1, 256, 0, 0),
                   (SPV, 2, 8, 1, 4, 16, S, 256, 0, 0), (LONG, 1, 8, 1, 4, 32, S, 256, LDS, 0), (2, 8, 16)),
    (32, 8, 32): (None, (FUSED, 1, 4, 1, 4, 32, 1, 256, 0, 4),
                  (SPV, 1, 4, 1, 4, 32, S, 256, 0, 4), (SPV, 1, 4, 1, 4, 32, S, 256, 0, 4), (4, 4, 8)),
}
# a GQA ratio outside {1, 2, 4, 8}, n_head no multiple of n_head_kv, a head_dim outside {32, 64, 128, 256}
UNSERVED = [(12, 4, 64), (32, 2, 64), (10, 4, 64), (8, 8, 96), (8, 8, 16), (8, 8, 512), (8, 0, 64)]


def check(got, want):
    if want is None:
        assert got[0] == NONE
    else:
        assert got == want


@pytest.mark.parametrize("geom", list(TABLE), ids=lambda g: "%d-%d-%d" % g)
def test_decode_plans(geom):
    dq, df, ds, dl, _ = TABLE[geom]
    check(plan(DQ, geom), dq)
    check(plan(DF, geom), df)
    check(plan(DS, geom), ds)
    check(plan(DS, geom, long_ok=True), dl)
    # long_ok matters to a step past 512 cells only
    check(plan(DQ, geom, long_ok=True), dq)
    check(plan(DF, geom, long_ok=True), df)


@pytest.mark.parametrize("geom", list(TABLE), ids=lambda g: "%d-%d-%d" % g)
@pytest.mark.parametrize("ntok", [1, 20, 64])
def test_batch_plans(geom, ntok):
    """BATCH_QUANT is the quantising decode plan with one grid row per token; BATCH_FUSED the fused
    kernel of a workgroup per kv head, never a workgroup per q head (qsplit 0)."""
    dq, _, _, _, (r, lpc, gx) = TABLE[geom]
    check(plan(BQ, geom, ntok=ntok), None if dq is None else dq[:6] + (ntok,) + dq[7:])
    check(plan(BF, geom, ntok=ntok), (FUSED, r, lpc, 1, 4, gx, ntok, 256, 0, 0))


@pytest.mark.parametrize("geom", UNSERVED, ids=lambda g: "%d-%d-%d" % g)
def test_unserved_geometry_has_no_plan(geom):
    for mode in (DQ, DF, DS, BQ, BF):
        for long_ok in (False, True):
            assert plan(mode, geom, long_ok=long_ok)[0] == NONE


def test_long_kernel_lds():
    g = (32, 32, 128)
    assert [plan(DS, g, n_ctx=n, long_ok=True)[8] for n in (512, 1024, 1040, 4096, 32768)] == [256, 256, 512, 1024, 8192]
    assert plan(DS, g, n_ctx=32768)[8] == 0


def test_bad_mode_is_an_error():
    with pytest.raises(engine.EngineError, match="bad mode"):
        engine.op_attn_plan(5, 32, 32, 128)


# attn_quant_supported(n_head, n_head_kv, head_dim) before it became the plan: the geometries it
# answered true for, of n_head in {4, 6, 8, 12, 16, 32, 64}, every n_head_kv dividing it, head_dim in
# {32, 64, 128, 256} (140 geometries)
QUANT_SUPPORTED = {
    (4, 1, 64), (4, 1, 128), (4, 2, 64), (4, 2, 128), (4, 4, 64), (4, 4, 128), (4, 4, 256),
    (6, 3, 128), (6, 6, 128), (6, 6, 256),
    (8, 1, 64), (8, 1, 128), (8, 2, 64), (8, 2, 128), (8, 4, 64), (8, 4, 128), (8, 8, 64), (8, 8, 128), (8, 8, 256),
    (12, 3, 64), (12, 3, 128), (12, 6, 64), (12, 6, 128), (12, 12, 64), (12, 12, 128), (12, 12, 256),
    (16, 2, 64), (16, 2, 128), (16, 4, 64), (16, 4, 128), (16, 8, 64), (16, 8, 128), (16, 16, 64), (16, 16, 128),
    (16, 16, 256),
    (32, 4, 64), (32, 4, 128), (32, 8, 64), (32, 8, 128), (32, 16, 128), (32, 16, 256), (32, 32, 64), (32, 32, 128),
    (32, 32, 256),
    (64, 8, 64), (64, 8, 128), (64, 16, 64), (64, 16, 128), (64, 16, 256), (64, 32, 128), (64, 32, 256), (64, 64, 64),
    (64, 64, 128), (64, 64, 256),
}


def test_quant_supported_as_recorded():
    sweep = [(nh, kv, hd) for nh in (4, 6, 8, 12, 16, 32, 64) for kv in range(1, nh + 1) if nh % kv == 0
             for hd in (32, 64, 128, 256)]
    assert len(sweep) == 140 and QUANT_SUPPORTED <= set(sweep) and len(QUANT_SUPPORTED) == 54
    for g in sweep:
        assert (plan(DQ, g)[0] != NONE) == (g in QUANT_SUPPORTED), g
