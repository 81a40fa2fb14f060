"""mmq_plan (mmq.hip, mmqs.hip), through mi_op_mmq_plan: which int8-MFMA batch GEMM kernel a launch
runs, with which template arguments, grid, block and LDS size.  A pure host function: no GPU.

The expected plans are the choices launch_mmq2, launch_mmqs and launch_mmqs_grouped made inline
before the plan existed, worked out by hand from them and written as literals (n_cu = 256):
  tiled  a row block is 2 row tiles of 32 rows (a pair: 16 gate + 16 up); the grid is
         roundup8(row blocks) x token blocks of 128 (grouped: x experts x ceil(grp_max / 128)) x
         split-K parts; one LDS stage when the grid reaches 2 * n_cu workgroups, else two; block 512;
         LDS bytes one / two stages: Q4_K 78848 / 124928, Q5_K 80896 / 129024, Q6_K 70656 / 141312,
         Q8_0 57344 / 114688
  short  K-parts of 4 superblocks; one token tile of k-quants: a wave per (row tile, K-part), no
         LDS (Q4_K / Q5_K lean, Q6_K not); else 4 row tiles per workgroup of 256, LDS 40960 (Q8_0,
         one tile), 73728 (Q8_0, two), 74752 (k-quants, two)."""
import re

import pytest

from blama_amd import engine

Q4_0, Q5_0, Q8_0, Q4_K, Q5_K, Q6_K, F16 = 2, 6, 8, 12, 13, 14, 1   # ggml type ids
NONE, TILED, SHORT, SHORT1, LEAN = range(5)                        # MmqKernel
N_CU = 256


def tiled(t, rows, npad, K, **kw):
    p = engine.op_mmq_plan(engine.MMQ_TILED, t, rows, npad, K, n_cu=N_CU, **kw)
    return p if p["kernel"] == NONE else tuple(p[f] for f in engine.MMQ_PLAN_FIELDS)


def short(t, rows, npad, K, **kw):
    p = engine.op_mmq_plan(engine.MMQ_SHORT, t, rows, npad, K, n_cu=0, **kw)
    return p if p["kernel"] == NONE else tuple(p[f] for f in engine.MMQ_PLAN_FIELDS)


# A plan: (kernel, T, pair, pre, gx, grouped, nst, nt, nrb, ntb, kp, grid_x, grid_y, grid_z, block, lds)
def T(t, nst, nrb, ntb, grid, lds, pair=0, pre=0, gx=0, grouped=0):
    return (TILED, t, pair, pre, gx, grouped, nst, 0, nrb, ntb, 0, grid, 1, 1, 512, lds)


def S(kernel, t, nt, nrt, kp, grid, block, lds, pair=0, grouped=0):
    gx, gy, gz = grid if isinstance(grid, tuple) else (grid, 1, 1)
    return (kernel, t, pair, 0, 0, grouped, 0, nt, nrt, 0, kp, gx, gy, gz, block, lds)


def test_tiled_7b_shapes():
    # W_q / W_o 4096 x 4096: 64 row blocks
    assert tiled(Q4_K, [4096], 32, 4096) == T(Q4_K, 2, 64, 1, 64, 124928)
    assert tiled(Q4_K, [4096], 128, 4096) == T(Q4_K, 2, 64, 1, 64, 124928)
    assert tiled(Q4_K, [4096], 512, 4096) == T(Q4_K, 2, 64, 4, 256, 124928)
    # gate/up pair 11008: 688 pair tiles, 344 row blocks
    assert tiled(Q4_K, [11008], 32, 4096, pair=True) == T(Q4_K, 2, 344, 1, 344, 124928, pair=1)
    assert tiled(Q4_K, [11008], 512, 4096, pair=True) == T(Q4_K, 1, 344, 4, 1376, 78848, pair=1)
    # down 4096 x 11008, plain and split over K
    assert tiled(Q4_K, [4096], 512, 11008) == T(Q4_K, 2, 64, 4, 256, 124928)
    assert tiled(Q4_K, [4096], 512, 11008, ksplit=2) == T(Q4_K, 1, 64, 4, 512, 78848)
    assert tiled(Q4_K, [4096], 128, 11008, ksplit=4) == T(Q4_K, 2, 64, 1, 256, 124928)
    assert tiled(Q4_K, [4096], 512, 11008, ksplit=4) == T(Q4_K, 1, 64, 4, 1024, 78848)
    # the output head 32000 x 4096: 500 row blocks, rounded up to 504
    assert tiled(Q6_K, [32000], 128, 4096) == T(Q6_K, 2, 500, 1, 504, 141312)
    assert tiled(Q6_K, [32000], 512, 4096) == T(Q6_K, 1, 500, 4, 2016, 70656)
    # Q / K / V as three segments of one launch
    assert tiled(Q4_K, [4096, 4096, 4096], 32, 4096) == T(Q4_K, 2, 192, 1, 192, 124928)
    assert tiled(Q4_K, [4096, 4096, 4096], 512, 4096) == T(Q4_K, 1, 192, 4, 768, 78848)
    assert tiled(Q5_K, [4096, 1024, 1024], 512, 4096) == T(Q5_K, 2, 96, 4, 384, 129024)
    assert tiled(Q8_0, [2048], 512, 2048) == T(Q8_0, 2, 32, 4, 128, 114688)


def test_tiled_stage_boundary():
    """One stage from 2 * n_cu = 512 workgroups on; 504 is the last grid below it."""
    assert tiled(Q6_K, [32000], 128, 4096) == T(Q6_K, 2, 500, 1, 504, 141312)
    assert tiled(Q4_K, [10752], 384, 256) == T(Q4_K, 2, 168, 3, 504, 124928)        # 168 row blocks x 3 token blocks
    assert tiled(Q4_K, [8192], 512, 256) == T(Q4_K, 1, 128, 4, 512, 78848)          # 128 x 4
    assert tiled(Q4_K, [4096], 512, 11008, ksplit=2) == T(Q4_K, 1, 64, 4, 512, 78848)   # 64 x 4 x 2 parts
    # the CU count is the device's: the same 512 workgroups on a card of 304 CUs take two stages
    p = engine.op_mmq_plan(engine.MMQ_TILED, Q4_K, [8192], 512, 256, n_cu=304)
    assert (p["nst"], p["lds"]) == (2, 124928)


def test_tiled_grouped():
    # Mixtral's experts: 8 x gate/up pair 14336 (896 pair tiles, 448 row blocks)
    assert tiled(Q5_K, [14336], 1280, 4096, pair=True, grp_n=8, grp_max=20) == \
        T(Q5_K, 1, 448, 10, 3584, 80896, pair=1, grouped=1)
    assert tiled(Q5_K, [14336], 1280, 4096, pair=True, grp_n=8, grp_max=512) == \
        T(Q5_K, 1, 448, 10, 14336, 80896, pair=1, grouped=1)
    # few rows: 16 row blocks x 8 experts = 128 workgroups, two stages
    assert tiled(Q6_K, [1024], 512, 4096, grp_n=8, grp_max=20) == T(Q6_K, 2, 16, 4, 128, 141312, grouped=1)
    assert tiled(Q6_K, [1024], 512, 4096, grp_n=8, grp_max=512) == T(Q6_K, 1, 16, 4, 512, 70656, grouped=1)


def test_tiled_pre_and_gx():
    assert tiled(Q4_K, [4096], 512, 4096, pre=True) == T(Q4_K, 2, 64, 4, 256, 124928, pre=1)
    assert tiled(Q4_K, [11008], 512, 4096, pair=True, pre=True) == T(Q4_K, 1, 344, 4, 1376, 78848, pair=1, pre=1)
    # a split launch stores plain parts: its kernel is not the PRE one
    assert tiled(Q4_K, [4096], 512, 4096, ksplit=2, pre=True) == T(Q4_K, 1, 64, 4, 512, 78848)
    # GPT-2 117M's fused attn_qkv with its bias: 72 row tiles, 36 row blocks -> 40, 2 token blocks
    assert tiled(Q8_0, [2304], 160, 768, gx=True) == T(Q8_0, 2, 36, 2, 80, 114688, gx=1)
    assert tiled(Q6_K, [768, 768, 768], 512, 768, gx=True) == T(Q6_K, 2, 36, 4, 160, 141312, gx=1)
    # Q4_0 / Q5_0 copies are Q8_0 tiles
    assert tiled(Q4_0, [4096], 512, 4096) == T(Q8_0, 2, 64, 4, 256, 114688)
    assert tiled(Q5_0, [4096], 512, 4096, gx=True) == T(Q8_0, 2, 64, 4, 256, 114688, gx=1)


SPLITK = "split-K \\(2 or 4 parts\\) is for a single EPI_ADD matrix"
GX = "bias / GELU launches take one plain matrix, no pre, no split-K"


@pytest.mark.parametrize("why,kw", [
    ("Q4_K / Q5_K / Q6_K / Q8_0 only", dict(t=F16)),
    (SPLITK, dict(ksplit=3)),
    (SPLITK, dict(ksplit=8)),
    (SPLITK, dict(ksplit=2, pair=True)),
    (SPLITK, dict(ksplit=2, grp_n=8, grp_max=20)),
    (SPLITK, dict(ksplit=2, rows=[4096, 4096])),
    (SPLITK, dict(ksplit=4, K=512)),            # fewer superblocks than parts
    (GX, dict(gx=True, pair=True)),
    (GX, dict(gx=True, pre=True)),
    (GX, dict(gx=True, ksplit=2)),
    (GX, dict(gx=True, grp_n=8, grp_max=20)),
])
def test_tiled_unserved(why, kw):
    kw = dict(kw)
    p = tiled(kw.pop("t", Q4_K), kw.pop("rows", [4096]), 512, kw.pop("K", 4096), **kw)
    assert isinstance(p, dict) and p["kernel"] == NONE
    assert re.search(why, p["why"]), p["why"]


def test_short_single_and_pair():
    # 4096 x 4096: 128 row tiles, 4 K-parts
    assert short(Q4_K, [4096], 32, 4096) == S(LEAN, Q4_K, 1, 128, 4, 512, 64, 0)
    assert short(Q4_K, [4096], 64, 4096) == S(SHORT, Q4_K, 2, 128, 4, 128, 256, 74752)
    assert short(Q5_K, [4096], 32, 4096) == S(LEAN, Q5_K, 1, 128, 4, 512, 64, 0)
    assert short(Q5_K, [4096], 64, 4096) == S(SHORT, Q5_K, 2, 128, 4, 128, 256, 74752)
    assert short(Q6_K, [4096], 32, 4096) == S(SHORT1, Q6_K, 1, 128, 4, 512, 64, 0)
    assert short(Q6_K, [4096], 64, 4096) == S(SHORT, Q6_K, 2, 128, 4, 128, 256, 74752)
    # Q8_0 2048 x 2048: 64 row tiles, 2 K-parts, the LDS form at one token tile too
    assert short(Q8_0, [2048], 32, 2048) == S(SHORT, Q8_0, 1, 64, 2, 32, 256, 40960)
    assert short(Q8_0, [2048], 64, 2048) == S(SHORT, Q8_0, 2, 64, 2, 32, 256, 73728)
    assert short(Q4_0, [2048], 32, 2048) == S(SHORT, Q8_0, 1, 64, 2, 32, 256, 40960)
    # pairs: 688 pair tiles
    assert short(Q4_K, [11008], 32, 4096, pair=True) == S(LEAN, Q4_K, 1, 688, 4, 2752, 64, 0, pair=1)
    assert short(Q4_K, [11008], 64, 4096, pair=True) == S(SHORT, Q4_K, 2, 688, 4, 688, 256, 74752, pair=1)
    assert short(Q5_K, [11008], 32, 4096, pair=True) == S(LEAN, Q5_K, 1, 688, 4, 2752, 64, 0, pair=1)
    assert short(Q6_K, [11008], 32, 4096, pair=True) == S(SHORT1, Q6_K, 1, 688, 4, 2752, 64, 0, pair=1)
    assert short(Q6_K, [1000], 64, 4096, pair=True) == S(SHORT, Q6_K, 2, 63, 4, 64, 256, 74752, pair=1)
    assert short(Q8_0, [5632], 32, 2048, pair=True) == S(SHORT, Q8_0, 1, 352, 2, 176, 256, 40960, pair=1)
    assert short(Q8_0, [5632], 64, 2048, pair=True) == S(SHORT, Q8_0, 2, 352, 2, 176, 256, 73728, pair=1)
    # K = 11008: 43 superblocks, 11 K-parts
    assert short(Q4_K, [4096], 32, 11008) == S(LEAN, Q4_K, 1, 128, 11, 1408, 64, 0)


def test_short_qkv_and_grouped():
    assert short(Q4_K, [4096, 4096, 4096], 32, 4096) == S(LEAN, Q4_K, 1, 384, 4, 1536, 64, 0)
    assert short(Q6_K, [4096, 1024, 1024], 64, 4096) == S(SHORT, Q6_K, 2, 192, 4, 192, 256, 74752)
    # Mixtral's experts over the padded MoE rows
    assert short(Q5_K, [14336], 256, 4096, pair=True, grp_n=8, grp_max=20) == \
        S(LEAN, Q5_K, 1, 896, 4, (3584, 8, 1), 64, 0, pair=1, grouped=1)
    assert short(Q5_K, [14336], 384, 4096, pair=True, grp_n=8, grp_max=64) == \
        S(LEAN, Q5_K, 1, 896, 4, (3584, 8, 2), 64, 0, pair=1, grouped=1)
    assert short(Q6_K, [4096], 256, 14336, grp_n=8, grp_max=33) == S(SHORT1, Q6_K, 1, 128, 14, (1792, 8, 2), 64, 0, grouped=1)


@pytest.mark.parametrize("why,kw", [
    ("mmqs: Q4_K / Q5_K / Q6_K / Q8_0 / Q4_0 / Q5_0 only", dict(t=F16)),
    ("mmqs grouped: Q4_K / Q5_K / Q6_K experts only", dict(t=Q8_0, npad=256, grp_n=8, grp_max=20)),
    ("mmqs grouped: Q4_K / Q5_K / Q6_K experts only", dict(t=Q4_0, npad=256, grp_n=8, grp_max=20)),
    ("mmqs: 1..64 tokens", dict(npad=96)),
    ("mmqs grouped: bad expert / row count", dict(npad=256, grp_n=8, grp_max=65)),
    ("mmqs: 1..3 matrices", dict(rows=[4096, 4096], pair=True)),
    ("mmqs: K must be a multiple of 256", dict(K=4000)),
])
def test_short_unserved(why, kw):
    kw = dict(kw)
    p = short(kw.pop("t", Q4_K), kw.pop("rows", [4096]), kw.pop("npad", 32), kw.pop("K", 4096), **kw)
    assert isinstance(p, dict) and p["kernel"] == NONE
    assert why in p["why"], p["why"]


def test_bad_form_is_an_error():
    with pytest.raises(engine.EngineError, match="form 0"):
        engine.op_mmq_plan(2, Q4_K, [4096], 32, 4096)


def moe_cap(n, E):
    """moe_rows_cap (kernels.h): the padded MoE rows of n picks over E experts."""
    return (n + E * 31 + 31) // 32 * 32


def test_cases_reach_the_instantiations_they_name():
    """What mmq_plan gives shapes of the GPU op tests (no GPU): between them test_gpu_batch_ops,
    test_gpu_gpt2_batch_ops, test_gpu_moe_ops and test_gpu_legacy_quant_ops reach one and two stages,
    the pair (AB), bias / GELU (GX) and grouped instantiations of mmq2_t, mmqs1_lean_t, mmqs1_t<Q6_K>,
    and mmqs_t at one token tile (Q8_0) and at two.  The PRE instantiations take GemmParams::pre, which
    no op entry point sets: the LoRA model tests (test_gpu_lora.py) run them."""
    reached = set()

    def see(got, want):
        assert got == want
        k = got[0]
        if k == TILED:
            reached.update({("nst", got[6]), ("AB", got[2]), ("GX", got[4]), ("grouped", got[5])})
        else:
            reached.add((k, got[1] == Q8_0, got[7]))

    # test_gpu_batch_ops.GEMM_CASES (the tiled form pinned), npad = the tokens rounded up to 32
    see(tiled(Q4_K, [4096], 64, 4096), T(Q4_K, 2, 64, 1, 64, 124928))
    see(tiled(Q4_K, [11008], 64, 4096, pair=True), T(Q4_K, 2, 344, 1, 344, 124928, pair=1))
    see(tiled(Q4_K, [11008], 512, 4096, pair=True), T(Q4_K, 1, 344, 4, 1376, 78848, pair=1))
    see(tiled(Q6_K, [32000], 128, 4096), T(Q6_K, 2, 500, 1, 504, 141312))
    see(tiled(Q8_0, [32000], 64, 2048), T(Q8_0, 2, 500, 1, 504, 114688))
    # test_gpu_batch_ops.MMQS_CASES
    see(short(Q4_K, [4096], 32, 4096), S(LEAN, Q4_K, 1, 128, 4, 512, 64, 0))
    see(short(Q4_K, [4096], 64, 4096), S(SHORT, Q4_K, 2, 128, 4, 128, 256, 74752))
    see(short(Q6_K, [4096], 32, 11008), S(SHORT1, Q6_K, 1, 128, 11, 1408, 64, 0))
    see(short(Q6_K, [1000], 64, 4096, pair=True), S(SHORT, Q6_K, 2, 63, 4, 64, 256, 74752, pair=1))
    see(short(Q8_0, [2048], 32, 5632), S(SHORT, Q8_0, 1, 64, 6, 96, 256, 40960))
    see(short(Q8_0, [2048], 64, 5632), S(SHORT, Q8_0, 2, 64, 6, 96, 256, 73728))
    # test_gpu_gpt2_batch_ops: bias at 129 tokens, GELU at the partial row tile
    see(tiled(Q8_0, [2304], 160, 768, gx=True), T(Q8_0, 2, 36, 2, 80, 114688, gx=1))
    see(tiled(Q6_K, [40], 32, 256, gx=True), T(Q6_K, 2, 1, 1, 8, 141312, gx=1))
    # test_gpu_moe_ops (N_EMBD 512, N_FF 768): mode 0 the tiled grouped launch, mode 1 the short one
    see(tiled(Q4_K, [768], moe_cap(66, 4), 512, pair=True, grp_n=4, grp_max=33),
        T(Q4_K, 2, 24, 2, 96, 124928, pair=1, grouped=1))
    see(tiled(Q4_K, [768], moe_cap(1024, 16), 512, pair=True, grp_n=16, grp_max=512),
        T(Q4_K, 1, 24, 12, 1536, 78848, pair=1, grouped=1))
    see(short(Q4_K, [768], moe_cap(128, 4), 512, pair=True, grp_n=4, grp_max=64),
        S(LEAN, Q4_K, 1, 48, 1, (48, 4, 2), 64, 0, pair=1, grouped=1))
    see(short(Q6_K, [512], moe_cap(66, 8), 768, grp_n=8, grp_max=33), S(SHORT1, Q6_K, 1, 16, 1, (16, 8, 2), 64, 0, grouped=1))
    # test_gpu_legacy_quant_ops: 320 rows, K 768, at 20, 33 (a pair) and 65 tokens
    see(short(Q4_0, [320], 32, 768), S(SHORT, Q8_0, 1, 10, 1, 3, 256, 40960))
    see(short(Q5_0, [320], 64, 768, pair=True), S(SHORT, Q8_0, 2, 20, 1, 5, 256, 73728, pair=1))
    see(tiled(Q4_0, [320], 96, 768), T(Q8_0, 2, 5, 1, 8, 114688))
    assert reached >= {("nst", 1), ("nst", 2), ("AB", 1), ("GX", 1), ("grouped", 1),
                       (LEAN, False, 1), (SHORT1, False, 1), (SHORT, True, 1), (SHORT, False, 2), (SHORT, True, 2)}
