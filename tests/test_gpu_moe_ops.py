"""Op-level parity of the mixture-of-experts kernels, one at a time, at the shapes a whole-model
run with random weights never produces: experts without rows, every token on the same two experts,
per-expert counts on the 32-row tile boundaries, more picks than moe_group_kernel has threads, 16
and 64 experts, every register-tile width of the router.  Nothing is waived: the routing near-tie
allowance of the whole-model tests (util.ROUTE_TIE) has no counterpart here.

  moe_group_kernel (kernels.hip), through mi_op_moe_group.  Integers, bit-exact against
      group_ref: counts per expert, offsets padded to 32, rows[r] = the source token (ascending
      within an expert, -1 on padding rows and past the last expert up to the capacity),
      rowsel[r] = r or -1, pos a permutation into the non-padding rows.

  router_kernel (kernels.hip), through mi_op_router.  Reference router_ref: float64
      rms_norm(x) * norm_w, logits, softmax, stable top-2, weights normalised over the two picks
      (LlamaOracle._ffn's arithmetic).
      Logit bound.  The kernel forms cur_i = fl(fl(x_i * scale) * nw_i): two roundings on top of
      scale's own error.  scale = 1 / sqrtf((float)(sum / n) + eps): the squares are rounded to f32
      (the double sum of them is then off by at most u = 2^-24 relative), the cast and the add of
      eps round once each, the square root halves those 3 u to 1.5 u and rounds once, the division
      once (both correctly rounded): 3.5 u, taken as 4 u.  A logit is a per-lane chain of
      m = n_embd / 64 fmas (one rounding each) followed by the 6 butterfly adds of wave_sum, so
      every product w_i * cur_i passes through at most m + 6 roundings after the 6 u of cur_i:
          |logit_gpu - logit_ref| <= gamma * sum_i |w_i * cur_i|,  gamma = k u / (1 - k u),
          k = n_embd / 64 + 6 + 6
      (Higham's gamma_k; 4.5e-6 at n_embd = 4096).  router_ref() evaluates it per token and expert.
      sel must equal the reference on every token, in slot order.  That is sound because the data
      (fixed seeds, ROUTER_SEEDS) keeps the reference probabilities of ranks 1, 2 and 3 apart by
      at least 100 x the largest logit bound of the token -- asserted on the CPU for every seed
      (test_router_reference_gaps); a probability gap never exceeds the logit gap.
      selw bound.  selw_0 = sigmoid(l_0 - l_1) exactly (the softmax denominator cancels), and the
      kernel's exponent l_0 - l_1 is off by at most
          D = eps_0 + eps_1 + u (|l_0 - lmax| + |l_1 - lmax| + 4 eps_max) + 10 u
      (the logit bounds; the rounding of lg - mx; expf within 2 ulp = 4 u and the product with
      1 / sum, u, for either pick), so |selw_k - ref_k| <= w_0 w_1 D e^D + 3 u w_k (sigmoid' =
      w_0 w_1, Lipschitz in the exponent; the add of the two picks, the division).
      The split-WO write-back x = (p0 + p1) + x is two f32 additions: bit-equal to numpy's.

  mmq2_t grouped / mmqs1 grouped (mmq.hip), through mi_op_moe_gemm.  Pick i is token i // 2
      through expert sel[i]: gemm_ref of that expert's matrix on that token's row, under the dense
      GEMM tests' bars (test_gpu_batch_ops.py): GEMM_TOL x sum_b |term_b| for one matrix, the
      SwiGLU bound of gemm_swiglu_ref for a gate/up pair.  The same bars reject the reference of
      the neighbouring expert (sel[i] + 1) % E on most elements, so they can tell experts apart.

  gemv_kernel's expert selection (gemv.hip), through mi_op_moe_decode.  h[k] against
      silu(g) * u of expert sel[k] under test_dgemv_swiglu_pair's bound (gemv_swiglu_ref); x_out
      against the float64 ((y0 w0 + y1 w1) + x) [+ addend] with y_k = mul_mat_vec(down[sel[k]],
      the GPU's own h[k]), within GEMV_TOL x (|w0| abs0 + |w1| abs1) for the two dots plus
      2^-22 x (|y0 w0| + |y1 w1| + |x| + |addend|) for the epilogue's roundings, fused or not."""
import functools

import numpy as np
import pytest

import ggml_ref as R
from blama_amd import engine
from gemm_ref_util import GEMM_TOL, _act_blocks, gemm_ref, gemm_swiglu_ref, gemv_ref, gemv_swiglu_ref
from util import rand_matrix, rand_x

gpu = pytest.mark.gpu

GEMV_TOL = 2e-5
U24 = 2.0 ** -24
N_EMBD, N_FF = 512, 768


# ------------------------------------------------------------------ routing patterns ---
def picks_random(ntok, E, rng):
    """Uniform random distinct pairs (E = 1: both slots expert 0, which the grouping accepts)."""
    if E == 1:
        return np.zeros((ntok, 2), np.int32)
    a = rng.integers(0, E, ntok)
    b = (a + 1 + rng.integers(0, E - 1, ntok)) % E
    return np.stack([a, b], 1).astype(np.int32)


def picks_fixed(ntok, a, b):
    return np.tile(np.array([a, b], np.int32), (ntok, 1))


# per-expert counts on the tile boundaries: a full tile, a tile and one row, none, one, 31
HAND_COUNTS = {
    4: [32, 33, 0, 1],
    8: [32, 33, 0, 1, 31, 1, 0, 0],
    16: [32, 33, 0, 1, 31, 1, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1],
}


def picks_counts(counts, rng):
    """Distinct pairs whose per-expert counts are exactly `counts` (each token takes the two experts
    with the most rows left; slot order and token order shuffled)."""
    rem = np.array(counts)
    assert rem.sum() % 2 == 0 and rem.max() * 2 <= rem.sum()
    out = []
    for _ in range(rem.sum() // 2):
        a, b = np.argsort(-rem, kind="stable")[:2]
        assert rem[a] > 0 and rem[b] > 0
        rem[a] -= 1
        rem[b] -= 1
        out.append((a, b) if rng.integers(2) else (b, a))
    sel = np.array(out, np.int32)[rng.permutation(len(out))]
    assert np.bincount(sel.reshape(-1), minlength=len(counts)).tolist() == list(counts)
    return sel


# ------------------------------------------------------------------------- grouping ---
def group_ref(sel, U, E, cap):
    """moe_group_kernel's contract in plain Python: (grp [2E+1], rows [cap], rowsel [cap], pos [n])."""
    sel = [int(e) for e in np.asarray(sel).reshape(-1)]
    cnt = [0] * E
    for e in sel:
        cnt[e] += 1
    off = [0]
    for e in range(E):
        off.append(off[e] + (cnt[e] + 31) // 32 * 32)
    assert off[E] <= cap
    rows, rowsel, pos, used = [-1] * cap, [-1] * cap, [], [0] * E
    for i, e in enumerate(sel):
        r = off[e] + used[e]
        used[e] += 1
        rows[r] = i // U
        rowsel[r] = r
        pos.append(r)
    return (np.array(off + cnt, np.int32), np.array(rows, np.int32), np.array(rowsel, np.int32),
            np.array(pos, np.int32))


GROUP_E = [1, 4, 8, 16]
GROUP_NTOK = [1, 16, 31, 32, 33, 64, 129, 512]     # n = 2 ntok picks: up to 4 per thread


def group_patterns(E, ntok):
    """(name, sel [ntok][2]) of one (E, ntok) grid point."""
    out = [("random", picks_random(ntok, E, np.random.default_rng(1000 * E + ntok)))]
    if E >= 2:
        out += [("first-two", picks_fixed(ntok, 0, 1)), ("last-two", picks_fixed(ntok, E - 2, E - 1))]
    if E == 16 and ntok == 16:   # a token per pair of experts: 32 picks on 512 rows, the most padding
        out.append(("spread", np.array([[(2 * t) % E, (2 * t + 1) % E] for t in range(ntok)], np.int32)))
    return out


def hand_patterns():
    return [(E, picks_counts(c, np.random.default_rng(E))) for E, c in HAND_COUNTS.items()]


def _all_group_cases():
    for E in GROUP_E:
        for ntok in GROUP_NTOK:
            for name, sel in group_patterns(E, ntok):
                yield f"E{E}-n{ntok}-{name}", E, sel
    for E, sel in hand_patterns():
        yield f"E{E}-hand", E, sel


def test_group_reference_contract():
    """group_ref itself, against the contract stated in words (no GPU)."""
    for what, E, sel in _all_group_cases():
        n = sel.size
        cap = engine.moe_rows_cap(n, E)
        grp, rows, rowsel, pos = group_ref(sel, 2, E, cap)
        off, cnt = grp[:E + 1], grp[E + 1:]
        assert cnt.tolist() == np.bincount(sel.reshape(-1), minlength=E).tolist(), what
        assert off[0] == 0 and all(o % 32 == 0 for o in off) and off[E] <= cap, what
        assert (np.diff(off) == (cnt + 31) // 32 * 32).all(), what
        live = np.zeros(cap, bool)
        for e in range(E):
            r = rows[off[e]:off[e] + cnt[e]]
            assert (r >= 0).all() and (np.diff(r) >= 0).all(), what          # tokens ascending
            assert (sel[r] == e).any(axis=1).all(), what                     # each routed to e
            live[off[e]:off[e] + cnt[e]] = True
        assert (rows[~live] == -1).all() and (rowsel[~live] == -1).all(), what
        assert (rowsel[live] == np.nonzero(live)[0]).all(), what
        assert sorted(pos.tolist()) == np.nonzero(live)[0].tolist(), what    # a permutation
        assert (rows[pos] == np.arange(n) // 2).all(), what
    assert [np.bincount(s.reshape(-1), minlength=E).tolist() for E, s in hand_patterns()] == \
        list(HAND_COUNTS.values())


def _check_group(what, E, sel):
    cap = engine.moe_rows_cap(sel.size, E)
    got = engine.op_moe_group(sel, 2, E)
    ref = group_ref(sel, 2, E, cap)
    for name, g, r in zip(("grp", "rows", "rowsel", "pos"), got, ref):
        assert g.shape == r.shape and np.array_equal(g, r), (what, name, np.nonzero(g != r)[0][:8].tolist())


@gpu
@pytest.mark.parametrize("ntok", GROUP_NTOK)
@pytest.mark.parametrize("E", GROUP_E)
def test_moe_group_matches_reference(gpu_lib, E, ntok):
    for name, sel in group_patterns(E, ntok):
        _check_group(f"E{E}-n{ntok}-{name}", E, sel)


@gpu
def test_moe_group_tile_boundary_counts(gpu_lib):
    for E, sel in hand_patterns():
        _check_group(f"E{E}-hand", E, sel)


@gpu
def test_moe_group_errors(gpu_lib):
    sel = picks_fixed(16, 0, 1)
    with pytest.raises(engine.EngineError, match="1..16 experts"):
        engine.op_moe_group(sel, 2, 17)
    with pytest.raises(engine.EngineError, match="row capacity too small"):
        engine.op_moe_group(sel, 2, 4, cap=engine.moe_rows_cap(sel.size, 4) - 32)


# --------------------------------------------------------------------------- router ---
ROUTER_NTOK = 5
ROUTER_W_STD = 0.04
# (n_embd, n_expert) -> (seed of norm_w and the router matrix, one seed per token row): chosen on
# the CPU so that test_router_reference_gaps holds for every token, with and without `part`
ROUTER_SEEDS = {
    (256, 4): (100, [0, 1, 2, 3, 4]),
    (256, 8): (101, [0, 1, 2, 3, 4]),
    (256, 16): (102, [0, 2, 3, 5, 6]),
    (256, 64): (103, [0, 3, 4, 5, 6]),
    (512, 4): (104, [0, 1, 2, 3, 4]),
    (512, 8): (105, [0, 1, 2, 3, 4]),
    (512, 16): (106, [0, 1, 2, 3, 4]),
    (512, 64): (107, [0, 1, 2, 3, 6]),
    (4096, 4): (108, [4, 8, 9, 11, 16]),
    (4096, 8): (109, [0, 2, 4, 5, 6]),
    (4096, 16): (110, [2, 9, 14, 26, 30]),
    (4096, 64): (111, [12, 18, 31, 32, 34]),
}


def router_data(n_embd, E):
    """(x [5][n_embd], part [2][5][n_embd], norm_w, W [E][n_embd]), f32, from ROUTER_SEEDS."""
    wseed, tseeds = ROUTER_SEEDS[(n_embd, E)]
    rng = np.random.default_rng(wseed)
    norm_w = (1.0 + 0.1 * rng.standard_normal(n_embd)).astype(np.float32)
    W = (rng.standard_normal((E, n_embd)) * ROUTER_W_STD).astype(np.float32)
    x = np.empty((ROUTER_NTOK, n_embd), np.float32)
    part = np.empty((2, ROUTER_NTOK, n_embd), np.float32)
    for t, s in enumerate(tseeds):
        x[t], part[0, t], part[1, t] = router_token(n_embd, s)
    return x, part, norm_w, W


def router_token(n_embd, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(n_embd).astype(np.float32), (0.5 * rng.standard_normal(n_embd)).astype(np.float32),
            (0.5 * rng.standard_normal(n_embd)).astype(np.float32))


def part_added(x, part):
    """The router's write-back, x = (p0 + p1) + x, in f32."""
    return ((part[0] + part[1]).astype(np.float32) + x).astype(np.float32)


def router_gamma(n_embd):
    k = n_embd // 64 + 6 + 6
    return k * U24 / (1.0 - k * U24)


def router_ref(x, norm_w, W, eps):
    """float64 router of the rows x [T][n_embd]: dict of logits, eps (the logit bound per token and
    expert), probs, order (stable, descending), sel [T][2], selw [T][2]."""
    x = x.astype(np.float64)
    n = x.shape[1]
    cur = x / np.sqrt((x * x).sum(1, keepdims=True) / n + eps) * norm_w.astype(np.float64)
    W = W.astype(np.float64)
    logits = cur @ W.T
    leps = router_gamma(n) * (np.abs(cur) @ np.abs(W).T)
    e = np.exp(logits - logits.max(1, keepdims=True))
    probs = e / e.sum(1, keepdims=True)
    order = np.argsort(-probs, axis=1, kind="stable")
    sel = order[:, :2]
    w = np.take_along_axis(probs, sel, 1)
    return dict(logits=logits, eps=leps, probs=probs, order=order, sel=sel.astype(np.int32),
                selw=w / w.sum(1, keepdims=True))


def router_gaps_ok(ref):
    """Every token: ranks 1, 2, 3 of the reference at least 100 logit bounds apart (probability)."""
    p = np.take_along_axis(ref["probs"], ref["order"][:, :3], 1)
    need = 100.0 * ref["eps"].max(1)
    return (p[:, 0] - p[:, 1] >= need) & (p[:, 1] - p[:, 2] >= need)


def selw_bound(ref):
    """|selw_gpu - selw_ref| per token and slot (module docstring)."""
    l = np.take_along_axis(ref["logits"], ref["sel"], 1)
    le = np.take_along_axis(ref["eps"], ref["sel"], 1)
    lmax = ref["logits"].max(1)
    D = le.sum(1) + U24 * (np.abs(l - lmax[:, None]).sum(1) + 4 * ref["eps"].max(1)) + 10 * U24
    w = ref["selw"]
    return (w[:, 0] * w[:, 1] * D * np.exp(D))[:, None] + 3 * U24 * w


ROUTER_SHAPES = [(n, E) for n in (256, 512, 4096) for E in (4, 8, 16, 64)]
ROUTER_EPS = 1e-5


def test_router_reference_gaps():
    """The precondition of `sel equals the reference`: for every parametrised seed, with and
    without part, on every token (no GPU)."""
    for n_embd, E in ROUTER_SHAPES:
        x, part, norm_w, W = router_data(n_embd, E)
        for xe in (x, part_added(x, part)):
            ok = router_gaps_ok(router_ref(xe, norm_w, W, ROUTER_EPS))
            assert ok.all(), (n_embd, E, ok.tolist())


def test_router_reference_is_the_oracles():
    """router_ref picks what LlamaOracle._ffn's arithmetic picks (soft_max, stable argsort, f32
    weights) on the same rows."""
    x, _, norm_w, W = router_data(512, 8)
    ref = router_ref(x, norm_w, W, ROUTER_EPS)
    for t in range(ROUTER_NTOK):
        cur = R.rms_norm(x[t], ROUTER_EPS) * norm_w
        probs = R.soft_max(R.mul_mat_vec(W, R.F32, 512, cur), 1.0)
        sel = np.argsort(-probs, kind="stable")[:2]
        w = probs[sel] / np.float32(probs[sel].sum(dtype=np.float32))
        assert sel.tolist() == ref["sel"][t].tolist()
        assert np.abs(w - ref["selw"][t]).max() < 1e-5


@gpu
@pytest.mark.parametrize("with_part", [False, True], ids=["nopart", "part"])
@pytest.mark.parametrize("pad", [0, 256], ids=["dense", "strided"])
@pytest.mark.parametrize("ntok", [1, 5])
@pytest.mark.parametrize("n_embd,E", ROUTER_SHAPES)
def test_router_matches_reference(gpu_lib, n_embd, E, ntok, pad, with_part):
    x, part, norm_w, W = router_data(n_embd, E)
    x, part = x[:ntok], np.ascontiguousarray(part[:, :ntok])
    xs = np.full((ntok, n_embd + pad), 7.25, np.float32)     # the stride's tail must stay as it is
    xs[:, :n_embd] = x
    sel, selw, x_out = engine.op_router(xs, norm_w, W, eps=ROUTER_EPS, n_embd=n_embd, part=part if with_part else None)
    xe = part_added(x, part) if with_part else x
    want = xs.copy()
    want[:, :n_embd] = xe
    assert np.array_equal(x_out.view(np.uint32), want.view(np.uint32))
    ref = router_ref(xe, norm_w, W, ROUTER_EPS)
    assert router_gaps_ok(ref).all()
    assert np.array_equal(sel, ref["sel"]), (sel.tolist(), ref["sel"].tolist())
    err, lim = np.abs(selw.astype(np.float64) - ref["selw"]), selw_bound(ref)
    print("router", n_embd, E, ntok, "max err/bound", float((err / lim).max()))
    assert (err <= lim).all(), (float((err / lim).max()), err.max())


def _tie_matrix(c, targets, rng):
    """Router rows whose logits on the normed row c are `targets`, plus a little noise."""
    W = np.outer(np.array(targets), c.astype(np.float64) / (c.astype(np.float64) ** 2).sum())
    return (W + 1e-4 * rng.standard_normal(W.shape)).astype(np.float32)


@gpu
def test_router_ties_go_to_the_lower_index(gpu_lib):
    """Byte-identical router rows give bit-identical logits: ggml_argsort keeps index order."""
    rng = np.random.default_rng(5)
    n_embd = 512
    x = rng.standard_normal((1, n_embd)).astype(np.float32)
    norm_w = (1.0 + 0.1 * rng.standard_normal(n_embd)).astype(np.float32)
    c = R.rms_norm(x[0], ROUTER_EPS) * norm_w
    # ranks 2 and 3 tied (experts 6 and 2), expert 4 on top
    W = _tie_matrix(c, [0.0, -1.0, 1.0, -0.5, 3.0, 0.2, 1.0, -2.0], rng)
    W[6] = W[2]
    sel, selw, _ = engine.op_router(x, norm_w, W, eps=ROUTER_EPS)
    ref = router_ref(x, norm_w, W, ROUTER_EPS)
    assert ref["sel"].tolist() == [[4, 2]] and sel.tolist() == [[4, 2]]
    assert (np.abs(selw - ref["selw"]) <= selw_bound(ref)).all()
    # ranks 1 and 2 tied (experts 5 and 1): both picked, in index order, with equal weights
    W = _tie_matrix(c, [0.0, 3.0, 1.0, -0.5, 1.5, 3.0, 1.0, -2.0], rng)
    W[5] = W[1]
    sel, selw, _ = engine.op_router(x, norm_w, W, eps=ROUTER_EPS)
    assert sel.tolist() == [[1, 5]]
    assert selw.tolist() == [[0.5, 0.5]]


@gpu
def test_router_errors(gpu_lib):
    def run(n_embd, E):
        engine.op_router(np.zeros((1, n_embd), np.float32), np.ones(n_embd, np.float32), np.zeros((E, n_embd), np.float32))
    with pytest.raises(engine.EngineError, match="too many experts"):
        run(512, 65)
    with pytest.raises(engine.EngineError, match="multiple of 256, at most 4096"):
        run(4352, 8)
    with pytest.raises(engine.EngineError, match="multiple of 256, at most 4096"):
        run(300, 8)


# --------------------------------------------------------------------- grouped GEMMs ---
STAGES = {
    # name: (rows, K, gate/up pair, one activation row per pick)
    "gateup": (N_FF, N_EMBD, True, False),
    "down": (N_EMBD, N_FF, False, True),
}
GEMM_ROWS_MAX = 512          # the most tokens a case uses (mode 0)


@functools.lru_cache(maxsize=4)
def _gemm_x(K, per_pick):
    """The activation rows every case shares: token (or pick) r of a case is row r."""
    n = GEMM_ROWS_MAX * (2 if per_pick else 1)
    X = np.stack([rand_x(K, seed=K * 10000 + 7 * i + per_pick) for i in range(n)])
    X[0, :256] = 0.0                                   # all-zero activation blocks (d = 0)
    X[40, :256] = 0.0
    return X


@functools.lru_cache(maxsize=4)
def _gemm_act(t_is_q80, K, per_pick):
    return _act_blocks(R.Q8_0 if t_is_q80 else R.Q4_K, _gemm_x(K, per_pick))[1]


@functools.lru_cache(maxsize=1)
def gemm_table(t, stage, E):
    """(raw, raw_up, ref [E][N][rows], lim [E][N][rows]): every row of _gemm_x through every
    expert, and its bound; pick i of a case reads ref[sel[i], row of i]."""
    rows, K, pair, per_pick = STAGES[stage]
    seed = 100 * t + 10 * E + (1 if pair else 2)
    raw = rand_matrix(t, E * rows, K, seed=seed)
    up = rand_matrix(t, E * rows, K, seed=seed + 5) if pair else None
    X = _gemm_x(K, per_pick)
    A = _gemm_act(t == R.Q8_0, K, per_pick)
    ref = np.empty((E, X.shape[0], rows))
    lim = np.empty_like(ref)
    one = R.row_bytes(t, K) * rows
    for e in range(E):
        g, bg = gemm_ref(t, raw[e * one:(e + 1) * one], rows, K, X, act=A)
        if pair:
            u, bu = gemm_ref(t, up[e * one:(e + 1) * one], rows, K, X, act=A)
            ref[e], lim[e] = gemm_swiglu_ref(g, bg, u, bu)
        else:
            ref[e], lim[e] = g, GEMM_TOL * bg + 1e-30
    return raw, up, ref, lim


def gemm_patterns(mode, E):
    ntoks = (1, 33, 64) if mode == 1 else (33, 130, 512)
    for ntok in ntoks:
        yield f"random-{ntok}", picks_random(ntok, E, np.random.default_rng(17 * E + ntok))
        yield f"first-two-{ntok}", picks_fixed(ntok, 0, 1)     # 64 / 512 rows on two experts, none on the rest
    yield "hand", picks_counts(HAND_COUNTS[E], np.random.default_rng(E + 1))


def pick_rows(sel, per_pick):
    n = sel.size
    return np.arange(n) if per_pick else np.arange(n) // 2


def wrong_expert_fraction(ref, lim, sel, per_pick, E, y=None):
    """The share of elements on which the neighbouring expert's reference lies outside the bound
    (of y; y None: of everything within the bound of the right reference)."""
    flat, r = sel.reshape(-1), pick_rows(sel, per_pick)
    wrong = (flat + 1) % E
    if y is None:
        return float((np.abs(ref[flat, r] - ref[wrong, r]) > lim[flat, r] + lim[wrong, r]).mean())
    return float((np.abs(y - ref[wrong, r]) > lim[wrong, r]).mean())


GEMM_CASES = [(mode, t, stage, E)
              for t in (R.Q4_K, R.Q5_K, R.Q6_K, R.Q8_0) for stage in STAGES
              for E in ((4, 8, 16) if t == R.Q4_K else (4, 8)) for mode in (0, 1)
              if not (mode == 1 and t == R.Q8_0)]


def test_wrong_expert_reference_is_told_apart():
    """The bounds separate neighbouring experts on the reference itself (no GPU)."""
    for t in (R.Q4_K, R.Q5_K, R.Q6_K, R.Q8_0):
        for stage, (_, _, _, per_pick) in STAGES.items():
            _, _, ref, lim = gemm_table(t, stage, 4)
            for what, sel in gemm_patterns(1, 4):
                assert wrong_expert_fraction(ref, lim, sel, per_pick, 4) > 0.9, (R.TYPE_NAME[t], stage, what)


@gpu
@pytest.mark.parametrize("mode,t,stage,E", GEMM_CASES,
                         ids=[f"{R.TYPE_NAME[c[1]]}-{c[2]}-E{c[3]}-{'short' if c[0] else 'tiled'}" for c in GEMM_CASES])
def test_moe_gemm_matches_oracle(gpu_lib, mode, t, stage, E):
    rows, K, pair, per_pick = STAGES[stage]
    raw, up, ref, lim = gemm_table(t, stage, E)
    X = _gemm_x(K, per_pick)
    for what, sel in gemm_patterns(mode, E):
        ntok = sel.shape[0]
        y = engine.op_moe_gemm(mode, t, raw, E, rows, K, X[:2 * ntok if per_pick else ntok], sel, raw_up=up,
                               per_pick=per_pick).astype(np.float64)
        flat, r = sel.reshape(-1), pick_rows(sel, per_pick)
        err, bound = np.abs(y - ref[flat, r]), lim[flat, r]
        bad = np.argwhere(err > bound)
        print("moe_gemm", R.TYPE_NAME[t], stage, E, mode, what, "max err/bound", float((err / bound).max()))
        assert bad.size == 0, (what, len(bad), bad[:5].tolist(), float((err / bound).max()))
        # picks of one token on different experts: different rows (an expert stride that is ignored)
        assert (y[0::2] != y[1::2]).any(axis=1).all(), what
        assert wrong_expert_fraction(ref, lim, sel, per_pick, E, y) > 0.9, what


@gpu
def test_moe_gemm_errors(gpu_lib):
    rows, K = 64, 256
    raw = rand_matrix(R.Q4_K, 4 * rows, K, seed=3)
    X = np.zeros((65, K), np.float32)
    with pytest.raises(engine.EngineError, match="short form"):
        engine.op_moe_gemm(1, R.Q4_K, raw, 4, rows, K, X, picks_fixed(65, 0, 1))
    with pytest.raises(engine.EngineError, match="short form"):
        engine.op_moe_gemm(1, R.Q8_0, rand_matrix(R.Q8_0, 4 * rows, K, seed=3), 4, rows, K, X[:4], picks_fixed(4, 0, 1))
    with pytest.raises(engine.EngineError, match="must differ"):
        engine.op_moe_gemm(0, R.Q4_K, raw, 4, rows, K, X[:4], picks_fixed(4, 2, 2))
    with pytest.raises(engine.EngineError, match="out of range"):
        engine.op_moe_gemm(0, R.Q4_K, raw, 4, rows, K, X[:4], picks_fixed(4, 0, 4))


# --------------------------------------------------------------------------- decode ---
DECODE_E = 8
DECODE_SEL = [(0, 1), (7, 0), (3, 3)]


def _row_subset(rows, wide):
    # the oracle on a row subset of the wide case's matrices (every workgroup's range is still sampled)
    return np.unique(np.r_[np.arange(0, rows, 37), np.arange(rows - 16, rows)]) if wide else None


@functools.lru_cache(maxsize=1)
def decode_data(t, n_embd, n_ff):
    seed = 10 * t + n_embd
    rng = np.random.default_rng(seed)
    d = dict(gate=rand_matrix(t, DECODE_E * n_ff, n_embd, seed=seed + 1),
             up=rand_matrix(t, DECODE_E * n_ff, n_embd, seed=seed + 2),
             down=rand_matrix(t, DECODE_E * n_embd, n_ff, seed=seed + 3),
             x=rand_x(n_embd, seed=seed + 4),
             norm_w=(1.0 + 0.1 * rng.standard_normal(n_embd)).astype(np.float32),
             addend=rand_x(n_embd, seed=seed + 5, scale=0.3), h_ref={})
    d["cur"] = (R.rms_norm(d["x"], ROUTER_EPS) * d["norm_w"]).astype(np.float32)
    return d


def _expert(raw, t, rows, K, e):
    one = R.row_bytes(t, K) * rows
    return raw[e * one:(e + 1) * one]


def decode_h_ref(d, t, n_embd, n_ff, e):
    """(silu(g) * u, bound) of expert e on the normed row, on the row subset (computed once)."""
    if e not in d["h_ref"]:
        rs = _row_subset(n_ff, n_embd > N_EMBD)
        g, ga = gemv_ref(t, _expert(d["gate"], t, n_ff, n_embd, e), n_embd, d["cur"], rs)
        u, ua = gemv_ref(t, _expert(d["up"], t, n_ff, n_embd, e), n_embd, d["cur"], rs)
        d["h_ref"][e] = gemv_swiglu_ref(g, ga, u, ua, GEMV_TOL)
    return d["h_ref"][e]


DECODE_CASES = [(t, N_EMBD, N_FF) for t in (R.Q4_K, R.Q5_K, R.Q6_K, R.Q8_0)] + [(R.Q5_K, 4096, 14336)]


@gpu
@pytest.mark.parametrize("with_addend", [False, True], ids=["plain", "addend"])
@pytest.mark.parametrize("sel", DECODE_SEL, ids=[f"sel{a}{b}" for a, b in DECODE_SEL])
@pytest.mark.parametrize("t,n_embd,n_ff", DECODE_CASES, ids=[f"{R.TYPE_NAME[c[0]]}-{c[1]}x{c[2]}" for c in DECODE_CASES])
def test_moe_decode_matches_oracle(gpu_lib, t, n_embd, n_ff, sel, with_addend):
    d = decode_data(t, n_embd, n_ff)
    selw = np.array([0.625, 0.375] if sel[0] != sel[1] else [0.3, 0.7], np.float32)
    addend = d["addend"] if with_addend else None
    h, x_out = engine.op_moe_decode(t, d["gate"], d["up"], d["down"], DECODE_E, n_embd, n_ff, d["x"], d["norm_w"],
                                    sel, selw, eps=ROUTER_EPS, addend=addend)
    rs = _row_subset(n_ff, n_embd > N_EMBD)
    for k in range(2):
        ref, bound = decode_h_ref(d, t, n_embd, n_ff, sel[k])
        err = np.abs((h[k] if rs is None else h[k][rs]).astype(np.float64) - ref)
        print("moe_decode h", R.TYPE_NAME[t], n_embd, sel, k, "max err/bound", float((err / bound).max()))
        assert np.all(err <= bound), (k, float((err / bound).max()))
    # the down launch on the GPU's own h: its Q8_K quantisation is then the reference's too
    xs = _row_subset(n_embd, n_embd > N_EMBD)
    ys, ab = [], []
    for k in range(2):
        y, a = gemv_ref(t, _expert(d["down"], t, n_embd, n_ff, sel[k]), n_ff, h[k], xs)
        ys.append(y)
        ab.append(a)
    pick = (lambda v: v.astype(np.float64)) if xs is None else (lambda v: v[xs].astype(np.float64))
    w0, w1 = float(selw[0]), float(selw[1])
    xr = pick(d["x"])
    ref = (ys[0] * w0 + ys[1] * w1) + xr
    bound = GEMV_TOL * (abs(w0) * ab[0] + abs(w1) * ab[1]) + 2.0 ** -22 * (np.abs(ys[0] * w0) + np.abs(ys[1] * w1) + np.abs(xr))
    if with_addend:
        ref = ref + pick(addend)
        bound = bound + 2.0 ** -22 * np.abs(pick(addend))
    err = np.abs(pick(x_out) - ref)
    print("moe_decode x", R.TYPE_NAME[t], n_embd, sel, "max err/bound", float((err / bound).max()))
    assert np.all(err <= bound), float((err / bound).max())
    if sel[0] != sel[1]:   # the two slots ran different experts
        assert not np.array_equal(h[0], h[1])
