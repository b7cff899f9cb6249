"""What the comparisons of tests/test_gpu_param_exact.py rest on, proved on the references of tests/param_exact_cases.py alone (no
GPU): every exact sum stays within the headroom that makes it exact in fp32 in any order (and an fp32 restatement under two random
summation orders returns the reference's bits); the representability conditions of the spectral backward hold in either
association, with the product rounded or not; the fp32 restatements of the Gaussian tiers stay inside the derived bounds; the
geometry mirrors show every path of the launches reached by a case; the index references agree with an independent statement of
the same maps; and every seeded defect changes the expected output of at least one case of its family.  Run with -s for the figures."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import param_exact_cases as P


def _same(a, b):
    """equality of two reference outputs, a NaN (an element a kernel leaves alone or must not produce) equal to itself"""
    a, b = torch.as_tensor(a), torch.as_tensor(b)
    if a.dtype == torch.bfloat16:
        return torch.equal(P.bits(a), P.bits(b))
    return a.shape == b.shape and torch.equal(torch.nan_to_num(a.double(), nan=1.25e9), torch.nan_to_num(b.double(), nan=1.25e9))


def _same_dict(a, b, keys=("u", "v", "sigma", "wv", "u_keep", "v_keep")):
    return all(_same(a[k], b[k]) for k in keys)


def _fp32_exact(t64):
    return torch.equal(t64.float().double(), t64)


# ---------------------------------------------------------------------------------------------------------------
# 1. spectral forward on exact singular pairs
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,K", sorted(set(P.SN_SHAPES + P.SN_SMALL)), ids=str)
def test_singular_pairs_are_exact_in_any_order(R, K):
    c = P.sn_case(R, K)
    p, q, a, b, W = c["p"], c["q"], c["a"], c["b"], c["W"]
    assert float(p @ p) == 4 ** a and float(q @ q) == 4 ** b
    if R > 3 and K > 3:
        assert bool((p != 0).all() and (q != 0).all()) and bool(c["E"].any())
    worst = max(P.sn_bounds(c, it) for it in (0, 1, 2))
    r0, r1, r2 = (P.sn_ref(W, p, q, it) for it in (0, 1, 2))
    # no iteration: u, v unchanged, sigma = p . (W q) = 4^(a+b)
    assert _same(r0["u"], p) and _same(r0["v"], q) and float(r0["sigma"]) == 4.0 ** (a + b)
    assert _same(r1["v"], q / 2.0 ** b) and _same(r1["u"], p / 2.0 ** a) and float(r1["sigma"]) == 2.0 ** (a + b)
    assert _same(r1["wv"], 2.0 ** b * p) and _same(r1["u_keep"], r1["u"]) and _same(r1["v_keep"], r1["v"])
    assert _same_dict(r1, r2), "a fixed point"
    for it, ref in ((0, r0), (1, r1), (2, r2)):
        assert all(_fp32_exact(ref[k]) for k in ("u", "v", "sigma", "wv"))
        for seed in (1, 2):
            got = P.sn_f32(W, p, q, it, seed)
            assert _same_dict(got, ref, ("u", "v", "sigma", "wv")), (R, K, it, seed)
    rank = int(torch.linalg.matrix_rank(W.double())) if R * K <= 130 * 216 else -1
    print(f"{R} x {K}: p.p = {4 ** a}, q.q = {4 ** b}, sigma = {2 ** (a + b)}, |W| <= {int(W.abs().max())}, rank {rank}, "
          f"largest sum |term| = {worst:.0f} of {P.LIMIT} granules")
    if (R, K) == (130, 216):
        assert (4 ** a, 4 ** b) == (256, 256) and rank == 41
    if (R, K) == (3, 60):
        assert sorted(p.tolist()) == [0.0, 0.0, 2.0]


def test_zero_weight_returns_exact_zeros_through_the_clamp():
    R, K = P.SN_ZERO
    c = P.sn_case(R, K)
    r = P.sn_ref(torch.zeros(R, K), c["p"], c["q"], 1)
    assert all(not bool(r[k].any()) and not bool(torch.isnan(r[k]).any()) for k in ("u", "v", "sigma", "u_keep", "v_keep"))
    assert bool(torch.isnan(P.sn_ref(torch.zeros(R, K), c["p"], c["q"], 1, defect="no_eps")["v"]).all())
    assert P.SN_EPS > 0 and 1.0 / P.SN_EPS < 3e38          # 0 * (1 / eps) is a finite product


def test_spectral_table_reaches_every_path():
    geo = {s: P.sn_geometry(*s) for s in P.SN_SHAPES}
    vec = {s: g for s, g in geo.items() if g.vector}
    assert any(max(g.quad_trips) == 0 and max(g.tail_rows) >= 1 for g in vec.values()), "tail loop only"
    assert any(g.quad_trips[0] == 1 and g.quad_trips[1] == 0 for g in vec.values()), "row group 0 alone takes the four-in-flight loop (R = 49)"
    assert any(max(g.quad_trips) >= 1 and min(g.tail_rows) >= 1 for g in vec.values()), "both row loops"
    assert any(min(g.quad_trips) >= 2 and min(g.tail_rows) >= 1 for g in vec.values()), "two trips and a tail in every row group"
    assert any(g.quad_trips[0] == 2 and g.quad_trips[15] == 1 for g in vec.values()), "a second trip for some row groups (R = 113)"
    assert any(max(g.quad_trips) >= 1 and max(g.tail_rows) == 0 for g in vec.values()), "no tail (R = 1024)"
    scal = {s: g for s, g in geo.items() if g.scalar_partial}
    assert {s[1] for s in scal} >= {81, 215} and any(s[0] > 48 for s in scal)
    assert {g.last_block_cols for g in vec.values()} >= {4, 60, 64} and any(g.col_blocks >= 2 and g.last_block_cols == 4 for g in vec.values())
    assert {g.col_blocks for g in geo.values()} >= {1, 2, 4, 9}
    assert {g.row_trips for g in geo.values()} >= {1, 2, 3} and {s[1] for s in geo} >= {4, 60, 64, 68, 81, 215, 576, 255, 256, 257, 516}
    assert {g.norm_trips_R for g in geo.values()} >= {1, 2, 4}
    assert {s[0] for s in geo} >= {1, 3, 15, 16, 17, 48, 49, 63, 64, 65, 112, 113, 130, 257, 1024}
    for R in {s[0] for s in geo}:                                       # the mirror visits every row once
        rows = sorted(r for quads, tail in P.cols_row_plan(R) for r in sum(quads, []) + tail)
        assert rows == list(range(R))
    # the whole table as ONE batch: one chunk, many prefix boundaries, unequal block counts on both prefixes
    (j0, n, col, row, offs), = P.sn_prefix(P.SN_SHAPES)
    assert n == len(P.SN_SHAPES) <= P.SN_MAX and len(set(np.diff(col))) >= 4 and len(set(np.diff(row))) >= 10
    # 45 small jobs: a second chunk whose scratch goes on where the first ended
    chunks = P.sn_prefix(P.SN_SMALL)
    assert len(chunks) == 2 and chunks[0][1] == P.SN_MAX and chunks[1][1] == 5
    assert chunks[1][4][0] == sum(R for R, _ in P.SN_SMALL[:P.SN_MAX]) > 0 and chunks[1][2][0] == 0


# ---------------------------------------------------------------------------------------------------------------
# 2. Gaussian tier of the forward: the fp32 restatement inside the derived bounds
# ---------------------------------------------------------------------------------------------------------------
def test_gaussian_forward_fp32_restatement_stays_inside_the_stage_bounds():
    worst = {"v": 0.0, "u": 0.0, "sigma": 0.0}
    for R, K in P.SN_SHAPES:
        d = P.sn_gauss_case(R, K)
        assert abs(float(d["u0"].double().norm()) - 1) < 1e-6 and abs(float(d["v0"].double().norm()) - 1) < 1e-6
        got = P.sn_f32(d["W"], d["u0"], d["v0"], 1, 3)
        sh = P.sn_gauss_check(d, got["u"], got["v"], got["sigma"], f"{R} x {K}")
        worst = {k: max(worst[k], sh[k]) for k in worst}
    print(f"fp32 restatement (sequential sums), largest |error| / bound: {worst}")
    # a wrong element is far outside: one dropped product of the largest case moves v by more than its bound
    d = P.sn_gauss_case(1024, 576)
    ref, bnd = P.normalize_stage(d["W"].t(), d["u0"])
    Wd = d["W"].clone()
    Wd[5, 7] = 0.0
    bad, _ = P.normalize_stage(Wd.t(), d["u0"])
    assert float(((bad - ref).abs() / bnd).max()) > 1.0


# ---------------------------------------------------------------------------------------------------------------
# 3. spectral backward
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,K", P.SG_SHAPES, ids=str)
def test_backward_exact_tier_is_representable_in_either_association(R, K):
    d = P.sg_case(R, K)
    head = P.bound(d["G"] * d["W"], 1.0)
    lg = np.log2(float(d["sigma"]))
    assert lg == round(lg) and float(d["G"].abs().max()) <= 4
    for acc in (False, True):
        ref = P.sg_ref(d, acc)
        assert _fp32_exact(ref) and bool((ref == ref.round()).all()) and float(ref.abs().max()) < 2 ** 22
        for assoc in (0, 1):
            s32, s64 = P.sg_steps(d, assoc, torch.float32), P.sg_steps(d, assoc, torch.float64)
            # every step of the fp32 restatement is its float64 value: no rounding anywhere, so an unrounded (fused) product
            # is the rounded one
            assert all(torch.equal(x.double(), y) for x, y in zip(s32, s64)), (R, K, assoc)
            assert torch.equal(s64[5] if acc else s64[4], ref)
    terms = (d["G"] * d["W"]).numpy().reshape(-1)
    for seed in (1, 2):
        assert float(P._sum32(terms, 0, np.random.default_rng(seed))) == d["dot"]
    print(f"{R} x {K}: <G, W> = {d['dot']:.0f}, sum |G W| = {head:.0f} of {P.LIMIT}, sigma = 2^{lg:.0f}, |out| <= {float(P.sg_ref(d, True).abs().max()):.0f}")


def test_backward_tables_reach_the_second_trips_and_the_gaussian_bound_holds_in_fp32():
    trips = {s: P.sg_trips(*s) for s in P.SG_SHAPES}
    assert {s[0] * s[1] for s in P.SG_SHAPES} >= {1, 255, 256, 257}
    assert trips[(130, 1040)] == (2, 1) and trips[(1024, 1040)][1] == 2 and 130 * 1040 - 512 * 256 < 8192 and 1024 * 1040 - P.GRID_CAP < 32768
    assert any(P.sg_case(*s)["dot"] == P.SG_DOT for s in P.SG_SHAPES)
    worst = 0.0
    for R, K in P.SG_GAUSS:
        d = P.sg_gauss_case(R, K)
        G, W, u, v, sg = d["G"], d["W"], d["u"], d["v"], d["sigma"][0]
        c = torch.from_numpy(np.asarray(P._sum32((G * W).numpy().reshape(-1), 0, np.random.default_rng(4)))) / sg
        for acc in (False, True):
            got = (G - (c * u).view(-1, 1) * v.view(1, -1)) / sg
            worst = max(worst, P.sg_check(d, got + d["old"] if acc else got, acc, f"{R} x {K}"))
    print(f"spectral backward, fp32 restatement: largest |error| / bound = {worst:.3g}")


# ---------------------------------------------------------------------------------------------------------------
# 4. staging references against an independent statement of the same maps
# ---------------------------------------------------------------------------------------------------------------
def test_shared_taps_and_tap_expand_references_are_the_3x3_convolution():
    """conv_shared as a 1x1 over the tap-expanded label map: wt @ tap_expand(x) == conv2d(x, w, padding=1), on integers"""
    g = torch.Generator().manual_seed(7)
    n, hid, c, cp = 2, 5, 3, 4
    ws = [P.int_tensor((hid, c, 3, 3), -4, 4, g) for _ in range(n)]
    bs = [P.int_tensor((hid,), -4, 4, g) for _ in range(n)]
    x = torch.zeros(2, 5, 4, cp)
    x[..., :c] = P.int_tensor((2, 5, 4, c), -4, 4, g)
    wt, bt = P.taps_prep_ref(ws, bs, cp)
    y = P.tap_expand_ref(x, 0, 5, 4).double() @ wt.double().t() + bt.double()
    want = torch.cat([F.conv2d(x[..., :c].permute(0, 3, 1, 2).double(), w.double(), b.double(), padding=1) for w, b in zip(ws, bs)], 1)
    assert torch.equal(y, want.permute(0, 2, 3, 1))
    # nearest down-sampling folded in: the source read at (h << down, w << down)
    src = P.tap_source((False, 8, 2, 1, 5, 4, False))
    assert torch.equal(P.tap_expand_ref(src, 2, 5, 4), P.tap_expand_ref(src[:, ::4, ::4].contiguous(), 0, 5, 4))
    un = F.unfold(src[:, ::4, ::4].permute(0, 3, 1, 2), 3, padding=1).view(1, 8, 9, 5, 4).permute(0, 3, 4, 2, 1).reshape(1, 5, 4, 72)
    assert torch.equal(P.tap_expand_ref(src, 2, 5, 4), un)


def test_staging_tables_and_references():
    for case in P.TAPS_CASES:
        n, hid, c, cp = case
        d = P.taps_case(*case)
        wt, bt = P.taps_prep_ref(d["ws"], d["bs"], cp)
        live = wt.view(n * hid, 9, cp)[:, :, :c]
        assert int(live.unique().numel()) == n * hid * 9 * c and float(live.min()) >= 1 and float(wt.max()) < 2 ** 24
        assert not bool(wt.view(n * hid, 9, cp)[:, :, c:].any()) and not bool(torch.signbit(wt).any())
        gw, gb = P.taps_grad_ref(wt, bt, n, hid, c, cp)                       # grad(prep(w)) == w
        assert all(torch.equal(a, b) for a, b in zip(gw, d["ws"])) and all(torch.equal(a, b) for a, b in zip(gb, d["bs"]))
        gw, _ = P.taps_grad_ref(d["dw"], d["db"], n, hid, c, cp)
        assert all(not bool((t == P.POISON).any()) for t in gw) and (c == cp or bool((d["dw"] == P.POISON).any()))
    assert P.grid_trips(4 * 4096 * 72) == 2 and P.grid_trips(4 * 4096 * 7 * 9) == 1 and any(c[2] == c[3] for c in P.TAPS_CASES)
    for C in P.VEC_C:
        gm, bt, ns = P.vec_case(C)
        bc, nsp = P.vec_prep_ref(gm, bt, ns)
        assert (bc.numel(), nsp.numel()) == P.vec_sizes(C) and int((bc != 0).sum()) == 2 * C and int((nsp != 0).sum()) == C
        for c in (0, C // 2, C - 1):
            assert float(bc[64 * (c // 32) + c % 32]) == float(gm[c]) and float(bc[64 * (c // 32) + 32 + c % 32]) == float(bt[c])
    assert 2 * len(P.VEC_C) + 1 > P.VEC_SPLIT, "the 33-item list takes the wrapper's 32-job split"
    assert {C % 32 for C in P.VEC_C} >= {0, 1, 31} and {C % 4 for C in P.VEC_C} == {0, 1, 2, 3} and P.vec_sizes(max(P.VEC_C))[0] > 2 * 256 * 4
    cs = P.TAP_CASES
    assert {(c[0], c[1]) for c in cs} == {(False, 8), (True, 8), (True, 16)} and {c[2] for c in cs} == {0, 1, 2}
    assert {(c[4], c[5]) for c in cs} >= {(1, 1), (2, 3), (5, 4)} and {c[6] for c in cs} == {False, True}
    for bf in (False, True):
        big = [P.tap_groups(c) for c in cs if c[0] == bf and P.tap_groups(c) > P.GRID_CAP]
        assert big and all(g < P.GRID_CAP + 4096 for g in big), "one size just past the cap of the grid"


# ---------------------------------------------------------------------------------------------------------------
# 5. element-wise
# ---------------------------------------------------------------------------------------------------------------
def test_elementwise_references_are_exact():
    assert {P.grid_trips(n) for n in P.EW_N} == {1, 2, 3} and P.grid_trips(1048576) == 1 and P.grid_trips(1048577) == 2
    assert {P.act_split(n)[1] for n in P.EW_N} >= {1, 3, 17, 31, 32} and all(a * b == n for n in P.EW_N for a, b in [P.act_split(n)])
    for n in P.EW_N:
        d = P.ew_operands(n)
        for sh, sd in P.SCALES:
            r = P.scale_ref(d["x"], sh, sd)
            assert torch.equal(P.scale_ref(d["x"], sh, sd, torch.float32).double(), r) and _fp32_exact(r)
        r = P.tanh_bwd_ref(d["dy"], d["y_tanh"])
        y = d["y_tanh"]
        assert torch.equal(P.tanh_bwd_ref(d["dy"], y, torch.float32).double(), r) and float(y.abs().max()) <= 1
        assert _fp32_exact((y.double() * y.double())) and bool((y * 16 == (y * 16).round()).all())
        ya = d["y_act"]
        for act, slope in P.ACT_VARIANTS:
            r = P.act_bwd_ref(d["dy"], ya, act, slope)
            assert torch.equal(P.act_bwd_ref(d["dy"], ya, act, slope, dtype=torch.float32).double(), r)
        if n >= 255:
            zero = ya == 0
            share = lambda m: float(m.double().mean())
            assert share(ya > 0) >= 0.24 and share(ya < 0) >= 0.24 and share(zero & torch.signbit(ya)) >= 0.24 and share(zero & ~torch.signbit(ya)) >= 0.24
            for k, val in enumerate((1.0, -1.0)):
                assert share(y == val) >= 0.12
            assert share((y == 0) & torch.signbit(y)) >= 0.12 and share((y == 0) & ~torch.signbit(y)) >= 0.12


# ---------------------------------------------------------------------------------------------------------------
# seeded defects
# ---------------------------------------------------------------------------------------------------------------
def _sn_defect(defect):
    hit = 0
    for R, K in P.SN_SHAPES:
        c = P.sn_case(R, K)
        hit += not _same_dict(P.sn_ref(c["W"], c["p"], c["q"], 1), P.sn_ref(c["W"], c["p"], c["q"], 1, defect=defect))
    return hit


def _find_defect():
    hit = 0
    for j, (R, K) in enumerate(P.SN_SHAPES):
        c = P.sn_case(R, K)
        hit += j > 0 and not _same_dict(P.sn_ref(c["W"], c["p"], c["q"], 1), P.sn_ref(c["W"], c["p"], c["q"], 1, first_block_lost=True))
    return hit


def _chunk_defect():
    wvs = [P.sn_ref(P.sn_case(R, K)["W"], P.sn_case(R, K)["p"], P.sn_case(R, K)["q"], 1)["wv"] for R, K in P.SN_SMALL]
    return int(not _same(P.sn_scratch_ref(P.SN_SMALL, wvs), P.sn_scratch_ref(P.SN_SMALL, wvs, "chunk_scratch")))


def _eps_defect():
    R, K = P.SN_ZERO
    c = P.sn_case(R, K)
    Z = torch.zeros(R, K)
    return int(not _same_dict(P.sn_ref(Z, c["p"], c["q"], 1), P.sn_ref(Z, c["p"], c["q"], 1, defect="no_eps")))


def _sg_defect(defect):
    return sum(not _same(P.sg_ref(P.sg_case(*s), acc), P.sg_ref(P.sg_case(*s), acc, defect)) for s in P.SG_SHAPES[:5] for acc in (False, True))


def _taps_defect(defect):
    hit = 0
    for case in P.TAPS_CASES[:6]:
        n, hid, c, cp = case
        d = P.taps_case(*case)
        hit += not _same(P.taps_prep_ref(d["ws"], d["bs"], cp)[0], P.taps_prep_ref(d["ws"], d["bs"], cp, defect)[0])
        if defect == "channel_major":
            hit += not all(_same(a, b) for a, b in zip(P.taps_grad_ref(d["dw"], d["db"], n, hid, c, cp)[0],
                                                       P.taps_grad_ref(d["dw"], d["db"], n, hid, c, cp, defect)[0]))
    return hit


def _vec_defect(defect):
    return sum(not all(_same(a, b) for a, b in zip(P.vec_prep_ref(*P.vec_case(C)), P.vec_prep_ref(*P.vec_case(C), defect=defect))) for C in P.VEC_C)


def _tap_defect(defect):
    hit = 0
    for case in P.TAP_CASES[:10]:
        src = P.tap_source(case)
        hit += not _same(P.tap_expand_ref(src, case[2], case[4], case[5]), P.tap_expand_ref(src, case[2], case[4], case[5], defect))
    return hit


def _act_defect():
    d = P.ew_operands(257)
    return sum(not _same(P.act_bwd_ref(d["dy"], d["y_act"], a, s), P.act_bwd_ref(d["dy"], d["y_act"], a, s, "act_ge")) for a, s in P.ACT_VARIANTS)


DEFECTS = [("gemv_cols: the 16-row tail skipped", lambda: _sn_defect("cols_skip_tail")),
           ("gemv_cols: the four-in-flight loop one trip short", lambda: _sn_defect("cols_quad_early")),
           ("gemv_cols: the partial last quad of the scalar path dropped", lambda: _sn_defect("cols_scalar_partial")),
           ("gemv_rows: one 256-stride trip", lambda: _sn_defect("rows_one_trip")),
           ("sn_find: a block on a prefix boundary given to the previous job", _find_defect),
           ("SN_MAX chunking: the second chunk's scratch starts at the first chunk's", _chunk_defect),
           ("normalisation without the eps clamp", _eps_defect),
           ("sigma from the un-normalised u", lambda: _sn_defect("sigma_unnormalised")),
           ("keep copies taken before the normalisation", lambda: _sn_defect("keep_before_norm")),
           ("sn_grad: u and v indexed with r and k swapped", lambda: _sg_defect("swap_uv")),
           ("sn_grad: c not divided by sigma", lambda: _sg_defect("c_not_divided")),
           ("sn_grad: accumulate ignored", lambda: _sg_defect("ignore_accumulate")),
           ("shared_taps: channel-major instead of tap-major", lambda: _taps_defect("channel_major")),
           ("shared_taps: pad columns left unwritten", lambda: _taps_defect("pad_unwritten")),
           ("vec_prep: gamma and beta halves swapped", lambda: _vec_defect("halves_swapped")),
           ("vec_prep: the last partial group not zero-padded", lambda: _vec_defect("no_zero_pad")),
           ("tap_expand: kh / kw swapped", lambda: _tap_defect("khkw_swapped")),
           ("tap_expand: down ignored", lambda: _tap_defect("down_ignored")),
           ("tap_expand: borders not zeroed", lambda: _tap_defect("borders")),
           ("act_bwd: y >= 0 instead of y > 0", _act_defect)]


@pytest.mark.parametrize("name,run", DEFECTS, ids=[d[0] for d in DEFECTS])
def test_seeded_defect_changes_a_reference(name, run):
    hit = run()
    print(f"{name}: changes {hit} case(s)")
    assert hit >= 1, name
