"""What the comparisons of tests/test_gpu_train_exact.py rest on, proved on the references of tests/train_exact_cases.py alone
(no GPU): every sum stays within the headroom that makes it exact in fp32 in any order; every tie, kink and zero-window share
is met; the geometry mirrors reach every edge of the launches; an fp32 restatement of each formula agrees with the float64
reference (bit for bit where the output is exact, within half of the derived bound where it is bounded); and every seeded
defect changes the expected output of at least one case of its family.  Run with -s to see the shares and fractions."""
import pytest
import torch

import train_exact_cases as E


def _same(a, b):
    """equality of two reference outputs, a NaN (an element the kernel must leave alone) equal to itself"""
    if a is None or b is None:
        return a is None and b is None
    a, b = torch.as_tensor(a), torch.as_tensor(b)
    if a.dtype == torch.bfloat16:
        return torch.equal(E.bits(a), E.bits(b))
    return torch.equal(torch.nan_to_num(a.double(), nan=1.25e9), torch.nan_to_num(b.double(), nan=1.25e9))


def _fam_loss():
    for n in E.LOSS_N:
        for v in E.loss_variants(n):
            yield n, v, E.loss_operands(n, E.loss_kind(v))
    for n, kind in E.LOSS_BF16_GRAD:
        for v in E.LOSS_BF16_GRAD_VARIANTS:
            yield n, v, E.loss_bf16_grad_operands(n, kind)


# ---------------------------------------------------------------------------------------------------------------
# 1. headroom, 4. fp32 restatements
# ---------------------------------------------------------------------------------------------------------------
def test_loss_sums_are_exact_and_the_fp32_restatement_agrees():
    worst = 0.0
    for n, v, (a, b) in _fam_loss():
        r = E.loss_ref(a, b, v)
        worst = max(worst, E.bound(r["terms"], 1.0, E.LOSS0 / v.lscale if v.accumulate else 0.0))
        if n <= 2 ** 20 or v.shift == (0, 0):
            r32 = E.loss_ref(a, b, v, dtype=torch.float32)
            assert _same(r32["loss"], r["loss"]), (n, v)
            assert v.grad_bf16 or _same(r32["grad"], r["grad"]), (n, v)
        assert torch.equal(r["loss"].float().double(), r["loss"]), (n, v)
    print(f"losses: largest sum |term| = {worst:.0f} of {E.LIMIT} granules")


def test_pool_and_elementwise_sums_are_exact_and_the_fp32_restatements_agree():
    for c in E.AVG_CASES:
        N, H, W, C, acc, _ = c
        d = E.avg_case(N, H, W, C, acc)
        r = E.avgpool_bwd_ref(d["dy"], H, W, d["dx0"])
        q = E.avg_case(N, H, W, C, acc)["dy"].double() / 36
        assert bool((q == q.round()).all()) and bool((r == r.round()).all())        # dy / count is an integer for every count
        assert float(r.abs().max()) <= 4 * 8 * 36 + 64 <= E.LIMIT                  # four windows of |dy / count| <= 288, + old
        assert torch.equal(E.avgpool_bwd_ref(d["dy"], H, W, d["dx0"], dtype=torch.float32).double(), r), c
    for c in E.DOWNSUM_CASES:
        d = E.downsum_case(*c)
        r = E.downsum_ref(d["dhi"], d["dlo0"])
        assert float(r.abs().max()) <= 4 * 127 + 64 and bool((r == r.round()).all())
        assert torch.equal(E.downsum_ref(d["dhi"], d["dlo0"], dtype=torch.float32).double(), r), c
    for c in E.ADD_CASES:
        d = E.add_case(*c)
        r = E.add_ref(d["a"], d["out0"], c[5])
        assert float(r.abs().max()) <= 510 and bool((r == r.round()).all())
        assert torch.equal(E.add_ref(d["a"], d["out0"], c[5], dtype=torch.float32).double(), r), c
    for c in E.AFFINE_CASES:
        d = E.affine_case(c)
        r = E.affine_ref(c, d)
        assert float(r.abs().max()) * 8 <= E.LIMIT and bool((r * 8 == (r * 8).round()).all())        # multiples of 1/8, far below 2^24
        assert torch.equal(E.affine_ref(c, d, torch.float32).double(), r), c


def test_batchnorm_backward_sums_are_exact_and_dx_keeps_half_its_bound():
    worst, exact = 0.0, []
    for c in E.BN_BWD:
        d = E.bn_case(c)
        head = E.bn_bound(c, d)
        ref = d["ref"]
        for k in ("s1", "s2"):
            assert torch.equal(ref[k].float().double(), ref[k]), (c, k)          # what the workspace holds is the exact sum
        assert bool((d["mean"][c.C:] == 0).all() and (d["rstd"][c.C:] == 0).all() and (d["scale"][c.C:] == 0).all())
        lg = torch.log2(d["rstd"][:c.C])
        assert bool((lg == lg.round()).all()), "rstd is a power of two"
        assert bool(torch.isnan(ref["dgamma"][c.C:]).all() and torch.isnan(ref["dbeta"][c.C:]).all())
        want, bnd = E.bn_dx_bound(d)
        got = E.bn_dx_steps(d, torch.float32)[0][-1]
        frac = float(((got.double() - want).abs() / bnd.clamp_min(2.0 ** -60)).max())
        worst = max(worst, frac)
        if E.bn_dx_exact(d):
            exact.append(E.bn_id(c))
        print(f"bn_bwd {E.bn_id(c)}: headroom {head:.0f} of {E.LIMIT}, fp32 dx uses {frac:.3f} of its bound" +
              (" (exact)" if exact and exact[-1] == E.bn_id(c) else ""))
    assert worst <= 0.5, worst
    assert exact, "no case makes dx exact"


def test_bn_finalize_references_are_well_conditioned():
    for case in E.BN_FIN:
        r = E.bn_fin_case(case)["ref"]
        # mean^2 / var <= 1e4: the cancellation of the double variance costs <= 1e4 * 2^-52, far below an fp32 ulp; the shift's
        # own cancellation (beta - mean * scale) likewise
        assert float(r["cancel"]) <= 1e4 and float(r["shift_cancel"]) <= 1e4, (case, float(r["cancel"]), float(r["shift_cancel"]))
        for k in ("mean", "rstd", "scale", "shift") + (("rm", "rv") if case[5] else ()):
            assert bool(E.within_one_ulp(r[k].float(), r[k]).all()) and bool(torch.isfinite(r[k]).all())
    assert {c[0] for c in E.BN_FIN} == {1, 2, 5} and all(c[2] >= c[1] for c in E.BN_FIN) and any(c[2] > c[1] for c in E.BN_FIN)
    assert any(c[0] * c[3] == 1 and c[5] for c in E.BN_FIN), "N * HW == 1 with running statistics"
    assert {(c[4], c[5]) for c in E.BN_FIN} == {(True, True), (True, False), (False, True), (False, False)}


def test_cross_entropy_structure_is_exact():
    for case in E.CE_CASES:
        d = E.ce_case(case)
        x, t = d["x"], d["t"]
        m = x.max(1, keepdim=True).values
        rest = torch.where(x == m, torch.full_like(x, -1e9), x)
        assert bool(((x == m).sum(1) == 1).all()) and (case[1] == 1 or float((rest - m).max()) <= -128.0 <= E.EXPF_ZERO_BELOW)
        assert float(m.abs().max()) <= 8
        r = E.ce_ref(x, t, E.CE_GSCALE)
        E.bound(r["terms"], 1.0)
        am = torch.where(r["valid"], d["am"], torch.zeros_like(d["am"]))
        oh = lambda idx: (torch.arange(case[1]).view(1, -1, 1, 1) == idx.unsqueeze(1)) & r["valid"].unsqueeze(1)
        assert torch.equal(r["grad"], E.CE_GSCALE * (oh(am).double() - oh(t.clamp(0, case[1] - 1)).double())), case
        assert torch.equal(r["terms"], torch.where(r["valid"], (m - x.gather(1, t.clamp(0, case[1] - 1).unsqueeze(1))).squeeze(1).double(),
                                                   torch.zeros(()).double())), case
        if case[4]:
            assert r["count"] == 0 and r["loss_sum"] == 0 and float(r["mean"]) == 0 and not bool(r["grad"].any())


def test_softmax_and_tv_references():
    for case in E.SOFTMAX_CASES:
        for pow2 in (False, True):
            d = E.softmax_case(case, pow2)
            top = d["x"] == d["x"].max(1, keepdim=True).values
            assert torch.equal(top.sum(1, keepdim=True), d["k"]) and float(torch.where(top, torch.zeros(()), d["x"] - d["x"].max(1, keepdim=True).values).min()) >= -136
            assert case[1] == 1 or bool((top | (d["x"] - d["x"].max(1, keepdim=True).values <= -128)).all())
        r = E.softmax_bwd_ref(d["y"], d["dy"])
        assert torch.equal(E.softmax_bwd_ref(d["y"], d["dy"], torch.float32).double(), r), case
    ks = {int(k) for case in E.SOFTMAX_CASES for k in E.softmax_case(case)["k"].unique()}
    assert {1, 2, 4, 13, 64} <= ks
    for case in E.TV_CASES:
        f = E.tv_case(case)["f"]
        r, r32 = E.tv_ref(f), E.tv_ref(f, torch.float32)
        gfrac = float((r32["grad"].double() - r["grad"]).abs().max()) / E.tv_grad_bound(r)
        lfrac = abs(float(r32["loss"]) - float(r["loss"])) / E.tv_loss_bound(r)
        zy = float((f[:, 1:] == f[:, :-1]).double().mean())
        zx = float((f[:, :, 1:] == f[:, :, :-1]).double().mean())
        print(f"tv {case}: zero differences {zy:.3f} / {zx:.3f}, fp32 grad uses {gfrac:.3f} of its bound, loss {lfrac:.2e}")
        assert gfrac <= 0.5 and lfrac <= 0.5
        assert case[1] * case[2] < 16 or (zy >= 0.1 and zx >= 0.05)
    assert any(2 * n * h * w > 1024 * 256 for n, h, w in E.TV_CASES)


# ---------------------------------------------------------------------------------------------------------------
# 2. shares
# ---------------------------------------------------------------------------------------------------------------
def test_constructed_shares():
    for n in E.LOSS_N:
        if n < 64:
            continue
        a, b = E.loss_operands(n, "diff")
        assert float((a == b).double().mean()) >= 1 / 7 - 1 / n
        a, _ = E.loss_operands(n, "hinge")
        assert float((a == -1).double().mean()) >= 0.2 - 1 / n and float((a == 1).double().mean()) >= 0.2 - 1 / n
        a, _ = E.loss_operands(n, "relu")
        zero = a == 0
        assert float((zero & torch.signbit(a)).double().mean()) >= 0.25 - 1 / n and float((zero & ~torch.signbit(a)).double().mean()) >= 0.25 - 1 / n
        assert bool((a.bfloat16().float() == a).all()) and bool(torch.equal(torch.signbit(a.bfloat16()), torch.signbit(a)))
    for n, kind in E.LOSS_BF16_GRAD:
        a, b = E.loss_bf16_grad_operands(n, kind)
        v = E.LOSS_BF16_GRAD_VARIANTS[0]
        g = (a.double() - b.double()) * 2 * v.gscale
        share = E.tie_share(g)
        up = float(((g % 4 == 3) & (g >= 256)).double().mean())
        print(f"loss bf16 gradient n={n} {kind}: ties {share:.3f}, of which rounding up {up:.3f}")
        assert share >= (0.9 if kind == "dense" else 0.01) and bool(((g < 256) | ((g >= 256) & (g < 384))).all())
    # pools: every pattern present; ties, zero windows and all four positions in the references
    for bf, shapes in E.POOL_SHAPES.items():
        for shape in shapes[1:]:
            d = E.pool_case(*shape, not bf)
            P = len(E.PATTERNS) - (1 if bf else 0)
            cnt = torch.bincount(d["pat"].reshape(-1), minlength=P)
            assert int(cnt.min()) >= d["pat"].numel() // P - 1
            w = E.to_windows(d["x"]).double()
            m = w.max(3, keepdim=True).values
            ties = float(((w == m).sum(3) > 1).double().mean())
            zeros = float((m == 0).double().mean())
            took = E.to_windows(E.maxpool_bwd_ref(d["x"], d["dy"], True)) != 0
            print(f"max pool {shape}: windows with a tie {ties:.3f}, all-zero windows {zeros:.3f}, gradient taken at position "
                  f"{[round(float(took[:, :, :, p].double().mean()), 3) for p in range(4)]}")
            assert ties >= 0.3 and zeros >= 0.1 and all(bool(took[:, :, :, p].any()) for p in range(4))
            assert not bool(took[(m == 0).expand_as(took)].any()), "a zero window passes no gradient under the ReLU"
            if bf:
                assert bool(((d["x"] >= 0)).all()), "a bf16-stored x is >= +0 or -0.0"
            assert bool(torch.signbit(d["x"][d["x"] == 0]).any()) and bool((~torch.signbit(d["x"][d["x"] == 0])).any())
    for c in E.DOWNSUM_CASES:
        if c[4] == 2 and c[1] * c[2] > 1:
            r = E.downsum_ref(E.downsum_case(*c)["dhi"])
            print(f"downsum bf16 {c}: ties {E.tie_share(r):.3f}")
            assert E.tie_share(r) >= 0.01 and float(r.min()) >= 256 and float(r.max()) < 512
    for c in E.ADD_CASES:
        if c[4] and c[5] and c[1] * c[2] > 1:
            d = E.add_case(*c)
            r = E.add_ref(d["a"], d["out0"], True)
            print(f"add_slice bf16 {c}: ties {E.tie_share(r):.3f}")
            assert E.tie_share(r) >= 0.01
    for case in E.CE_CASES:
        N, C, H, W, all_ign = case
        if N * H * W >= 64 and not all_ign:
            d = E.ce_case(case)
            t, am = d["t"], d["am"]
            sh = lambda m: float(m.double().mean())
            assert sh(t == am) >= 0.45 and sh(t == E.IGNORE) >= 0.1 and sh(t == -1) >= 0.1 and sh(t == C) >= 0.1
            assert C == 1 or 0.05 <= sh((t != am) & (t >= 0) & (t < C)) <= 0.13


# ---------------------------------------------------------------------------------------------------------------
# 3. geometry
# ---------------------------------------------------------------------------------------------------------------
def test_loss_table_reaches_every_path():
    seen = set()
    for n, v, _ in _fam_loss():
        geo = E.loss_geometry(n, E.loss_vec(v))
        tags = {("mode", v.mode, v.bf16, geo.vec), ("relu", v.relu, v.bf16), ("b_none", not v.with_b), ("no_grad", not v.want_grad),
                ("acc", v.accumulate), ("shift", v.shift, v.bf16), ("lscale", v.lscale), ("gscale", v.gscale)}
        if geo.nb == E.LOSS_BLOCK_CAP:
            tags.add(("cap", geo.vec))
        if geo.vec_trips >= 2:
            tags.add("vec_second_trip")
        if geo.tail_trips >= 2:
            tags.add("tail_second_trip")
        if geo.vec and geo.tail_start < n:
            tags.add("tail_behind_vec")
        if v.grad_bf16:
            tags.add(("grad_bf16", geo.vec))
        if 1 < geo.nb < E.LOSS_BLOCK_CAP:
            tags.add("several_blocks")
        seen |= tags
    want = {("mode", m, bf, vec) for m in range(5) for bf in (False, True) for vec in (0, 1)}
    want |= {("relu", True, False), ("relu", True, True), ("b_none", True), ("no_grad", True), ("acc", True), ("acc", False),
             ("cap", 0), ("cap", 1), "vec_second_trip", "tail_second_trip", "tail_behind_vec", ("grad_bf16", 0), ("grad_bf16", 1),
             "several_blocks"}
    want |= {("shift", s, bf) for s in ((0, 0), (1, 0), (0, 1), (1, 1)) for bf in (False, True)}
    assert want <= seen, want - seen
    assert len({t for t in seen if t[0] == "lscale"}) >= 3 and len({t for t in seen if t[0] == "gscale"}) >= 3
    for n in E.LOSS_N:          # the mirror itself: one pass of the grid on either path
        for vec in (0, 1):
            g = E.loss_geometry(n, vec)
            assert g.nb == min(-(-n // 256), 1024) and g.one_pass == g.nb * 256 * (4 if vec else 1)


def test_pool_tables_reach_the_second_trip_and_every_extent():
    for (tile, reps) in E.MAXPOOL_BIG.values():
        N, H, W, C = tile
        total = E.groups(N, H // 2 * reps[0], W // 2 * reps[1], C)
        assert E.GRID_CAP < total < E.GRID_CAP + 4096, total             # just past the cap: the smallest size with a second trip
    tile, reps, (H, W) = E.AVG_BIG
    assert (E.avg_out(H), E.avg_out(W)) == (tile[1] * reps[0], tile[2] * reps[1]) and E.GRID_CAP < E.groups(1, H, W, tile[3]) < E.GRID_CAP + 4096
    hw = {(c[1], c[2]) for c in E.AVG_CASES}
    assert {h for h, _ in hw} >= {1, 2, 3, 4, 5, 7, 8} and {w for _, w in hw} >= {1, 2, 3, 4, 5, 7, 8}
    assert {(h % 2, w % 2) for h, w in hw} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert {(c[4], c[5]) for c in E.AVG_CASES} == {(False, False), (False, True), (True, False), (True, True)}
    assert {c[4] for c in E.DOWNSUM_CASES} == {0, 1, 2}
    for bf, shapes in E.POOL_SHAPES.items():
        assert shapes[0] == (1, 2, 2, 8 if bf else 4) and shapes[1][0] == 2 and (shapes[1][1] // 2) % 2 == 1 and (shapes[1][2] // 2) % 2 == 1


def test_batchnorm_table_reaches_every_edge():
    rem_after_run, never, nbs = set(), False, set()
    pb_off, short_last, capped = False, False, False
    for c in E.BN_BWD:
        npix = c.N * c.H * c.W
        g = E.bn_geometry(npix, c.C)
        nbs.add(g.nb)
        capped |= -(-npix // E.BN_ROW_PIXELS) > E.BN_ROWS and g.nb == E.BN_ROWS
        pb_off |= g.PB % g.R != 0
        short_last |= g.nb > 1 and g.blocks[-1][1] - g.blocks[-1][0] < g.PB
        for p0, p1, rows in g.blocks:
            assert sum(4 * it + rem for it, rem in rows) == p1 - p0              # the mirror visits every pixel once
            rem_after_run |= {rem for it, rem in rows if it > 0}
            never |= all(it == 0 for it, _ in rows)
            assert all(rem <= 3 for it, rem in rows if it > 0) and all(rem <= 3 for _, rem in rows)
    assert rem_after_run >= {0, 1, 2, 3} and never and pb_off and short_last and capped and nbs >= {1, 2, 3, 256}, \
        (rem_after_run, never, pb_off, short_last, capped, nbs)
    geo = {c.C: E.bn_geometry(c.N * c.H * c.W, c.C) for c in E.BN_BWD}
    assert set(geo) >= {4, 12, 13, 256, 1024, 1040}
    assert (geo[12].R, geo[12].idle) == (85, 1) and geo[13].C4 == 4 and geo[1024].R == 1 and (geo[1040].trips, geo[1040].last_trip) == (2, 4)
    assert any(c.sliced for c in E.BN_BWD) and any(c.dx_acc for c in E.BN_BWD) and any(c.dgb_acc for c in E.BN_BWD)
    assert any(c.N * c.H * c.W * ((c.C + 3) // 4) > E.GRID_CAP for c in E.BN_BWD)
    assert all(c.N * c.H * c.W <= 4096 or c.C <= 16 for c in E.BN_BWD), "large npix only with small C"


def test_cross_entropy_table():
    cs = E.CE_CASES
    assert {c[1] for c in cs} >= {1, 2, 13, 64} and {c[0] for c in cs} >= {1, 3} and {c[2] * c[3] for c in cs} >= {1, 255, 257}
    assert any(c[4] for c in cs) and any(E.CE_BLOCKS * 256 < c[0] * c[2] * c[3] <= E.CE_BLOCKS * 256 + 256 for c in cs)


# ---------------------------------------------------------------------------------------------------------------
# 5. seeded defects
# ---------------------------------------------------------------------------------------------------------------
def _loss_defect(defect):
    hit = 0
    for n, v, (a, b) in _fam_loss():
        if n > 2 ** 18 + 1 and defect not in ("skip_second_trip",):
            continue
        if defect == "skip_second_trip" and (n <= 2 ** 18 or v.mode != E.L1):
            continue
        r, bad = E.loss_ref(a, b, v), E.loss_ref(a, b, v, defect=defect)
        hit += not (_same(r["loss"], bad["loss"]) and _same(r["grad"], bad["grad"]))
    return hit


def _pool_defect(defect):
    hit = 0
    for _, xb, _, relu in E.MAXPOOL_BWD_ENTRIES:
        for shape in E.POOL_SHAPES[xb]:
            d = E.pool_case(*shape, not (xb or relu))
            hit += not _same(E.maxpool_bwd_ref(d["x"], d["dy"], relu), E.maxpool_bwd_ref(d["x"], d["dy"], relu, defect))
    return hit


def _avg_defect(defect):
    return sum(not _same(E.avgpool_bwd_ref(E.avg_case(*c[:5])["dy"], c[1], c[2], E.avg_case(*c[:5])["dx0"]),
                         E.avgpool_bwd_ref(E.avg_case(*c[:5])["dy"], c[1], c[2], E.avg_case(*c[:5])["dx0"], defect)) for c in E.AVG_CASES)


def _downsum_defect(defect, bf16_only=False):
    hit = 0
    for c in E.DOWNSUM_CASES:
        d = E.downsum_case(*c)
        good, bad = E.downsum_ref(d["dhi"], d["dlo0"]), E.downsum_ref(d["dhi"], d["dlo0"], defect)
        if c[4] == 2:
            good, bad = E.store_bf16(good), E.store_bf16(bad, defect)
        elif bf16_only:
            continue
        hit += not _same(good, bad)
    return hit


def _add_defect(defect):
    hit = 0
    for c in E.ADD_CASES:
        d = E.add_case(*c)
        good, bad = E.add_ref(d["a"], d["out0"], c[5]), E.add_ref(d["a"], d["out0"], c[5], defect)
        if c[4]:
            good, bad = E.store_bf16(good), E.store_bf16(bad, defect)
        hit += not _same(good, bad)
    return hit


def _bn_defect(defect):
    hit = 0
    for c in E.BN_BWD:
        if c.reps > 1:
            continue
        d = E.bn_case(c)
        bad = E.bn_sums_ref(c, d, defect)
        hit += not all(_same(d["ref"][k], bad[k]) for k in ("s1", "s2", "dgamma", "dbeta"))
    return hit


def _ce_defect(defect):
    hit = 0
    for case in E.CE_CASES:
        d = E.ce_case(case)
        r, bad = E.ce_ref(d["x"], d["t"], E.CE_GSCALE), E.ce_ref(d["x"], d["t"], E.CE_GSCALE, defect)
        hit += not (r["count"] == bad["count"] and r["loss_sum"] == bad["loss_sum"] and _same(r["mean"], bad["mean"]) and _same(r["grad"], bad["grad"]))
    return hit


DEFECTS = [("a dropped last tail element", lambda: _loss_defect("drop_tail")),
           ("a skipped element at the start of the second trip", lambda: _loss_defect("skip_second_trip")),
           ("x >= -1 at the hinge", lambda: _loss_defect("hinge_ge")),
           ("ReLU mask x >= 0", lambda: _loss_defect("relu_ge")),
           ("a truncating bf16 store (loss gradient)", lambda: _loss_defect("trunc_bf16")),
           ("a truncating bf16 store (down-sum)", lambda: _downsum_defect("trunc_bf16", True)),
           ("a truncating bf16 store (add_slice)", lambda: _add_defect("trunc_bf16")),
           ("an ignored accumulate (loss)", lambda: _loss_defect("ignore_accumulate")),
           ("an ignored accumulate (avg pool)", lambda: _avg_defect("ignore_accumulate")),
           ("an ignored accumulate (down-sum)", lambda: _downsum_defect("ignore_accumulate")),
           ("an ignored accumulate (add_slice)", lambda: _add_defect("ignore_accumulate")),
           ("an ignored accumulate (BatchNorm dgamma / dbeta)", lambda: _bn_defect("ignore_accumulate")),
           ("last-maximum routing", lambda: _pool_defect("last_max")),
           ("ReLU gate m >= 0", lambda: _pool_defect("gate_ge")),
           ("avg-pool count always 9", lambda: _avg_defect("count9")),
           ("a down-sum second-row offset of one pixel", lambda: _downsum_defect("row_offset")),
           ("the last pixel of a BN partial row dropped", lambda: _bn_defect("drop_row_end")),
           ("a pad channel leaking into dgamma", lambda: _bn_defect("pad_leak")),
           ("the second g0 trip reading the first trip's mean", lambda: _bn_defect("g0_mean")),
           ("ignored pixels counted", lambda: _ce_defect("count_ignored")),
           ("the ignored-pixel gradient not zeroed", lambda: _ce_defect("ignored_grad")),
           ("a sample stride of HW instead of C * HW", lambda: _ce_defect("sample_stride"))]


@pytest.mark.parametrize("name,run", DEFECTS, ids=[d[0] for d in DEFECTS])
def test_seeded_defect_changes_a_reference(name, run):
    hit = run()
    print(f"{name}: changes {hit} case(s)")
    assert hit >= 1, name


# ---------------------------------------------------------------------------------------------------------------
# the wrapper's layout contract
# ---------------------------------------------------------------------------------------------------------------
def test_maxpool2x2_bwd_refuses_a_sliced_act():
    """the entry points take ONE channel stride for x, dy and dx: a channel slice of a wider tensor must not get that far"""
    import hr_viton_amd  # noqa: F401
    from hr_viton_amd import ops, train_ops as T
    wide, dense = torch.zeros(1, 4, 4, 16), torch.zeros(1, 2, 2, 8)
    with pytest.raises(AssertionError, match="dense"):
        T.maxpool2x2_bwd(ops.Act(wide, 8, 4), ops.Act(dense, 8))
    with pytest.raises(AssertionError, match="dense"):
        T.maxpool2x2_bwd(ops.Act(torch.zeros(1, 4, 4, 8), 8), ops.Act(torch.zeros(1, 2, 2, 16), 8, 8))
