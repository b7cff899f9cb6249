"""The conditions tests/test_gpu_sample_exact.py rests on, proved on the references of tests/sample_exact_cases.py alone (no GPU, no
project import): every exact case is exact (the fp32 restatement of the coordinate and weight arithmetic equals the float64 one bit
for bit and every sum obeys the 2^22 rule), the references agree with float64 F.grid_sample / F.interpolate and autograd, the
edges the cases claim are there, the derived bounds leave room, and the comparison functions reject each injected fault."""
import pytest
import torch
import torch.nn.functional as F

import sample_exact_cases as E

F64, F32 = E.F64, E.F32
POISON = 1.5e4
TILED = [c for c in E.WARP_BWD_CASES if c.C >= 16]


def _close(a, b, what):
    assert a.shape == b.shape, what
    assert float((a - b).abs().max()) <= 1e-10 * max(1.0, float(b.abs().max())), f"{what}: {float((a - b).abs().max())}"


def _warp_ref(d, **kw):
    g = d["case"].geom
    return E.warp_reference(d["src"], d["flow_up"], g.norm_x, g.norm_y, d["dout"], d["old_dsrc"], d["old_dflow"], **kw)


# ---------------------------------------------------------------------------------------------------------------
# exactness
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 16, 17, 24, 32, 33, 48])
def test_the_base_grid_is_torch_linspace(n):
    """bit for bit in float64 and, at the dyadic extents, in fp32; elsewhere torch's own fp32 evaluation may round differently, within
    the 3 u that `warp_delta` allows the base grid"""
    assert float((E.linspace_m1_1(n, F64) - torch.linspace(-1, 1, n, dtype=F64)).abs().max()) <= 2.0 ** -51, n
    got, want = E.linspace_m1_1(n, F32), torch.linspace(-1, 1, n, dtype=F32)
    if n in (2, 17, 33):
        assert torch.equal(E.linspace_m1_1(n, F64), torch.linspace(-1, 1, n, dtype=F64))
        assert torch.equal(got, want) and torch.equal(got.double(), E.linspace_m1_1(n, F64)), n
    assert float((got.double() - E.linspace_m1_1(n, F64)).abs().max()) <= 3 * E.U and float((got - want).abs().max()) <= 3 * E.U


@pytest.mark.parametrize("c", E.WARP_BWD_CASES, ids=lambda c: c.name)
def test_warp_adjoint_case_is_exact(c):
    d = E.warp_bwd_case(c.name)
    g = c.geom
    assert torch.equal(d["flow_up"].float().double(), d["flow_up"]), "the flow is an fp32 number"
    assert E.same_taps(E.warp_case_taps(d, F32), E.warp_case_taps(d, F64))
    got = E.warp_bound(d["src"], d["flow_up"], g.norm_x, g.norm_y, d["dout"], d["old_dsrc"], d["old_dflow"], c.name)
    print(c.name, {k: f"2^{torch.tensor(max(v, 1.0)).log2().item():.1f}" for k, v in got.items()})


@pytest.mark.parametrize("c", E.WARP_FWD_EXACT, ids=lambda c: c.name)
def test_warp_forward_case_is_exact(c):
    d = E.warp_fwd_case(c)
    up32 = torch.einsum("oi,nijc,qj->noqc", E.bilinear_matrix(c.Ho, c.fh, 0.5, F32).float(), d["flow"].float(),
                        E.bilinear_matrix(c.Wo, c.fw, 0.5, F32).float())
    assert torch.equal(up32.double(), d["flow_up"]), "the x2 up-sampling of the flow is exact in fp32"
    assert torch.equal(E.bilinear_matrix(c.Ho, c.fh, 0.5, F32), E.bilinear_matrix(c.Ho, c.fh, 0.5))
    t32 = E.taps(*E.coords(d["flow_up"], c.H, c.W, c.norm_x, c.norm_y, F32), c.H, c.W)
    assert E.same_taps(t32, d["ref"]["taps"])
    a = E.sample(d["src"], d["ref"]["taps"], absolute=True)
    E.bound({"out": (a["out"], E.finest_step(*[w for _, _, w, _ in E._four(t32)]))}, c.name)
    # the kernel's documented source index holds the taps inside the flow: i1 <= fh - 1 without the clamp
    assert int(0.5 * (c.Ho - 1 + 0.5) - 0.5) + 1 <= c.fh - 1 and int(0.5 * (c.Wo - 1 + 0.5) - 0.5) + 1 <= c.fw - 1


@pytest.mark.parametrize("c", E.GRID_CASES, ids=lambda c: c.name)
def test_grid_case_is_exact_and_is_torch(c):
    d = E.grid_case(c)
    assert torch.equal(d["grid"].float().double(), d["grid"])
    assert E.same_taps(E.grid_taps(c, d["grid"], F32), E.grid_taps(c, d["grid"], F64))
    E.grid_bound(c, d)
    inp, grid = d["inp"].clone().requires_grad_(True), d["grid"].clone().requires_grad_(True)
    out = F.grid_sample(inp, grid, mode="bilinear", padding_mode="border", align_corners=False)
    out.backward(d["dout"])
    _close(d["ref"]["out"], out.detach(), "out")
    _close(d["ref"]["din"], inp.grad, "din")
    _close(d["ref"]["dgrid"], grid.grad, "dgrid")


@pytest.mark.parametrize("c", E.WARP_BWD_CASES, ids=lambda c: c.name)
def test_warp_reference_is_torch(c):
    d = E.warp_bwd_case(c.name)
    g = c.geom
    src = d["src"].permute(0, 3, 1, 2).clone().requires_grad_(True)
    flow = d["flow_up"].clone().requires_grad_(True)
    grid = torch.stack([flow[..., 0] / g.norm_x + torch.linspace(-1, 1, g.Wo, dtype=F64)[None, None, :],
                        flow[..., 1] / g.norm_y + torch.linspace(-1, 1, g.Ho, dtype=F64)[None, :, None]], -1)
    out = F.grid_sample(src, grid, mode="bilinear", padding_mode="border", align_corners=False)
    out.backward(d["dout"].permute(0, 3, 1, 2))
    r = E.warp_reference(d["src"], d["flow_up"], g.norm_x, g.norm_y, d["dout"])
    _close(r["out"], out.detach().permute(0, 2, 3, 1), "out")
    _close(r["dsrc"], src.grad.permute(0, 2, 3, 1), "dsrc")
    _close(r["dflow"], flow.grad, "dflow")


@pytest.mark.parametrize("c", E.WARP_FWD_EXACT + E.WARP_FWD_CONTRACT, ids=lambda c: c.name)
def test_warp_forward_reference_is_torch(c):
    d = E.warp_fwd_case(c)
    fup = F.interpolate(d["flow"].permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
    if c.Ho == 2 * c.fh:                       # (torch cannot express the odd extents: (Ho + 1) / 2 rows at ratio 0.5)
        _close(d["flow_up"], fup, "flow_up")
    grid = torch.stack([d["flow_up"][..., 0] / c.norm_x + torch.linspace(-1, 1, c.Wo, dtype=F64)[None, None, :],
                        d["flow_up"][..., 1] / c.norm_y + torch.linspace(-1, 1, c.Ho, dtype=F64)[None, :, None]], -1)
    out = F.grid_sample(d["src"].permute(0, 3, 1, 2), grid, mode="bilinear", padding_mode="border", align_corners=False)
    _close(d["ref"]["out"], out.permute(0, 2, 3, 1), "out")


# ---------------------------------------------------------------------------------------------------------------
# the edges are present
# ---------------------------------------------------------------------------------------------------------------
def _census_ok(cen, what):
    for k in ("x_lo", "x_hi", "y_lo", "y_hi"):
        assert cen[k] >= 8, (what, k, cen)
    assert cen["x_int"] >= 0.05 * cen["total"] and cen["y_int"] >= 0.05 * cen["total"], (what, cen)
    assert cen["interior"] >= 0.4 * cen["total"], (what, cen)


def test_the_adjoint_tables_reach_their_edges():
    cen = None
    for c in E.WARP_BWD_CASES:
        d = E.warp_bwd_case(c.name)
        g = c.geom
        one = E.edge_census(*E.coords(d["flow_up"], g.H, g.W, g.norm_x, g.norm_y, F64), g.H, g.W)
        cen = one if cen is None else E.add_census(cen, one)
        if c.pattern == "edges":
            _census_ok(one, c.name)
    _census_ok(cen, "warp table")
    cen = None
    for c in E.GRID_CASES:
        d = E.grid_case(c)
        one = E.edge_census(E.unnormalise(d["grid"][..., 0], c.W, F64), E.unnormalise(d["grid"][..., 1], c.H, F64), c.H, c.W)
        cen = one if cen is None else E.add_census(cen, one)
    _census_ok(cen, "grid table")
    print("grid table", cen)


def test_the_tiles_fit_and_do_not_fit_where_claimed():
    seen = set()
    for c in TILED:
        tl = E.tiles(E.warp_case_taps(E.warp_bwd_case(c.name)))
        g = c.geom
        assert len(tl) == c.N * 6 and min(t.live for t in tl) == 1 and max(t.live for t in tl) == 256, "ragged last tiles"
        first = [t for t in tl if (t.ty if g.H > g.W else t.tx) == 0]
        rest = [t for t in tl if t not in first]
        span = lambda t: (t.y_hi - t.y_lo) if g.H > g.W else (t.x_hi - t.x_lo)
        if c.pattern in ("smooth", "corner"):
            assert all(t.fits for t in tl), c.name
        if c.pattern == "edges":             # both far borders in the first rows / columns: those tiles fall back, the others --
            assert not any(t.fits for t in first) and all(t.fits for t in rest), c.name     # with the border hits of the other axis -- fit
        if c.pattern == "spread":
            assert not any(t.fits for t in first) and all(t.fits for t in rest) and all(span(t) == 31 for t in first), c.name
        if c.pattern == "bb23":
            assert all(t.fits and span(t) == 23 for t in first) and all(t.fits for t in rest), c.name
        if c.pattern == "bb24":
            assert all((not t.fits) and span(t) == 24 for t in first) and all(t.fits for t in rest), c.name
        if c.pattern in ("spread", "bb23", "bb24"):
            seen.add((c.pattern, "y" if g.H > g.W else "x"))
        assert E.WB == 24 and E.WT == 16
    assert seen == {(p, a) for p in ("spread", "bb23", "bb24") for a in "xy"}
    chunks = sorted({c.C for c in E.WARP_BWD_CASES})
    assert {4, 12}.issubset(chunks) and 16 in chunks and {24, 40}.issubset(chunks) and 68 in chunks
    assert [c % E.WCH for c in (24, 40, 68)] == [8, 8, 4] and -(-68 // E.WCH) == 5


# ---------------------------------------------------------------------------------------------------------------
# the resizes
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scaled", [False, True], ids=["size", "scale_factor"])
def test_resize_matrices_are_torch(scaled):
    for (i, o, r) in (E.SCALED_PAIRS if scaled else E.SIZE_PAIRS):
        x = torch.arange(i * 3, dtype=F64).reshape(1, 1, i, 3).mul(0.37).sin().requires_grad_(True)
        kw = dict(scale_factor=(1 / r, 1.0)) if scaled else dict(size=(o, 3))
        y = F.interpolate(x, mode="bilinear", align_corners=False, **kw)
        assert y.shape[2] == o
        dy = torch.arange(o * 3, dtype=F64).reshape(1, 1, o, 3).mul(0.11).cos()
        y.backward(dy)
        R, I3 = E.bilinear_matrix(o, i, r), torch.eye(3, dtype=F64)
        _close(E.resize_fwd(x.detach().permute(0, 2, 3, 1), R, I3), y.detach().permute(0, 2, 3, 1), f"bilinear {i}->{o}")
        _close(E.resize_adj(dy.permute(0, 2, 3, 1), R, I3), x.grad.permute(0, 2, 3, 1), f"bilinear adjoint {i}->{o}")
        if not scaled:
            x2 = x.detach().clone().requires_grad_(True)
            y2 = F.interpolate(x2, size=(o, 3), mode="nearest")
            y2.backward(dy)
            S = E.nearest_matrix(o, i)
            assert torch.equal(E.resize_fwd(x2.detach().permute(0, 2, 3, 1), S, I3), y2.detach().permute(0, 2, 3, 1)), (i, o)
            _close(E.resize_adj(dy.permute(0, 2, 3, 1), S, I3), x2.grad.permute(0, 2, 3, 1), f"nearest adjoint {i}->{o}")


def test_the_dyadic_ratios_are_exact():
    for hp, wp in E.dyadic_sweep():
        d = E.resize_case(hp, wp, 8)
        (H, Ho, rh), (W, Wo, rw) = hp, wp
        assert E.resize_is_exact(Ho, H, rh, Wo, W, rw, d["x"].abs() + 0, False) and E.resize_is_exact(Ho, H, rh, Wo, W, rw, d["dy"].abs() + 4, True), (hp, wp)
    exact = [p for p in E.sweep() if E.resize_is_exact(p[0][1], p[0][0], p[0][2], p[1][1], p[1][0], p[1][2], E.resize_case(p[0], p[1], 4)["dy"].abs() + 4, True)]
    print(f"{len(exact)} of {len(E.sweep())} pairs of the sweep are exact")
    assert 5 <= len(exact) < len(E.sweep())
    assert 1 in E.INS and 1 in E.OUTS and 96 in E.OUTS


def test_the_candidate_range_misses_no_contributor():
    for (i, o, r) in E.ALL_PAIRS:
        assert torch.equal(E.gather_matrix(o, i, r), E.bilinear_matrix(o, i, r, F32)), (i, o)


# ---------------------------------------------------------------------------------------------------------------
# the derived bounds leave room
# ---------------------------------------------------------------------------------------------------------------
def _sample_f32(src, t):
    """the four-tap sum in fp32, taps in the kernel's order"""
    N, H, W, Cc = src.shape
    n_idx = torch.arange(N)[:, None, None].expand_as(t.x0)
    out = torch.zeros(t.x0.shape + (Cc,), dtype=F32)
    for dy, dx, w, ok in E._four(t):
        v = src.float()[n_idx, (t.y0 + dy).clamp_max(H - 1), (t.x0 + dx).clamp_max(W - 1)] * ok[..., None].float()
        out = out + v * w[..., None]
    return out


def _resize_f32(x, ty, tx):
    """the bilinear resize in fp32, tap by tap (both taps of the far border, or of a 1-pixel input, read the same pixel)"""
    x = x.float()
    (y0, y1, a0, a1, _), (x0, x1, b0, b1, _) = ty, tx
    at = lambda iy, ix: x[:, iy][:, :, ix]
    a0, a1, b0, b1 = a0[None, :, None, None], a1[None, :, None, None], b0[None, None, :, None], b1[None, None, :, None]
    return a0 * (b0 * at(y0, x0) + b1 * at(y0, x1)) + a1 * (b0 * at(y1, x0) + b1 * at(y1, x1))


def test_the_bounds_leave_room():
    worst = {"warp": 0.0, "resize_fwd": 0.0, "resize_adj": 0.0}
    for c in E.WARP_FWD_CONTRACT:
        d = E.warp_fwd_case(c)
        t32 = E.taps(*E.coords(d["flow_up"], c.H, c.W, c.norm_x, c.norm_y, F32), c.H, c.W)
        assert not E.same_taps(t32, d["ref"]["taps"]), "an even extent is off the dyadic grid"
        worst["warp"] = max(worst["warp"], E.check_bounded(_sample_f32(d["src"], t32), d["ref"]["out"], E.warp_fwd_bound(c, d), c.name))
    inexact = 0
    for hp, wp in E.sweep():
        (H, Ho, rh), (W, Wo, rw) = hp, wp
        d = E.resize_case(hp, wp, 4)
        Ry, Rx = E.bilinear_matrix(Ho, H, rh), E.bilinear_matrix(Wo, W, rw)
        Ry32, Rx32 = E.bilinear_matrix(Ho, H, rh, F32).float(), E.bilinear_matrix(Wo, W, rw, F32).float()
        inexact += not (E.same_bilinear_taps(Ho, H, rh) and E.same_bilinear_taps(Wo, W, rw))
        f32 = _resize_f32(d["x"], E.bilinear_taps(Ho, H, rh, F32), E.bilinear_taps(Wo, W, rw, F32)) + d["addend"].float()
        worst["resize_fwd"] = max(worst["resize_fwd"], E.check_bounded(f32, E.resize_fwd(d["x"], Ry, Rx) + d["addend"],
                                                                       E.resize_fwd_bound(d["x"], Ho, Wo, rh, rw, d["addend"]), f"fwd {hp} {wp}"))
        a32 = torch.einsum("oi,noqc,qj->nijc", Ry32, d["dy"].float(), Rx32) + d["old"].float()
        worst["resize_adj"] = max(worst["resize_adj"], E.check_bounded(a32, E.resize_adj(d["dy"], Ry, Rx) + d["old"],
                                                                       E.resize_adjoint_bound(d["dy"], H, W, rh, rw, d["old"]), f"adj {hp} {wp}"))
    print("largest fraction of a bound in use:", {k: round(v, 3) for k, v in worst.items()}, f"({inexact} inexact pairs)")
    assert inexact >= 20
    assert all(0.0 < v <= 0.5 for v in worst.values()), worst


# ---------------------------------------------------------------------------------------------------------------
# the assertions bite
# ---------------------------------------------------------------------------------------------------------------
def _rejected(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


def test_a_dropped_tap_is_rejected():
    hits = 0
    for c in E.WARP_BWD_CASES:
        d = E.warp_bwd_case(c.name)
        want = _warp_ref(d)
        for k in range(4):
            got = _warp_ref(d, dtype=F32, drop_tap=k)
            hits += _rejected(lambda: E.check_equal(got["dsrc"], want["dsrc"], "dsrc")) and _rejected(lambda: E.check_equal(got["out"], want["out"], "out"))
    assert hits >= 4 * (len(E.WARP_BWD_CASES) - 2)         # (a tap of the all-clamped cases may carry no weight)
    for c in E.GRID_CASES:
        d = E.grid_case(c)
        got = E.grid_reference(d["inp"], d["grid"], d["dout"], F32, drop_tap=3)
        assert _rejected(lambda: E.check_equal(got["out"], d["ref"]["out"], "out")) and _rejected(lambda: E.check_equal(got["din"], d["ref"]["din"], "din"))


def test_the_fp32_restatement_passes_where_the_faults_fail():
    for c in E.WARP_BWD_CASES:
        d = E.warp_bwd_case(c.name)
        want, got = _warp_ref(d), _warp_ref(d, dtype=F32)
        for k in ("out", "dsrc", "dflow"):
            E.check_equal(got[k], want[k], f"{c.name} {k}")


def test_a_strict_gradient_mask_is_rejected():
    hits = []
    for c in E.WARP_BWD_CASES:
        d = E.warp_bwd_case(c.name)
        if _rejected(lambda: E.check_equal(_warp_ref(d, dtype=F32, strict_mask=True)["dflow"], _warp_ref(d)["dflow"], "dflow")):
            hits.append(c.name)
    assert any("edges" in h for h in hits) and len(hits) >= 5, hits
    for c in E.GRID_CASES:
        d = E.grid_case(c)
        got = E.grid_reference(d["inp"], d["grid"], d["dout"], F32, strict_mask=True)
        assert _rejected(lambda: E.check_equal(got["dgrid"], d["ref"]["dgrid"], "dgrid")) == c.placed, c.name


def test_a_wrong_window_is_rejected():
    hits = {"cell": [], "flush_row": []}
    for c in TILED:
        d = E.warp_bwd_case(c.name)
        g, t, want = c.geom, E.warp_case_taps(d, F32), _warp_ref(d)["dsrc"]
        E.check_equal(E.tiled_dsrc_model(g.H, g.W, t, d["dout"], d["old_dsrc"]), want, c.name)
        for f in hits:
            if _rejected(lambda: E.check_equal(E.tiled_dsrc_model(g.H, g.W, t, d["dout"], d["old_dsrc"], fault=f), want, c.name)):
                hits[f].append(c.name)
    assert sorted(hits["cell"]) == sorted(c.name for c in TILED if c.pattern == "bb24"), hits["cell"]      # only the 24 cases see it
    assert len(hits["flush_row"]) >= len(TILED) - 2, hits["flush_row"]


def test_a_shortened_candidate_range_is_rejected():
    for fault in ("lo", "hi"):
        hits = 0
        for hp, wp in E.sweep():
            (H, Ho, rh), (W, Wo, rw) = hp, wp
            d = E.resize_case(hp, wp, 4)
            want = E.resize_adj(d["dy"], E.bilinear_matrix(Ho, H, rh), E.bilinear_matrix(Wo, W, rw)) + d["old"]
            got = E.resize_adj(d["dy"], E.gather_matrix(Ho, H, rh, fault), E.gather_matrix(Wo, W, rw, fault)) + d["old"]
            if E.resize_is_exact(Ho, H, rh, Wo, W, rw, d["dy"].abs() + 4, True):
                hits += _rejected(lambda: E.check_equal(got, want, "adjoint"))
            else:
                hits += _rejected(lambda: E.check_bounded(got, want, E.resize_adjoint_bound(d["dy"], H, W, rh, rw, d["old"]), "adjoint"))
        print(f"range shortened at {fault}: rejected on {hits} of {len(E.sweep())} pairs")
        assert hits >= 10, (fault, hits)


def test_an_ignored_channel_offset_is_rejected():
    c = E.WARP_BWD_CASES[0]
    d = E.warp_bwd_case(c.name)
    g = c.geom
    wide = torch.full((c.N, g.H, g.W, c.C + 8), POISON, dtype=F64)
    wide[..., 4:4 + c.C] = d["src"]
    for coff, fails in ((4, False), (0, True)):
        got = E.warp_reference(wide[..., coff:coff + c.C], d["flow_up"], g.norm_x, g.norm_y, dtype=F32)["out"]
        assert _rejected(lambda: E.check_equal(got, _warp_ref(d)["out"], "out")) == fails
    # ... and a write that ignores it lands outside the slice
    before = torch.full((c.N, g.Ho, g.Wo, c.C + 8), POISON, dtype=F32)
    good, bad = before.clone(), before.clone()
    good[..., 4:4 + c.C] = 1.0
    bad[..., 0:c.C] = 1.0
    E.check_outside(good, before, 4, c.C, "out")
    assert _rejected(lambda: E.check_outside(bad, before, 4, c.C, "out"))
    hp, wp = E.dyadic_sweep()[0]
    r = E.resize_case(hp, wp, 8)
    wide = torch.full(r["dy"].shape[:3] + (16,), POISON, dtype=F64)
    wide[..., 4:12] = r["dy"]
    Ry, Rx = E.bilinear_matrix(hp[1], hp[0], hp[2]), E.bilinear_matrix(wp[1], wp[0], wp[2])
    assert _rejected(lambda: E.check_equal(E.resize_adj(wide[..., 0:8], Ry, Rx), E.resize_adj(r["dy"], Ry, Rx), "adjoint"))
