"""The sampling kernels against the float64 references of tests/sample_exact_cases.py (why the comparisons are exact, and the derived
bounds where they are not: that module's docstring; tests/test_sample_exact_cases_cpu.py proves the conditions on the references
alone and that these comparisons reject a dropped tap, a strict gradient mask, a wrong window cell, a skipped flush row, a shortened
candidate range and an ignored channel offset).

  warp adjoint (flow_warp_bwd_kernel, flow_warp_dsrc_tiled_kernel)   torch.equal: d_src into a pre-filled accumulator, d_flow with and
                                                                     without accumulation, each alone, default route and
                                                                     HRV_WARP_BWD_TILED=0
  warp forward (flow_warp_kernel)                                    torch.equal at odd extents; at even extents flow_up torch.equal,
                                                                     the output within warp_fwd_bound per element
  grid_sample NCHW forward / backward                                torch.equal through functional.grid_sample and autograd
  bilinear resize forward / adjoint                                  torch.equal wherever the fp32 and float64 matrices coincide
                                                                     (x2, x4, x8, /2, ...), else within resize_fwd_bound /
                                                                     resize_adjoint_bound per element
  nearest resize forward / adjoint, resize_planes nearest            torch.equal

Every Act operand is a slice (offset 4, 8 pad channels) of a poisoned tensor; everything outside the slice keeps its poison."""
import pytest
import torch

import sample_exact_cases as E
from test_gpu_norm_bwd_instances import POISON, _Buf

pytestmark = pytest.mark.gpu
F64 = torch.float64


def _mods():
    import hr_viton_amd  # noqa: F401
    from hr_viton_amd import _lib, functional, glue, ops, train_ops
    return _lib, ops, train_ops, functional, glue


def _act(ops, t, **kw):
    """t [N, H, W, C] (float64, CPU) as a slice of a poisoned tensor -> (Act, _Buf)"""
    b = _Buf(t.shape[0], t.shape[1], t.shape[2], t.shape[3], False, fill=t.cuda(), **kw)
    return ops.Act(b.t, b.C, b.coff), b


def _blank(ops, N, H, W, Cn):
    b = _Buf(N, H, W, Cn, False)
    return ops.Act(b.t, b.C, b.coff), b


def _val(b):
    return b.t[..., b.coff:b.coff + b.C].cpu()


def _intact(what, *bufs, inputs=()):
    torch.cuda.synchronize()
    for b in bufs:
        assert b.pad_intact(), f"{what}: written outside a slice"
    for b, t in inputs:
        assert b.pad_intact() and torch.equal(_val(b).double(), t), f"{what}: an input changed"


def _auto(got, want, exact, bnd, what):
    """torch.equal where the case is exact, the derived bound per element where it is not"""
    if exact:
        E.check_equal(got, want, what)
        return 0.0
    return E.check_bounded(got, want, bnd, what)


# ---------------------------------------------------------------------------------------------------------------
# group 1: warp adjoint
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", E.WARP_BWD_CASES, ids=lambda c: c.name)
def test_warp_adjoint_exact(c, monkeypatch):
    _lib, ops, T, _, _ = _mods()
    d, g = E.warp_bwd_case(c.name), c.geom
    ref = E.warp_reference(d["src"], d["flow_up"], g.norm_x, g.norm_y, d["dout"], d["old_dsrc"], d["old_dflow"])
    plain = ref["dflow"] - d["old_dflow"]
    fup = d["flow_up"].float().cuda().contiguous()
    for route in (None, "0"):                       # the default (tiled from 16 channels) and the per-pixel scatter
        if route is None:
            monkeypatch.delenv("HRV_WARP_BWD_TILED", raising=False)
        else:
            monkeypatch.setenv("HRV_WARP_BWD_TILED", route)
        _lib.reload_env()
        what = f"{c.name} route {route}"
        (sa, sb), (da, db) = _act(ops, d["src"]), _act(ops, d["dout"])
        ins = ((sb, d["src"]), (db, d["dout"]))
        # d_src into the accumulator and d_flow accumulated
        ga, gb = _act(ops, d["old_dsrc"])
        dflow = d["old_dflow"].float().cuda().contiguous()
        T.flow_warp_bwd(sa, fup, g.norm_x, g.norm_y, da, ga, dflow, True)
        _intact(what, gb, inputs=ins)
        E.check_equal(_val(gb), ref["dsrc"], what + " dsrc")
        E.check_equal(dflow, ref["dflow"], what + " dflow accumulated")
        # both, d_flow written
        ga, gb = _act(ops, d["old_dsrc"])
        dflow = torch.full_like(dflow, POISON)
        T.flow_warp_bwd(sa, fup, g.norm_x, g.norm_y, da, ga, dflow, False)
        _intact(what, gb, inputs=ins)
        E.check_equal(_val(gb), ref["dsrc"], what + " dsrc (2)")
        E.check_equal(dflow, plain, what + " dflow")
        # each alone
        ga, gb = _act(ops, d["old_dsrc"])
        T.flow_warp_bwd(sa, fup, g.norm_x, g.norm_y, da, ga, None)
        _intact(what, gb, inputs=ins)
        E.check_equal(_val(gb), ref["dsrc"], what + " dsrc alone")
        dflow = d["old_dflow"].float().cuda().contiguous()
        T.flow_warp_bwd(sa, fup, g.norm_x, g.norm_y, da, None, dflow, True)
        _intact(what, inputs=ins)
        E.check_equal(dflow, ref["dflow"], what + " dflow alone")


# ---------------------------------------------------------------------------------------------------------------
# groups 2 and 3: warp forward
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", E.WARP_FWD_EXACT + E.WARP_FWD_CONTRACT, ids=lambda c: c.name)
def test_warp_forward(c):
    _lib, ops, _, _, _ = _mods()
    d = E.warp_fwd_case(c)
    (sa, sb), (oa, ob) = _act(ops, d["src"]), _blank(ops, c.N, c.Ho, c.Wo, c.C)
    _, fup = ops.flow_warp(sa, d["flow"].float().cuda().contiguous(), c.Ho, c.Wo, 0.5, 0.5, c.norm_x, c.norm_y, out=oa)
    _intact(c.name, ob, inputs=((sb, d["src"]),))
    E.check_equal(fup, d["flow_up"], c.name + " flow_up")
    exact = c in E.WARP_FWD_EXACT
    worst = _auto(_val(ob), d["ref"]["out"], exact, None if exact else E.warp_fwd_bound(c, d), c.name + " out")
    print(f"{c.name}: {'exact' if exact else f'worst |error| / bound = {worst:.3g}'}")
    oa2, ob2 = _blank(ops, c.N, c.Ho, c.Wo, c.C)
    _, none = ops.flow_warp(sa, d["flow"].float().cuda().contiguous(), c.Ho, c.Wo, 0.5, 0.5, c.norm_x, c.norm_y, out=oa2, want_flow_up=False)
    torch.cuda.synchronize()
    assert none is None and torch.equal(ob2.t, ob.t), "the output does not depend on whether flow_up is wanted"


# ---------------------------------------------------------------------------------------------------------------
# group 4: grid_sample with an explicit grid
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", E.GRID_CASES, ids=lambda c: c.name)
def test_grid_sample_exact(c):
    _, _, _, HF, _ = _mods()
    d = E.grid_case(c)
    for need_in, need_grid in ((True, True), (True, False), (False, True)):
        inp = d["inp"].float().cuda().requires_grad_(need_in)
        grid = d["grid"].float().cuda().requires_grad_(need_grid)
        out = HF.grid_sample(inp, grid, padding_mode="border")
        E.check_equal(out, d["ref"]["out"], c.name + " out")
        out.backward(d["dout"].float().cuda())
        torch.cuda.synchronize()
        if need_in:
            E.check_equal(inp.grad, d["ref"]["din"], c.name + " din")
        if need_grid:
            E.check_equal(grid.grad, d["ref"]["dgrid"], c.name + " dgrid")
        assert (inp.grad is None) == (not need_in) and (grid.grad is None) == (not need_grid)
        assert torch.equal(inp.detach().cpu().double(), d["inp"]) and torch.equal(grid.detach().cpu().double(), d["grid"])


# ---------------------------------------------------------------------------------------------------------------
# group 5: bilinear resize
# ---------------------------------------------------------------------------------------------------------------
def _geom(hp, wp):
    (H, Ho, rh), (W, Wo, rw) = hp, wp
    return H, Ho, rh, W, Wo, rw


def _planes(t):
    """[N, H, W, C] float64 -> NCHW fp32 on the device"""
    return t.permute(0, 3, 1, 2).float().contiguous().cuda()


def _bilinear_forward(pairs, C, must_be_exact):
    _, ops, _, HF, glue = _mods()
    worst, n_exact = 0.0, 0
    for hp, wp in pairs:
        H, Ho, rh, W, Wo, rw = _geom(hp, wp)
        d = E.resize_case(hp, wp, C)
        Ry, Rx = E.bilinear_matrix(Ho, H, rh), E.bilinear_matrix(Wo, W, rw)
        want = E.resize_fwd(d["x"], Ry, Rx)
        exact = E.resize_is_exact(Ho, H, rh, Wo, W, rw, d["x"].abs() + 8, False)
        assert exact or not must_be_exact, (hp, wp)
        n_exact += exact
        what = f"bilinear {H}x{W} -> {Ho}x{Wo}"
        bnd = None if exact else E.resize_fwd_bound(d["x"], Ho, Wo, rh, rw)
        bnd_add = None if exact else E.resize_fwd_bound(d["x"], Ho, Wo, rh, rw, d["addend"])
        (xa, xb), (aa, ab) = _act(ops, d["x"]), _act(ops, d["addend"])
        ins = ((xb, d["x"]), (ab, d["addend"]))
        oa, ob = _blank(ops, d["x"].shape[0], Ho, Wo, C)
        ops.resize_bilinear(xa, Ho, Wo, rh, rw, out=oa)
        _intact(what, ob, inputs=ins)
        worst = max(worst, _auto(_val(ob), want, exact, bnd, what))
        oa, ob = _blank(ops, d["x"].shape[0], Ho, Wo, C)
        ops.resize_bilinear(xa, Ho, Wo, rh, rw, addend=aa, out=oa)
        _intact(what, ob, inputs=ins)
        worst = max(worst, _auto(_val(ob), want + d["addend"], exact, bnd_add, what + " + addend"))
        if rh == H / Ho and rw == W / Wo:                     # the size= form: the NCHW planes kernel takes in / out itself
            got = glue.resize_nchw(_planes(d["x"]), (Ho, Wo), "bilinear")
            worst = max(worst, _auto(got.permute(0, 2, 3, 1), want, exact, bnd, what + " planes"))
            got = HF.interpolate(_planes(d["x"]), size=(Ho, Wo), mode="bilinear")
            worst = max(worst, _auto(got.permute(0, 2, 3, 1), want, exact, bnd, what + " interpolate"))
    return worst, n_exact


def test_bilinear_forward_dyadic_ratios_exact():
    _bilinear_forward(E.dyadic_sweep(), 8, True)


def test_bilinear_forward_size_pairs():
    worst, n_exact = _bilinear_forward(E.sweep(), 4, False)
    print(f"bilinear forward: {n_exact} of {len(E.sweep())} pairs exact, worst |error| / bound of the others = {worst:.3g}")


def _bilinear_adjoint(pairs, must_be_exact):
    _, ops, T, HF, _ = _mods()
    worst, n_exact = 0.0, 0
    for k, (hp, wp) in enumerate(pairs):
        H, Ho, rh, W, Wo, rw = _geom(hp, wp)
        d = E.resize_case(hp, wp, 4)
        Ry, Rx = E.bilinear_matrix(Ho, H, rh), E.bilinear_matrix(Wo, W, rw)
        want = E.resize_adj(d["dy"], Ry, Rx)
        exact = E.resize_is_exact(Ho, H, rh, Wo, W, rw, d["dy"].abs() + 4, True)
        assert exact or not must_be_exact, (hp, wp)
        n_exact += exact
        acc = k % 2 == 1
        what = f"bilinear adjoint {Ho}x{Wo} -> {H}x{W} accumulate={int(acc)}"
        bnd = None if exact else E.resize_adjoint_bound(d["dy"], H, W, rh, rw)
        bnd_acc = None if exact else E.resize_adjoint_bound(d["dy"], H, W, rh, rw, d["old"])
        # VEC = 4: an Act; VEC = 1: the same Act at an odd stride and offset, and the dense 2-channel form
        for vec, kw in ((4, {}), (1, dict(pad=5, coff=3))):
            (ya, yb), (xa, xb) = _act(ops, d["dy"], **kw), _act(ops, d["old"], **kw)
            T.resize_bilinear_bwd(ya, H, W, rh, rw, dx=xa, accumulate=acc)
            _intact(what, xb, inputs=((yb, d["dy"]),))
            worst = max(worst, _auto(_val(xb), want + d["old"] if acc else want, exact, bnd_acc if acc else bnd, f"{what} VEC={vec}"))
        got = T.resize_bilinear_bwd_dense(d["dy"][..., :2].float().contiguous().cuda(), H, W, rh, rw)
        worst = max(worst, _auto(got, want[..., :2], exact, None if exact else bnd[..., :2], what + " dense"))
        got = T.resize_bilinear_bwd(ya, H, W, rh, rw)          # the adjoint allocates its own result
        worst = max(worst, _auto(got.t[..., :4], want, exact, bnd, what + " allocated"))
        if rh == H / Ho and rw == W / Wo:
            x = torch.zeros(d["old"].shape[0], 4, H, W, device="cuda", requires_grad=True)
            HF.interpolate(x, size=(Ho, Wo), mode="bilinear").backward(_planes(d["dy"]))
            worst = max(worst, _auto(x.grad.permute(0, 2, 3, 1), want, exact, bnd, what + " interpolate"))
    return worst, n_exact


def test_bilinear_adjoint_dyadic_ratios_exact():
    _bilinear_adjoint(E.dyadic_sweep(), True)


def test_bilinear_adjoint_size_pairs():
    """in 1..12 against out 1..96 and the 1 / scale_factor ratios, one launch per pair, different pairs in H and W"""
    worst, n_exact = _bilinear_adjoint(E.sweep(), False)
    print(f"bilinear adjoint: {n_exact} of {len(E.sweep())} pairs exact, worst |error| / bound of the others = {worst:.3g}")


# ---------------------------------------------------------------------------------------------------------------
# group 6: nearest resize
# ---------------------------------------------------------------------------------------------------------------
def test_nearest_size_pairs_exact():
    _, ops, T, HF, glue = _mods()
    size_pairs = [(hp, wp) for hp, wp in E.sweep() if hp in E.SIZE_PAIRS and wp in E.SIZE_PAIRS]
    assert len(size_pairs) >= 40
    for k, (hp, wp) in enumerate(size_pairs):
        H, Ho, _, W, Wo, _ = _geom(hp, wp)
        d = E.resize_case(hp, wp, 4)
        Sy, Sx = E.nearest_matrix(Ho, H), E.nearest_matrix(Wo, W)
        fwd, adj = E.resize_fwd(d["x"], Sy, Sx), E.resize_adj(d["dy"], Sy, Sx)
        what = f"nearest {H}x{W} <-> {Ho}x{Wo}"
        N = d["x"].shape[0]
        (xa, xb), (aa, ab), (ya, yb) = _act(ops, d["x"]), _act(ops, d["addend"]), _act(ops, d["dy"])
        ins = ((xb, d["x"]), (ab, d["addend"]), (yb, d["dy"]))
        oa, ob = _blank(ops, N, Ho, Wo, 4)
        ops.resize_nearest(xa, Ho, Wo, out=oa)
        _intact(what, ob, inputs=ins)
        E.check_equal(_val(ob), fwd, what + " forward")
        oa, ob = _blank(ops, N, Ho, Wo, 4)
        ops.resize_nearest(xa, Ho, Wo, addend=aa, out=oa)
        _intact(what, ob, inputs=ins)
        E.check_equal(_val(ob), fwd + d["addend"], what + " forward + addend")
        E.check_equal(ops.resize_nearest_dense(d["x"][..., :2].float().contiguous().cuda(), Ho, Wo), fwd[..., :2], what + " dense")
        acc = k % 2 == 1
        ga, gb = _act(ops, d["old"])
        T.resize_nearest_bwd(ya, H, W, dx=ga, accumulate=acc)
        _intact(what, gb, inputs=ins)
        E.check_equal(_val(gb), adj + d["old"] if acc else adj, what + f" adjoint accumulate={int(acc)}")
        E.check_equal(T.resize_nearest_bwd(ya, H, W).t[..., :4], adj, what + " adjoint allocated")
        E.check_equal(T.resize_nearest_bwd_dense(d["dy"][..., :2].float().contiguous().cuda(), H, W), adj[..., :2], what + " adjoint dense")
        E.check_equal(glue.resize_nchw(_planes(d["x"]), (Ho, Wo), "nearest").permute(0, 2, 3, 1), fwd, what + " planes")
        x = _planes(d["x"]).requires_grad_(True)
        y = HF.interpolate(x, size=(Ho, Wo), mode="nearest")
        y.backward(_planes(d["dy"]))
        E.check_equal(y.permute(0, 2, 3, 1), fwd, what + " interpolate")
        E.check_equal(x.grad.permute(0, 2, 3, 1), adj, what + " interpolate adjoint")
