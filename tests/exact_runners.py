"""The bodies of the zero-tolerance tests as functions ``run_<family>(case, ...)``: one case of tests/exact_cases.py (or of
tests/spade_uniform_cases.py) through its HIP kernel, against the float64 reference with torch.equal.  Callers:
tests/test_gpu_exact_integer.py and tests/test_gpu_spade_uniform.py at the device's own grid, tests/test_gpu_small_grid.py with the
persistent grid cut to 8 CUs.  Nothing here knows the grid: a runner asserts the same bits whatever the launch plan was.

``LOCATE[0]``: an optional callable (index tuple of a mismatch) -> str that a caller sets around a run; ``_assert_exact`` appends
what it returns to each printed mismatch (the small-grid tests name the tile, the block and the unit's position in its run)."""
import torch

import exact_cases as E
import spade_uniform_cases as U

LOCATE = [None]


def _mods():
    import hr_viton_amd  # noqa: F401
    from hr_viton_amd import _lib, ops, train_ops as T
    return ops, T, _lib


def _setenv(monkeypatch, **kw):
    from hr_viton_amd import _lib
    for k, v in kw.items():
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, str(v))
    _lib.reload_env()


class _mixed:
    def __init__(self, on=True):
        self.on = on

    def __enter__(self):
        from hr_viton_amd import train_ops as T
        self.T, self.old = T, T.MMA_BF16[0]
        T.MMA_BF16[0] = self.on

    def __exit__(self, *a):
        self.T.MMA_BF16[0] = self.old
        return False


def _bf(t):
    return t.to(torch.bfloat16).cuda()


def _assert_exact(what, got, ref64, bf16):
    """``got`` (device, NHWC or any layout ``ref64`` shares) against the float64 reference: torch.equal on values; bf16-stored
    outputs against the nearest-even rounding of the reference.  Prints the count and the first mismatches."""
    got = got.detach().cpu()
    assert got.dtype == (torch.bfloat16 if bf16 else torch.float32), (what, got.dtype)
    want = E.to_bf16_rne(ref64) if bf16 else ref64.to(torch.float32)
    if not bf16:
        assert torch.equal(want.double(), ref64), what
    assert got.shape == want.shape, (what, got.shape, want.shape)
    g, w = got.float(), want.float()
    if torch.equal(g, w):
        return
    bad = (g != w).nonzero()
    lines = [f"{what}: {bad.shape[0]} of {g.numel()} differ (index..., got, want, float64 reference)"]
    for ix in bad[:8].tolist():
        t = tuple(ix)
        where = f"  [{LOCATE[0](t)}]" if LOCATE[0] is not None else ""
        lines.append(f"  {t}: got {g[t].item()!r} want {w[t].item()!r} ref {ref64[t].item()!r}{where}")
    if LOCATE[0] is not None:
        lines[0] += " -- first at " + LOCATE[0](tuple(bad[0].tolist()))
    print("\n".join(lines))
    raise AssertionError(lines[0])


def _cpad(C, bf16):
    g = 8 if bf16 else 4
    return (C + g - 1) // g * g


def _sentinel(N, H, W, C, bf16, lo=8, hi=8):
    """An output slice [lo, lo + C) of a wider tensor filled with 7 (the slice keeps its channels padded to one 16-byte group)."""
    ops, _, _ = _mods()
    t = torch.full((N, H, W, lo + _cpad(C, bf16) + hi), 7.0, device="cuda", dtype=torch.bfloat16 if bf16 else torch.float32)
    return t, ops.Act(t, C, lo)


def _untouched(t, lo, C, pad_zero=True):
    """The neighbours of the slice still hold the sentinel; the slice's own pad channels hold zeros (``pad_zero``: kernels that store
    whole 16-byte groups) or the sentinel (the generic engine's scalar epilogue stops at the last real channel)."""
    Cp = _cpad(C, t.dtype == torch.bfloat16)
    pad = t[..., lo + C:lo + Cp]
    return (bool((t[..., :lo] == 7.0).all()) and bool((t[..., lo + Cp:] == 7.0).all()) and
            bool((pad == (0.0 if pad_zero else 7.0)).all()))


def _assert_wraps(fam, case):
    """``case`` is the family's case with more tiles than resident blocks (two per CU; spade_gb: one): the persistent loop of a block
    runs over several tiles instead of one (tile, pass) unit per block."""
    _, _, lib = _mods()
    if E.WRAP[fam][0] == case:
        cus = int(lib.load().hrv_persistent_cus())
        assert E.wrap_tiles(fam) > (1 if fam.startswith("gb_") else 2) * cus, (fam, E.wrap_tiles(fam), cus)


def _kernels(recs):
    return [r[5] for r in recs if r[0] in ("conv", "wgrad")]


# ---------------------------------------------------------------------------------------------------------------
# generic engine, bf16 tiles
# ---------------------------------------------------------------------------------------------------------------
def run_engine(case, cfg, monkeypatch=None, splitk=0):
    ops, T, _lib = _mods()
    name, _, Cin, Cout, k, N, H, W, out_bf16, act, res, wscale, sigma = case
    d = E.engine(case)
    x = ops.Act(_bf(d["xall"]), Cin, d["coff"])
    w, b = d["w"].cuda(), d["b"].cuda()
    sg = None if sigma is None else torch.tensor([sigma], device="cuda")
    r = None
    if res:
        r = ops.Act(_bf(d["res"]) if res == "bf16" else d["res"].cuda(), Cout)
    oall, out = _sentinel(N, H, W, Cout, out_bf16)
    a = {None: ops.ACT_NONE, "relu": ops.ACT_RELU, "lrelu": ops.ACT_LRELU}[act]
    packed, _ = T.pack_weight_dev(w, [x.Cp], [x.C], cfg, 0, 1, k // 2, wscale=wscale, sigma=sg, bf16=True)
    lib = _lib.load()
    asked, real = [], lib.hrv_conv2d_workspace_bytes

    def spy(d):
        asked.append(int(real(d)))
        return asked[-1]

    if monkeypatch is not None:
        monkeypatch.setattr(lib, "hrv_conv2d_workspace_bytes", spy)
    ops.profile_begin()
    T._run_engine([(x, 0, x.C)], packed, Cout, cfg, N, H, W, H, W, k, k, 1, k // 2, k // 2, out, shift=b, residual=r, act=a, slope=0.5,
                  name=name, mma_bf16=True)
    recs = ops.profile_end(kernels=True)
    assert _kernels(recs) == [f"conv_mfma_kernel[tile {cfg}]"], recs
    if monkeypatch is not None:
        # the split really happened: the launch path splits only into a workspace of the size it asked for (min(splitk, K-tiles)
        # partial planes of M x padded columns), which _run_engine then hands it; split-K off asks for none
        M, bn = N * H * W, lib.hrv_conv2d_tile_bn(cfg)
        assert len(asked) == 1 and (asked[0] == 0 if splitk <= 1 else asked[0] >= 2 * M * ((Cout + bn - 1) // bn * bn) * 4), (asked, splitk)
    _assert_exact(name, oall[..., 8:8 + Cout], d["want"]["out"], out_bf16)
    assert _untouched(oall, 8, Cout, pad_zero=False), name


def run_engine_probe(case):
    """The probe of test_gpu_exact_integer.py's docstring: the plain generic bf16 tile at its default configuration."""
    ops, T, _ = _mods()
    from hr_viton_amd.conv_dispatch import engine_tile
    _, _, Cin, Cout, k, N, H, W = case[:8]
    cfg = engine_tile("mb", N * H * W, Cout, True, k, k, 1, 1, 1, 0, Cin, N, H, W)
    assert cfg in (8, 9), cfg
    run_engine(case, cfg)


def run_engine_splitk(case, splitk, monkeypatch):
    _setenv(monkeypatch, HRV_CONV_SPLITK=splitk)
    run_engine(case, case[1], monkeypatch if case[1] not in (17, 18) else None, splitk)


# ---------------------------------------------------------------------------------------------------------------
# conv_p2.hip
# ---------------------------------------------------------------------------------------------------------------
def run_p2_fwd(case):
    ops, T, _ = _mods()
    Cin, Cout, N, H, W, out_bf16, act, res = case
    d = E.p2_fwd(case)
    _assert_wraps("p2_fwd", case)
    x = ops.Act(_bf(d["xall"]), Cin, d["coff"])
    r = None
    if res:
        r = ops.Act(_bf(d["rall"]) if res == "bf16" else d["rall"].cuda(), Cout, d["rcoff"])
    oall, out = _sentinel(N, H, W, Cout, out_bf16)
    a = {None: ops.ACT_NONE, "relu": ops.ACT_RELU, "lrelu": ops.ACT_LRELU}[act]
    T.conv_p2(x, T.conv_p2_pack(0, d["w"].cuda(), None, Cin, Cout), Cout, out, bias=d["b"].cuda(), act=a, slope=0.5, residual=r, name="t")
    torch.cuda.synchronize()
    _assert_exact("conv_p2 mode 0", oall[..., 8:8 + Cout], d["want"]["out"], out_bf16)
    assert _untouched(oall, 8, Cout)


def run_p2_dgrad(case):
    """Mode 1: conv^T(dY) [+ g] [* act'(x)] [+ g behind the mask: conv_dgrad's add_after]."""
    ops, T, _ = _mods()
    Ck, Ccol, N, H, W, out_bf16, mslope, res = case
    d = E.p2_dgrad(case)
    _assert_wraps("p2_dgrad", case)
    mask = None if d["mask"] is None else ops.Act(_bf(d["mask"]), Ccol)
    r = None if d["res"] is None else ops.Act(d["res"].cuda(), Ccol)
    oall, out = _sentinel(N, H, W, Ccol, out_bf16)
    T.conv_p2(ops.Act(_bf(d["dy"]), Ck), T.conv_p2_pack(1, d["w"].cuda(), None, Ck, Ccol), Ccol, out, mask=mask, mask_slope=mslope or 0.0,
              residual=r, res_after_mask=res == "after", name="t")
    torch.cuda.synchronize()
    _assert_exact("conv_p2 mode 1", oall[..., 8:8 + Ccol], d["want"]["out"], out_bf16)
    assert _untouched(oall, 8, Ccol)


def run_p2_pair(case):
    ops, T, _ = _mods()
    C_, N, H, W, cs_mult, out_bf16 = case[:6]
    d = E.pair_dgrad(case)
    _assert_wraps("p2_pair", case)
    hid = case[6] if len(case) > 6 else 128
    actv = ops.Act(_bf(d["actv_all"]), hid, d["coff"])
    dall = torch.full((N, H, W, hid * cs_mult), 7.0, device="cuda", dtype=torch.bfloat16 if out_bf16 else torch.float32)
    dact = ops.Act(dall, hid, d["coff"])
    T.conv_p2(ops.Act(_bf(d["dgb"]), 2 * C_), T.conv_p2_pack(2, d["wg"].cuda(), d["wb"].cuda(), 2 * C_, hid), hid, dact, mask=actv,
              mask_slope=0.0, name="t")
    torch.cuda.synchronize()
    _assert_exact("conv_p2 mode 2", dall[..., d["coff"]:], d["want"]["out"], out_bf16)
    assert bool((dall[..., :d["coff"]] == 7.0).all())


def run_p2_image(case):
    ops, T, _ = _mods()
    N, H, W = case
    d = E.p2_image(case)
    x = ops.to_nhwc(d["img"].cuda(), bf16=True)
    assert x.bf16 and x.C == 3 and x.cstride % 8 == 0 and bool((x.t[..., 3:] == 0).all())
    out = ops.alloc(N, H, W, 64, "cuda", bf16=True)
    T.conv_p2(x, T.conv_p2_pack(0, d["w"].cuda(), None, 3, 64), 64, out, bias=d["b"].cuda(), act=ops.ACT_RELU, name="t")
    dxt = torch.full((N, H, W, 4), 7.0, device="cuda")
    T.conv_p2(ops.Act(_bf(d["dy"]), 64), T.conv_p2_pack(1, d["wd"].cuda(), None, 64, 3), 3, ops.Act(dxt, 3), name="t")
    torch.cuda.synchronize()
    _assert_exact("features.0", out.t, d["want"]["out"], True)
    _assert_exact("features.0 dgrad", dxt[..., :3], d["want"]["dx"], False)
    assert bool((dxt[..., 3] == 0).all())                  # the pad lane receives zero


# ---------------------------------------------------------------------------------------------------------------
# spade_gb.hip
# ---------------------------------------------------------------------------------------------------------------
def _stats(N, C_, rstd):
    return torch.zeros(N, C_, device="cuda"), torch.full((N, C_), rstd, device="cuda")


def run_gb_fwd(case):
    ops, T, _ = _mods()
    C_, N, H, W, cs_mult, rstd, noise, act, save = case
    d = E.gb_fwd(case)
    _assert_wraps("gb_fwd", case)
    actv = ops.Act(_bf(d["actv_all"]), 128, d["coff"])
    x = ops.Act(d["x"].cuda(), C_)
    z, ns = (d["z"].cuda(), d["ns"].cuda()) if noise else (None, None)
    mean, rs = _stats(N, C_, rstd)
    oall, out = _sentinel(N, H, W, C_, True)
    g1p = torch.full((N, H, W, C_), 5.0, device="cuda", dtype=torch.bfloat16)
    T.spade_gb_forward(actv, x, mean, rs, z, ns, T.spade_gb_pack(0, d["wg"].cuda(), d["wb"].cuda()), d["bg"].cuda(), d["bb"].cuda(),
                       ops.ACT_LRELU if act else ops.ACT_NONE, 0.5, out, g1p if save else None, "t", 1.0, 1.0)
    torch.cuda.synchronize()
    _assert_exact("spade_gb out", oall[..., 8:8 + C_], d["want"]["out"], True)
    assert _untouched(oall, 8, C_)
    if save:
        _assert_exact("spade_gb 1+gamma", g1p, d["want"]["g1p"], True)
    else:
        assert bool((g1p == 5.0).all())


def run_gb_dgrad(case):
    ops, T, _ = _mods()
    C_, N, H, W, cs_mult, out_bf16 = case
    d = E.pair_dgrad(case)
    _assert_wraps("gb_dgrad", case)
    hid = 128
    actv = ops.Act(_bf(d["actv_all"]), hid, d["coff"])
    dall = torch.full((N, H, W, hid * cs_mult), 7.0, device="cuda", dtype=torch.bfloat16 if out_bf16 else torch.float32)
    T.spade_gb_dgrad(ops.Act(_bf(d["dgb"]), 2 * C_), T.spade_gb_pack(1, d["wg"].cuda(), d["wb"].cuda()), C_, actv, 0.0,
                     ops.Act(dall, hid, d["coff"]), "t")
    torch.cuda.synchronize()
    _assert_exact("spade_gb dgrad", dall[..., d["coff"]:], d["want"]["out"], out_bf16)
    assert bool((dall[..., :d["coff"]] == 7.0).all())


# ---------------------------------------------------------------------------------------------------------------
# spade_fused.hip
# ---------------------------------------------------------------------------------------------------------------
def run_fused(case):
    ops, T, _ = _mods()
    C_, N, H, W, shift, rstd, noise, act, save = case
    d = E.fused(case)
    _assert_wraps("fused", case)
    seg = ops.Act(_bf(d["seg"]), 7)
    x = ops.Act(d["x"].cuda(), C_)
    z, ns = (d["z"].cuda(), d["ns"].cuda()) if noise else (None, None)
    mean, rs = _stats(N, C_, rstd)
    oall, out = _sentinel(N, H, W, C_, True)
    g1p = torch.full((N, H, W, C_), 5.0, device="cuda", dtype=torch.bfloat16)
    aall = torch.full((N, H, W, 384), 7.0, device="cuda", dtype=torch.bfloat16)
    pk = T.spade_fused_pack(d["wsh"].cuda(), d["bsh"].cuda(), d["wg"].cuda(), d["wb"].cuda())
    T.spade_fused_forward(seg, shift, x, mean, rs, z, ns, pk, d["bg"].cuda(), d["bb"].cuda(), ops.ACT_LRELU if act else ops.ACT_NONE, 0.5,
                          out, g1p if save else None, ops.Act(aall, 128, 128) if save else None, "t")
    torch.cuda.synchronize()
    if save:           # (first: a wrong actv explains a wrong output)
        _assert_exact("spade_fused actv", aall[..., 128:256], d["want"]["actv"], True)
        assert bool((aall[..., :128] == 7.0).all()) and bool((aall[..., 256:] == 7.0).all())
        _assert_exact("spade_fused 1+gamma", g1p, d["want"]["g1p"], True)
    else:
        assert bool((g1p == 5.0).all()) and bool((aall == 7.0).all())
    _assert_exact("spade_fused out", oall[..., 8:8 + C_], d["want"]["out"], True)
    assert _untouched(oall, 8, C_)


# ---------------------------------------------------------------------------------------------------------------
# conv_s2.hip
# ---------------------------------------------------------------------------------------------------------------
def run_s2_fwd(case):
    ops, T, _ = _mods()
    Cin, Cout, N, H, W, out_bf16, act, wscale, sigma = case
    d = E.s2_fwd(case)
    _assert_wraps("s2_fwd", case)
    x = ops.Act(_bf(d["xall"]), Cin, d["coff"])
    sg = None if sigma is None else torch.tensor([sigma], device="cuda")
    Ho, Wo = H // 2 + 1, W // 2 + 1
    oall, out = _sentinel(N, Ho, Wo, Cout, out_bf16)
    pk = T.conv_s2_pack(T.S2_FWD, d["w"].cuda(), Cin, Cout, sigma=sg, wscale=wscale)
    T.conv_s2(T.S2_FWD, x, pk, Cout, out, bias=d["b"].cuda(), act=ops.ACT_LRELU if act else ops.ACT_NONE, slope=0.5, name="t")
    torch.cuda.synchronize()
    _assert_exact("conv_s2 forward", oall[..., 8:8 + Cout], d["want"]["out"], out_bf16)
    assert _untouched(oall, 8, Cout)


def run_s2_dgrad(case):
    """(conv^T(dY) [+ tap]) [* lrelu'(x)] with slope 0.5."""
    ops, T, _ = _mods()
    Ck, Cph, N, H, W, out_bf16, extra = case
    d = E.s2_dgrad(case)
    tap = None
    if d["tap"] is not None:
        tap = ops.Act(d["tap"].cuda() if extra == "res32" else _bf(d["tap"]), Cph)
    mask = None if d["xin"] is None else ops.Act(_bf(d["xin"]), Cph)
    _assert_wraps("s2_dgrad", case)
    oall, out = _sentinel(N, H, W, Cph, out_bf16)
    pk = T.conv_s2_pack(T.S2_DGRAD, d["w"].cuda(), Ck, 4 * Cph, Cph)
    T.conv_s2(T.S2_DGRAD, ops.Act(_bf(d["dy"]), Ck), pk, 4 * Cph, out, Cph=Cph, residual=tap, mask=mask, mask_slope=0.5, name="t")
    torch.cuda.synchronize()
    _assert_exact("conv_s2 dgrad", oall[..., 8:8 + Cph], d["want"]["out"], out_bf16)
    assert _untouched(oall, 8, Cph)


def run_s2_cells(case):
    """The 2x2 form over the space-to-depth image, also with [hi | lo | hi] operands (split3): integers leave lo = 0, the three
    products must still sum to the exact result."""
    ops, T, _ = _mods()
    Cin, Cout, N, H, W, split3 = case
    d = E.s2_cells(case)
    K = 4 * d["Cq"]
    Ho, Wo = H // 2 + 1, W // 2 + 1
    oall, out = _sentinel(N, Ho, Wo, Cout, not split3)
    if split3:
        src = T.split3(ops.Act(d["xs"].cuda(), K))
        pk = T.conv_s2_pack(T.S2_CELLS, d["w2"].cuda(), 3 * K, Cout, split3=True)
        T.conv_s2(T.S2_CELLS, src, pk, Cout, out, bias=d["b"].cuda(), name="t")
    else:
        pk = T.conv_s2_pack(T.S2_CELLS, d["w2"].cuda(), K, Cout)
        T.conv_s2(T.S2_CELLS, ops.Act(_bf(d["xs"]), K), pk, Cout, out, bias=d["b"].cuda(), act=ops.ACT_LRELU, slope=0.5, name="t")
    torch.cuda.synchronize()
    _assert_exact("conv_s2 cells", oall[..., 8:8 + Cout], d["want"]["out"], not split3)
    assert _untouched(oall, 8, Cout)


def run_s2_split3_fwd(case):
    ops, T, _ = _mods()
    Cin, Cout, N, H, W = case
    d = E.s2_split3_fwd(case)
    src = T.split3(ops.Act(d["x"].cuda(), Cin))
    assert bool((src.t[..., Cin:2 * Cin] == 0).all())            # integers: the lo third is empty
    oall, out = _sentinel(N, H // 2 + 1, W // 2 + 1, Cout, False)
    T.conv_s2(T.S2_FWD, src, T.conv_s2_pack(T.S2_FWD, d["w"].cuda(), 3 * Cin, Cout, split3=True), Cout, out, bias=d["b"].cuda(), name="t")
    torch.cuda.synchronize()
    _assert_exact("conv_s2 split3", oall[..., 8:8 + Cout], d["want"]["out"], False)
    assert _untouched(oall, 8, Cout)


# ---------------------------------------------------------------------------------------------------------------
# weight gradients
# ---------------------------------------------------------------------------------------------------------------
def run_wgrad(case):
    """conv_wgrad_tr classes 0-8, wgrad_s2, the conv_wgrad_bf16 fallback at 528 source channels and the fp32 kernel, with the fused
    bias gradient, accumulate=True and channel slices; the launch record names the kernel the plan picked."""
    ops, T, _ = _mods()
    name, kernel, cin, cout, k, stride, pad, N, H, W, wide, accumulate, mixed = case
    d = E.wgrad(case)

    def act(t):
        t = t.to(torch.bfloat16) if mixed else t
        if not wide:
            return ops.Act(t.cuda(), t.shape[3])
        C_ = t.shape[3]
        full = torch.full(t.shape[:3] + (C_ + 24,), 3.0, dtype=t.dtype)      # neighbours of the slice must not leak in
        full[..., 16:16 + C_] = t
        return ops.Act(full.cuda(), C_, 16)

    base = 8 if wide else 0
    dw = torch.full((cout, cin + base, k, k), 7.0, device="cuda")
    db = torch.full((cout,), 7.0, device="cuda")
    if accumulate:
        dw[:, base:] = d["dw0"].cuda()
        db.copy_(d["db0"].cuda())
    with _mixed(mixed):
        ops.profile_begin()
        T.conv_wgrad(act(d["dy"]), act(d["x"]), 0, base, cin + base, k, k, stride, pad, dw, accumulate=accumulate, name=name, dbias=db,
                     dbias_accumulate=accumulate)
        recs = ops.profile_end(kernels=True, variants=True)
    assert kernel in _kernels(recs), _kernels(recs)
    _assert_exact(name + " dW", dw[:, base:].contiguous(), d["want"]["dw"], False)
    _assert_exact(name + " db", db, d["want"]["db"], False)
    assert bool((dw[:, :base] == 7.0).all()), "columns outside [ci_base, ci_base + C) stay untouched"


# ---------------------------------------------------------------------------------------------------------------
# thin_conv.hip, conv_cout1.hip
# ---------------------------------------------------------------------------------------------------------------
def run_thin(case, monkeypatch):
    ops, T, _ = _mods()
    cin, cout, k, N, H, W = case
    d = E.thin(case)
    _setenv(monkeypatch, HRV_CONV_P2="0")                       # (the layer is below conv_p2's tile gate anyway)
    with _mixed():
        ops.profile_begin()
        y = T.conv_forward_dev(d["w"].cuda(), [(ops.Act(_bf(d["x"]), cin), 0)], 1, k // 2, shift=d["b"].cuda(), act=ops.ACT_LRELU, slope=0.5,
                               name="t", out_bf16=True)
        dx = T.conv_dgrad(ops.Act(_bf(d["dy"]), cout), d["wd"].cuda(), H, W, 1, k // 2, name="t.dgrad")
        recs = ops.profile_end(kernels=True)
    assert _kernels(recs) == ["thin_conv_kernel", "thin_conv_kernel"], recs
    _assert_exact("thin_conv forward", y.t[..., :cout], d["want"]["out"], True)
    _assert_exact("thin_conv dgrad", dx.t[..., :cin], d["want"]["dx"], False)


def run_cout1(case):
    ops, T, _ = _mods()
    Cin, K, pad, N, H, W = case
    d = E.cout1(case)
    wide = torch.full((N, H, W, Cin + 8), 3.0)
    wide[..., 4:4 + Cin] = d["x"]
    with _mixed(False):
        ops.profile_begin()
        y = T.conv_forward_dev(d["w"].cuda(), [(ops.Act(wide.cuda(), Cin, 4), 0)], 1, pad, shift=d["b"].cuda(), name="t")
        dx = T.conv_dgrad(ops.Act(torch.nn.functional.pad(d["dy"], (0, 3)).cuda(), 1), d["w"].cuda(), H, W, 1, pad, add=ops.Act(d["add"].cuda(), Cin),
                          name="t.dgrad")
        recs = ops.profile_end(kernels=True)
    assert _kernels(recs) == ["cout1_kernel", "cout1_kernel"], recs
    _assert_exact("cout1 forward", y.t[..., :1], d["want"]["out"], False)
    assert bool((y.t[..., 1:] == 0).all())
    _assert_exact("cout1 dgrad", dx.t[..., :Cin], d["want"]["dx"], False)


# ---------------------------------------------------------------------------------------------------------------
# spade_fused.hip with a tile plan (tests/spade_uniform_cases.py; N = 2 everywhere)
# ---------------------------------------------------------------------------------------------------------------
UN = 2


def _useg(name, H, W, shift):
    ops, _, _ = _mods()
    return ops.Act(U.label_map(name, H, W, shift).cuda(), 7)


def _bits(t):
    return t.contiguous().view(torch.int16)


def _uniform_forward(T, ops, seg, shift, x, d, w, pk, C_, H, W, noise, save, tiles):
    """one forward into sentinel-filled buffers: (out slice tensor, 1 + gamma, actv tensor)"""
    N = UN
    oall = torch.full((N, H, W, 8 + C_ + 8), 7.0, device="cuda", dtype=torch.bfloat16)
    g1p = torch.full((N, H, W, C_), 5.0, device="cuda", dtype=torch.bfloat16)
    aall = torch.full((N, H, W, 384), 7.0, device="cuda", dtype=torch.bfloat16)
    z, ns = (d["z"].cuda(), w["ns"].cuda()) if noise else (None, None)
    T.spade_fused_forward(seg, shift, x, d["mean"].cuda(), d["rstd"].cuda(), z, ns, pk, w["bg"].cuda(), w["bb"].cuda(), ops.ACT_LRELU, 0.2,
                          ops.Act(oall, C_, 8), g1p if save else None, ops.Act(aall, 128, 128) if save else None, "t", tiles=tiles)
    torch.cuda.synchronize()
    return oall, g1p, aall


def run_uniform_plan_on_equals_plan_off(case, wraps=False):
    """Returns the plan's (heavy, light) counts, which the run has asserted against U.classify."""
    ops, T, _lib = _mods()
    N = UN
    H, W, shift, name, C_ = case
    if wraps:
        assert N * ((H + 15) // 16) * ((W + 15) // 16) > 2 * int(_lib.load().hrv_persistent_cus())
    w, d = U.weights(C_), U.inputs(H, W, C_)
    seg = _useg(name, H, W, shift)
    if C_ == 80:
        x = ops.ActUp(ops.Act(d["x"][0].cuda(), 64), ops.Act(d["x"][1].cuda(), 16))
    elif C_ == 32:
        x = ops.Act(d["x"].to(torch.bfloat16).cuda(), C_)
    else:
        x = ops.Act(d["x"].cuda(), C_)
    pk = T.spade_fused_pack(w["wsh"].cuda(), w["bsh"].cuda(), w["wg"].cuda(), w["wb"].cuda())
    want = U.classify(U.label_map(name, H, W, shift), shift, N, H, W)
    plan = T.spade_tile_plan(seg, shift, N, H, W)
    assert plan.counts() == (len(want["heavy"]), len(want["light"]))
    if name in ("one_class", "edge3", "multihot") or (name == "speckle" and shift == 1):
        assert plan.counts()[1] > 0
    if name == "random":
        assert plan.counts()[1] == 0
    for noise in (False, True):
        for save in (False, True):
            off = _uniform_forward(T, ops, seg, shift, x, d, w, pk, C_, H, W, noise, save, None)
            on = _uniform_forward(T, ops, seg, shift, x, d, w, pk, C_, H, W, noise, save, plan)
            for what, a, b in zip(("out", "1 + gamma", "actv"), off, on):
                assert torch.equal(_bits(a), _bits(b)), (what, noise, save, int((_bits(a) != _bits(b)).sum()))
            # (and the forward without a plan wrote something: the sentinel is gone from the slice, the neighbours keep it)
            assert not bool((off[0][..., 8:8 + C_] == 7.0).all()) and bool((on[0][..., :8] == 7.0).all()) and bool((on[0][..., 8 + C_:] == 7.0).all())
            if save:
                assert bool((on[2][..., :128] == 7.0).all()) and bool((on[2][..., 256:] == 7.0).all())
            else:
                assert bool((on[1] == 5.0).all()) and bool((on[2] == 7.0).all())
    return plan.counts()


def _assert_exact_uniform(what, got, ref64):
    want = E.to_bf16_rne(ref64)
    got = got.detach().cpu()
    assert got.dtype == torch.bfloat16 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    bad = int((got.float() != want.float()).sum())
    assert bad == 0, f"{what}: {bad} of {got.numel()} differ from the float64 reference"


def run_uniform_exact(case):
    """Returns the plan's (heavy, light) counts; the light count has been asserted against U.classify and is > 0."""
    ops, T, _ = _mods()
    N = UN
    H, W, shift, name, C_, rstd, noise, act, save = case
    d = U.exact(case)
    seg = ops.Act(d["seg"].to(torch.bfloat16).cuda(), 7)
    plan = T.spade_tile_plan(seg, shift, N, H, W)
    assert plan.counts()[1] == len(U.classify(U.label_map(name, H, W, shift), shift, N, H, W)["light"]) > 0
    x = ops.Act(d["x"].cuda(), C_)
    z, ns = (d["z"].cuda(), d["ns"].cuda()) if noise else (None, None)
    mean, rs = torch.zeros(N, C_, device="cuda"), torch.full((N, C_), rstd, device="cuda")
    oall = torch.full((N, H, W, 8 + C_ + 8), 7.0, device="cuda", dtype=torch.bfloat16)
    g1p = torch.full((N, H, W, C_), 5.0, device="cuda", dtype=torch.bfloat16)
    aall = torch.full((N, H, W, 384), 7.0, device="cuda", dtype=torch.bfloat16)
    pk = T.spade_fused_pack(d["wsh"].cuda(), d["bsh"].cuda(), d["wg"].cuda(), d["wb"].cuda())
    T.spade_fused_forward(seg, shift, x, mean, rs, z, ns, pk, d["bg"].cuda(), d["bb"].cuda(), ops.ACT_LRELU if act else ops.ACT_NONE, 0.5,
                          ops.Act(oall, C_, 8), g1p if save else None, ops.Act(aall, 128, 128) if save else None, "t", tiles=plan)
    torch.cuda.synchronize()
    if save:
        _assert_exact_uniform("actv", aall[..., 128:256], d["want"]["actv"])
        _assert_exact_uniform("1 + gamma", g1p, d["want"]["g1p"])
    _assert_exact_uniform("out", oall[..., 8:8 + C_], d["want"]["out"])
    assert bool((oall[..., :8] == 7.0).all()) and bool((oall[..., 8 + C_:] == 7.0).all())
    return plan.counts()
