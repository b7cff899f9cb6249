"""The loss, pool, down-sum, add_slice kernels (csrc/train.hip) and the BatchNorm training, softmax, cross-entropy and TV kernels
(csrc/cond_train.hip) against the float64 references of tests/train_exact_cases.py (why every sum is exact in fp32 in any order;
tests/test_train_exact_cases_cpu.py proves the conditions on the references alone, and that these assertions fail on each seeded
defect).

  loss value and gradient, loss_out after accumulation, pools, down-sum, add_slice, affine_act,
  s1 / s2 (in the workspace), dgamma, dbeta, cross-entropy sum / count / gradient, softmax       torch.equal
  bf16 stores (MSE gradient, down-sum mode 2, add_slice)                                        the bit pattern of round-to-nearest-even
  bn_finalize                                                                                   the float64 value rounded to fp32, or its neighbour
  BatchNorm dx, TV gradient and loss                                                            the derived bounds of the case module

Every output buffer starts as NaN (or as the old value where the kernel accumulates) and every operand sits where the case says:
in a slice of a poisoned tensor, or in a view shifted by one element for the losses.  Nothing here depends on the order of a sum."""
import pytest
import torch

import train_exact_cases as E

pytestmark = pytest.mark.gpu
NAN = float("nan")


def _mods():
    import hr_viton_amd  # noqa: F401
    from hr_viton_amd import _lib, ops, train_ops as T
    return _lib, ops, T


class _Slice:
    """channels [coff, coff + C) of a [N, H, W, cs] device tensor: the slice is the operand (``fill``) or the result (NaN until
    written), everything around it is poison.  sliced=False: the dense tensor"""

    def __init__(self, shape, bf16=False, sliced=True, fill=None):
        N, H, W, Cn = shape
        g = 8 if bf16 else 4                            # one 16-byte (fp32) / 8-byte-aligned (bf16) group
        self.C, self.coff, self.cs = Cn, (g if sliced else 0), Cn + (3 * g if sliced else 0)
        self.t = torch.full((N, H, W, self.cs), E.POISON, dtype=torch.bfloat16 if bf16 else torch.float32, device="cuda")
        self.view().copy_(torch.full(shape, NAN) if fill is None else fill)

    def view(self):
        return self.t[..., self.coff:self.coff + self.C]

    def act(self, ops, Cn=None):
        return ops.Act(self.t, self.C if Cn is None else Cn, self.coff)

    def intact(self):
        m = torch.ones(self.cs, dtype=torch.bool, device="cuda")
        m[self.coff:self.coff + self.C] = False
        return bool((self.t[..., m] == E.POISON).all())


def _equal(got, want64, what):
    """torch.equal of a CPU result with the float64 reference (bf16: with its round-to-nearest-even, on the bit pattern)"""
    if got.dtype == torch.bfloat16:
        want = want64 if want64.dtype == torch.bfloat16 else E.to_bf16_rne(want64)
        g, w = E.bits(got), E.bits(want)
    else:
        g, w = got.double(), want64.double()
    if not torch.equal(g, w):
        bad = (g != w).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError(f"{what}: {len(bad)} of {w.numel()} differ, first at {list(i)}: {float(got[i])!r} vs {float(want64[i])!r}")


# ---------------------------------------------------------------------------------------------------------------
# losses
# ---------------------------------------------------------------------------------------------------------------
def _shifted(t, shift, bf16):
    """t as the view buf[shift : shift + n] of an aligned, poisoned buffer"""
    n = t.numel()
    buf = torch.full((n + 1,), E.POISON, dtype=torch.bfloat16 if bf16 else torch.float32, device="cuda")
    v = buf[shift:shift + n]
    v.copy_(t)
    assert (v.data_ptr() % (8 if bf16 else 16) == 0) == (shift == 0)
    return v


def _run_loss(T, n, v, a, b, dev):
    key = lambda name, s: (name, E.loss_kind(v), v.bf16, s)
    for name, t, s in (("a", a, v.shift[0]), ("b", b, v.shift[1])):
        if key(name, s) not in dev:
            dev[key(name, s)] = _shifted(t, s, v.bf16)
    da, db = dev[key("a", v.shift[0])], (dev[key("b", v.shift[1])] if v.with_b else None)
    out = torch.full((1,), E.LOSS0 if v.accumulate else NAN, device="cuda")
    grad = T.loss(da, db, v.mode | (E.RELU_MASK if v.relu else 0), v.lscale, v.gscale, out, accumulate=v.accumulate,
                  want_grad=v.want_grad, grad_bf16=v.grad_bf16)
    torch.cuda.synchronize()
    return out.cpu(), None if grad is None else grad.cpu()


@pytest.mark.parametrize("n", E.LOSS_N)
def test_loss_value_and_gradient(n):
    _lib, ops, T = _mods()
    dev = {}
    for v in E.loss_variants(n):
        a, b = E.loss_operands(n, E.loss_kind(v))
        ref = E.loss_ref(a, b, v)
        out, grad = _run_loss(T, n, v, a, b, dev)
        _equal(out, ref["loss"], f"n={n} {v} loss")
        assert (grad is None) == (not v.want_grad)
        if grad is not None:
            assert grad.dtype == torch.float32
            _equal(grad, ref["grad"], f"n={n} {v} grad")


@pytest.mark.parametrize("n,kind", E.LOSS_BF16_GRAD)
def test_loss_bf16_gradient_rounds_to_nearest_even(n, kind):
    _lib, ops, T = _mods()
    a, b = E.loss_bf16_grad_operands(n, kind)
    for v in E.LOSS_BF16_GRAD_VARIANTS:
        ref = E.loss_ref(a, b, v)
        out, grad = _run_loss(T, n, v, a, b, {})
        _equal(out, ref["loss"], f"n={n} {v} loss")
        assert grad.dtype == torch.bfloat16
        _equal(grad, ref["grad"], f"n={n} {v} grad")
    print(f"loss bf16 gradient n={n} {kind}: {E.tie_share(a.double() - b.double()):.3f} exact ties, 16-byte and scalar store")


@pytest.mark.parametrize("n", [1, 5, 1025, 262145, 1048583])
def test_loss_writes_every_gradient_element_and_nothing_behind(n):
    """the C entry points on a NaN-filled gradient with 8 elements behind it: fp32 and bf16 operands, both paths, both gradient types"""
    _lib, ops, T = _mods()
    lib = _lib.load()
    ws = torch.empty(4096, device="cuda")
    runs = [(E.LossVariant(E.L1, False, bf, s, True, True, False, 0.5, 2.0, False), E.loss_operands(n, "diff"))
            for bf, s in ((False, (0, 0)), (False, (1, 1)), (True, (0, 0)), (True, (1, 0)))]
    if n == 1025:
        runs += [(v, E.loss_bf16_grad_operands(1024, "sparse")) for v in E.LOSS_BF16_GRAD_VARIANTS]
    for v, (a, b) in runs:
        m = a.numel()
        da, db = _shifted(a, v.shift[0], v.bf16), _shifted(b, v.shift[1], v.bf16)
        grad = torch.full((m + 8,), NAN, dtype=torch.bfloat16 if v.grad_bf16 else torch.float32, device="cuda")
        out = torch.full((1,), E.LOSS0 if v.accumulate else NAN, device="cuda")
        fn = lib.hrv_loss_bf16in_f32 if v.bf16 else lib.hrv_loss_f32
        _lib.check(fn(da.data_ptr(), db.data_ptr(), m, v.mode | (E.GRAD_BF16 if v.grad_bf16 else 0), v.lscale, v.gscale, grad.data_ptr(),
                      ws.data_ptr(), out.data_ptr(), 1 if v.accumulate else 0, None), "hrv_loss")
        torch.cuda.synchronize()
        ref = E.loss_ref(a, b, v)
        _equal(out.cpu(), ref["loss"], f"n={m} {v} loss")
        _equal(grad[:m].cpu(), ref["grad"], f"n={m} {v} grad")
        assert bool(torch.isnan(grad[m:].float()).all()), f"n={m} {v}: written behind the gradient"


# ---------------------------------------------------------------------------------------------------------------
# max pool
# ---------------------------------------------------------------------------------------------------------------
def _dt(bf16):
    return torch.bfloat16 if bf16 else torch.float32


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_maxpool_forward(bf16):
    _lib, ops, T = _mods()
    for shape in E.POOL_SHAPES[bf16]:
        d = E.pool_case(*shape, not bf16)
        x = d["x"].cuda().to(_dt(bf16))
        assert torch.equal(torch.signbit(x.float().cpu()), torch.signbit(d["x"]))          # -0.0 arrives as -0.0
        y = T.maxpool2x2(ops.Act(x, shape[3]))
        torch.cuda.synchronize()
        assert y.t.dtype == _dt(bf16)
        _equal(y.t.cpu().float(), E.maxpool_ref(d["x"]), f"maxpool {shape}")


def _maxpool_bwd(_lib, name, x, dy, gb):
    N, H, W, Cn = x.shape
    dx = torch.full((N, H, W, Cn), NAN, dtype=_dt(gb), device="cuda")
    _lib.check(getattr(_lib.load(), name)(x.data_ptr(), dy.data_ptr(), N, H, W, Cn, dx.data_ptr(), None), name)
    torch.cuda.synchronize()
    return dx


@pytest.mark.parametrize("entry", E.MAXPOOL_BWD_ENTRIES, ids=[e[0] for e in E.MAXPOOL_BWD_ENTRIES])
def test_maxpool_backward_first_maximum_takes_the_gradient(entry):
    _lib, ops, T = _mods()
    name, xb, gb, relu = entry
    for shape in E.POOL_SHAPES[xb]:
        d = E.pool_case(*shape, not (xb or relu))
        x, dy = d["x"].cuda().to(_dt(xb)), d["dy"].cuda().to(_dt(gb))
        want = E.maxpool_bwd_ref(d["x"], d["dy"], relu)
        dx = _maxpool_bwd(_lib, name, x, dy, gb)
        _equal(dx.cpu().float(), want, f"{name} {shape}")                      # (every position written: a NaN left fails)
        via = T.maxpool2x2_bwd(ops.Act(x, shape[3]), ops.Act(dy, shape[3]), relu=relu)
        torch.cuda.synchronize()
        assert via.t.dtype == _dt(gb) and torch.equal(via.t, dx), f"{name} {shape}: the wrapper"


@pytest.mark.parametrize("name", sorted(E.MAXPOOL_BIG))
def test_maxpool_backward_second_grid_trip(name):
    _lib, ops, T = _mods()
    _, xb, gb, relu = next(e for e in E.MAXPOOL_BWD_ENTRIES if e[0] == name)
    tile, (rh, rw) = E.MAXPOOL_BIG[name]
    d = E.pool_case(*tile, False)
    rep = lambda t, dt: t.cuda().to(dt).repeat(1, rh, rw, 1)
    x, dy = rep(d["x"], _dt(xb)), rep(d["dy"], _dt(gb))
    assert E.groups(*dy.shape) > E.GRID_CAP
    dx = _maxpool_bwd(_lib, name, x, dy, gb)
    want = rep(E.maxpool_bwd_ref(d["x"], d["dy"], relu).float(), _dt(gb))
    assert torch.equal(dx, want), f"{name}: {int((dx != want).sum())} of {want.numel()} differ"


# ---------------------------------------------------------------------------------------------------------------
# avg pool backward, down-sum, add_slice
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", E.AVG_CASES, ids=str)
def test_avgpool_backward(case):
    _lib, ops, T = _mods()
    N, H, W, Cn, acc, sliced = case
    d = E.avg_case(N, H, W, Cn, acc)
    dy = _Slice(d["dy"].shape, sliced=sliced, fill=d["dy"])
    dx = _Slice((N, H, W, Cn), sliced=sliced, fill=d["dx0"])
    T.avgpool3x3s2_bwd(dy.act(ops), H, W, dx.act(ops), accumulate=acc)
    torch.cuda.synchronize()
    _equal(dx.view().cpu(), E.avgpool_bwd_ref(d["dy"], H, W, d["dx0"]), f"avgpool_bwd {case}")
    assert dy.intact() and dx.intact()


def test_avgpool_backward_second_grid_trip():
    _lib, ops, T = _mods()
    tile, (rh, rw), (H, W) = E.AVG_BIG
    t = E.avg_big_dy()
    dy = t.cuda().repeat(1, rh, rw, 1)
    dx = ops.Act(torch.full((1, H, W, tile[3]), NAN, device="cuda"), tile[3])
    assert E.groups(1, H, W, tile[3]) > E.GRID_CAP
    T.avgpool3x3s2_bwd(ops.Act(dy, tile[3]), H, W, dx, accumulate=False)
    want = E.avgpool_bwd_ref(t.repeat(1, rh, rw, 1), H, W).float().cuda()
    torch.cuda.synchronize()
    assert torch.equal(dx.t, want), f"{int((dx.t != want).sum())} of {want.numel()} differ"


@pytest.mark.parametrize("case", E.DOWNSUM_CASES, ids=str)
def test_downsum(case):
    _lib, ops, T = _mods()
    N, Hl, Wl, Cn, mode = case
    d = E.downsum_case(*case)
    dhi = _Slice(d["dhi"].shape, fill=d["dhi"])
    dlo = _Slice((N, Hl, Wl, Cn), bf16=mode == 2, fill=d["dlo0"])
    T.downsum2x2(dhi.act(ops), dlo.act(ops), accumulate=mode == 1)
    torch.cuda.synchronize()
    want = E.downsum_ref(d["dhi"], d["dlo0"])
    _equal(dlo.view().cpu(), want, f"downsum {case}")
    assert dhi.intact() and dlo.intact()
    if mode == 2:
        print(f"downsum bf16 {case}: {E.tie_share(want):.3f} exact ties")


@pytest.mark.parametrize("case", E.ADD_CASES, ids=str)
def test_add_slice(case):
    _lib, ops, T = _mods()
    N, H, W, Cn, bf16, acc = case
    d = E.add_case(*case)
    a = _Slice(d["a"].shape, bf16=bf16, fill=d["a"])
    out = _Slice(d["a"].shape, bf16=bf16, fill=d["out0"] if acc else None)
    T.add_slice(a.act(ops), out.act(ops), acc)
    torch.cuda.synchronize()
    _equal(out.view().cpu(), E.add_ref(d["a"], d["out0"], acc), f"add_slice {case}")
    assert a.intact() and out.intact()


# ---------------------------------------------------------------------------------------------------------------
# BatchNorm
# ---------------------------------------------------------------------------------------------------------------
def _bn_operands(c, d):
    rep = lambda t: t.cuda().repeat(1, c.reps, 1, 1)
    shape = (c.N, c.H, c.W, d["Cp"])
    dy, x = _Slice(shape, sliced=c.sliced, fill=rep(d["dy"])), _Slice(shape, sliced=c.sliced, fill=rep(d["x"]))
    dx = _Slice(shape, sliced=c.sliced, fill=None if d["dx0"] is None else rep(d["dx0"]))
    return dy, x, dx, [d[k].cuda() for k in ("mean", "rstd", "scale")]


@pytest.mark.parametrize("c", E.BN_BWD, ids=E.bn_id)
def test_bn_backward(c):
    _lib, ops, T = _mods()
    lib = _lib.load()
    d = E.bn_case(c)
    Cp, npix, ref = d["Cp"], d["npix"], d["ref"]
    dy, x, dx, (mean, rstd, scale) = _bn_operands(c, d)
    elems = lib.hrv_bn_bwd_workspace_elems(c.C)
    assert elems == E.BN_ROWS * 2 * Cp + 2 * Cp
    ws = torch.full((elems,), NAN, device="cuda")
    dg, db = torch.full((Cp + 4,), NAN, device="cuda"), torch.full((Cp + 4,), NAN, device="cuda")
    if c.dgb_acc:
        dg[:c.C], db[:c.C] = d["dg0"].cuda(), d["db0"].cuda()
    _lib.check(lib.hrv_bn_bwd_nhwc_f32(dy.t.data_ptr(), dy.cs, dy.coff, x.t.data_ptr(), x.cs, x.coff, c.C, npix, mean.data_ptr(), rstd.data_ptr(),
                                       scale.data_ptr(), ws.data_ptr(), dx.t.data_ptr(), dx.cs, dx.coff, 1 if c.dx_acc else 0, dg.data_ptr(),
                                       db.data_ptr(), 1 if c.dgb_acc else 0, None), "hrv_bn_bwd_nhwc_f32")
    torch.cuda.synchronize()
    what = f"bn_bwd {E.bn_id(c)}"
    sums = ws[E.BN_ROWS * 2 * Cp:].cpu()
    _equal(sums[:Cp], ref["s1"], what + " s1")
    _equal(sums[Cp:], ref["s2"], what + " s2")
    _equal(dg[:c.C].cpu(), ref["dgamma"][:c.C], what + " dgamma")
    _equal(db[:c.C].cpu(), ref["dbeta"][:c.C], what + " dbeta")
    assert bool(torch.isnan(dg[c.C:]).all() and torch.isnan(db[c.C:]).all()), what + ": dgamma / dbeta written at c >= C"
    got = dx.view().cpu()
    frac = E.bn_dx_check(got, d, c.reps, what)
    exact = E.bn_dx_exact(d)
    if exact:
        _equal(got, E.bn_dx_bound(d)[0].repeat(1, c.reps, 1, 1), what + " dx (exact)")
    print(f"{what}: dx worst |error| / bound = {frac:.3g}" + (" (exact)" if exact else ""))
    assert dy.intact() and x.intact() and dx.intact(), what + ": written outside the slice"
    if not c.dgb_acc:                                    # the wrapper: its own workspace, the same bits
        dy2, x2, dx2, _ = _bn_operands(c, d)
        dg2, db2 = torch.full((Cp,), NAN, device="cuda"), torch.full((Cp,), NAN, device="cuda")
        T.bn_bwd(dy2.act(ops, c.C), x2.act(ops, c.C), T.BNStats(mean, rstd, scale, None), dg2, db2, dx2.act(ops, c.C), c.dx_acc)
        torch.cuda.synchronize()
        assert torch.equal(dx2.t, dx.t) and torch.equal(dg2[:c.C], dg[:c.C]) and torch.equal(db2[:c.C], db[:c.C]), what + ": the wrapper"


@pytest.mark.parametrize("case", E.BN_FIN, ids=str)
def test_bn_finalize(case):
    _lib, ops, T = _mods()
    lib = _lib.load()
    N, Cn, cs, HW, affine, running = case
    d = E.bn_fin_case(case)
    dev = {k: (None if v is None else v.cuda()) for k, v in d.items() if k != "ref"}
    outs = {k: torch.full((Cn + 4,), NAN, device="cuda") for k in ("mean", "rstd", "scale", "shift")}
    if running:
        outs["rm"], outs["rv"] = torch.full((Cn + 4,), NAN, device="cuda"), torch.full((Cn + 4,), NAN, device="cuda")
        outs["rm"][:Cn], outs["rv"][:Cn] = dev["rm"], dev["rv"]
    p = lambda t: None if t is None else t.data_ptr()
    _lib.check(lib.hrv_bn_finalize_f32(p(dev["mean_nc"]), p(dev["rstd_nc"]), N, Cn, cs, E.BN_EPS_IN, HW, p(dev["gamma"]), p(dev["beta"]), E.BN_EPS,
                                       E.BN_MOMENTUM, p(outs.get("rm")), p(outs.get("rv")), p(outs["mean"]), p(outs["rstd"]), p(outs["scale"]),
                                       p(outs["shift"]), None), "hrv_bn_finalize_f32")
    torch.cuda.synchronize()
    neighbours = 0
    for k, t in outs.items():
        got, want = t[:Cn].cpu(), d["ref"][k]
        ok = E.within_one_ulp(got, want)
        assert bool(ok.all()), f"bn_finalize {case} {k}: {int((~ok).sum())} of {Cn} beyond one ulp, first c = {int((~ok).nonzero()[0])}: " \
                               f"{float(got[(~ok).nonzero()[0]])!r} vs {float(want[(~ok).nonzero()[0]])!r}"
        assert bool(torch.isnan(t[Cn:]).all()), f"bn_finalize {case} {k}: written past C"
        neighbours += int((got != want.float()).sum())
    print(f"bn_finalize {case}: {neighbours} of {len(outs) * Cn} outputs are the neighbour of the rounded float64 value")


@pytest.mark.parametrize("case", E.AFFINE_CASES, ids=str)
def test_affine_act(case):
    _lib, ops, T = _mods()
    N, H, W, Cn, act, res, slope = case
    d = E.affine_case(case)
    x = _Slice((N, H, W, Cn), fill=d["x"])
    r = _Slice((N, H, W, Cn), fill=d["res"]) if res else None
    out = _Slice((N, H, W, Cn))
    T.affine_act(x.act(ops), d["scale"].cuda(), d["shift"].cuda(), act, None if r is None else r.act(ops), slope, out.act(ops))
    torch.cuda.synchronize()
    _equal(out.view().cpu(), E.affine_ref(case, d), f"affine_act {case}")
    assert x.intact() and out.intact() and (r is None or r.intact())


# ---------------------------------------------------------------------------------------------------------------
# cross entropy, softmax, TV
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", E.CE_CASES, ids=str)
def test_cross_entropy(case):
    _lib, ops, T = _mods()
    from hr_viton_amd import functional as HF
    lib = _lib.load()
    N, Cn, H, W, _ = case
    d = E.ce_case(case)
    x, t = d["x"].cuda(), d["t"].cuda()
    ref = E.ce_ref(d["x"], d["t"], E.CE_GSCALE)
    # the C entry: raw gradient with gscale, count; then without a gradient
    grad = torch.full((x.numel() + 8,), NAN, device="cuda")
    ws, out = torch.full((1024,), NAN, device="cuda"), torch.full((2,), NAN, device="cuda")
    _lib.check(lib.hrv_cross_entropy_nchw_f32(x.data_ptr(), t.data_ptr(), N, Cn, H * W, E.CE_GSCALE, grad.data_ptr(), ws.data_ptr(),
                                              out.data_ptr(), None), "hrv_cross_entropy_nchw_f32")
    torch.cuda.synchronize()
    nb = min(-(-N * H * W // 256), E.CE_BLOCKS)
    assert float(ws[:nb].double().sum()) == ref["loss_sum"] and float(ws[nb:2 * nb].double().sum()) == ref["count"], f"{case}: partial sums"
    _equal(out[:1].cpu(), ref["mean"], f"ce {case} mean")
    assert float(out[1]) == ref["count"], (case, float(out[1]), ref["count"])
    _equal(grad[:x.numel()].view_as(x).cpu(), ref["grad"], f"ce {case} grad")
    assert bool(torch.isnan(grad[x.numel():]).all())
    out2 = torch.full((2,), NAN, device="cuda")
    _lib.check(lib.hrv_cross_entropy_nchw_f32(x.data_ptr(), t.data_ptr(), N, Cn, H * W, 1.0, None, ws.data_ptr(), out2.data_ptr(), None),
               "hrv_cross_entropy_nchw_f32")
    torch.cuda.synchronize()
    assert torch.equal(out2, out), f"{case}: with_grad=False"
    # the value and backward paths of functional.cross_entropy2d: grad = (softmax - onehot) * fl(1 / max(count, 1))
    with torch.no_grad():
        assert torch.equal(HF.cross_entropy2d(x, t).reshape(1).cpu(), ref["mean"]), f"{case}: no_grad"
    xr = x.clone().requires_grad_(True)
    loss = HF.cross_entropy2d(xr, t)
    loss.backward()
    torch.cuda.synchronize()
    _equal(loss.detach().reshape(1).cpu(), ref["mean"], f"ce {case} functional mean")
    s = float(torch.ones(1, device="cuda") / torch.tensor([max(ref["count"], 1.0)], device="cuda"))       # (torch's own division, as the op's backward)
    _equal(xr.grad.cpu(), E.ce_ref(d["x"], d["t"], 1.0)["grad"] * s, f"ce {case} functional grad")


@pytest.mark.parametrize("case", E.SOFTMAX_CASES, ids=str)
def test_softmax(case):
    _lib, ops, T = _mods()
    from hr_viton_amd import functional as HF
    d = E.softmax_case(case)
    y = HF.softmax(d["x"].cuda())
    torch.cuda.synchronize()
    _equal(y.cpu(), d["y"], f"softmax {case}")
    d = E.softmax_case(case, True)                     # k a power of two at every pixel: the backward is exact
    x = d["x"].cuda().requires_grad_(True)
    y = HF.softmax(x)
    y.backward(d["dy"].cuda())
    torch.cuda.synchronize()
    _equal(y.detach().cpu(), d["y"], f"softmax {case} (powers of two)")
    _equal(x.grad.cpu(), E.softmax_bwd_ref(d["y"], d["dy"]), f"softmax_bwd {case}")


@pytest.mark.parametrize("case", E.TV_CASES, ids=str)
def test_tv_loss(case):
    _lib, ops, T = _mods()
    from hr_viton_amd import functional as HF
    lib = _lib.load()
    N, H, W = case
    f = E.tv_case(case)["f"]
    ref = E.tv_ref(f)
    gb, lb = E.tv_grad_bound(ref), E.tv_loss_bound(ref)
    fd = f.cuda()
    grad = torch.full((f.numel() + 8,), NAN, device="cuda")
    ws, out = torch.full((1024,), NAN, device="cuda"), torch.full((1,), NAN, device="cuda")
    _lib.check(lib.hrv_tv_loss_f32(fd.data_ptr(), N, H, W, grad.data_ptr(), ws.data_ptr(), out.data_ptr(), None), "hrv_tv_loss_f32")
    torch.cuda.synchronize()
    assert bool(torch.isnan(grad[f.numel():]).all()) and not bool(torch.isnan(grad[:f.numel()]).any())
    gerr = float((grad[:f.numel()].view_as(fd).cpu().double() - ref["grad"]).abs().max())
    lerr = abs(float(out[0].double()) - float(ref["loss"]))
    print(f"tv {case}: gradient worst |error| / bound = {gerr / gb:.3g}, loss |error| / bound = {lerr / lb:.3g}")
    assert gerr <= gb and lerr <= lb, (case, gerr / gb, lerr / lb)
    fr = fd.clone().requires_grad_(True)
    loss = HF.tv_loss(fr)
    loss.backward()
    torch.cuda.synchronize()
    assert torch.equal(loss.detach().reshape(1), out) and torch.equal(fr.grad, grad[:f.numel()].view_as(fd)), f"{case}: functional.tv_loss"
    out2 = torch.full((1,), NAN, device="cuda")
    _lib.check(lib.hrv_tv_loss_f32(fd.data_ptr(), N, H, W, None, ws.data_ptr(), out2.data_ptr(), None), "hrv_tv_loss_f32")
    torch.cuda.synchronize()
    assert torch.equal(out2, out), f"{case}: without a gradient"
