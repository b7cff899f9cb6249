"""Every compile-time instance of the SPADE / InstanceNorm backward (csrc/norm_bwd.hip) against the generic run-time
kernels on the same descriptor: HRV_NORM_BWD_GENERIC=1 forces the generic kernels, which are the kernels every result came from
before the instances existed.  Same statements in the same order, so every output is compared with torch.equal -- dx, dnh,
[dgamma | dbeta], the noise-scale gradient and the whole workspace (slab partials, m1 / m2 rows) -- including the poisoned pad
channels around each output slice, which must also still hold the poison.  Descriptors outside the table run on the generic kernels
either way (hrv_diag_norm_bwd_route says which kernels serve a descriptor)."""
import ctypes as C

import pytest
import torch

import norm_bwd_instance_cases as K

pytestmark = pytest.mark.gpu

POISON = 1.5e4          # exact in bf16 and fp32
ACT_NONE, ACT_LRELU = 0, 2


class _Buf:
    """a [N][H][W][cstride] tensor with a C-channel slice at coff: the slice is the operand, the rest is poison"""

    def __init__(self, N, H, W, Cn, bf16, pad=8, coff=4, fill=None):
        self.C, self.coff, self.cs = Cn, coff, Cn + pad
        self.t = torch.full((N, H, W, self.cs), POISON, dtype=torch.bfloat16 if bf16 else torch.float32, device="cuda")
        self.bf16 = bf16
        if fill is not None:
            self.t[..., coff:coff + Cn] = fill.to(self.t.dtype)

    def set(self, d, name, stride_name=None):
        setattr(d, name, self.t.data_ptr())
        setattr(d, (stride_name or name) + "_cstride", self.cs)
        setattr(d, (stride_name or name) + "_coff", self.coff)

    def pad_intact(self):
        m = torch.ones(self.cs, dtype=torch.bool, device="cuda")
        m[self.coff:self.coff + self.C] = False
        return bool((self.t[..., m] == POISON).all())


def _one_norm(case, N, H, W, Cn, seed, x, dx, given=None):
    """descriptor of one norm of ``case`` over x (a _Buf or an (lo, hi) pair of them) + everything it writes.  The operands are
    drawn from ``seed``, or taken from ``given`` (tests/test_gpu_norm_exact.py): mean, rstd, dout, and what the kind carries of
    z, ns, out, slope, g1p; optionally dns0, an old noise-scale gradient that is accumulated into"""
    from hr_viton_amd import _lib
    g = torch.Generator(device="cuda").manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g)
    pick = lambda name, draw: given[name].to("cuda", torch.float32).contiguous() if given is not None else draw()
    mixed = case.kind != "f32"
    d = _lib.hrv_norm_bwd_t()
    d.N, d.H, d.W, d.C = N, H, W, Cn
    keep = []
    if isinstance(x, tuple):
        lo, hi = x
        lo.set(d, "x")
        d.x_up_channels, d.x2, d.x2_cstride, d.x2_coff = lo.C, hi.t.data_ptr(), hi.cs, hi.coff
    else:
        x.set(d, "x")
    mean, rstd = pick("mean", lambda: rnd(N, Cn) * 0.3), pick("rstd", lambda: rnd(N, Cn).abs() + 0.5)
    d.mean, d.rstd = mean.data_ptr(), rstd.data_ptr()
    keep += [mean, rstd]
    noise = case.kind != "inorm"
    dns = None
    if noise:
        z, ns, dns = pick("z", lambda: rnd(N, W, H)), pick("ns", lambda: rnd(Cn) * 0.1), torch.full((Cn,), POISON, device="cuda")
        if given is not None and "dns0" in given:
            dns, d.dns_accumulate = given["dns0"].to("cuda", torch.float32).contiguous(), 1
        d.noise_z, d.noise_scale, d.dnoise_scale = z.data_ptr(), ns.data_ptr(), dns.data_ptr()
        keep += [z, ns]
    dout_v = pick("dout", lambda: rnd(N, H, W, Cn) * 0.1)
    dgb = None
    if case.kind == "spade":          # dout lives in the dbeta half of a bf16 [dgamma | dbeta]
        dgb = _Buf(N, H, W, 2 * Cn, True)
        dgb.t[..., dgb.coff + Cn:dgb.coff + 2 * Cn] = dout_v.to(torch.bfloat16)
        dgb.set(d, "dgb")
        d.dgb_bf16 = 1
        d.dout, d.dout_cstride, d.dout_coff, d.dout_bf16 = dgb.t.data_ptr(), dgb.cs, dgb.coff + Cn, 1
        d.act = ACT_NONE
    else:
        io = {"f32": (False, False), "bf16": (True, True), "mixed": (True, False)}[case.io]
        dout = _Buf(N, H, W, Cn, io[0], fill=dout_v)
        out = _Buf(N, H, W, Cn, io[1], fill=pick("out", lambda: rnd(N, H, W, Cn)))
        dout.set(d, "dout")
        out.set(d, "out")
        d.dout_bf16, d.out_bf16, d.act, d.act_slope = int(io[0]), int(io[1]), ACT_LRELU, given["slope"] if given is not None else 0.2
        keep += [dout, out]
        if case.kind == "f32":
            dgb = _Buf(N, H, W, 2 * Cn, False)
            dgb.set(d, "dgb")
    if case.kind != "inorm":
        g1p = _Buf(N, H, W, Cn, case.g1p == "bf16", fill=pick("g1p", lambda: 1.0 + rnd(N, H, W, Cn) * 0.2))
        g1p.set(d, "g1p")
        d.g1p_bf16 = int(g1p.bf16)
        keep.append(g1p)
    dnh = _Buf(N, H, W, Cn, mixed, pad=4, coff=0)
    dnh.set(d, "dnh")
    d.dnh_bf16 = int(mixed)
    dx.set(d, "dx")
    d.dx_bf16, d.dx_accumulate = int(dx.bf16), int(case.dx == "acc")
    ws = torch.zeros(_lib.load().hrv_norm_bwd_workspace_elems(N, H, W, Cn), device="cuda")
    d.workspace = ws.data_ptr()
    outs = {"dnh": dnh, "dx": dx}
    if dgb is not None:
        outs["dgb"] = dgb
    return d, outs, {"workspace": ws, **({"dnoise_scale": dns} if dns is not None else {})}, keep


def _run(case, ext, generic, monkeypatch):
    """-> (route, {name: tensor incl. its padding}, {name: pad channels still poisoned})"""
    from hr_viton_amd import _lib
    lib = _lib.load()
    monkeypatch.setenv("HRV_NORM_BWD_GENERIC", "1" if generic else "0")
    _lib.reload_env()
    N, H, W, Cn = ext
    g = torch.Generator(device="cuda").manual_seed(7)
    if case.up:
        x = (_Buf(N, H // 2, W // 2, Cn - 16, False, fill=torch.randn(N, H // 2, W // 2, Cn - 16, device="cuda", generator=g)),
             _Buf(N, H, W, 16, False, fill=torch.randn(N, H, W, 16, device="cuda", generator=g)))
    else:
        x = _Buf(N, H, W, Cn, False, fill=torch.randn(N, H, W, Cn, device="cuda", generator=g))
    dx = _Buf(N, H, W, Cn, case.dx == "bf16", fill=torch.randn(N, H, W, Cn, device="cuda", generator=g) if case.dx == "acc" else None)
    da, outs_a, flat_a, keep_a = _one_norm(case, N, H, W, Cn, 11, x, dx)
    res = [("a", outs_a, flat_a)]
    if case.pair:
        db, outs_b, flat_b, keep_b = _one_norm(case, N, H, W, Cn, 12, x, dx)
        outs_b.pop("dx")
        res.append(("b", outs_b, flat_b))
        route = lib.hrv_diag_norm_bwd_route(C.byref(da), C.byref(db))
        _lib.check(lib.hrv_spade_norm_bwd2_nhwc_f32(C.byref(da), C.byref(db), None), "hrv_spade_norm_bwd2_nhwc_f32")
    else:
        route = lib.hrv_diag_norm_bwd_route(C.byref(da), None)
        _lib.check(lib.hrv_spade_norm_bwd_nhwc_f32(C.byref(da), None), "hrv_spade_norm_bwd_nhwc_f32")
    torch.cuda.synchronize()
    tensors, pads = {}, {}
    for tag, outs, flat in res:
        for k, b in outs.items():
            tensors[f"{tag}.{k}"] = b.t
            pads[f"{tag}.{k}"] = b.pad_intact()
        for k, t in flat.items():
            tensors[f"{tag}.{k}"] = t
    return route, tensors, pads


@pytest.mark.parametrize("ext", K.EXTENTS, ids=lambda e: "x".join(map(str, e)))
@pytest.mark.parametrize("case", K.CASES, ids=lambda c: c.id)
def test_an_instance_equals_the_generic_kernels_bit_for_bit(case, ext, monkeypatch):
    route_g, want, pads_g = _run(case, ext, True, monkeypatch)
    route_i, got, pads_i = _run(case, ext, False, monkeypatch)
    assert route_g == 0, "HRV_NORM_BWD_GENERIC=1 routes every stage to the generic kernels"
    assert route_i == case.route, f"stages on an instance: {route_i}, expected {case.route}"
    assert want.keys() == got.keys()
    for k in want:
        assert not torch.isnan(want[k].float()).any(), k
        assert torch.equal(want[k], got[k]), f"{k}: {int((want[k] != got[k]).sum())} of {want[k].numel()} elements differ"
    assert all(pads_g.values()) and all(pads_i.values()), (pads_g, pads_i)
    # the outputs were written at all (an untouched buffer would still be poison / zero)
    assert not bool((got["a.dx"][..., 4:4 + ext[3]] == POISON).any())
    assert bool((got["a.workspace"] != 0).any())
    if "a.dnoise_scale" in got:
        assert not bool((got["a.dnoise_scale"] == POISON).any())


def test_the_cases_ran_every_instance_of_the_library():
    """(the CPU test pins the three lists to each other; here the library on the GPU box is asked once more)"""
    from hr_viton_amd import train_ops as T
    assert sorted(T.norm_bwd_instances()) == K.instance_lines()


def test_the_pair_gate_follows_the_instances_and_the_switch(monkeypatch):
    """hrv_spade_norm_bwd2_supported: never for a pair whose stages are not both instances, never with the generic kernels forced"""
    from hr_viton_amd import _lib
    lib = _lib.load()
    by_id = {c.id: c for c in K.CASES}
    for cid, generic, may in (("outside_pair_all_f32", False, False), ("outside_pair_materialised_bf16_g1p", False, False),
                              ("pair_fine", True, False)):
        case = by_id[cid]
        monkeypatch.setenv("HRV_NORM_BWD_GENERIC", "1" if generic else "0")
        _lib.reload_env()
        N, H, W, Cn = K.EXTENTS[0]
        if case.up:
            x = (_Buf(N, H // 2, W // 2, Cn - 16, False), _Buf(N, H, W, 16, False))
        else:
            x = _Buf(N, H, W, Cn, False)
        dx = _Buf(N, H, W, Cn, False)
        da, *_a = _one_norm(case, N, H, W, Cn, 1, x, dx)
        db, *_b = _one_norm(case, N, H, W, Cn, 2, x, dx)
        assert bool(lib.hrv_spade_norm_bwd2_supported(C.byref(da), C.byref(db))) == may, cid
