"""The InstanceNorm statistics (csrc/norm.hip) and the SPADE / InstanceNorm backward (csrc/norm_bwd.hip) against float64 CPU
references on dyadic operands (tests/norm_exact_cases.py: why every sum is exact in fp32 in any order; tests/
test_norm_exact_cases_cpu.py proves the conditions on the references alone, and that these assertions fail on a dropped pixel or
a swapped finalize row).  The extents reach both finalize strides (more than 16 / 64 slabs), the slab cap with and without an
empty last slab, a cap made by HRV_NORM_SLABS_MAX, and channel counts on both sides of a chunk; every operand sits in a slice of
a poisoned tensor.

  mean / rstd                    the float64 value rounded to fp32, or its neighbour
  dnh, dbeta, fp32 dgamma        torch.equal;  bf16 dgamma: torch.equal with the exact value rounded to nearest-even
  m1, m2 (in the workspace)      torch.equal with (S / HW in float64).to(float32)
  dx, dnoise_scale               the derived bounds of norm_exact_cases.dx_check / dns_check, with the kernel's own m1 / m2

Nothing here depends on the order of the sums or on the slab rule, so a rewrite of these kernels is accepted against this file
unchanged."""
import ctypes as C

import pytest
import torch

import norm_exact_cases as E
from test_gpu_norm_bwd_instances import POISON, _Buf, _one_norm

pytestmark = pytest.mark.gpu


def _mods():
    import hr_viton_amd  # noqa: F401
    from hr_viton_amd import _lib, ops
    return _lib, ops


def _switches(monkeypatch, e, generic=None):
    """HRV_NORM_SLABS_MAX of the extent (and the generic kernels forced or not); every workspace is sized after this.  (monkeypatch
    restores the environment, conftest's fixture reloads the library's cache after that.)"""
    _lib, _ = _mods()
    if e.cap:
        monkeypatch.setenv("HRV_NORM_SLABS_MAX", str(e.cap))
    else:
        monkeypatch.delenv("HRV_NORM_SLABS_MAX", raising=False)
    if generic is not None:
        monkeypatch.setenv("HRV_NORM_BWD_GENERIC", "1" if generic else "0")
    _lib.reload_env()
    lib = _lib.load()
    assert lib.hrv_instnorm_workspace_elems(1, e.H, e.W, 4) == E.geometry(e.H, e.W, 4, e.cap).NB * 8     # the switch arrived
    return lib


# ---------------------------------------------------------------------------------------------------------------
# statistics
# ---------------------------------------------------------------------------------------------------------------
def _act(ops, t, bf16=False):
    """t [N, H, W, C] as a slice (coff 4, 8 pad channels) of a poisoned tensor"""
    b = _Buf(t.shape[0], t.shape[1], t.shape[2], t.shape[3], bf16, fill=t.cuda())
    return ops.Act(b.t, b.C, b.coff), b


def _padded(ns, Cp):
    out = torch.zeros(Cp)
    out[:ns.numel()] = ns
    return out.cuda()


def _stats_direct(lib, _lib, x, z, ns, eps=1e-5):
    """the four C entry points with mean / rstd buffers that carry 8 poisoned elements past N * C.  x: a _Buf (fp32 or bf16) or
    an (lo, hi) pair of them; z, ns: None, one noise term, or a pair of them (the two-norm pass).  -> [(mean, rstd) [N, C]]"""
    up = isinstance(x, tuple)
    N, H, W = (x[1] if up else x).t.shape[:3]
    Cn = x[0].C + x[1].C if up else x.C
    two = isinstance(z, (tuple, list))
    ws = torch.zeros((2 if two else 1) * lib.hrv_instnorm_workspace_elems(N, H, W, Cn), device="cuda")
    st = [torch.full((N * Cn + 8,), POISON, device="cuda") for _ in range(4 if two else 2)]
    ptr = lambda t: None if t is None else t.data_ptr()
    if up:
        lo, hi = x
        _lib.check(lib.hrv_instnorm_stats2_up_nhwc_f32(lo.t.data_ptr(), lo.cs, lo.coff, lo.C, hi.t.data_ptr(), hi.cs, hi.coff, N, H, W, Cn,
                                                       z[0].data_ptr(), ns[0].data_ptr(), z[1].data_ptr(), ns[1].data_ptr(), eps, ws.data_ptr(),
                                                       *[t.data_ptr() for t in st], None), "hrv_instnorm_stats2_up_nhwc_f32")
    elif two:
        _lib.check(lib.hrv_instnorm_stats2_nhwc_f32(x.t.data_ptr(), N, H, W, Cn, x.cs, x.coff, z[0].data_ptr(), ns[0].data_ptr(),
                                                    z[1].data_ptr(), ns[1].data_ptr(), eps, ws.data_ptr(), *[t.data_ptr() for t in st], None),
                   "hrv_instnorm_stats2_nhwc_f32")
    else:
        fn = lib.hrv_instnorm_stats_nhwc_bf16 if x.bf16 else lib.hrv_instnorm_stats_nhwc_f32
        _lib.check(fn(x.t.data_ptr(), N, H, W, Cn, x.cs, x.coff, ptr(z), ptr(ns), eps, ws.data_ptr(), st[0].data_ptr(), st[1].data_ptr(), None),
                   "hrv_instnorm_stats_nhwc")
    torch.cuda.synchronize()
    for t in st:
        assert bool((t[N * Cn:] == POISON).all()), "mean / rstd written past N * C"
    return [(st[i][:N * Cn].view(N, Cn).cpu(), st[i + 1][:N * Cn].view(N, Cn).cpu()) for i in range(0, len(st), 2)]


def _check_pair(got, ref, what):
    E.stats_check(got[0].cpu(), got[1].cpu(), ref, what)


@pytest.mark.parametrize("e", E.STATS_EXTENTS, ids=E.ext_id)
def test_statistics_against_float64(e, monkeypatch):
    _lib, ops = _mods()
    lib = _switches(monkeypatch, e)
    c = E.stats_case(e)
    z = [t.cuda() for t in c["z"]]
    got = {}
    for bf16 in (False, True):
        a, buf = _act(ops, c["x"], bf16)
        ns = [_padded(t, a.Cp) for t in c["ns"]]
        for key, zz, nn in (("plain", None, None), ("a", z[0], ns[0]), ("b", z[1], ns[1])):
            mean, rstd = ops.instnorm_stats(a, zz, nn)
            got[bf16, key] = (mean[:, :e.C].cpu(), rstd[:, :e.C].cpu())
            _check_pair(got[bf16, key], c["ref"][key], f"instnorm_stats {'bf16' if bf16 else 'fp32'} {key}")
        assert buf.pad_intact()
    # the two-norm pass: the same values, and bit for bit the two single passes
    a, buf = _act(ops, c["x"])
    ns = [t.cuda() for t in c["ns"]]
    for k, pair in zip("ab", ops.instnorm_stats2(a, z[0], ns[0], z[1], ns[1])):
        _check_pair(pair, c["ref"][k], f"instnorm_stats2 {k}")
        assert torch.equal(pair[0].cpu(), got[False, k][0]) and torch.equal(pair[1].cpu(), got[False, k][1]), k
    # ... and over x = cat(up2(lo), hi), never materialised
    for up_c in E.stats_up_splits(e):
        lo, hi, _v, ref = E.stats_up_parts(c, up_c)
        (la, lb), (ha, hb) = _act(ops, lo), _act(ops, hi)
        if up_c % 16 == 0:
            res = ops.instnorm_stats2(ops.ActUp(la, ha), z[0], ns[0], z[1], ns[1])
        else:                                          # (ops.ActUp takes the generator's multiples of 16 only)
            res = _stats_direct(lib, _lib, (lb, hb), z, ns)
        am, _ = _act(ops, torch.cat([E._up2(lo), hi], -1))
        for k, pair, zz, nn in zip("ab", res, z, ns):
            _check_pair(pair, ref[k], f"instnorm_stats2 up_c={up_c} {k}")
            single = ops.instnorm_stats(am, zz, nn)
            assert torch.equal(pair[0].cpu(), single[0].cpu()) and torch.equal(pair[1].cpu(), single[1].cpu()), (up_c, k)
        assert lb.pad_intact() and hb.pad_intact()


def test_statistics_keep_the_shift(monkeypatch):
    """x = 2048 + {-2..2}: exact with the shift by pixel 0, far beyond fp32 without it"""
    _lib, ops = _mods()
    e = E.SHIFT_CASE
    _switches(monkeypatch, e)
    c = E.stats_case(e, True)
    a, _buf = _act(ops, c["x"])
    z, ns = [t.cuda() for t in c["z"]], [t.cuda() for t in c["ns"]]
    _check_pair(ops.instnorm_stats(a), c["ref"]["plain"], "shifted plain")
    _check_pair(ops.instnorm_stats(a, z[0], ns[0]), c["ref"]["a"], "shifted a")
    for k, pair in zip("ab", ops.instnorm_stats2(a, z[0], ns[0], z[1], ns[1])):
        _check_pair(pair, c["ref"][k], f"shifted stats2 {k}")


@pytest.mark.parametrize("e", [E.STATS_EXTENTS[8], E.LARGE[4]], ids=E.ext_id)
def test_statistics_write_nothing_past_their_n_times_c_results(e, monkeypatch):
    """every entry point on result buffers with poisoned elements behind mean / rstd [N][C]"""
    _lib, ops = _mods()
    lib = _switches(monkeypatch, e)
    c = E.stats_case(e)
    z, ns = [t.cuda() for t in c["z"]], [t.cuda() for t in c["ns"]]
    x32 = _act(ops, c["x"])[1]
    _check_pair(_stats_direct(lib, _lib, x32, None, None)[0], c["ref"]["plain"], "fp32 plain")
    _check_pair(_stats_direct(lib, _lib, x32, z[0], ns[0])[0], c["ref"]["a"], "fp32 a")
    if e.C % 8 == 0:
        _check_pair(_stats_direct(lib, _lib, _act(ops, c["x"], True)[1], z[1], ns[1])[0], c["ref"]["b"], "bf16 b")
    for k, pair in zip("ab", _stats_direct(lib, _lib, x32, z, ns)):
        _check_pair(pair, c["ref"][k], f"stats2 {k}")
    for up_c in E.stats_up_splits(e):
        lo, hi, _v, ref = E.stats_up_parts(c, up_c)
        for k, pair in zip("ab", _stats_direct(lib, _lib, (_act(ops, lo)[1], _act(ops, hi)[1]), z, ns)):
            _check_pair(pair, ref[k], f"stats2 up {k}")


# ---------------------------------------------------------------------------------------------------------------
# backward
# ---------------------------------------------------------------------------------------------------------------
RUNS = E.backward_runs()


@pytest.mark.parametrize("run", RUNS, ids=E.run_id)
def test_backward_against_float64(run, monkeypatch):
    form, e, generic = run
    _lib, _ = _mods()
    lib = _switches(monkeypatch, e, generic)
    d = E.bwd_case(form.id, e)
    N, H, W, Cn = e.N, e.H, e.W, e.C
    geo = E.geometry(H, W, Cn, e.cap)
    if form.up:
        x = (_Buf(N, H // 2, W // 2, d["lo"].shape[-1], False, fill=d["lo"].cuda()), _Buf(N, H, W, d["hi"].shape[-1], False, fill=d["hi"].cuda()))
    else:
        x = _Buf(N, H, W, Cn, False, fill=d["x"].cuda())
    dx = _Buf(N, H, W, Cn, form.dx == "bf16", fill=None if d["dx0"] is None else d["dx0"].cuda())
    norms = []
    for k, o in enumerate(d["norms"]):
        given = dict(o)
        if k == 0 and d["dns0"] is not None:
            given["dns0"] = d["dns0"]
        norms.append(_one_norm(form, N, H, W, Cn, 0, x, dx, given=given))
    da = norms[0][0]
    if form.pair:
        db = norms[1][0]
        route = lib.hrv_diag_norm_bwd_route(C.byref(da), C.byref(db))
        _lib.check(lib.hrv_spade_norm_bwd2_nhwc_f32(C.byref(da), C.byref(db), None), "hrv_spade_norm_bwd2_nhwc_f32")
    else:
        route = lib.hrv_diag_norm_bwd_route(C.byref(da), None)
        _lib.check(lib.hrv_spade_norm_bwd_nhwc_f32(C.byref(da), None), "hrv_spade_norm_bwd_nhwc_f32")
    torch.cuda.synchronize()
    assert route == (0 if generic else form.route), route
    total = lib.hrv_norm_bwd_workspace_elems(N, H, W, Cn)          # [slab partials | m1 [N][C] | m2 [N][C]]
    assert total == N * geo.NB * Cn * 2 + 2 * N * Cn
    terms = []
    for k, ((_desc, outs, flat, _keep), o, r) in enumerate(zip(norms, d["norms"], d["refs"])):
        what = f"{E.run_id(run)} norm {'ab'[k]}"
        dnh = outs["dnh"].t[..., :Cn].cpu().double()
        assert torch.equal(dnh, r["dnh"]), f"{what} dnh: {int((dnh != r['dnh']).sum())} of {dnh.numel()} differ"
        if "dgb" in outs:
            b = outs["dgb"]
            dgamma, dbeta = b.t[..., b.coff:b.coff + Cn].cpu(), b.t[..., b.coff + Cn:b.coff + 2 * Cn].cpu()
            want = E.to_bf16_rne(r["dgamma"]) if b.bf16 else r["dgamma"].float()
            assert torch.equal(dgamma, want), f"{what} dgamma: {int((dgamma != want).sum())} of {want.numel()} differ"
            assert torch.equal(dbeta.double(), r["dbeta"]), f"{what} dbeta"
        ws = flat["workspace"]
        assert ws.numel() == total
        m1, m2 = ws[total - 2 * N * Cn:total - N * Cn].view(N, Cn).cpu(), ws[total - N * Cn:].view(N, Cn).cpu()
        E.m_check(m1, m2, r, what)
        term, bracket = E.dx_term(r, m1, m2)
        terms.append((term, bracket))
        if "dnoise_scale" in flat:
            worst = E.dns_check(flat["dnoise_scale"].cpu(), term, bracket, o["z"], geo, old=d["dns0"] if k == 0 else None, what=what)
            print(f"{what}: dnoise_scale worst |error| / bound = {worst:.3g}")
        for name, b in outs.items():
            assert b.pad_intact(), f"{what} {name}: padding overwritten"
            assert not bool(torch.isnan(b.t.float()).any()), f"{what} {name}: NaN"
    worst = E.dx_check(dx.t[..., dx.coff:dx.coff + Cn].cpu(), terms, old=d["dx0"], bf16=dx.bf16, what=E.run_id(run))
    print(f"{E.run_id(run)}: dx worst |error| / bound = {worst:.3g}")
