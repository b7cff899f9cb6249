"""The spectral-norm kernels, the per-step staging kernels (csrc/train.hip, tap_expand of csrc/glue.hip) and scale / tanh_bwd /
act_bwd against the references of tests/param_exact_cases.py (why every sum of the exact tiers is exact in fp32 in any order, how the
bounds of the Gaussian tiers are derived; tests/test_param_exact_cases_cpu.py proves the conditions on the references alone, and that
these assertions fail on each seeded defect).

  spectral forward on exact singular pairs (per layer, the whole table as one batch, 45 jobs in two chunks), W = 0,
  spectral backward on integer operands, scale, tanh_bwd, act_bwd                                   torch.equal
  shared_taps_prep / _grad, spade_vec_prep / _multi, tap_expand                                     the bit pattern
  spectral forward and backward on Gaussian operands                                                the derived bounds, stage by stage

Every output buffer starts as NaN (or as the old value where the kernel accumulates), operands and results sit inside poisoned
buffers wherever the entry point lets the test own the buffer, and where a Python wrapper allocates its own output the C entry point
runs on buffers of the test and the wrapper has to return the same bits.  Nothing here depends on the order of a sum.  The used
shares of the derived bounds go to test_diagnostics/param_exact_shares.txt."""
import ctypes as C

import pytest
import torch

import param_exact_cases as P
from conftest import diag_path

pytestmark = pytest.mark.gpu
NAN = float("nan")
PAD = 8                    # elements of poison on either side of an operand: 32 bytes (fp32) / 16 bytes (bf16), so 16-byte aligned
_SHARES = {}


def _mods():
    import hr_viton_amd  # noqa: F401
    from hr_viton_amd import _lib, ops, train_ops as T
    return _lib, ops, T


class _Buf:
    """a flat operand (``fill``) or result (NaN until written) inside a poisoned device buffer"""

    def __init__(self, fill=None, n=None, dtype=torch.float32, init=NAN):
        n = fill.numel() if fill is not None else n
        self.n = n
        self.t = torch.full((n + 2 * PAD,), P.POISON, dtype=dtype, device="cuda")
        self.v = self.t[PAD:PAD + n]
        if fill is not None:
            self.v.copy_(fill.reshape(-1))
        else:
            self.v.fill_(init)
        assert self.v.data_ptr() % 16 == 0

    def ptr(self):
        return self.v.data_ptr()

    def intact(self):
        return bool((self.t[:PAD] == P.POISON).all() and (self.t[PAD + self.n:] == P.POISON).all())


def _equal(got, want, what):
    """torch.equal of a result with the float64 reference (which has to be exact in fp32), on the device that holds the result"""
    w = want.to(torch.float32)
    assert torch.equal(w.double(), want.double()), f"{what}: the reference is not exact in fp32"
    w = w.to(got.device).reshape(got.shape)
    if not torch.equal(got, w):
        bad = ((got != w) | torch.isnan(got)).reshape(-1).nonzero()
        i = int(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {w.numel()} differ, first at {i}: {float(got.reshape(-1)[i])!r} vs {float(w.reshape(-1)[i])!r}")


def _same_bits(got, want, what):
    g, w = P.bits(got), P.bits(want.to(got.device))
    if not torch.equal(g, w.reshape(g.shape)):
        bad = (g != w.reshape(g.shape)).reshape(-1).nonzero()
        raise AssertionError(f"{what}: {len(bad)} of {g.numel()} bit patterns differ, first at {int(bad[0])}")


def _note(key, value):
    _SHARES[key] = max(_SHARES.get(key, 0.0), value)
    with open(diag_path("param_exact_shares.txt"), "w") as f:
        f.write("largest |error| / derived bound seen by tests/test_gpu_param_exact.py in this run\n")
        for k in sorted(_SHARES):
            f.write(f"{k:40s} {_SHARES[k]:.4g}\n")


# ---------------------------------------------------------------------------------------------------------------
# 1. spectral forward on exact singular pairs
# ---------------------------------------------------------------------------------------------------------------
def _sn_dev(W, u, v):
    return _Buf(W), _Buf(u), _Buf(v)


def _sn_per_layer(_lib, W, u0, v0, iters):
    """the C entry point on buffers of the test -> (W, u, v, sigma, scratch) buffers"""
    R, K = W.shape
    bw, bu, bv = _sn_dev(W, u0, v0)
    sig, scr = _Buf(n=1), _Buf(n=R)
    _lib.check(_lib.load().hrv_spectral_norm_f32(bw.ptr(), R, K, bu.ptr(), bv.ptr(), iters, P.SN_EPS, scr.ptr(), sig.ptr(), None),
               "hrv_spectral_norm_f32")
    torch.cuda.synchronize()
    return bw, bu, bv, sig, scr


def _check_sn(bufs, W, ref, what):
    bw, bu, bv, sig, scr = bufs
    _equal(bv.v, ref["v"], what + " v")
    _equal(bu.v, ref["u"], what + " u")
    _equal(sig.v, ref["sigma"], what + " sigma")
    _equal(scr.v, ref["wv"], what + " W v (scratch)")
    assert torch.equal(bw.v.cpu(), W.reshape(-1)), what + ": W was modified"
    assert all(b.intact() for b in bufs), what + ": written outside a buffer"


@pytest.mark.parametrize("R,K", P.SN_SHAPES, ids=str)
def test_spectral_per_layer_on_exact_singular_pairs(R, K):
    _lib, ops, T = _mods()
    c = P.sn_case(R, K)
    for iters in (0, 1, 2):
        ref = P.sn_ref(c["W"], c["p"], c["q"], iters)
        bufs = _sn_per_layer(_lib, c["W"], c["p"], c["q"], iters)
        _check_sn(bufs, c["W"], ref, f"{R} x {K}, {iters} iteration(s)")
        # the wrapper (its own scratch and sigma): the same bits
        bw, bu, bv = _sn_dev(c["W"], c["p"], c["q"])
        sigma = T.spectral_sigma(bw.v.view(R, K), bu.v, bv.v, iters)
        torch.cuda.synchronize()
        assert torch.equal(sigma, bufs[3].v) and torch.equal(bu.v, bufs[1].v) and torch.equal(bv.v, bufs[2].v), f"{R} x {K}: the wrapper"


def _batch_items(shapes, zero_last=False):
    """device buffers (W, u0 = p, v0 = q) per job and the operands on the CPU; ``zero_last``: one more job with W = 0"""
    cpu = [(P.sn_case(R, K)["W"], P.sn_case(R, K)["p"], P.sn_case(R, K)["q"]) for R, K in shapes]
    if zero_last:
        c = P.sn_case(*P.SN_ZERO)
        cpu.append((torch.zeros(*P.SN_ZERO), c["p"], c["q"]))
    return cpu, [_sn_dev(W, u, v) for W, u, v in cpu]


@pytest.mark.parametrize("iters", [0, 1, 2])
def test_spectral_batch_of_the_whole_table(iters):
    """every shape of the table (and W = 0) as the jobs of ONE batch: sn_find crosses a prefix boundary per job, with unequal block
    counts on both prefixes"""
    _lib, ops, T = _mods()
    cpu, dev = _batch_items(P.SN_SHAPES, zero_last=True)
    sig, uk, vk = T.SpectralBatch([(bw.v.view(W.shape), bu.v, bv.v) for (W, _, _), (bw, bu, bv) in zip(cpu, dev)]).run(iters)
    torch.cuda.synchronize()
    for j, ((W, u0, v0), (bw, bu, bv)) in enumerate(zip(cpu, dev)):
        ref = P.sn_ref(W, u0, v0, iters)
        what = f"job {j} ({W.shape[0]} x {W.shape[1]}), {iters} iteration(s)"
        _equal(bv.v, ref["v"], what + " v")
        _equal(bu.v, ref["u"], what + " u")
        _equal(sig[j], ref["sigma"], what + " sigma")
        _equal(uk[j], ref["u_keep"], what + " u_keep")
        _equal(vk[j], ref["v_keep"], what + " v_keep")
        assert torch.equal(bw.v.cpu(), W.reshape(-1)) and bw.intact() and bu.intact() and bv.intact(), what


def test_spectral_batch_second_chunk_continues_the_scratch():
    """45 jobs: a second SN_MAX chunk.  The C entry point on a NaN-filled scratch of exactly sum(R) floats: job j's W v sits at its
    running offset across the chunks, and sigma / u_keep / v_keep are buffers of the test"""
    _lib, ops, T = _mods()
    shapes = P.SN_SMALL
    cpu, dev = _batch_items(shapes)
    refs = [P.sn_ref(W, u0, v0, 1) for W, u0, v0 in cpu]
    n, sR, sK = len(shapes), sum(R for R, _ in shapes), sum(K for _, K in shapes)
    assert n > P.SN_MAX
    scr, sig, uk, vk = _Buf(n=sR), _Buf(n=n), _Buf(n=sR), _Buf(n=sK)
    jobs = (_lib.hrv_sn_job_t * n)()
    ro = ko = 0
    for j, ((R, K), (bw, bu, bv)) in enumerate(zip(shapes, dev)):
        J = jobs[j]
        J.w, J.u, J.v, J.R, J.K = bw.ptr(), bu.ptr(), bv.ptr(), R, K
        J.sigma, J.u_keep, J.v_keep = sig.ptr() + 4 * j, uk.ptr() + 4 * ro, vk.ptr() + 4 * ko
        ro, ko = ro + R, ko + K
    _lib.check(_lib.load().hrv_spectral_norm_batched_f32(jobs, n, 1, P.SN_EPS, scr.ptr(), None), "hrv_spectral_norm_batched_f32")
    torch.cuda.synchronize()
    _equal(scr.v, P.sn_scratch_ref(shapes, [r["wv"] for r in refs]), "scratch")
    _equal(sig.v, torch.cat([r["sigma"] for r in refs]), "sigma")
    _equal(uk.v, torch.cat([r["u_keep"] for r in refs]), "u_keep")
    _equal(vk.v, torch.cat([r["v_keep"] for r in refs]), "v_keep")
    for j, (r, (bw, bu, bv)) in enumerate(zip(refs, dev)):
        _equal(bu.v, r["u"], f"job {j} u")
        _equal(bv.v, r["v"], f"job {j} v")
    assert all(b.intact() for b in (scr, sig, uk, vk)) and all(b.intact() for bufs in dev for b in bufs)
    # the wrapper (its own buffers and the shared scratch): the same bits
    cpu2, dev2 = _batch_items(shapes)
    sig2, uk2, vk2 = T.SpectralBatch([(bw.v.view(W.shape), bu.v, bv.v) for (W, _, _), (bw, bu, bv) in zip(cpu2, dev2)]).run(1)
    torch.cuda.synchronize()
    assert torch.equal(torch.cat(sig2), sig.v) and torch.equal(torch.cat(uk2), uk.v) and torch.equal(torch.cat(vk2), vk.v)
    assert all(torch.equal(a[1].v, b[1].v) and torch.equal(a[2].v, b[2].v) for a, b in zip(dev, dev2))


def test_spectral_zero_weight_gives_exact_zeros():
    """W = 0: only the eps clamp stands between 0 * (1 / 0) and the result"""
    _lib, ops, T = _mods()
    R, K = P.SN_ZERO
    c = P.sn_case(R, K)
    Z = torch.zeros(R, K)
    for iters in (1, 2):
        bufs = _sn_per_layer(_lib, Z, c["p"], c["q"], iters)
        _check_sn(bufs, Z, P.sn_ref(Z, c["p"], c["q"], iters), f"W = 0, {iters} iteration(s)")
        assert not bool(bufs[1].v.any()) and not bool(bufs[2].v.any()) and float(bufs[3].v) == 0.0


# ---------------------------------------------------------------------------------------------------------------
# 2. spectral forward on Gaussian operands, stage by stage
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,K", P.SN_SHAPES, ids=str)
def test_spectral_per_layer_gaussian_stages(R, K):
    _lib, ops, T = _mods()
    d = P.sn_gauss_case(R, K)
    bufs = _sn_per_layer(_lib, d["W"], d["u0"], d["v0"], 1)
    sh = P.sn_gauss_check(d, bufs[1].v.cpu(), bufs[2].v.cpu(), bufs[3].v.cpu(), f"{R} x {K} per layer")
    print(f"{R} x {K} per layer: |error| / bound = " + ", ".join(f"{k} {s:.3g}" for k, s in sh.items()))
    for k, s in sh.items():
        _note(f"spectral forward per layer, {k}", s)
    assert all(b.intact() for b in bufs) and torch.equal(bufs[0].v.cpu(), d["W"].reshape(-1))


def test_spectral_batch_gaussian_stages():
    _lib, ops, T = _mods()
    cases = [P.sn_gauss_case(R, K) for R, K in P.SN_SHAPES]
    dev = [_sn_dev(d["W"], d["u0"], d["v0"]) for d in cases]
    sig, uk, vk = T.SpectralBatch([(bw.v.view(d["W"].shape), bu.v, bv.v) for d, (bw, bu, bv) in zip(cases, dev)]).run(1)
    torch.cuda.synchronize()
    for j, (d, (bw, bu, bv)) in enumerate(zip(cases, dev)):
        sh = P.sn_gauss_check(d, bu.v.cpu(), bv.v.cpu(), sig[j].cpu(), f"job {j} {tuple(d['W'].shape)}")
        for k, s in sh.items():
            _note(f"spectral forward batched, {k}", s)
        assert torch.equal(uk[j], bu.v) and torch.equal(vk[j], bv.v) and bw.intact() and bu.intact() and bv.intact()
    print("batched: |error| / bound = " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(_SHARES.items()) if "batched" in k))


# ---------------------------------------------------------------------------------------------------------------
# 3. spectral backward
# ---------------------------------------------------------------------------------------------------------------
def _sn_bwd(_lib, d, accumulate):
    R, K = d["G"].shape
    ops_ = [_Buf(d[k]) for k in ("G", "W", "u", "v", "sigma")]
    out = _Buf(d["old"]) if accumulate else _Buf(n=R * K)
    ws = _Buf(n=1024)
    _lib.check(_lib.load().hrv_spectral_norm_bwd_f32(*[b.ptr() for b in ops_[:5]], R, K, ws.ptr(), out.ptr(), 1 if accumulate else 0, None),
               "hrv_spectral_norm_bwd_f32")
    torch.cuda.synchronize()
    assert all(b.intact() for b in ops_ + [out, ws]), "written outside a buffer"
    for b, k in zip(ops_, ("G", "W", "u", "v", "sigma")):
        assert torch.equal(b.v.cpu(), d[k].reshape(-1)), f"{k} was modified"
    return out, ws, ops_


@pytest.mark.parametrize("R,K", P.SG_SHAPES, ids=str)
def test_spectral_backward_exact(R, K):
    _lib, ops, T = _mods()
    d = P.sg_case(R, K)
    for acc in (False, True):
        out, ws, ops_ = _sn_bwd(_lib, d, acc)
        assert float(ws.v[512]) == d["dot"], f"<G, W> = {float(ws.v[512])!r}, not {d['dot']!r}"
        _equal(out.v, P.sg_ref(d, acc), f"{R} x {K} accumulate={acc}")
        out2 = _Buf(d["old"]) if acc else _Buf(n=R * K)
        G, W, u, v, sg = (b.v for b in ops_)
        T.spectral_grad(G.view(R, K), W.view(R, K), u, v, sg, out2.v.view(R, K), accumulate=acc)
        torch.cuda.synchronize()
        assert torch.equal(out2.v, out.v) and out2.intact(), f"{R} x {K}: the wrapper"


@pytest.mark.parametrize("R,K", P.SG_GAUSS, ids=str)
def test_spectral_backward_gaussian(R, K):
    _lib, ops, T = _mods()
    d = P.sg_gauss_case(R, K)
    for acc in (False, True):
        out, _, _ = _sn_bwd(_lib, d, acc)
        share = P.sg_check(d, out.v.cpu().view(R, K), acc, f"{R} x {K} accumulate={acc}")
        print(f"spectral backward {R} x {K} accumulate={acc}: |error| / bound = {share:.3g}")
        _note("spectral backward", share)


# ---------------------------------------------------------------------------------------------------------------
# 4. staging kernels
# ---------------------------------------------------------------------------------------------------------------
def _ptrs(bufs):
    return (C.c_void_p * len(bufs))(*[b.ptr() for b in bufs])


@pytest.mark.parametrize("case", P.TAPS_CASES, ids=str)
def test_shared_taps_prep_and_grad(case):
    _lib, ops, T = _mods()
    lib = _lib.load()
    n, hid, c, cp = case
    d = P.taps_case(*case)
    ws, bs = [_Buf(w) for w in d["ws"]], [_Buf(b) for b in d["bs"]]
    wt, bt = _Buf(n=n * hid * 9 * cp), _Buf(n=n * hid)
    _lib.check(lib.hrv_shared_taps_prep_f32(_ptrs(ws), _ptrs(bs), n, hid, c, cp, wt.ptr(), bt.ptr(), None), "hrv_shared_taps_prep_f32")
    torch.cuda.synchronize()
    rw, rb = P.taps_prep_ref(d["ws"], d["bs"], cp)
    _same_bits(wt.v, rw.reshape(-1), f"{case} wt")                      # (+0 in the pad columns: a NaN left or a -0.0 fails)
    _same_bits(bt.v, rb, f"{case} bt")
    assert wt.intact() and bt.intact() and all(b.intact() for b in ws + bs)
    wt2, bt2 = T.shared_taps_prep([b.v.view(hid, c, 3, 3) for b in ws], [b.v for b in bs], cp)
    torch.cuda.synchronize()
    assert tuple(wt2.shape) == (n * hid, 9 * cp, 1, 1) and torch.equal(P.bits(wt2).reshape(-1), P.bits(wt.v)) and torch.equal(P.bits(bt2), P.bits(bt.v))
    # the inverse map: POISON in the pad columns of dw must not reach any gw
    dw, db = _Buf(d["dw"]), _Buf(d["db"])
    gws, gbs = [_Buf(n=hid * c * 9) for _ in range(n)], [_Buf(n=hid) for _ in range(n)]
    T.shared_taps_grad(dw.v.view(n * hid, 9 * cp), db.v, [g.v.view(hid, c, 3, 3) for g in gws], [g.v for g in gbs], cp)
    torch.cuda.synchronize()
    rgw, rgb = P.taps_grad_ref(d["dw"], d["db"], n, hid, c, cp)
    for i in range(n):
        _same_bits(gws[i].v, rgw[i].reshape(-1), f"{case} gw[{i}]")
        _same_bits(gbs[i].v, rgb[i], f"{case} gb[{i}]")
    assert all(g.intact() for g in gws + gbs) and dw.intact() and db.intact()
    # grad(prep(w)) == w
    back, backb = [_Buf(n=hid * c * 9) for _ in range(n)], [_Buf(n=hid) for _ in range(n)]
    T.shared_taps_grad(wt.v.view(n * hid, 9 * cp), bt.v, [g.v.view(hid, c, 3, 3) for g in back], [g.v for g in backb], cp)
    torch.cuda.synchronize()
    assert all(torch.equal(P.bits(g.v), P.bits(w.v)) for g, w in zip(back + backb, ws + bs)), f"{case}: grad(prep(w)) != w"


def _vec_single(_lib, gm, bt, ns):
    Cn = gm.numel()
    ncols, Cp = P.vec_sizes(Cn)
    ins = [_Buf(t) for t in (gm, bt, ns)]
    bc, nsp = _Buf(n=ncols), _Buf(n=Cp)
    _lib.check(_lib.load().hrv_spade_vec_prep_f32(*[b.ptr() for b in ins], Cn, bc.ptr(), nsp.ptr(), None), "hrv_spade_vec_prep_f32")
    torch.cuda.synchronize()
    assert bc.intact() and nsp.intact() and all(b.intact() for b in ins)
    return bc, nsp, ins


@pytest.mark.parametrize("Cn", P.VEC_C)
def test_spade_vec_prep(Cn):
    _lib, ops, T = _mods()
    gm, bt, ns = P.vec_case(Cn)
    bc, nsp, ins = _vec_single(_lib, gm, bt, ns)
    rbc, rns = P.vec_prep_ref(gm, bt, ns)
    _same_bits(bc.v, rbc, f"C={Cn} bias")
    _same_bits(nsp.v, rns, f"C={Cn} noise scale")
    bc2, ns2 = T.spade_vec_prep(*[b.v for b in ins])
    torch.cuda.synchronize()
    assert torch.equal(P.bits(bc2), P.bits(bc.v)) and torch.equal(P.bits(ns2), P.bits(nsp.v)), f"C={Cn}: the wrapper"


def test_spade_vec_prep_multi():
    """the whole table as the jobs of one call: the grid is sized by the largest C, and the blocks of a small job must write nothing
    outside its slice (poison between the slices); then 33 items through the wrapper, which takes the 32-job split"""
    _lib, ops, T = _mods()
    lib = _lib.load()
    Cs = P.VEC_C
    n = len(Cs)
    cases = [P.vec_case(Cn, j) for j, Cn in enumerate(Cs)]
    ins = [[_Buf(t) for t in c] for c in cases]
    GAP = 4
    ob, on = [0], [0]
    for Cn in Cs:
        ob.append(ob[-1] + P.vec_sizes(Cn)[0] + GAP)
        on.append(on[-1] + P.vec_sizes(Cn)[1] + GAP)
    bc_all, ns_all = _Buf(n=ob[-1], init=P.POISON), _Buf(n=on[-1], init=P.POISON)
    for j, Cn in enumerate(Cs):                                         # NaN where a job writes, poison between the slices
        bc_all.v[ob[j]:ob[j] + P.vec_sizes(Cn)[0]] = NAN
        ns_all.v[on[j]:on[j] + P.vec_sizes(Cn)[1]] = NAN
    I = C.c_int32 * n
    _lib.check(lib.hrv_spade_vec_prep_multi_f32(n, _ptrs([b[0] for b in ins]), _ptrs([b[1] for b in ins]), _ptrs([b[2] for b in ins]), I(*Cs),
                                                I(*ob[:n]), I(*on[:n]), bc_all.ptr(), ns_all.ptr(), None), "hrv_spade_vec_prep_multi_f32")
    torch.cuda.synchronize()
    want_bc, want_ns = torch.full((ob[-1],), P.POISON), torch.full((on[-1],), P.POISON)
    for j, c in enumerate(cases):
        rbc, rns = P.vec_prep_ref(*c)
        want_bc[ob[j]:ob[j] + rbc.numel()], want_ns[on[j]:on[j] + rns.numel()] = rbc, rns
    _same_bits(bc_all.v, want_bc, "multi bias")
    _same_bits(ns_all.v, want_ns, "multi noise scale")
    assert bc_all.intact() and ns_all.intact() and all(b.intact() for bs in ins for b in bs)
    # 33 items through the wrapper: every result has the bits of the single call
    items = [P.vec_case(Cn, j) for j, Cn in enumerate(Cs + Cs + Cs[:1])]
    assert len(items) == P.VEC_SPLIT + 1
    got = T.spade_vec_prep_multi([tuple(t.cuda() for t in it) for it in items])
    torch.cuda.synchronize()
    for it, (bc, nsp) in zip(items, got):
        sbc, sns, _ = _vec_single(_lib, *it)
        assert torch.equal(P.bits(bc), P.bits(sbc.v)) and torch.equal(P.bits(nsp), P.bits(sns.v)), f"C={it[0].numel()}: multi != single"
        _same_bits(bc, P.vec_prep_ref(*it)[0], f"C={it[0].numel()} wrapper bias")


@pytest.mark.parametrize("case", P.TAP_CASES, ids=str)
def test_tap_expand(case):
    _lib, ops, T = _mods()
    bf16, Cp, down, N, H, W, sliced = case
    src = P.tap_source(case)
    dt = torch.bfloat16 if bf16 else torch.float32
    es, g = (2, 8) if bf16 else (4, 4)                                  # element size, elements of one 16-byte group
    coff, cs = (g, Cp + 3 * g) if sliced else (0, Cp)
    wide = torch.full((N, H << down, W << down, cs), P.POISON, dtype=dt, device="cuda")
    wide[..., coff:coff + Cp] = src.cuda()
    ref = P.tap_expand_ref(src, down, H, W)
    out = _Buf(n=ref.numel(), dtype=dt)
    _lib.check(_lib.load().hrv_tap_expand_nhwc(wide.data_ptr(), N, H, W, Cp * es // 16, cs * es // 16, coff * es // 16, down, 3, 3, 1, out.ptr(), None),
               "hrv_tap_expand_nhwc")
    torch.cuda.synchronize()
    _same_bits(out.v, ref.reshape(-1), f"{case}")
    assert out.intact()
    via = ops.tap_expand(ops.Act(wide, Cp, coff), down, 3)
    torch.cuda.synchronize()
    assert tuple(via.t.shape) == (N, H, W, 9 * Cp) and via.C == 9 * Cp and torch.equal(P.bits(via.t).reshape(-1), P.bits(out.v)), f"{case}: the wrapper"
    m = torch.ones(cs, dtype=torch.bool, device="cuda")
    m[coff:coff + Cp] = False
    assert bool((wide[..., m] == P.POISON).all()) and torch.equal(P.bits(wide[..., coff:coff + Cp]), P.bits(src.cuda()))


# ---------------------------------------------------------------------------------------------------------------
# 5. element-wise kernels
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", P.EW_N)
def test_scale(n):
    _lib, ops, T = _mods()
    d = P.ew_operands(n)
    for s_host, s_dev in P.SCALES:
        x = _Buf(d["x"])
        sd = None if s_dev is None else _Buf(torch.tensor([s_dev]))
        T.scale_(x.v, s_host, None if sd is None else sd.v)
        torch.cuda.synchronize()
        _equal(x.v, P.scale_ref(d["x"], s_host, s_dev), f"scale n={n} s_host={s_host} s_dev={s_dev}")
        assert x.intact() and (sd is None or (sd.intact() and float(sd.v) == s_dev))


@pytest.mark.parametrize("n", P.EW_N)
def test_tanh_bwd(n):
    _lib, ops, T = _mods()
    d = P.ew_operands(n)
    dy, y, out = _Buf(d["dy"]), _Buf(d["y_tanh"]), _Buf(n=n)
    assert torch.equal(torch.signbit(y.v.cpu()), torch.signbit(d["y_tanh"]))                 # -0.0 arrives as -0.0
    _lib.check(_lib.load().hrv_tanh_bwd_f32(dy.ptr(), y.ptr(), n, out.ptr(), None), "hrv_tanh_bwd_f32")
    torch.cuda.synchronize()
    _equal(out.v, P.tanh_bwd_ref(d["dy"], d["y_tanh"]), f"tanh_bwd n={n}")
    assert dy.intact() and y.intact() and out.intact()
    assert torch.equal(T.tanh_bwd(dy.v, y.v), out.v), f"tanh_bwd n={n}: the wrapper"


class _Slice:
    """channels [coff, coff + Cn) of a [1, npix, 1, cs] device tensor; everything around the slice is poison"""

    def __init__(self, npix, Cn, coff, cs, fill):
        self.Cn, self.coff = Cn, coff
        self.t = torch.full((1, npix, 1, cs), P.POISON, device="cuda")
        self.set(fill)

    def view(self):
        return self.t[..., self.coff:self.coff + self.Cn]

    def set(self, fill):
        self.view().copy_(fill.view(1, -1, 1, self.Cn))

    def intact(self):
        m = torch.ones(self.t.shape[3], dtype=torch.bool, device="cuda")
        m[self.coff:self.coff + self.Cn] = False
        return bool((self.t[..., m] == P.POISON).all())


@pytest.mark.parametrize("n", P.EW_N)
def test_act_bwd(n):
    """n channel groups (the grid's unit) as npix x C4; d and y are channel slices of poisoned tensors with different strides and
    offsets; the rule is dact's y > 0: +0 and -0.0 take the slope (0 for ReLU)"""
    _lib, ops, T = _mods()
    npix, c4 = P.act_split(n)
    Cn = 4 * c4
    d = P.ew_operands(4 * n)
    dsl = _Slice(npix, Cn, 4, Cn + 8, d["dy"])
    ysl = _Slice(npix, Cn, 8, Cn + 12, d["y_act"])
    assert torch.equal(torch.signbit(ysl.view().cpu().reshape(-1)), torch.signbit(d["y_act"]))
    for act, slope in P.ACT_VARIANTS:
        dsl.set(d["dy"])
        T.act_bwd_(ops.Act(dsl.t, Cn, 4), ops.Act(ysl.t, Cn, 8), act, slope)
        torch.cuda.synchronize()
        _equal(dsl.view().reshape(-1), P.act_bwd_ref(d["dy"], d["y_act"], act, slope), f"act_bwd n={n} act={act} slope={slope}")
        assert dsl.intact() and ysl.intact() and torch.equal(ysl.view().reshape(-1).cpu(), d["y_act"])
