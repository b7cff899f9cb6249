"""The convolution dispatchers on both sides of every kernel gate: every case of tests/conv_dispatch_cases.py through its public
entry point (train_ops.conv_forward_dev / conv_dgrad / conv_wgrad), checked for the kernel family that served it, a per-element error
against the float64 reference within the reference-derived limit, the family conv_dispatch planned before the call, untouched poison
around output slices, zero pad channels and accumulation exactly once.  One table of all cases goes to test_diagnostics/conv_dispatch.txt in any event."""
import os

import pytest
import torch

import conv_dispatch_cases as T
from conftest import diag_path

pytestmark = pytest.mark.gpu

_ROWS, _SERVED = {}, set()


@pytest.fixture(scope="module", autouse=True)
def _table():
    yield
    with open(diag_path("conv_dispatch.txt"), "w") as f:
        f.write("%-28s %-5s %-4s %-36s %-36s %9s %9s  %s\n" % ("case", "entry", "mode", "expected family", "served by", "E/2^-24", "err/limit",
                                                                 "worst element (coordinates mod 32) / failure"))
        for cid in [c.id for c in T.CASES]:
            if cid in _ROWS:
                f.write(_ROWS[cid] + "\n")
        served = sorted(_SERVED)
        f.write("\nfamilies served: " + ", ".join(served) + "\n")
        f.write("families expected and never served: " + (", ".join(sorted(set(T.FAMILIES) - set(served))) or "none") + "\n")


def _nchw(a):
    return a.t[..., a.coff:a.coff + a.C].float().cpu().permute(0, 3, 1, 2).contiguous()


def _check_surroundings(a, what, pad_zero=True):
    """poison outside the slice's 16-byte-padded channel range untouched; pad channels of the slice zero"""
    from hr_viton_amd import ops
    t = a.t.float().cpu()
    cp = ops._cpad(a.C, a.bf16)
    outside = torch.cat([t[..., :a.coff], t[..., a.coff + cp:]], -1)
    assert outside.numel() == 0 or bool((outside == T.POISON).all()), f"{what}: the tensor around the output slice was written"
    if pad_zero and cp > a.C:
        assert bool((t[..., a.coff + a.C:a.coff + cp] == 0).all()), f"{what}: pad channels are not zero"


def _coords(shape, i):
    return tuple(int(v) % 32 for v in torch.unravel_index(torch.tensor(i), shape))


@pytest.mark.parametrize("cid", [c.id for c in T.CASES])
def test_conv_dispatch(cid, monkeypatch):
    from hr_viton_amd import _lib, ops, train_ops as tops
    assert (T.ACT_NONE, T.ACT_RELU, T.ACT_LRELU, T.ACT_TANH) == (_lib.ACT_NONE, _lib.ACT_RELU, _lib.ACT_LRELU, _lib.ACT_TANH)
    c = T.BY_ID[cid]
    torch.set_num_threads(min(16, torch.get_num_threads()))
    for k, v in c.env.items():
        monkeypatch.setenv(k, v)
    _lib.load()
    _lib.reload_env()
    d = T.make_inputs(c)
    ref = T.reference(c, d)
    d["ref"] = ref[0]
    K = T.k_terms(c)
    head = "%-28s %-5s %-4s %-36s" % (c.id, c.entry, c.mode, c.family)
    _ROWS[cid] = head + " | (did not return)"
    prev = tops.MMA_BF16[0]
    tops.MMA_BF16[0] = c.mode != "f32"
    ops.profile_begin()
    try:
        try:
            kw = T.entry_kwargs(c, d)
            plan = T.plan(c, kw)                # (before the call: plan and launch cannot drift apart)
            got = {"fwd": tops.conv_forward_dev, "dgrad": tops.conv_dgrad, "wgrad": tops.conv_wgrad}[c.entry](**kw)
            res = (kw["dw"], kw["dbias"]) if c.entry == "wgrad" else (got, kw["out"] is not None)
        finally:
            recs = ops.profile_end(kernels=True, variants=True)
            tops.MMA_BF16[0] = prev
    except Exception as e:          # 1. the call returns: an error of the library is a failure of the case
        _ROWS[cid] = head + " | %-36s %9s %9s  %s: %s" % ("-", "-", "-", type(e).__name__, str(e)[:160])
        raise
    fams = []
    for r in recs:
        if r[0] in ("conv", "wgrad") and r[5] not in fams:
            fams.append(r[5])
    served = "+".join(fams)
    _SERVED.update(fams)
    checks = []
    if c.entry == "wgrad":
        dw, db = res
        p = c.p
        ct = p["cin_tot"] or p["C"]
        sl = slice(p["ci_base"], p["ci_base"] + p["C"])
        want, A = ref[0], ref[1]
        if p["accumulate"]:         # 5. the prior contents were added exactly once
            want, A = want + d["dw0"][:, sl].double(), A + d["dw0"][:, sl].double().abs()
        got = dw.cpu()
        checks.append(("dw", got[:, sl], want, A, K, False))
        rest = torch.ones(ct, dtype=torch.bool)
        rest[sl] = False            # 4. the other slices of a wider dW keep their contents
        assert torch.equal(got[:, rest], d["dw0"][:, rest]), f"{cid}: dW outside [ci_base, ci_base + C) was written"
        if db is not None:
            wb, Ab = ref[2], ref[3]
            if p["dbias_accumulate"]:
                wb, Ab = wb + d["db0"].double(), Ab + d["db0"].double().abs()
            checks.append(("dbias", db.cpu(), wb, Ab, K, False))
    else:
        out, sliced = res
        if sliced:
            _check_surroundings(out, cid)
        else:                       # (an output the entry point allocated: its pad channels read as zero)
            t = out.t.float().cpu()
            assert bool((t[..., out.C:] == 0).all()), f"{cid}: pad channels of the allocated output are not zero"
        assert out.bf16 == T.output_is_bf16(c), (cid, out.bf16)
        checks.append(("out", _nchw(out), ref[0], ref[1], K, out.bf16))
    worst = (0.0, 0.0, "")
    for what, got, want, A, k, obf in checks:
        assert got.shape == want.shape, (cid, what, got.shape, want.shape)
        assert bool(torch.isfinite(got).all()), f"{cid}: {what} holds NaN / Inf"
        x, i = T.excess(got, want, A, k, obf)
        e, _ = T.e_units(got, want, A)
        if x >= worst[1]:
            worst = (e, x, f"{what}{_coords(want.shape, i)}")
    _ROWS[cid] = head + " | %-36s %9.2f %9.3f  %s" % (served, worst[0], worst[1], worst[2])
    print("\n" + _ROWS[cid])
    assert served == c.family, f"{cid}: served by {served}, the table expects {c.family}"           # 2.
    assert plan.family == served, f"{cid}: conv_dispatch planned {plan.family}, the profile record reports {served}"
    for kind, name, count in T.LAUNCHES.get(cid, ()):       # (the side of a gate whose two sides share a family)
        n = sum(1 for r in recs if r[0] == kind and name in r[1])
        assert n == count, f"{cid}: {n} launches of kind {kind!r} {name!r}, the table expects {count}: {[(r[0], r[1]) for r in recs]}"
    assert worst[1] <= 1.0, f"{cid}: error / limit = {worst[1]:.3f} at {worst[2]} (E = {worst[0]:.2f} * 2^-24, family {served})"     # 3.
