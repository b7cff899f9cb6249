"""tests/norm_exact_cases.py on the CPU alone: the geometry mirror is the library's slab rule and reaches every edge the GPU test
(tests/test_gpu_norm_exact.py) is there for, the operands meet the conditions its exact comparisons rest on, the float64 reference
is the formula torch autograd differentiates, every compile-time instance is run by some case -- and the assertions themselves
fail on a reference with one pixel dropped from a slab or two finalize rows swapped."""
import math
import os
import re

import pytest
import torch
import torch.nn.functional as F

import norm_bwd_instance_cases as K
import norm_exact_cases as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _geo(e):
    return E.geometry(e.H, e.W, e.C, e.cap)


# ---------------------------------------------------------------------------------------------------------------
# geometry
# ---------------------------------------------------------------------------------------------------------------
def test_the_mirror_is_the_slab_rule_of_the_library(monkeypatch):
    """NORM_GCAP from the header; the slab count from the library itself (through the workspace size), with and without the switch"""
    import hr_viton_amd  # noqa: F401
    from hr_viton_amd import _lib
    lib = _lib.load()
    with open(os.path.join(ROOT, "hr-viton_amd", "csrc", "hrv_common.h"), encoding="utf-8") as f:
        src = f.read()
    assert int(re.search(r"constexpr int NORM_GCAP = (\d+);", src).group(1)) == E.NORM_GCAP
    assert re.search(r"nb = \(HW \+ 127\) / 128, cap = norm_slab_cap\(\)", src) and re.search(r"e \? atoi\(e\) : 256;", src)
    for e in E.STATS_EXTENTS + [E.Extent(1, 1024, 768, None, 80), E.Extent(1, 3, 1, None, 4), E.Extent(1, 300, 300, 1000, 4)]:
        if e.cap:
            monkeypatch.setenv("HRV_NORM_SLABS_MAX", str(e.cap))
        else:
            monkeypatch.delenv("HRV_NORM_SLABS_MAX", raising=False)
        _lib.reload_env()
        nb = _geo(e).NB
        assert lib.hrv_instnorm_workspace_elems(e.N, e.H, e.W, e.C) == e.N * nb * e.C * 2, e
        assert lib.hrv_norm_bwd_workspace_elems(e.N, e.H, e.W, e.C) == e.N * nb * e.C * 2 + e.N * e.C * 2, e


def test_the_extents_reach_the_edges_they_are_there_for():
    by = {(e.H, e.W, e.cap): _geo(e) for e in E.LARGE}
    by.update({(H, W, cap): E.geometry(H, W, 4, cap) for _, H, W, cap in E.SMALL})
    g = by[(4, 4, None)]
    assert (g.NB, g.slabs, g.GB, g.R) == (1, [16], 1, 256) and g.R > g.PB            # more rows in flight than pixels in the slab
    assert by[(12, 11, None)].slabs == [66, 66]
    g = by[(48, 43, None)]                                                            # first stride of the backward finalize
    assert g.NB == 17 == E.FIN_LANES_BWD + 1 and g.last == 112 and g.empty == 0
    g = by[(96, 86, None)]                                                            # first stride of the statistics finalize
    assert g.NB == 65 == E.FIN_LANES_STATS + 1 and g.last == 64 and g.empty == 0
    g = by[(136, 242, None)]                                                          # the natural cap, no empty slab
    assert 136 * 242 == 32912 and (g.NB, g.PB, g.last, g.empty) == (E.SLAB_CAP, 129, 17, 0) and g.PB > E.SLAB_PIXELS
    g = by[(164, 200, None)]                                                          # the natural cap with an empty slab
    assert 164 * 200 == 32800 and (g.NB, g.PB, g.empty) == (E.SLAB_CAP, 129, 1) and g.slabs[254:] == [34, 0]
    assert by[(22, 20, 3)].slabs == [147, 147, 146]                                   # the switch-made cap
    g = by[(48, 44, 2)]                                                               # two long chains
    assert g.slabs == [1056, 1056] and g.walk >= 8
    for e in E.LARGE:
        assert sum(_geo(e).slabs) == e.H * e.W and e.C in (8, 12) and e.N * e.H * e.W * e.C * 4 <= 1.6 * 2 ** 20
    assert any(e.N == 2 for e in E.STATS_EXTENTS) and sum(E.can_up(e) for e in E.LARGE) >= 4


def test_the_channel_counts_reach_idle_threads_and_a_partly_live_last_chunk():
    want = {4: (1, 256, 0, 1, 1), 12: (3, 85, 1, 1, 3), 80: (20, 12, 16, 1, 20), 256: (64, 4, 0, 1, 64), 260: (64, 4, 0, 2, 1),
            1040: (64, 4, 0, 5, 4)}
    for c, (gb, r, idle, chunks, live_last) in want.items():
        g = E.geometry(12, 11, c)
        assert (g.GB, g.R, g.idle, g.chunks, g.live_last) == (gb, r, idle, chunks, live_last), c
    assert sorted(want) == E.ALL_C
    assert {e.C for e in E.STATS_EXTENTS if (e.H, e.W) in ((4, 4), (12, 11))} == set(E.ALL_C)
    ups = {u for e in E.STATS_EXTENTS for u in E.stats_up_splits(e)}
    assert any(u < 256 for u in ups) and any(u > 256 for u in ups) and 256 in ups       # both sides of a chunk, and its edge


# ---------------------------------------------------------------------------------------------------------------
# which form runs where
# ---------------------------------------------------------------------------------------------------------------
RUNS = E.backward_runs()


def test_every_instance_of_the_library_is_run_by_some_case():
    import hr_viton_amd  # noqa: F401
    from hr_viton_amd import train_ops as T
    assert sorted({h for form, _, generic in RUNS if not generic for h in form.hits}) == sorted(T.norm_bwd_instances())


def test_every_form_runs_at_every_extent_it_can_and_every_channel_count_under_singles_and_pairs():
    ids = [E.run_id(r) for r in RUNS]
    assert len(ids) == len(set(ids))
    for form in K.CASES:
        mine = [(e, g) for f, e, g in RUNS if f.id == form.id]
        for e in E.LARGE:
            assert ((e, False) in mine) == (not form.up or E.can_up(e)), (form.id, e)
        for e in E.GENERIC_AGAIN:
            assert ((e, True) in mine) == (not form.up or E.can_up(e)), (form.id, e)
        assert any((e.H, e.W) == (4, 4) for e, _ in mine) and (form.up or any(e.N == 2 for e, _ in mine)), form.id
    for pair in (False, True):
        for up in (False, True):
            cs = {e.C for f, e, _ in RUNS if f.pair == pair and f.up == up and e.H * e.W <= 256}
            assert cs >= set(E.ALL_C[1:]) and (up or cs == set(E.ALL_C)), (pair, up, cs)
    # both generic extents are the ones the issue of these tests names, and every up-sampled form reaches the cap and the empty slab
    assert [(e.H, e.W, e.cap) for e in E.GENERIC_AGAIN] == [(48, 43, None), (22, 20, 3)]
    assert all(E.can_up(e) for e in E.LARGE if (e.H, e.W) in ((136, 242), (164, 200), (22, 20), (48, 44)))


# ---------------------------------------------------------------------------------------------------------------
# the conditions of the exact comparisons
# ---------------------------------------------------------------------------------------------------------------
def _stats_terms(v):
    d = v - v[:, :1, :1, :]
    return d, d * d, v, v * v


@pytest.mark.parametrize("e", E.STATS_EXTENTS, ids=E.ext_id)
def test_statistics_case_meets_the_conditions(e):
    c = E.stats_case(e)
    assert torch.equal(c["x"].to(torch.bfloat16).float(), c["x"])                     # the bf16 entry point reads the same values
    k = c["const"]
    for name, v in c["v"].items():
        for t in _stats_terms(v):
            assert E.headroom(t) <= E.LIMIT, (name, E.headroom(t))
        mean, rstd = c["ref"][name]
        assert torch.equal(v[..., k], torch.full_like(v[..., k], 1.0)) and bool((rstd[:, k] == 1.0 / math.sqrt(E.EPS)).all())
        # the finalize forms E[d^2] - E[d]^2 in double: far from cancelling all 53 bits (constant channels are exactly 0)
        d = _stats_terms(v)[0].reshape(e.N, -1, e.C)
        var = ((d - d.mean(1, keepdim=True)) ** 2).mean(1)
        live = var > 0
        assert int((~live).sum()) == e.N and float(((d * d).mean(1)[live] / var[live]).max()) <= 2.0 ** 20
    for up_c in E.stats_up_splits(e):
        lo, hi, v, ref = E.stats_up_parts(c, up_c)
        assert lo.shape[-1] == up_c and lo.shape[-1] + hi.shape[-1] == e.C and up_c % 16 in (0, 4, 8)
        for t in (t for vv in v.values() for t in _stats_terms(vv)):
            assert E.headroom(t) <= E.LIMIT


def test_the_shifted_case_is_exact_only_with_the_shift():
    """x = 2048 + {-2..2}: d and d^2 keep their headroom, the unshifted sum of x^2 does not even fit fp32's 24 bits"""
    e = E.SHIFT_CASE
    c = E.stats_case(e, True)
    assert torch.equal(c["x"].double().float(), c["x"]) and float(c["x"].min()) == 2046.0 and float(c["x"].max()) == 2050.0
    for name, v in c["v"].items():
        d, d2, u, u2 = _stats_terms(v)
        assert E.headroom(d) <= E.LIMIT and E.headroom(d2) <= E.LIMIT
        assert E.headroom(u2) > 2 ** 24, name
    # a kernel that loses the shift sums x^2 in fp32: its variance misses the one-ulp assertion
    x = c["x"].reshape(e.N, -1, e.C)
    s1, s2 = torch.zeros(e.N, e.C), torch.zeros(e.N, e.C)
    for p in range(x.shape[1]):
        s1, s2 = s1 + x[:, p], s2 + x[:, p] * x[:, p]
    m = s1.double() / x.shape[1]
    lost = (1.0 / torch.sqrt((s2.double() / x.shape[1] - m * m).clamp_min(0) + E.EPS)).float()
    with pytest.raises(AssertionError):
        E.stats_check(c["ref"]["plain"][0].float(), lost, c["ref"]["plain"])


@pytest.mark.parametrize("run", [r for r in RUNS if not r[2]], ids=E.run_id)
def test_backward_case_meets_the_conditions(run):
    form, e, _ = run
    d = E.bwd_case(form.id, e)
    for o, r in zip(d["norms"], d["refs"]):
        assert E.headroom(r["dnh"]) <= E.LIMIT and E.headroom(r["dnh"] * r["nh"]) <= E.LIMIT, \
            (E.headroom(r["dnh"]), E.headroom(r["dnh"] * r["nh"]))
        assert E.bf16_exact(r["dnh"])                                # a sum may take dnh before or after its bf16 store
        assert set(o["rstd"].unique().tolist()) <= {0.25, 0.5, 1.0, 2.0}
        for k in ("dout", "g1p", "out"):                             # every bf16-stored operand is held exactly
            assert k not in o or E.bf16_exact(o[k].double()), k
        for k in ("dgamma", "dbeta", "dnh", "nh"):                   # ... and fp32 holds every element-wise result
            assert torch.equal(r[k].float().double(), r[k]), k
        if not E.wide(e):
            assert float(d["x64"].abs().max()) <= 2 and float(r["dnh"].abs().max()) <= 4 and float(r["nh"].abs().max()) <= 4
        elif form.kind == "spade":                                   # dgamma is stored as bf16: the store's rounding is exercised
            assert E.tie_share(r["dgamma"]) >= 0.01, E.tie_share(r["dgamma"])
            assert E.needs_rounding_share(r["dgamma"]) >= 0.10, E.needs_rounding_share(r["dgamma"])
    if e.N == 2:                                                     # statistics planted per sample: a swapped n / c index shows
        o = d["norms"][0]
        assert not torch.equal(o["mean"][0], o["mean"][1]) and not torch.equal(o["rstd"][0], o["rstd"][1])


def test_f64_to_bf16_rne_is_one_rounding_to_nearest_even():
    t = torch.cat([torch.arange(-2100, 2101, dtype=torch.float64) / 16, torch.tensor([0.0, 257.0, 259.0, -257.0, -259.0, 1e-9, -3e-7])])
    assert torch.equal(E.f64_to_bf16_rne(t), t.float().to(torch.bfloat16))                    # fp32-exact values: torch's own rounding
    up = torch.tensor([256.0 + 1.0 + 2.0 ** -30, -(256.0 + 1.0 + 2.0 ** -30), 256.0 + 1.0 - 2.0 ** -30], dtype=torch.float64)
    assert E.f64_to_bf16_rne(up).tolist() == [258.0, -258.0, 256.0]      # just past a tie: through fp32 first it would fall to even


# ---------------------------------------------------------------------------------------------------------------
# the reference itself
# ---------------------------------------------------------------------------------------------------------------
def test_the_float64_reference_is_what_autograd_differentiates():
    """fp32 torch autograd of out = lrelu(nh * (1 + gamma) + beta) with the statistics taken from v itself, against norm_ref /
    dx_term fed those statistics (in float64, m1 / m2 unrounded)"""
    g = torch.Generator().manual_seed(5)
    N, H, W, C = 2, 12, 11, 12
    x = torch.randn(N, H, W, C, generator=g).requires_grad_()
    ns = (torch.randn(C, generator=g) * 0.5).requires_grad_()
    z = torch.randn(N, W, H, generator=g)
    g1p = (1 + torch.randn(N, H, W, C, generator=g) * 0.3).requires_grad_()
    beta = torch.randn(N, H, W, C, generator=g).requires_grad_()
    v = x + z.permute(0, 2, 1).unsqueeze(-1) * ns
    mean, var = v.mean((1, 2), keepdim=True), v.var((1, 2), unbiased=False, keepdim=True)
    out = F.leaky_relu((v - mean) / torch.sqrt(var + E.EPS) * g1p + beta, 0.25)
    dout = torch.randn(out.shape, generator=g)
    out.backward(dout)
    m64, r64 = E.stats_ref(v.detach().double())
    o = dict(mean=m64, rstd=r64, z=z, ns=ns.detach(), g1p=g1p.detach(), dout=dout, out=out.detach(), slope=0.25)
    r = E.norm_ref(x.detach().double(), o)
    dx, _ = E.dx_term(r, r["S1"] / r["hw"], r["S2"] / r["hw"])
    dns = (dx * z.double().permute(0, 2, 1).unsqueeze(-1)).sum((0, 1, 2))
    for name, got, want in (("dx", dx, x.grad), ("dgamma", r["dgamma"], g1p.grad), ("dbeta", r["dbeta"], beta.grad), ("dns", dns, ns.grad)):
        err = float((got - want.double()).abs().max() / want.double().abs().max())
        assert err < 1e-5, (name, err)


# ---------------------------------------------------------------------------------------------------------------
# sensitivity: the assertions of the GPU test fail on a subtly wrong result
# ---------------------------------------------------------------------------------------------------------------
def _slab_sums(t, geo):
    """[N, NB, C] float64: a term summed per slab"""
    N, C = t.shape[0], t.shape[-1]
    f = t.reshape(N, -1, C)
    return torch.stack([f[:, b * geo.PB:b * geo.PB + n].sum(1) for b, n in enumerate(geo.slabs)], 1)


@pytest.mark.parametrize("e,slab", [(E.LARGE[3], 254), (E.LARGE[3], 0), (E.LARGE[5], 1)], ids=["164x200-last", "164x200-first", "48x44-cap2"])
@pytest.mark.parametrize("how", ["dropped", "doubled"])
def test_one_pixel_dropped_or_doubled_at_a_slab_seam_fails_the_m1_m2_assertion(e, slab, how):
    geo = _geo(e)
    d = E.bwd_case("norm_0_coarse", e)
    r = d["refs"][0]
    part1, part2 = _slab_sums(r["dnh"], geo), _slab_sums(r["dnh"] * r["nh"], geo)
    assert torch.equal(part1.sum(1), r["S1"]) and torch.equal(part2.sum(1), r["S2"])
    E.m_check((part1.sum(1) / r["hw"]).float(), (part2.sum(1) / r["hw"]).float(), r)          # the slab sums as they are: passes
    px = slab * geo.PB + geo.slabs[slab] - 1                                                    # the last pixel of the slab
    t1 = r["dnh"].reshape(e.N, -1, e.C)[:, px]
    t2 = (r["dnh"] * r["nh"]).reshape(e.N, -1, e.C)[:, px]
    assert bool((t1 != 0).any()) and bool((t2 != 0).any())
    s = -1.0 if how == "dropped" else 1.0
    m1, m2 = ((r["S1"] + s * t1) / r["hw"]).float(), ((r["S2"] + s * t2) / r["hw"]).float()
    # every channel whose term is not zero moves, although one pixel of 32800 is 3e-5 of the sum
    assert bool(((m1 != r["m1"]) == (t1 != 0)).all()) and bool(((m2 != r["m2"]) == (t2 != 0)).all())
    with pytest.raises(AssertionError):
        E.m_check(m1, r["m2"], r)
    with pytest.raises(AssertionError):
        E.m_check(r["m1"], m2, r)


@pytest.mark.parametrize("e,slab", [(E.LARGE[3], 254), (E.LARGE[5], 1)], ids=["164x200", "48x44-cap2"])
def test_one_pixel_dropped_from_a_slab_fails_the_statistics_assertion(e, slab):
    geo = _geo(e)
    c = E.stats_case(e)
    v = c["v"]["a"]
    f = v.reshape(e.N, -1, e.C)
    E.stats_check(c["ref"]["a"][0].float(), c["ref"]["a"][1].float(), c["ref"]["a"])
    px = slab * geo.PB + geo.slabs[slab] - 1
    keep = torch.ones(f.shape[1], dtype=torch.bool)
    keep[px] = False
    hw = f.shape[1]
    mean = f[:, keep].sum(1) / hw                                                              # the pixel is missing from the sums only
    var = ((f[:, keep] ** 2).sum(1) / hw - mean ** 2).clamp_min(0)
    with pytest.raises(AssertionError):
        E.stats_check(mean.float(), (1.0 / torch.sqrt(var + E.EPS)).float(), c["ref"]["a"])


def test_two_finalize_rows_swapped_fail_both_assertions():
    e = E.LARGE[1]                      # 96 x 86: 65 slabs, the first stride of the statistics finalize
    c = E.stats_case(e)
    mean, rstd = (t.float() for t in c["ref"]["a"])
    i, j = 0, 1
    assert float(mean[0, i]) != float(mean[0, j])
    sw = torch.arange(e.C)
    sw[i], sw[j] = j, i
    with pytest.raises(AssertionError):
        E.stats_check(mean[:, sw], rstd[:, sw], c["ref"]["a"])
    r = E.bwd_case("norm_0_coarse", e)["refs"][0]
    assert float(r["m1"][0, i]) != float(r["m1"][0, j])
    with pytest.raises(AssertionError):
        E.m_check(r["m1"][:, sw], r["m2"][:, sw], r)
    # ... and a finalize that strides wrongly (the slabs past its lanes left out) fails as well
    geo = _geo(e)
    part = _slab_sums(c["v"]["a"] - c["v"]["a"][:, :1, :1], geo)
    short = part[:, :E.FIN_LANES_STATS].sum(1) / (e.H * e.W) + c["v"]["a"][:, 0, 0]
    with pytest.raises(AssertionError):
        E.stats_check(short.float(), rstd, c["ref"]["a"])


def test_the_dx_bound_is_far_below_the_effect_of_a_wrong_m1():
    """dx_check passes the float64 value rounded to fp32 and fails when m1 moves by one pixel's worth"""
    e = E.LARGE[5]
    d = E.bwd_case("norm_0_coarse", e)
    r = d["refs"][0]
    term, br = E.dx_term(r, r["m1"], r["m2"])
    assert E.dx_check(term.float(), [(term, br)]) <= 0.5
    assert E.dx_check(E.f64_to_bf16_rne(term), [(term, br)], bf16=True) <= 1.0
    wrong, _ = E.dx_term(r, r["m1"] + 0.25 / r["hw"], r["m2"])
    with pytest.raises(AssertionError):
        E.dx_check(wrong.float(), [(term, br)])
    z = d["norms"][0]["z"]
    dns = (term * z.double().permute(0, 2, 1).unsqueeze(-1)).sum((0, 1, 2))
    assert E.dns_check(dns.float(), term, br, z, _geo(e)) <= 1.0
