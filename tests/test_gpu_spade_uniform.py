"""The fused SPADE forward with a tile plan (csrc/spade_tiles.hip, spade_uniform_kernel of csrc/spade_fused.hip): the classifier's
lists against the pure-Python reference, the forward with the plan against the forward without it bit for bit (out, 1 + gamma,
actv), and two cases in exact-integer form against float64 (tests/spade_uniform_cases.py).  Every forward case also asserts the
light count the reference gives: a run that sent every tile down the matrix path would pass the comparison alone."""
import pytest
import torch

import exact_cases as E
import spade_uniform_cases as U

pytestmark = pytest.mark.gpu

N = 2


def _mods():
    import hr_viton_amd  # noqa: F401
    from hr_viton_amd import ops, train_ops as T
    return ops, T


def _seg(name, H, W, shift):
    ops, _ = _mods()
    return ops.Act(U.label_map(name, H, W, shift).cuda(), 7)


@pytest.mark.parametrize("shape", U.SHAPES, ids=U.case_id)
@pytest.mark.parametrize("name", U.MAPS)
def test_classifier_lists(shape, name):
    _, T = _mods()
    H, W, shift = shape
    want = U.classify(U.label_map(name, H, W, shift), shift, N, H, W)
    plan = T.spade_tile_plan(_seg(name, H, W, shift), shift, N, H, W)
    heavy, light, rep = plan.lists()
    assert plan.counts() == (len(want["heavy"]), len(want["light"]))
    assert heavy == want["heavy"] and light == want["light"] and rep == want["rep"]


def _bits(t):
    return t.contiguous().view(torch.int16)


def _forward(T, ops, seg, shift, x, d, w, pk, C_, H, W, noise, save, tiles):
    """one forward into sentinel-filled buffers: (out slice tensor, 1 + gamma, actv tensor)"""
    oall = torch.full((N, H, W, 8 + C_ + 8), 7.0, device="cuda", dtype=torch.bfloat16)
    g1p = torch.full((N, H, W, C_), 5.0, device="cuda", dtype=torch.bfloat16)
    aall = torch.full((N, H, W, 384), 7.0, device="cuda", dtype=torch.bfloat16)
    z, ns = (d["z"].cuda(), w["ns"].cuda()) if noise else (None, None)
    T.spade_fused_forward(seg, shift, x, d["mean"].cuda(), d["rstd"].cuda(), z, ns, pk, w["bg"].cuda(), w["bb"].cuda(), ops.ACT_LRELU, 0.2,
                          ops.Act(oall, C_, 8), g1p if save else None, ops.Act(aall, 128, 128) if save else None, "t", tiles=tiles)
    torch.cuda.synchronize()
    return oall, g1p, aall


@pytest.mark.parametrize("case", U.FORWARD + U.WRAP, ids=U.case_id)
def test_plan_on_equals_plan_off(case):
    ops, T = _mods()
    H, W, shift, name, C_ = case
    if case in U.WRAP:
        from hr_viton_amd import _lib
        assert N * ((H + 15) // 16) * ((W + 15) // 16) > 2 * int(_lib.load().hrv_persistent_cus())
    w, d = U.weights(C_), U.inputs(H, W, C_)
    seg = _seg(name, H, W, shift)
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
            off = _forward(T, ops, seg, shift, x, d, w, pk, C_, H, W, noise, save, None)
            on = _forward(T, ops, seg, shift, x, d, w, pk, C_, H, W, noise, save, plan)
            for what, a, b in zip(("out", "1 + gamma", "actv"), off, on):
                assert torch.equal(_bits(a), _bits(b)), (what, noise, save, int((_bits(a) != _bits(b)).sum()))
            # (and the forward without a plan wrote something: the sentinel is gone from the slice, the neighbours keep it)
            assert not bool((off[0][..., 8:8 + C_] == 7.0).all()) and bool((on[0][..., :8] == 7.0).all()) and bool((on[0][..., 8 + C_:] == 7.0).all())
            if save:
                assert bool((on[2][..., :128] == 7.0).all()) and bool((on[2][..., 256:] == 7.0).all())
            else:
                assert bool((on[1] == 5.0).all()) and bool((on[2] == 7.0).all())


def _assert_exact(what, got, ref64):
    want = E.to_bf16_rne(ref64)
    got = got.detach().cpu()
    assert got.dtype == torch.bfloat16 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    bad = int((got.float() != want.float()).sum())
    assert bad == 0, f"{what}: {bad} of {got.numel()} differ from the float64 reference"


@pytest.mark.parametrize("case", U.EXACT, ids=U.case_id)
def test_exact_integer_with_plan(case):
    ops, T = _mods()
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
        _assert_exact("actv", aall[..., 128:256], d["want"]["actv"])
        _assert_exact("1 + gamma", g1p, d["want"]["g1p"])
    _assert_exact("out", oall[..., 8:8 + C_], d["want"]["out"])
    assert bool((oall[..., :8] == 7.0).all()) and bool((oall[..., 8 + C_:] == 7.0).all())


def test_plan_is_cached_on_the_label_map(monkeypatch):
    ops, T = _mods()
    H, W, shift = U.SHAPES[0]
    seg = _seg("one_class", H, W, shift)
    monkeypatch.setenv("HRV_SPADE_UNIFORM_MIN_TILES", "1")
    monkeypatch.delenv("HRV_SPADE_UNIFORM", raising=False)
    p1 = T.spade_tile_plan_for(seg, shift, N, H, W)
    assert p1 is not None and T.spade_tile_plan_for(seg, shift, N, H, W) is p1
    assert T.spade_tile_plan_for(_seg("one_class", H, W, shift), shift, N, H, W) is not p1        # a new label map: a new plan
    monkeypatch.setenv("HRV_SPADE_UNIFORM_MIN_TILES", "100000")
    assert T.spade_tile_plan_for(seg, shift, N, H, W) is None
    monkeypatch.setenv("HRV_SPADE_UNIFORM_MIN_TILES", "1")
    monkeypatch.setenv("HRV_SPADE_UNIFORM", "0")
    assert T.spade_tile_plan_for(seg, shift, N, H, W) is None
