"""GPU: adaptive discriminator augmentation (the gated kernels and the controller of csrc/diffaug.hip, hr_viton_amd/diffaug.py
AdaptiveAugment) against the restatements of tests/ada_cases.py -- geometry under gates to the bit, color inside the bound of
tests/diffaug_cases.py under the effective flags, the end points p = 0 / p = 1 against the plain and the ungated launches, the strict
fp64 edge, the controller's whole state to the bit (eager and replayed), the pair form, train steps, a captured adaptive iteration,
checkpoints and the script."""
import copy
import functools
import re

import pytest
import torch

import ada_cases as A
import diffaug_cases as D

pytestmark = pytest.mark.gpu
IDS = lambda s: "x".join(map(str, s))  # noqa: E731
CA = 7
GEOMETRIES = (D.GEOMETRY, D.TRANSLATION, D.CUTOUT)


def _mods():
    import hr_viton_amd  # noqa: F401
    from hr_viton_amd import diffaug, ops
    from hr_viton_amd import train_ops as T
    return diffaug, ops, T


def _p(v):
    return torch.tensor([v], dtype=torch.float64).cuda()


@functools.lru_cache(maxsize=None)
def _gauss(shape):
    N, H, W = shape
    return D.gauss_inputs(N, H, W, 100 + H)


@functools.lru_cache(maxsize=None)
def _grad(shape, seed):
    N, H, W = shape
    return torch.randn(N, H, W, 12, generator=torch.Generator().manual_seed(seed))


def _forward(parse, img, u, flags, ug=None, p=None, mean=None):
    """the stand-alone op on the device, gated when ``ug`` is given -> (the NHWC activation, the leaf image on the device)"""
    diffaug, ops, _ = _mods()
    x = img.cuda().requires_grad_()
    gate = None if ug is None else (ug.cuda(), p if isinstance(p, torch.Tensor) else _p(p))
    out = diffaug.diffaug_concat(ops.Act(parse.cuda(), CA), x, u.cuda(), flags, mean=None if mean is None else mean.cuda(), gate=gate)
    assert out.C == CA + 3 and tuple(out.t.shape) == (*parse.shape[:3], 12)
    return out, x


# ---------------------------------------------------------------------------------------------------------------
# 1. geometry under gates
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", D.SHAPES, ids=IDS)
def test_geometry_under_every_forced_mask_equals_the_gated_restatement(shape):
    N, H, W = shape
    parse, fake, _ = _gauss(shape)
    g = _grad(shape, H)
    p, seen = _p(A.GATE_P), set()
    for names, u, masks, ug in A.paired_batches(H, W, N):
        seen.update(masks)
        for flags in GEOMETRIES:
            out, x = _forward(parse, fake, u, flags, ug, p)
            assert torch.equal(out.t.detach().cpu().double(), A.forward_ref(parse, CA, fake, u, ug, A.GATE_P, flags)), (names, masks, flags)
            out.t.backward(g.cuda())
            assert torch.equal(x.grad.cpu().double(), A.backward_ref(g, CA, u, ug, A.GATE_P, flags)), (names, masks, flags)
    assert seen == set(range(8))


# ---------------------------------------------------------------------------------------------------------------
# 2. color under gates
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", D.POW2_SHAPES, ids=IDS)
def test_color_under_every_mask_is_exact_on_integer_images(shape):
    """s = 1, k and beta powers of two, HW a power of two, a mean with two fractional bits: no rounding anywhere, gated or not"""
    N, H, W = shape
    parse, _, _ = D.gauss_inputs(N, H, W, 100 + H)
    img = D.int_image(N, H, W, 5 + H)
    g = D.int_values((N, H, W, 12), 6 + H)
    ub, p, seen = D.batches(D.forced_rows(H, W), N), _p(A.GATE_P), set()
    for u0, u2 in ((0.75, 0.0), (0.0, 0.5), (0.25, 0.0), (0.5, 0.5)):          # beta = 1/4, -1/2, -1/4, 0; k = 1/2, 1
        for i, (masks, ug) in enumerate(A.gate_batches(N)):
            names, u = ub[(3 * i) % len(ub)]
            seen.update(masks)
            u = u.clone()
            u[:, 0], u[:, 1], u[:, 2] = u0, 0.5, u2
            out, x = _forward(parse, img, u, D.ALL, ug, p)
            want = A.forward_ref(parse, CA, img, u, ug, A.GATE_P, D.ALL, mean=D.mean_ref(img))
            assert torch.equal(want.float().double(), want)
            assert torch.equal(out.t.detach().cpu().double(), want), (names, masks, u0, u2)
            out.t.backward(g.cuda())
            err = (x.grad.cpu().double() - A.backward_ref(g, CA, u, ug, A.GATE_P, D.ALL)).abs()
            assert bool((err <= A.backward_bound(g, CA, u, ug, A.GATE_P, D.ALL)).all()), (names, masks, u0, u2, float(err.max()))
            if u2 == 0.5:      # k = 1: no term carries the 1 / (3 HW), the backward is exact too
                assert float(err.max()) == 0.0, (names, masks, u0)
    assert seen == set(range(8))


@pytest.mark.parametrize("flags", [D.ALL, D.COLOR], ids=["all", "color"])
@pytest.mark.parametrize("shape", D.SHAPES, ids=IDS)
def test_color_on_gaussian_data_is_inside_the_bound_of_the_effective_flags(shape, flags, capsys):
    """the bound of tests/diffaug_cases.py, evaluated per sample with flags & mask: no new tolerance.  The forced gate table at
    GATE_P and a random one at p = 0.5; the measured maxima, as shares of the bound, are printed"""
    N, H, W = shape
    parse, fake, real = _gauss(shape)
    gen = torch.Generator().manual_seed(H + 2)
    g = _grad(shape, H + 2)
    worst_f = worst_b = 0.0
    for i, (names, u, masks, ug) in enumerate(A.paired_batches(H, W, N)):
        u = u.clone()
        u[:, :3] = torch.rand(N, 3, generator=gen)
        for img, gates, p in ((fake, ug, A.GATE_P), (real, A.random_gates(N, H + i), 0.5)):
            out, x = _forward(parse, img, u, flags, gates, p)
            M = D.mean_ref(img)
            want, bound = A.forward_ref(parse, CA, img, u, gates, p, flags, mean=M), A.forward_bound(CA, img, u, gates, p, flags, M)
            err = (out.t.detach().cpu().double() - want).abs()
            assert bool((err <= bound).all()), (names, masks, float((err - bound).max()))
            worst_f = max(worst_f, float((err / bound.clamp_min(1e-300)).max()))
            out.t.backward(g.cuda())
            want, bound = A.backward_ref(g, CA, u, gates, p, flags), A.backward_bound(g, CA, u, gates, p, flags)
            err = (x.grad.cpu().double() - want).abs()
            assert bool((err <= bound).all()), (names, masks, float((err - bound).max()))
            worst_b = max(worst_b, float((err / bound.clamp_min(1e-300)).max()))
    with capsys.disabled():
        print(f"\n[ada] {IDS(shape)} flags {flags}: worst error / bound  forward {worst_f:.3f}  backward {worst_b:.3f}")
    assert 0.0 < worst_f <= 1.0 and 0.0 < worst_b <= 1.0


# ---------------------------------------------------------------------------------------------------------------
# 3. the gradient sum under gates
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", D.SHAPES + D.POW2_SHAPES[1:], ids=IDS)
def test_gsum_under_gates_is_exact_on_integers_and_reproducible(shape):
    _, ops, T = _mods()
    N, H, W = shape
    g = D.int_values((N, H, W, 12), H + 2)
    gg = _grad(shape, H)
    p = _p(A.GATE_P)
    for names, u, masks, ug in A.paired_batches(H, W, N)[::2]:
        for flags in (D.ALL, D.COLOR):
            s1 = T.diffaug_gsum_gated(ops.Act(g.cuda(), CA + 3), CA, u.cuda(), flags, ug.cuda(), p)
            assert s1.dtype == torch.float64 and torch.equal(s1.cpu(), A.gsum_ref(g, CA, u, ug, A.GATE_P, flags)), (names, masks, flags)
            r1 = T.diffaug_gsum_gated(ops.Act(gg.cuda(), CA + 3), CA, u.cuda(), flags, ug.cuda(), p)
            r2 = T.diffaug_gsum_gated(ops.Act(gg.cuda(), CA + 3), CA, u.cuda(), flags, ug.cuda(), p)
            assert torch.equal(r1.view(torch.int64), r2.view(torch.int64))
            want = A.gsum_ref(gg, CA, u, ug, A.GATE_P, flags)
            assert float((r1.cpu() - want).abs().max()) <= 1e-12 * float(gg.abs().sum())


# ---------------------------------------------------------------------------------------------------------------
# 4. the end points, 5. the strict edge
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", D.SHAPES, ids=IDS)
def test_p_zero_is_the_plain_assembly_and_p_one_the_ungated_twin(shape):
    _, ops, T = _mods()
    N, H, W = shape
    parse, fake, _ = _gauss(shape)
    g = _grad(shape, H + 3)
    plain = torch.empty(N, H, W, 12).cuda()
    T.concat_nhwc_nchw(ops.Act(parse.cuda(), CA), fake.cuda(), ops.Act(plain, CA + 3))
    plain_d = ops.to_nchw(ops.Act(g.cuda(), CA + 3), CA, 3)
    for i, (names, u) in enumerate(D.batches(D.forced_rows(H, W), N)[::3]):
        u = u.clone()
        u[:, :3] = torch.rand(N, 3, generator=torch.Generator().manual_seed(i))
        ug = A.random_gates(N, H + i)
        ug[0, :3] = torch.tensor([0.0, D.TOP, 0.0])          # the smallest and the largest uniform
        for flags in (D.ALL, D.GEOMETRY, D.COLOR):
            out, x = _forward(parse, fake, u, flags, ug, 0.0)
            assert torch.equal(out.t.detach().view(torch.int32), plain.view(torch.int32)), (names, flags)
            out.t.backward(g.cuda())
            assert torch.equal(x.grad.view(torch.int32), plain_d.view(torch.int32)), (names, flags)
            twin, y = _forward(parse, fake, u, flags)
            out, x = _forward(parse, fake, u, flags, ug, 1.0)
            assert torch.equal(out.t.detach().view(torch.int32), twin.t.detach().view(torch.int32)), (names, flags)
            assert not torch.equal(out.t.detach(), plain)
            twin.t.backward(g.cuda())
            out.t.backward(g.cuda())
            assert torch.equal(x.grad.view(torch.int32), y.grad.view(torch.int32)), (names, flags)


@pytest.mark.parametrize("shape", D.SHAPES[1:3], ids=IDS)
def test_the_comparison_is_strict_and_made_in_fp64(shape):
    N, H, W = shape
    parse, fake, _ = _gauss(shape)
    g = _grad(shape, H + 4)
    u = torch.rand(N, 8, generator=torch.Generator().manual_seed(H))
    # ug bitwise (float)p: not below p, nothing applies -- the plain copy
    ug = torch.full((N, 4), 0.5)
    out, x = _forward(parse, fake, u, D.ALL, ug, 0.5)
    none, y = _forward(parse, fake, u, 0)
    assert torch.equal(out.t.detach().view(torch.int32), none.t.detach().view(torch.int32))
    out.t.backward(g.cuda())
    assert torch.equal(x.grad.cpu(), g[..., CA:CA + 3].permute(0, 3, 1, 2))
    # p = 0.25 + 2^-40 rounds to ug = 0.25 in fp32 but lies above it in fp64: everything applies
    ug = torch.full((N, 4), 0.25)
    assert float(torch.tensor(A.EDGE_P, dtype=torch.float64).float()) == 0.25
    out, x = _forward(parse, fake, u, D.ALL, ug, A.EDGE_P)
    twin, y = _forward(parse, fake, u, D.ALL)
    assert torch.equal(out.t.detach().view(torch.int32), twin.t.detach().view(torch.int32)) and not torch.equal(out.t.detach(), none.t.detach())
    assert torch.equal(out.t.detach().cpu().double()[..., :CA], A.forward_ref(parse, CA, fake, u, ug, A.EDGE_P, D.ALL)[..., :CA])
    out.t.backward(g.cuda())
    twin.t.backward(g.cuda())
    assert torch.equal(x.grad.view(torch.int32), y.grad.view(torch.int32))
    # and one sample on each side of the edge in the same launch
    if N > 1:
        ug = torch.full((N, 4), 0.25)
        ug[1] = 0.25 + 2.0 ** -24
        out, _ = _forward(parse, fake, u, D.GEOMETRY, ug, A.EDGE_P)
        assert torch.equal(out.t.detach().cpu().double(), A.forward_ref(parse, CA, fake, u, ug, A.EDGE_P, D.GEOMETRY))
        assert A.gate_mask(ug[0].numpy(), A.EDGE_P) == D.ALL and A.gate_mask(ug[1].numpy(), A.EDGE_P) == 0


def test_other_gates_are_rejected():
    diffaug, ops, T = _mods()
    N, H, W = 1, 8, 8
    parse, fake, _ = _gauss((N, H, W))
    u, ug = torch.full((N, 8), 0.5).cuda(), torch.full((N, 4), 0.5).cuda()
    act = ops.Act(parse.cuda(), CA)
    with pytest.raises(ops.HrvError):          # three gate columns
        diffaug.diffaug_concat(act, fake.cuda(), u, "cutout", gate=(ug[:, :3], _p(0.5)))
    with pytest.raises(ops.HrvError):          # p in fp32
        diffaug.diffaug_concat(act, fake.cuda(), u, "cutout", gate=(ug, torch.tensor([0.5]).cuda()))
    with pytest.raises(ops.HrvError):          # p on the host
        diffaug.diffaug_concat(act, fake.cuda(), u, "cutout", gate=(ug, torch.tensor([0.5], dtype=torch.float64)))
    with pytest.raises(ops.HrvError, match="pair"):          # an AdaptiveAugment takes (u, ug)
        diffaug.resolve_aug(diffaug.AdaptiveAugment("cutout", fixed_p=0.5), u, N, u.device, "t")
    with pytest.raises(ops.HrvError):          # a controller call on a record of the wrong size
        T.ada_update(torch.zeros(8, dtype=torch.float64).cuda(), 1, 0.5, 0.25, 2, 1.0, torch.zeros(8, dtype=torch.float64).cuda())
    with pytest.raises(ops.HrvError):          # five scales
        T.ada_update(torch.zeros(A.DHEAD_WORDS, dtype=torch.float64).cuda(), 5, 0.5, 0.25, 2, 1.0, torch.zeros(8, dtype=torch.float64).cuda())


# ---------------------------------------------------------------------------------------------------------------
# 6. the controller
# ---------------------------------------------------------------------------------------------------------------
def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int64)


@pytest.mark.parametrize("which", ["hand", "rounded"])
def test_chained_controller_launches_equal_the_restatement_to_the_bit_eager_and_replayed(which):
    _, _, T = _mods()
    cfg, seq = (A.HAND, A.HAND_SEQ) if which == "hand" else (A.ROUNDED, A.rounded_seq())
    want = A.run_sequence(cfg, seq)
    assert len(seq) >= 14
    args = (cfg["num_d"], cfg["target"], cfg["step"], cfg["interval"], cfg["p_max"])
    rec = torch.zeros(A.DHEAD_WORDS, dtype=torch.float64).cuda()
    state = torch.tensor(A.initial_state(cfg["p_init"]), dtype=torch.float64).cuda()
    eager = []
    for i, item in enumerate(seq):
        rec.copy_(A.make_record(item[0], item[1]))
        T.ada_update(rec, *args, state)
        eager.append(state.cpu().clone())
        assert torch.equal(_bits(eager[-1]), _bits(torch.tensor(want[i], dtype=torch.float64))), (i, eager[-1].tolist(), want[i])
    # one captured launch, replayed over the same records, follows the eager sequence
    state_g = torch.tensor(A.initial_state(cfg["p_init"]), dtype=torch.float64).cuda()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        T.ada_update(rec, *args, state_g)
    torch.cuda.synchronize()
    assert torch.equal(state_g.cpu(), torch.tensor(A.initial_state(cfg["p_init"]), dtype=torch.float64))      # (a capture launches nothing)
    for i, item in enumerate(seq):
        rec.copy_(A.make_record(item[0], item[1]))
        graph.replay()
        assert torch.equal(_bits(state_g), _bits(eager[i])), i


# ---------------------------------------------------------------------------------------------------------------
# 7. the discriminator's pair form
# ---------------------------------------------------------------------------------------------------------------
def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-12)).item()


@pytest.mark.parametrize("policy", ["translation,cutout", "color,translation,cutout"])
def test_pair_form_with_fixed_p_equals_the_plain_pair_form_on_restated_inputs(policy):
    """the pair-form test of tests/test_gpu_diffaug.py with AdaptiveAugment(fixed_p=0.5) and injected (u, ug): sample 0 keeps color and
    translation, sample 1 cutout.  Predictions, d(fake) and parameter gradients bit-identical under the geometry policy; with color
    inside that test's tolerances (1e-4 of the largest value; 2e-2 for gradients through sign() terms)."""
    from test_gpu_train_step import _setup
    diffaug, ops, _ = _mods()
    from hr_viton_amd.losses import GANLoss, L1Loss
    opt, gen, Dn, x, seg, real, noise = _setup(seed=21, H=128, W=96, wmul=6.0)
    N, H, W = 2, 128, 96
    Dn.cuda().train()
    D2 = copy.deepcopy(Dn)
    g = torch.Generator().manual_seed(5)
    fake = torch.rand(N, 3, H, W, generator=g) * 2 - 1
    u = torch.rand(N, 8, generator=g)
    ug = torch.tensor([[A.ON, A.ON, A.OFF, 0.0], [A.OFF, A.OFF, A.ON, 0.0]])
    aug = diffaug.AdaptiveAugment(policy, fixed_p=A.GATE_P)
    geometry = not aug.color
    parse = torch.cat((seg.permute(0, 2, 3, 1), torch.zeros(N, H, W, 1)), dim=3).contiguous()
    cg, cf = GANLoss("hinge"), L1Loss()
    pair = (u.cuda(), ug.cuda())

    def loss(pf, pr):
        tot = cg(pf, True, for_discriminator=False)
        for i in range(len(pf)):
            for j in range(len(pf[i]) - 1):
                tot = tot + cf(pf[i][j], pr[i][j].detach()) * 10.0 / len(pf)
        return tot

    fa = fake.cuda().requires_grad_()
    pf_a, pr_a = Dn.forward_pair(ops.Act(parse.cuda(), CA), fa, real.cuda(), aug=aug, aug_u=pair)
    loss(pf_a, pr_a).sum().backward()
    in_f = A.forward_ref(parse, CA, fake, u, ug, A.GATE_P, aug.flags, mean=D.mean_ref(fake)).float()
    in_r = A.forward_ref(parse, CA, real, u, ug, A.GATE_P, aug.flags, mean=D.mean_ref(real)).float()
    assert torch.equal(in_f[..., :CA], in_r[..., :CA]) and not torch.equal(in_f[0, ..., :CA], parse[0, ..., :CA])
    assert not torch.equal(in_f[1, ..., :CA], parse[1, ..., :CA])
    # (the gates did select: the ungated transform differs from the gated one on both samples)
    full = D.forward_ref(parse, CA, fake, u, aug.flags, mean=D.mean_ref(fake)).float()
    assert not torch.equal(full[0], in_f[0]) and not torch.equal(full[1], in_f[1])
    parse_aug = torch.cat((in_f[..., :CA], torch.zeros(N, H, W, 1)), dim=3).contiguous()
    fb = in_f[..., CA:CA + 3].permute(0, 3, 1, 2).contiguous().cuda().requires_grad_()
    rb = in_r[..., CA:CA + 3].permute(0, 3, 1, 2).contiguous().cuda()
    pf_b, pr_b = D2.forward_pair(ops.Act(parse_aug.cuda(), CA), fb, rb)
    loss(pf_b, pr_b).sum().backward()
    gin = torch.zeros(N, H, W, 12)
    gin[..., CA:CA + 3] = fb.grad.cpu().permute(0, 2, 3, 1)
    want = A.backward_ref(gin, CA, u, ug, A.GATE_P, aug.flags)
    flat = lambda p: [t for s_ in p for t in s_]  # noqa: E731
    assert float(fa.grad.abs().max()) > 0
    if geometry:
        for a, b in zip(flat(pf_a) + flat(pr_a), flat(pf_b) + flat(pr_b)):
            assert torch.equal(a, b)
        assert torch.equal(fa.grad.cpu().double(), want)
    else:
        for a, b in zip(flat(pf_a) + flat(pr_a), flat(pf_b) + flat(pr_b)):
            assert _rel(a, b) < 1e-4
        assert _rel(fa.grad, want) < 2e-2
    # the discriminator step's form: no gradient to the images, every parameter gradient as on the restated inputs
    for m in (Dn, D2):
        m.zero_grad()
    pf_a, pr_a = Dn.forward_pair(ops.Act(parse.cuda(), CA), fake.cuda(), real.cuda(), aug=aug, aug_u=pair)
    (cg(pf_a, False, for_discriminator=True) + cg(pr_a, True, for_discriminator=True)).sum().backward()
    pf_b, pr_b = D2.forward_pair(ops.Act(parse_aug.cuda(), CA), fb.detach(), rb)
    (cg(pf_b, False, for_discriminator=True) + cg(pr_b, True, for_discriminator=True)).sum().backward()
    some = 0
    for (n_, p), (_, q) in zip(Dn.named_parameters(), D2.named_parameters()):
        assert (p.grad is None) == (q.grad is None), n_
        if p.grad is not None:
            some += 1
            if geometry:
                assert torch.equal(p.grad, q.grad), n_
            else:
                assert _rel(p.grad, q.grad) < 2e-2, n_
    assert some > 0


# ---------------------------------------------------------------------------------------------------------------
# 8. train steps at the end points, 9. the adaptive run, eager and captured
# ---------------------------------------------------------------------------------------------------------------
def _uniforms(steps, N, seed=17):
    """per step ((u_G, ug_G), (u_D, ug_D)) on the device"""
    g = torch.Generator().manual_seed(seed)
    draw = lambda: (torch.rand(N, 8, generator=g).cuda(), torch.rand(N, 4, generator=g).cuda())  # noqa: E731
    return [(draw(), draw()) for _ in range(steps)]


def _train(steps, aug=None, aug_u=None, head=None, records=None):
    """``steps`` eager iterations of the small step of tests/test_gpu_lecam.py; ``aug_u``: per step what the step takes (None: drawn)"""
    from test_gpu_lecam import _build, _snapshot
    _, ops, _ = _mods()
    from hr_viton_amd import pipeline
    from hr_viton_amd.losses import GANLoss, L1Loss
    opt, gen, Dn, og, od, inputs, nz = _build()
    for i in range(steps):
        losses, _ = pipeline.generator_train_step(opt, gen, Dn, GANLoss("hinge"), L1Loss(), None, og, od, inputs["x"],
                                                  ops.Act(inputs["parse7"], 7), inputs["im"], noise=nz[0], noise_d=nz[1], aug=aug,
                                                  aug_u=None if aug_u is None else aug_u[i], lecam=head)
        if records is not None:
            records.append(head.stats().cpu().clone())
    return _snapshot(gen, Dn), {k: float(v.detach()) for k, v in losses.items()}


def _same(a, b):
    assert list(a) == list(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_three_train_steps_at_p_zero_and_p_one_end_where_the_plain_and_the_ungated_steps_end():
    diffaug, _, _ = _mods()
    from hr_viton_amd.lecam import LeCam
    us = _uniforms(3, 2)
    policy = "color,translation,cutout"
    plain, lp = _train(3, head=LeCam(0.0))
    zero, lz = _train(3, diffaug.AdaptiveAugment(policy, fixed_p=0.0), us, LeCam(0.0))
    _same(plain, zero)
    assert lp == lz
    twin, lt = _train(3, diffaug.DiffAugment(policy), [(g[0], d[0]) for g, d in us], LeCam(0.0))
    one, lo = _train(3, diffaug.AdaptiveAugment(policy, fixed_p=1.0), us, LeCam(0.0))
    _same(twin, one)
    assert lt == lo
    assert any(not torch.equal(plain[k], twin[k]) for k in plain if k.startswith("D."))       # the augmentation did act
    # a fixed p needs no head
    nohead, _ = _train(3, diffaug.AdaptiveAugment(policy, fixed_p=1.0), us)
    bare, _ = _train(3, diffaug.DiffAugment(policy), [(g[0], d[0]) for g, d in us])
    _same(nohead, bare)


def _adaptive(target, **kw):
    diffaug, _, _ = _mods()
    # batch 2, interval 2, kimg 0.032: step = 2 * 2 / 32 = 1/8
    return diffaug.AdaptiveAugment("color,translation,cutout", target=target, kimg=0.032, interval=2, p_init=0.25, **kw)


@functools.lru_cache(maxsize=None)
def _target():
    """a target one quarter below the mean r_t of the first window (above it when that leaves [-1, 1]), which a run at the constant
    p = p_init shows: until the first window closes the adaptive run is that run"""
    diffaug, _, _ = _mods()
    from hr_viton_amd import _lib
    from hr_viton_amd.lecam import LeCam
    recs = []
    _train(2, diffaug.AdaptiveAugment("color,translation,cutout", fixed_p=0.25), _uniforms(6, 2), LeCam(0.0), recs)
    rt = lambda r: (float(r[_lib.DHEAD_STATE + _lib.DHEAD_RT]) + float(r[_lib.DHEAD_STATE + _lib.DHEAD_SCALE_WORDS + _lib.DHEAD_RT])) / 2.0  # noqa: E731
    m = (rt(recs[0]) + rt(recs[1])) / 2.0
    return (m - 0.25, +1) if m - 0.25 >= -1.0 else (m + 0.25, -1)


def test_six_adaptive_steps_move_p_as_the_restatement_fed_with_the_recorded_r_t():
    from hr_viton_amd.lecam import LeCam
    target, sign = _target()
    aug, head, recs = _adaptive(target), LeCam(0.0), []
    assert aug.step_size(2) == 0.125
    _train(6, aug, _uniforms(6, 2), head, recs)
    st, states = A.initial_state(0.25), []
    for r in recs:
        st = A.controller_step(st, r.tolist(), 2, target, 0.125, 2, 1.0)
        states.append(st)
    assert torch.equal(_bits(aug.state()), _bits(torch.tensor(st, dtype=torch.float64))), (aug.scalars(), st)
    s = aug.scalars()
    assert s["updates"] == 3.0 and s["steps"] == 6.0 and s["seen"] == 0.0
    assert states[1][A.P] == 0.25 + sign * 0.125          # the first window moved p in the direction the target was chosen for
    assert len({tuple(r.tolist()) for r in recs}) == 6          # six different records
    assert aug.p_tensor().data_ptr() == aug.state().data_ptr() and float(aug.p_tensor().cpu()) == s["p"]


def test_graphed_adaptive_iteration_follows_the_eager_sequence_while_a_window_closes_in_the_replays():
    """Three eager warm-up iterations + two replays of graph.GraphedTrainStep(aug=adaptive, lecam=) end in the bits of five eager
    iterations from the same seed -- weights, the head's record and the controller's state; the draws of (u, ug), the gated launches
    and the controller are inside the capture.  interval = 2: the second window closes in the first replay."""
    from test_gpu_lecam import _build, _snapshot
    from hr_viton_amd.graph import GraphedTrainStep
    from hr_viton_amd.lecam import LeCam
    from hr_viton_amd.losses import GANLoss, L1Loss
    target, _ = _target()
    aug_e, head_e, recs = _adaptive(target), LeCam(0.0), []
    want, want_losses = _train(5, aug_e, None, head_e, recs)
    p3 = A.initial_state(0.25)
    for r in recs[:3]:
        p3 = A.controller_step(p3, r.tolist(), 2, target, 0.125, 2, 1.0)
    assert aug_e.scalars()["updates"] == 2.0 and aug_e.scalars()["p"] != p3[A.P]          # p moved after the warm-up iterations
    aug_g, head_g = _adaptive(target), LeCam(0.0)
    opt, gen, Dn, og, od, inputs, nz = _build()
    gs = GraphedTrainStep(opt, gen, Dn, GANLoss("hinge"), L1Loss(), None, og, od, inputs, noise=nz[0], noise_d=nz[1], warmup=3,
                          aug=aug_g, lecam=head_g)
    for _ in range(2):
        losses_g, _ = gs(inputs)
    got = _snapshot(gen, Dn)
    _same(want, got)
    for k, v in want_losses.items():
        assert float(losses_g[k].detach()) == v, (k, float(losses_g[k].detach()), v)
    assert torch.equal(_bits(aug_e.state()), _bits(aug_g.state())), (aug_e.scalars(), aug_g.scalars())
    assert torch.equal(_bits(head_e.stats()), _bits(head_g.stats()))


# ---------------------------------------------------------------------------------------------------------------
# 10. checkpoints
# ---------------------------------------------------------------------------------------------------------------
def test_a_reloaded_state_continues_the_sequence_bitwise(tmp_path):
    diffaug, ops, _ = _mods()
    from hr_viton_amd.lecam import LeCam
    cfg, seq = A.HAND, A.HAND_SEQ
    want = A.run_sequence(cfg, seq)
    # batch 2, interval 2, kimg 0.016: step = 1/4
    mk = lambda: diffaug.AdaptiveAugment("color,cutout", target=cfg["target"], kimg=0.016, interval=2, p_max=cfg["p_max"])  # noqa: E731
    head = LeCam(0.0)
    head._buffers(torch.device("cuda", torch.cuda.current_device()))
    head.num_D = cfg["num_d"]

    def launch(aug, item):
        head.stats().copy_(A.make_record(item[0], item[1]))
        aug.update(head, 2)
        return aug.state().cpu().clone()

    first = mk()
    assert first.step_size(2) == cfg["step"]
    with pytest.raises(ops.HrvError):
        first.update(LeCam(0.0), 2)          # a head that has not run
    cut = 4                                  # inside an open window, right after the poisoned step
    for i in range(cut):
        got = launch(first, seq[i])
    assert got[A.SEEN] == 1.0 and got[A.ACC] == 1.0
    torch.save(first.state_dict(), str(tmp_path / "ada.pth"))
    second = mk()
    second.load_state_dict(torch.load(str(tmp_path / "ada.pth"), map_location="cpu"))
    assert second.scalars() == first.scalars()          # (before its first launch: what the file left for it)
    for i in range(cut, len(seq)):
        a, b = launch(first, seq[i]), launch(second, seq[i])
        assert torch.equal(_bits(a), _bits(b)) and torch.equal(_bits(a), _bits(torch.tensor(want[i], dtype=torch.float64))), i
    # onto an object that already has its device state
    third = mk()
    third.draw(2, "cuda")
    third.load_state_dict(first.state_dict())
    assert torch.equal(_bits(third.state()), _bits(first.state()))


# ---------------------------------------------------------------------------------------------------------------
# 11. the script
# ---------------------------------------------------------------------------------------------------------------
GEN_ARGV = ["--synthetic", "-b", "2", "--fine_height", "256", "--fine_width", "192", "--num_upsampling_layers", "more", "--ngf", "8",
            "--ndf", "8", "--tocg_ngf", "8", "--max_steps", "2", "--num_test_visualize", "0", "--no_vgg_loss", "--display_count", "1",
            "--lpips_count", "1000", "--save_count", "1000"]


def test_train_generator_with_and_without_the_flags(tmp_path, capsys):
    import train_generator as tg
    diffaug, ops, _ = _mods()

    def run(name, extra):
        torch.manual_seed(0)
        ops.profile_begin()
        try:
            tg.main(["--name", name, "--checkpoint_dir", str(tmp_path / "ck"), "--tensorboard_dir", str(tmp_path / "tb")] + GEN_ARGV + extra)
        finally:
            recs = ops.profile_end()
        names = [r[1] for r in recs]
        sd = {k: torch.load(str(tmp_path / "ck" / name / f), map_location="cpu") for k, f in
              (("gen", "gen_model_final.pth"), ("dis", "dis_model_final.pth"))}
        return names, sd, capsys.readouterr().out

    count = lambda names, n: sum(1 for x in names if x == n)  # noqa: E731
    # batch 2, interval 1, kimg 0.016: step = 1/8; a target of -1 can only be met from above
    flags = ["--diffaug", "color,translation,cutout", "--ada_target", "-1", "--ada_interval", "1", "--ada_kimg", "0.016", "--ada_p_init", "0.5"]
    names_a, sd_a, out_a = run("a", flags)
    assert (count(names_a, "diffaug_mean"), count(names_a, "diffaug_concat_gated"), count(names_a, "diffaug_gsum_gated"),
            count(names_a, "diffaug_bwd_gated"), count(names_a, "ada_update"), count(names_a, "dhead_reduce")) == (4, 8, 2, 2, 2, 2), \
        [n for n in names_a if "diffaug" in n or n.startswith("ada_")]
    assert count(names_a, "concat_nhwc_nchw") == 0 and count(names_a, "diffaug_concat") == 0
    ps = [float(v) for v in re.findall(r"ada_p: (\S+?),?(?:\s|$)", out_a)]
    assert len(ps) == 2 and all(0.0 <= v <= 1.0 for v in ps), out_a
    assert len(re.findall(r"r_t: -?\d\.\d+/-?\d\.\d+", out_a)) == 2, out_a          # the head was switched on with weight 0
    saved = torch.load(str(tmp_path / "ck" / "a" / "ada_final.pth"), map_location="cpu")
    assert saved["state"][A.STEPS] == 2.0 and saved["state"][A.UPDATES] == 2.0 and saved["state"][A.SEEN] == 0.0
    assert float(saved["state"][A.P]) == ps[-1] and saved["target"] == -1.0 and saved["interval"] == 1
    for sd in sd_a.values():
        assert all(bool(torch.isfinite(v).all()) for v in sd.values() if v.is_floating_point())
    fresh = diffaug.AdaptiveAugment("color,translation,cutout", target=-1.0, interval=1, kimg=0.016)
    fresh.load_state_dict(saved)                 # strict
    # without the flags: no such launch, the option line it always printed, and two runs end in the same bits
    names_p, sd_p, out_p = run("p", [])
    names_q, sd_q, out_q = run("q", [])
    assert not [n for n in names_p + names_q if "diffaug" in n or n.startswith("ada_") or "dhead" in n]
    assert count(names_p, "concat_nhwc_nchw") == 8
    assert "ada_" not in out_p and "diffaug" not in out_p
    for which in ("gen", "dis"):
        assert list(sd_p[which]) == list(sd_q[which])
        for k, v in sd_p[which].items():
            w = sd_q[which][k]
            assert torch.equal(v.view(torch.int32), w.view(torch.int32)) if v.dtype == torch.float32 else torch.equal(v, w), (which, k)
    assert any(not torch.equal(sd_a["dis"][k], sd_p["dis"][k]) for k in sd_p["dis"] if sd_p["dis"][k].is_floating_point())
