"""GPU: DiffAugment inside the PatchGAN input assembly (csrc/diffaug.hip, hr_viton_amd/diffaug.py) against the restatements of
tests/diffaug_cases.py -- geometry to the bit, color inside the bound derived there, the two reductions exactly and reproducibly,
the discriminator's pair form against itself fed the restated-augmented inputs, a captured draw + assembly, the script, and the
captured iteration against the eager one."""
import copy
import functools
import re

import pytest
import torch

import diffaug_cases as D

pytestmark = pytest.mark.gpu
IDS = lambda s: "x".join(map(str, s))  # noqa: E731
CA = 7


def _mods():
    import hr_viton_amd  # noqa: F401
    from hr_viton_amd import diffaug, ops
    from hr_viton_amd import train_ops as T
    return diffaug, ops, T


@functools.lru_cache(maxsize=None)
def _gauss(shape):
    N, H, W = shape
    return D.gauss_inputs(N, H, W, 100 + H)


def _forward(parse, img, u, flags, mean=None):
    """the stand-alone op on the device -> ([N,H,W,12] on the host, the leaf image on the device)"""
    diffaug, ops, _ = _mods()
    x = img.cuda().requires_grad_()
    out = diffaug.diffaug_concat(ops.Act(parse.cuda(), CA), x, u.cuda(), flags, mean=None if mean is None else mean.cuda())
    assert out.C == CA + 3 and tuple(out.t.shape) == (*parse.shape[:3], 12)
    return out, x


# ---------------------------------------------------------------------------------------------------------------
# 1. geometry: a pure gather and select
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", D.SHAPES, ids=IDS)
def test_geometry_forward_and_backward_equal_the_index_restatement(shape):
    N, H, W = shape
    parse, fake, _ = _gauss(shape)
    gen = torch.Generator().manual_seed(H)
    g = torch.randn(N, H, W, 12, generator=gen)
    for names, u in D.batches(D.forced_rows(H, W), N):
        for flags in (D.GEOMETRY, D.TRANSLATION, D.CUTOUT):
            out, x = _forward(parse, fake, u, flags)
            want = D.forward_ref(parse, CA, fake, u, flags)
            assert torch.equal(out.t.detach().cpu().double(), want), (names, flags)
            out.t.backward(g.cuda())
            assert torch.equal(x.grad.cpu().double(), D.backward_ref(g, CA, u, flags)), (names, flags)
    # no transform at all: the plain assembly and the plain slice
    u = D.batches(D.forced_rows(H, W), N)[-1][1]
    out, x = _forward(parse, fake, u, 0)
    assert torch.equal(out.t.detach().cpu()[..., :CA], parse[..., :CA]) and torch.equal(out.t.detach().cpu()[..., CA:CA + 3], fake.permute(0, 2, 3, 1))
    assert float(out.t.detach()[..., CA + 3:].abs().max()) == 0.0
    out.t.backward(g.cuda())
    assert torch.equal(x.grad.cpu(), g[..., CA:CA + 3].permute(0, 3, 1, 2))


@pytest.mark.parametrize("shape", D.SHAPES[1:3], ids=IDS)
def test_a_nan_behind_the_mask_stays_out(shape):
    N, H, W = shape
    parse, fake, _ = _gauss(shape)
    gen = torch.Generator().manual_seed(H + 1)
    g = torch.randn(N, H, W, 12, generator=gen)
    hidden_src = hidden_dst = 0
    for names, u in D.batches(D.forced_rows(H, W), N):
        bad_img, bad_parse, bad_g = fake.clone(), parse.clone(), g.clone()
        for n in range(N):
            V = D.valid_map(u[n].numpy(), D.GEOMETRY, H, W)
            ty, tx = D.decode(u[n].numpy(), D.GEOMETRY, H, W)[1][:2]
            used = torch.zeros(H, W, dtype=torch.bool)
            vy, vx = torch.nonzero(V, as_tuple=True)
            used[vy + ty, vx + tx] = True                      # the sources some unmasked destination reads
            bad_img[n][:, ~used] = float("nan")
            bad_parse[n][~used] = float("nan")
            bad_g[n][~V] = float("nan")                         # the gradient of every masked destination
            hidden_src += int((~used).sum())
            hidden_dst += int((~V).sum())
        out, x = _forward(bad_parse, bad_img, u, D.GEOMETRY)
        assert torch.equal(out.t.detach().cpu().double(), D.forward_ref(parse, CA, fake, u, D.GEOMETRY)), names
        out.t.backward(bad_g.cuda())
        assert torch.equal(x.grad.cpu().double(), D.backward_ref(g, CA, u, D.GEOMETRY)), names
    assert hidden_src > 0 and hidden_dst > 0


# ---------------------------------------------------------------------------------------------------------------
# 2. color
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", D.POW2_SHAPES, ids=IDS)
def test_color_is_exact_on_integer_images(shape):
    """s = 1, k and beta powers of two, HW a power of two, a mean with two fractional bits: no rounding anywhere"""
    N, H, W = shape
    parse, _, _ = _gauss((N, H, W))
    img = D.int_image(N, H, W, 5 + H)
    g = D.int_values((N, H, W, 12), 6 + H)
    for u0, u2 in ((0.75, 0.0), (0.0, 0.5), (0.25, 0.0), (0.5, 0.5)):          # beta = 1/4, -1/2, -1/4, 0; k = 1/2, 1
        for names, u in D.batches(D.forced_rows(H, W), N)[::4]:
            u = u.clone()
            u[:, 0], u[:, 1], u[:, 2] = u0, 0.5, u2
            out, x = _forward(parse, img, u, D.ALL)
            want = D.forward_ref(parse, CA, img, u, D.ALL, mean=D.mean_ref(img))
            assert torch.equal(want.float().double(), want)
            assert torch.equal(out.t.detach().cpu().double(), want), (names, u0, u2)
            out.t.backward(g.cuda())
            err = (x.grad.cpu().double() - D.backward_ref(g, CA, u, D.ALL)).abs()
            assert bool((err <= D.backward_bound(g, CA, u, D.ALL)).all()), (names, u0, u2, float(err.max()))
            if u2 == 0.5:      # k = 1: no term carries the 1 / (3 HW), the backward is exact too
                assert float(err.max()) == 0.0, (names, u0)


@pytest.mark.parametrize("flags", [D.ALL, D.COLOR], ids=["all", "color"])
@pytest.mark.parametrize("shape", D.SHAPES, ids=IDS)
def test_color_on_gaussian_data_is_inside_the_bound(shape, flags, capsys):
    """|kernel - float64| <= 8 * 2^-24 * (k s |x| + k |1 - s| |m| + |1 - k| |M| + |beta|), and the same on the backward's terms; the
    measured maxima, as shares of the bound, are printed"""
    N, H, W = shape
    parse, fake, real = _gauss(shape)
    gen = torch.Generator().manual_seed(H + 2)
    g = torch.randn(N, H, W, 12, generator=gen)
    worst_f = worst_b = 0.0
    for names, u in D.batches(D.forced_rows(H, W), N):
        u = u.clone()
        u[:, :3] = torch.rand(N, 3, generator=gen)
        for img in (fake, real):
            out, x = _forward(parse, img, u, flags)
            M = D.mean_ref(img)
            want, bound = D.forward_ref(parse, CA, img, u, flags, mean=M), D.forward_bound(CA, img, u, flags, M)
            err = (out.t.detach().cpu().double() - want).abs()
            assert bool((err <= bound).all()), (names, float((err - bound).max()))
            worst_f = max(worst_f, float((err / bound.clamp_min(1e-300)).max()))
            out.t.backward(g.cuda())
            want, bound = D.backward_ref(g, CA, u, flags), D.backward_bound(g, CA, u, flags)
            err = (x.grad.cpu().double() - want).abs()
            assert bool((err <= bound).all()), (names, float((err - bound).max()))
            worst_b = max(worst_b, float((err / bound.clamp_min(1e-300)).max()))
    with capsys.disabled():
        print(f"\n[diffaug] {IDS(shape)} flags {flags}: worst error / bound  forward {worst_f:.3f}  backward {worst_b:.3f}")
    assert 0.0 < worst_f <= 1.0 and 0.0 < worst_b <= 1.0


@pytest.mark.parametrize("shape", D.SHAPES + D.POW2_SHAPES[1:], ids=IDS)
def test_mean_and_gsum_are_exact_on_integers_and_reproducible(shape):
    _, ops, T = _mods()
    N, H, W = shape
    fake, real = D.int_values((N, 3, H, W), H), D.int_values((N, 3, H, W), H + 1, -3, 90)
    fc, rc = fake.cuda(), real.cuda()
    m1, m2 = T.diffaug_mean(fc, rc), T.diffaug_mean(fc, rc)
    assert torch.equal(m1.cpu(), torch.cat((D.mean_ref(fake), D.mean_ref(real))))
    assert torch.equal(m1.view(torch.int32), m2.view(torch.int32))
    assert torch.equal(T.diffaug_mean(rc).cpu(), D.mean_ref(real))
    # Gaussian data: reproducible to the bit, and the fp64 sum rounded once
    _, gf, gr = _gauss(shape) if shape in D.SHAPES else D.gauss_inputs(N, H, W, 3)
    a, b = T.diffaug_mean(gf.cuda(), gr.cuda()), T.diffaug_mean(gf.cuda(), gr.cuda())
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    want = torch.cat((gf, gr)).double().mean(dim=(1, 2, 3))
    assert float((a.cpu().double() - want).abs().max()) <= 2.0 ** -24 * float(want.abs().max()) + 1e-12
    g = D.int_values((N, H, W, 12), H + 2)
    gg = torch.randn(N, H, W, 12, generator=torch.Generator().manual_seed(H))
    for names, u in D.batches(D.forced_rows(H, W), N)[::2]:
        for flags in (D.ALL, D.COLOR):
            s1 = T.diffaug_gsum(ops.Act(g.cuda(), CA + 3), CA, u.cuda(), flags)
            assert s1.dtype == torch.float64 and torch.equal(s1.cpu(), D.gsum_ref(g, CA, u, flags)), (names, flags)
            r1 = T.diffaug_gsum(ops.Act(gg.cuda(), CA + 3), CA, u.cuda(), flags)
            r2 = T.diffaug_gsum(ops.Act(gg.cuda(), CA + 3), CA, u.cuda(), flags)
            assert torch.equal(r1.view(torch.int64), r2.view(torch.int64))
            want = D.gsum_ref(gg, CA, u, flags)
            assert float((r1.cpu() - want).abs().max()) <= 1e-12 * float(gg.abs().sum())


def test_other_shapes_are_rejected():
    diffaug, ops, T = _mods()
    N, H, W = 1, 8, 8
    parse, fake, _ = _gauss((N, H, W))
    u = torch.full((N, 8), 0.5).cuda()
    with pytest.raises(ops.HrvError):          # a parse map with channel stride 12
        diffaug.diffaug_concat(ops.Act(torch.zeros(N, H, W, 12).cuda(), 7), fake.cuda(), u, "cutout")
    with pytest.raises(ops.HrvError):          # 4 image channels
        diffaug.diffaug_concat(ops.Act(parse.cuda(), 7), torch.zeros(N, 4, H, W).cuda(), u, "cutout")
    with pytest.raises(ops.HrvError):          # uniforms of the wrong shape
        diffaug.diffaug_concat(ops.Act(parse.cuda(), 7), fake.cuda(), u[:, :7], "cutout")
    with pytest.raises(ops.HrvError, match="PatchGAN shape"):          # a gradient with channel stride 8
        T.diffaug_bwd(ops.Act(torch.zeros(N, H, W, 8).cuda(), 8), 5, u, None, D.GEOMETRY)
    with pytest.raises(ops.HrvError, match="means"):                   # color without the means
        T.diffaug_concat(ops.Act(parse.cuda(), 7), fake.cuda(), u, None, D.COLOR, ops.Act(torch.empty(N, H, W, 12).cuda(), 10))


# ---------------------------------------------------------------------------------------------------------------
# 3. the discriminator's pair form
# ---------------------------------------------------------------------------------------------------------------
def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-12)).item()


@pytest.mark.parametrize("policy", ["translation,cutout", "color,translation,cutout"])
def test_pair_form_with_aug_equals_the_plain_pair_form_on_restated_inputs(policy):
    """_DiscPairFn with ``aug`` against the same function without it, fed the restated-augmented parse map, fake and real image, on the
    same weights and spectral-norm state (the tiny discriminator of tests/test_gpu_train_step.py): predictions bit-identical under the
    geometry policy and within that file's PatchGAN tolerance (1e-4 of the largest value) with color; d(fake) = the restated adjoint
    of the plain path's input gradient (with color: within 2e-2, the tolerance that file gives gradients through sign() terms)."""
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
    aug = diffaug.DiffAugment(policy)
    geometry = not aug.color
    parse = torch.cat((seg.permute(0, 2, 3, 1), torch.zeros(N, H, W, 1)), dim=3).contiguous()
    cg, cf = GANLoss("hinge"), L1Loss()

    def loss(pf, pr):
        tot = cg(pf, True, for_discriminator=False)
        for i in range(len(pf)):
            for j in range(len(pf[i]) - 1):
                tot = tot + cf(pf[i][j], pr[i][j].detach()) * 10.0 / len(pf)
        return tot

    fa = fake.cuda().requires_grad_()
    pf_a, pr_a = Dn.forward_pair(ops.Act(parse.cuda(), CA), fa, real.cuda(), aug=aug, aug_u=u.cuda())
    loss(pf_a, pr_a).sum().backward()
    # the plain pair form on the restated-augmented inputs
    in_f = D.forward_ref(parse, CA, fake, u, aug.flags, mean=D.mean_ref(fake)).float()
    in_r = D.forward_ref(parse, CA, real, u, aug.flags, mean=D.mean_ref(real)).float()
    assert torch.equal(in_f[..., :CA], in_r[..., :CA]) and not torch.equal(in_f[..., :CA], parse[..., :CA])
    parse_aug = torch.cat((in_f[..., :CA], torch.zeros(N, H, W, 1)), dim=3).contiguous()
    fb = in_f[..., CA:CA + 3].permute(0, 3, 1, 2).contiguous().cuda().requires_grad_()
    pf_b, pr_b = D2.forward_pair(ops.Act(parse_aug.cuda(), CA), fb, in_r[..., CA:CA + 3].permute(0, 3, 1, 2).contiguous().cuda())
    loss(pf_b, pr_b).sum().backward()
    gin = torch.zeros(N, H, W, 12)
    gin[..., CA:CA + 3] = fb.grad.cpu().permute(0, 2, 3, 1)
    want = D.backward_ref(gin, CA, u, aug.flags)
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
    pf_a, pr_a = Dn.forward_pair(ops.Act(parse.cuda(), CA), fake.cuda(), real.cuda(), aug=aug, aug_u=u.cuda())
    (cg(pf_a, False, for_discriminator=True) + cg(pr_a, True, for_discriminator=True)).sum().backward()
    pf_b, pr_b = D2.forward_pair(ops.Act(parse_aug.cuda(), CA), fb.detach(), in_r[..., CA:CA + 3].permute(0, 3, 1, 2).contiguous().cuda())
    (cg(pf_b, False, for_discriminator=True) + cg(pr_b, True, for_discriminator=True)).sum().backward()
    for (n_, p), (_, q) in zip(Dn.named_parameters(), D2.named_parameters()):
        assert (p.grad is None) == (q.grad is None), n_
        if p.grad is not None and geometry:
            assert torch.equal(p.grad, q.grad), n_


# ---------------------------------------------------------------------------------------------------------------
# 4. capture
# ---------------------------------------------------------------------------------------------------------------
def test_a_captured_draw_and_assembly_augments_anew_at_every_replay():
    diffaug, ops, _ = _mods()
    shape = (3, 64, 48)
    N, H, W = shape
    parse, fake, _ = _gauss(shape)
    pc, fc = parse.cuda(), fake.cuda()
    aug = diffaug.DiffAugment("color,translation,cutout")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        diffaug.diffaug_concat(ops.Act(pc, CA), fc, aug.draw(N, fc.device), aug)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        u = aug.draw(N, fc.device)
        out = diffaug.diffaug_concat(ops.Act(pc, CA), fc, u, aug).t
    seen = []
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        seen.append((u.cpu().clone(), out.cpu().clone()))
    assert not torch.equal(seen[0][0], seen[1][0]) and not torch.equal(seen[0][1], seen[1][1])
    M = D.mean_ref(fake)
    for ui, oi in seen:
        assert bool((ui >= 0).all()) and bool((ui < 1).all())
        want, bound = D.forward_ref(parse, CA, fake, ui, D.ALL, mean=M), D.forward_bound(CA, fake, ui, D.ALL, M)
        assert bool(((oi.double() - want).abs() <= bound).all())
        assert torch.equal(oi[..., :CA].double(), want[..., :CA])


# ---------------------------------------------------------------------------------------------------------------
# 5. the script
# ---------------------------------------------------------------------------------------------------------------
GEN_ARGV = ["--synthetic", "-b", "2", "--fine_height", "256", "--fine_width", "192", "--num_upsampling_layers", "more", "--ngf", "8",
            "--ndf", "8", "--tocg_ngf", "8", "--max_steps", "2", "--num_test_visualize", "0", "--no_vgg_loss", "--display_count", "1",
            "--lpips_count", "1000", "--save_count", "1000"]


def test_train_generator_with_and_without_the_flag(tmp_path, capsys):
    import train_generator as tg
    _, ops, _ = _mods()

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

    names_a, sd_a, out_a = run("a", ["--diffaug", "color,translation,cutout"])
    names_p, sd_p, out_p = run("p", [])
    names_q, sd_q, out_q = run("q", [])
    # with the flag: per iteration 2 calls x (1 mean + 2 assemblies), and the generator step's gsum + bwd; finite losses
    count = lambda names, n: sum(1 for x in names if x == n)  # noqa: E731
    assert (count(names_a, "diffaug_mean"), count(names_a, "diffaug_concat"), count(names_a, "diffaug_gsum"), count(names_a, "diffaug_bwd")) \
        == (4, 8, 2, 2), [n for n in names_a if n.startswith("diffaug")]
    assert count(names_a, "concat_nhwc_nchw") == 0
    assert "diffaug='color,translation,cutout'" in out_a
    vals = [float(v) for v in re.findall(r"(?:G_loss|G_adv_loss|D_loss|D_fake_loss|D_real_loss): (\S+?),?(?:\s|$)", out_a)]
    assert len(vals) == 10 and all(v == v and abs(v) < 1e6 for v in vals), out_a
    for sd in sd_a.values():
        assert all(bool(torch.isfinite(v).all()) for v in sd.values() if v.is_floating_point())
    # without it: no such launch, the option line it always printed, and two runs end in the same bits
    assert not [n for n in names_p + names_q if "diffaug" in n] and count(names_p, "concat_nhwc_nchw") == 8
    assert "diffaug" not in out_p
    for which in ("gen", "dis"):
        assert list(sd_p[which]) == list(sd_q[which])
        for k, v in sd_p[which].items():
            w = sd_q[which][k]
            assert torch.equal(v.view(torch.int32), w.view(torch.int32)) if v.dtype == torch.float32 else torch.equal(v, w), (which, k)
    assert any(not torch.equal(sd_a["dis"][k], sd_p["dis"][k]) for k in sd_p["dis"] if sd_p["dis"][k].is_floating_point())


def test_graphed_iteration_with_aug_follows_the_eager_sequence():
    """graph.GraphedTrainStep(aug=...): the uniforms are drawn inside the captured region from the device generator, so from the same
    seed three eager warm-up iterations + two replays consume the draws five eager iterations consume and end in the same bits
    (injected SPADE noise: the augmentation is the only consumer of the generator)."""
    from test_gpu_train_step import _setup
    diffaug, ops, _ = _mods()
    from hr_viton_amd import gen_train, pipeline
    from hr_viton_amd.graph import GraphedTrainStep
    from hr_viton_amd.losses import GANLoss, L1Loss
    from hr_viton_amd.optim import Adam
    aug = diffaug.DiffAugment("color,translation,cutout")

    def build():
        opt, gen, Dn, x, seg, real, noise = _setup(seed=33, wmul=6.0)          # 2 x 256 x 128
        opt.lambda_feat = 10.0
        gen.cuda().train()
        Dn.cuda().train()
        og = Adam(gen.parameters(), lr=1e-3, betas=(0.0, 0.9), device_step=True)
        od = Adam(Dn.parameters(), lr=2e-3, betas=(0.0, 0.9), device_step=True)
        g = torch.Generator().manual_seed(5)
        n_el = gen_train.noise_elems(gen, x.shape[0])
        nz = [gen_train.noise_planes(gen, x.shape[0], torch.randn(n_el, generator=g).cuda()) for _ in range(2)]
        inputs = {"x": x.cuda(), "parse7": ops.to_nhwc(seg.cuda()).t, "im": real.cuda()}
        torch.manual_seed(99)
        return opt, gen, Dn, og, od, inputs, nz

    def snapshot(gen, Dn):
        torch.cuda.synchronize()
        sd = {"G." + k: v.detach().cpu().clone() for k, v in gen.state_dict().items()}
        sd.update({"D." + k: v.detach().cpu().clone() for k, v in Dn.state_dict().items()})
        return sd

    opt, gen, Dn, og, od, inputs, nz = build()
    for _ in range(5):
        losses_e, _ = pipeline.generator_train_step(opt, gen, Dn, GANLoss("hinge"), L1Loss(), None, og, od, inputs["x"],
                                                    ops.Act(inputs["parse7"], 7), inputs["im"], noise=nz[0], noise_d=nz[1], aug=aug)
    want, want_losses = snapshot(gen, Dn), {k: float(v.detach()) for k, v in losses_e.items()}
    opt, gen, Dn, og, od, inputs, nz = build()
    for _ in range(5):
        pipeline.generator_train_step(opt, gen, Dn, GANLoss("hinge"), L1Loss(), None, og, od, inputs["x"],
                                      ops.Act(inputs["parse7"], 7), inputs["im"], noise=nz[0], noise_d=nz[1])
    plain = snapshot(gen, Dn)
    assert any(not torch.equal(want[k], plain[k]) for k in want if k.startswith("D."))       # the augmentation did act
    opt, gen, Dn, og, od, inputs, nz = build()
    gs = GraphedTrainStep(opt, gen, Dn, GANLoss("hinge"), L1Loss(), None, og, od, inputs, noise=nz[0], noise_d=nz[1], warmup=3, aug=aug)
    for _ in range(2):
        losses_g, _ = gs(inputs)
    got = snapshot(gen, Dn)
    assert all(v == v for v in want_losses.values())
    for k in want:
        assert torch.equal(want[k], got[k]), k
    for k, v in want_losses.items():
        assert float(losses_g[k]) == v, (k, float(losses_g[k]), v)
