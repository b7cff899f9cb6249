"""GPU: the fused loss head of the discriminator step (hr_viton_amd.lecam, csrc/dhead.hip) against the float64 restatement of
tests/lecam_cases.py, against the four-call GANLoss path it replaces, inside the pair-form step, under capture and in the script."""
import copy
import re

import pytest
import torch

import lecam_cases as L

pytestmark = pytest.mark.gpu
CA = 7


def _mods():
    import hr_viton_amd  # noqa: F401
    from hr_viton_amd import _lib, lecam, ops
    return lecam, ops, _lib


def _place(pairs, off=0):
    """[(x_fake, x_real)] (CPU, any float dtype) -> the same as fp32 device LEAVES laid out as the discriminator hands them out: one
    buffer per scale, the real half n floats behind the fake half (4-byte aligned only when n is odd); ``off`` shifts the whole
    scale by that many floats from the allocator's boundary (the other alignment)."""
    out = []
    for f, r in pairs:
        n = f.numel()
        buf = torch.zeros(2 * n + off + 4, dtype=torch.float32, device="cuda")
        buf[off:off + n] = f.reshape(-1).float().cuda()
        buf[off + n:off + 2 * n] = r.reshape(-1).float().cuda()
        out.append((buf[off:off + n].view(f.shape).detach().requires_grad_(), buf[off + n:off + 2 * n].view(r.shape).detach().requires_grad_()))
    return out


def _run(head, leaves, g=(1.0, 1.0, 1.0)):
    """one forward + backward of the head -> (losses fp32 CPU [3], [(d_fake, d_real)] CPU, record CPU fp64)"""
    for f, r in leaves:
        f.grad = r.grad = None
    out = head.d_losses([[f] for f, _ in leaves], [[r] for _, r in leaves])
    (g[0] * out["D_Fake"] + g[1] * out["D_Real"] + g[2] * out["D_LeCam"]).sum().backward()
    torch.cuda.synchronize()
    losses = torch.cat([out["D_Fake"], out["D_Real"], out["D_LeCam"]]).detach().cpu()
    return losses, [(f.grad.cpu().clone(), r.grad.cpu().clone()) for f, r in leaves], head.stats().cpu().clone()


def _state(rec, lib, k, name):
    return float(rec[lib.DHEAD_STATE + lib.DHEAD_SCALE_WORDS * k + getattr(lib, "DHEAD_" + name)])


def _int_pairs(shapes, seed):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randint(-8, 9, s, generator=g).float(), torch.randint(-8, 9, s, generator=g).float()) for s in shapes]


# ---------------------------------------------------------------------------------------------------------------
# 1. raw sums
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(L.CASES))
def test_raw_sums_are_exact_on_integers_from_both_alignments_and_reproducible(case):
    lecam, ops, lib = _mods()
    assert lib.DHEAD_SLOTS == L.SLOTS
    pairs = _int_pairs(L.CASES[case], seed=11)
    ref = L.Restated(0.0)
    names = ("SUM_REAL", "SUM_FAKE", "SIGN_REAL", "HINGE_REAL", "HINGE_FAKE", "SUMSQ_REAL", "SUMSQ_FAKE", "NONFINITE_K")
    keys = ("sum_real", "sum_fake", "sign_real", "hinge_real", "hinge_fake", "sumsq_real", "sumsq_fake", "nonfinite")
    for off in (0, 1):
        leaves = _place(pairs, off)
        if off == 0:
            assert all((r.data_ptr() % 16 == 0) == (r.numel() % 4 == 0) for _, r in leaves)
        recs = []
        for _ in range(2):
            head = lecam.LeCam(0.0)
            _, _, rec = _run(head, leaves)
            recs.append(rec)
        assert torch.equal(recs[0].view(torch.int64), recs[1].view(torch.int64))
        for k, (f, r) in enumerate(pairs):
            want = ref.sums(f, r)
            for name, key in zip(names, keys):
                got = float(recs[0][lib.DHEAD_SUMS + lib.DHEAD_SCALE_WORDS * k + getattr(lib, "DHEAD_" + name)])
                assert got == float(want[key]), (case, off, k, name, got, want[key])


# ---------------------------------------------------------------------------------------------------------------
# 2. chained exactness
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["paper", "relu"])
@pytest.mark.parametrize("n", L.EXACT["n"])
def test_six_chained_steps_equal_the_restatement_exactly(form, n):
    lecam, ops, lib = _mods()
    E = L.EXACT
    ns = [n, max(1, n // 2)]
    data = L.exact_logits(ns, E["steps"], seed=7 + n)
    ref = L.Restated(E["weight"], E["decay"], E["start"], form)
    head = lecam.LeCam(E["weight"], E["decay"], E["start"], form)
    for step, pairs in enumerate(data):
        want = ref.step(pairs)
        losses, grads, rec = _run(head, _place(pairs))
        assert float(rec[lib.DHEAD_COUNT]) == ref.count == step + 1
        assert float(rec[lib.DHEAD_LAMBDA]) == want["lambda"]
        for k in range(len(ns)):
            assert _state(rec, lib, k, "ANCHOR_REAL") == ref.anchor_real[k], (step, k)
            assert _state(rec, lib, k, "ANCHOR_FAKE") == ref.anchor_fake[k], (step, k)
            assert _state(rec, lib, k, "RT_AVG") == ref.rt_avg[k] and _state(rec, lib, k, "RT") == want["r_t"][k]
            assert (_state(rec, lib, k, "MEAN_REAL"), _state(rec, lib, k, "MEAN_FAKE")) == want["means"][k]
            for got, exact in zip(grads[k], want["grads"][k]):
                assert torch.equal(exact.float().double(), exact) and torch.equal(got, exact.float()), (step, k)
        assert torch.equal(losses, torch.tensor(want["losses"], dtype=torch.float64).float()), (step, losses, want["losses"])
    assert want["lambda"] == E["weight"] and float(losses[2]) > 0


# ---------------------------------------------------------------------------------------------------------------
# 3. gaussian logits inside the derived bound
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["paper", "relu"])
@pytest.mark.parametrize("case", sorted(L.CASES))
def test_gaussian_logits_are_inside_the_bound(case, form, capsys):
    lecam, ops, lib = _mods()
    shapes = L.CASES[case]
    weight, decay, g = 0.3, 0.9, (0.5, 2.0, 1.5)
    ref, head = L.Restated(weight, decay, 0, form), lecam.LeCam(weight, decay, 0, form)
    worst = 0.0
    for step in range(2):       # (the second step uses the decay)
        pairs = L.gaussian_logits(shapes, seed=100 + step)
        want = ref.step(pairs, g=g)
        losses, grads, rec = _run(head, _place(pairs), g=g)
        n_max = max(L.numel(s) for s in shapes)
        for j in range(3):
            bound = L.loss_bound(want["losses"][j], want["mag"][j], n_max)
            err = abs(float(losses[j].double()) - want["losses"][j])
            worst = max(worst, err / bound)
            assert err <= bound, (case, form, step, j, err, bound)
        K = len(shapes)
        for k, (f, r) in enumerate(pairs):
            n = f.numel()
            c = (g[2] / K) * want["lambda"] * 2.0 / n
            for half, x, anchor in ((0, f, ref.anchor_real[k]), (1, r, ref.anchor_fake[k])):
                bound = L.grad_bound(want["hinge"][k][half], want["reg"][k][half], x.double(), anchor, c, n)
                err = (grads[k][half].double() - want["grads"][k][half]).abs()
                assert bool((err <= bound).all()), (case, form, step, k, half, float((err / bound).max()))
                worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
    with capsys.disabled():
        print("\n[dhead %s %s] worst share of the bound: %.3f" % (case, form, worst))


# ---------------------------------------------------------------------------------------------------------------
# 4. weight 0 against the four GANLoss calls
# ---------------------------------------------------------------------------------------------------------------
# gaussian logits on every shape of the table (num_D = 1, 2, 3); integer logits on the exact family (power-of-two n and num_D: the
# means are then exact in fp32 on both paths)
_W0 = [("gaussian", c) for c in sorted(L.CASES)] + [("integer", "%d_x%d" % (n, k)) for n in L.EXACT["n"] for k in (1, 2)]


@pytest.mark.parametrize("data,case", _W0)
def test_weight_zero_is_the_four_call_path(case, data):
    lecam, ops, lib = _mods()
    from hr_viton_amd.losses import GANLoss
    if data == "gaussian":
        shapes = L.CASES[case]
        pairs = L.gaussian_logits(shapes, seed=5)
    else:
        n, k = (int(v) for v in case.split("_x"))
        shapes = [(1, 1, 1, n), (1, 1, 1, max(1, n // 2))][:k]
        pairs = _int_pairs(shapes, seed=5)
    K = len(shapes)
    losses, grads, _ = _run(lecam.LeCam(0.0), _place(pairs))
    leaves = _place(pairs)
    crit = GANLoss("hinge")
    d_fake = crit([[f] for f, _ in leaves], False, for_discriminator=True)
    d_real = crit([[r] for _, r in leaves], True, for_discriminator=True)
    sum([d_fake, d_real]).mean().backward()
    torch.cuda.synchronize()
    assert float(losses[2]) == 0.0 and not bool(torch.signbit(losses[2]))
    old = torch.cat([d_fake, d_real]).detach().cpu()
    if data == "integer":
        assert torch.equal(losses[:2], old), (losses, old)
    else:
        assert L.ulp_distance(losses[:2], old) <= 1, (losses, old)
    for (f, r), (gf, gr) in zip(leaves, grads):
        for a, b in ((f.grad.cpu(), gf), (r.grad.cpu(), gr)):
            if K in (1, 2):
                assert torch.equal(a, b)
            else:
                assert L.ulp_distance(a, b) <= 1


# ---------------------------------------------------------------------------------------------------------------
# 5. start
# ---------------------------------------------------------------------------------------------------------------
def test_before_start_the_gradient_is_the_hinge_one_while_the_anchors_move():
    lecam, ops, lib = _mods()
    shapes = L.CASES["n5_255_256"]
    head, plain = lecam.LeCam(0.3, 0.9, start=3), lecam.LeCam(0.0, 0.9)
    anchors = []
    for step in range(4):
        pairs = L.gaussian_logits(shapes, seed=40 + step)
        losses, grads, rec = _run(head, _place(pairs))
        _, grads0, _ = _run(plain, _place(pairs))
        same = all(torch.equal(a, b) for ga, gb in zip(grads, grads0) for a, b in zip(ga, gb))
        anchors.append(_state(rec, lib, 1, "ANCHOR_REAL"))
        assert float(rec[lib.DHEAD_COUNT]) == step + 1
        if step < 3:
            assert same and float(losses[2]) == 0.0 and float(rec[lib.DHEAD_LAMBDA]) == 0.0
        else:
            assert not same and float(losses[2]) > 0.0 and float(rec[lib.DHEAD_LAMBDA]) == 0.3
    assert len(set(anchors)) == 4


# ---------------------------------------------------------------------------------------------------------------
# 6. poisoned step
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
@pytest.mark.parametrize("form", ["paper", "relu"])
def test_a_non_finite_logit_leaves_anchors_average_and_count_alone(bad, form):
    lecam, ops, lib = _mods()
    shapes = L.CASES["n257_1023"]
    head, ref = lecam.LeCam(0.3, 0.9, 0, form), L.Restated(0.3, 0.9, 0, form)
    for step in range(2):
        pairs = L.gaussian_logits(shapes, seed=60 + step)
        ref.step(pairs)
        _, _, before = _run(head, _place(pairs))
    pairs = L.gaussian_logits(shapes, seed=70)
    pairs[1][0].view(-1)[123] = bad           # one fake logit of the second scale
    losses, _, after = _run(head, _place(pairs))
    keep = [lib.DHEAD_COUNT] + [lib.DHEAD_STATE + lib.DHEAD_SCALE_WORDS * k + j for k in range(2)
                                for j in (lib.DHEAD_ANCHOR_REAL, lib.DHEAD_ANCHOR_FAKE, lib.DHEAD_RT_AVG)]
    assert torch.equal(before[keep].view(torch.int64), after[keep].view(torch.int64))
    assert float(after[lib.DHEAD_NONFINITE]) == 1.0 and float(after[lib.DHEAD_COUNT]) == 2.0
    assert not bool(torch.isfinite(losses[2])) and not bool(torch.isfinite(losses.sum())) and not bool(torch.isfinite(losses[0]))
    # the next clean step continues from the old count and the old anchors
    pairs = L.gaussian_logits(shapes, seed=71)
    want = ref.step(pairs)
    losses, _, rec = _run(head, _place(pairs))
    assert float(rec[lib.DHEAD_COUNT]) == 3.0 == ref.count and float(rec[lib.DHEAD_NONFINITE]) == 0.0
    assert bool(torch.isfinite(losses).all())
    for k in range(2):
        assert abs(_state(rec, lib, k, "ANCHOR_REAL") - ref.anchor_real[k]) <= 1e-12
        assert abs(_state(rec, lib, k, "ANCHOR_FAKE") - ref.anchor_fake[k]) <= 1e-12
    assert abs(float(losses[2]) - want["losses"][2]) <= L.loss_bound(want["losses"][2], want["mag"][2], 1023)


def test_other_logits_are_rejected():
    lecam, ops, lib = _mods()
    head = lecam.LeCam(0.1)
    x = torch.zeros(2, 1, 4, 4, device="cuda")
    with pytest.raises(ops.HrvError):
        head.d_losses([[x.bfloat16()]], [[x.bfloat16()]])
    with pytest.raises(ops.HrvError):
        head.d_losses([[x]], [[x[:1]]])
    with pytest.raises(ops.HrvError):
        head.d_losses([[x]] * 5, [[x]] * 5)
    # a strided view gets a contiguous copy and its gradient comes back in the view's shape
    wide = torch.randn(2, 1, 4, 8, device="cuda")
    f, r = wide[..., ::2].detach().requires_grad_(), wide[..., 1::2].detach().requires_grad_()
    out = head.d_losses([[f]], [[r]])
    sum(out.values()).sum().backward()
    assert f.grad.shape == f.shape and float(f.grad.abs().sum()) > 0


# ---------------------------------------------------------------------------------------------------------------
# 7. the pair-form step
# ---------------------------------------------------------------------------------------------------------------
def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-12)).item()


def test_pair_form_parameter_gradients_are_the_plain_ones_plus_an_autograd_regulariser(capsys):
    """D step on the tiny discriminator of tests/test_gpu_train_step.py: forward_pair -> the head, against forward_pair -> the four
    GANLoss calls + the regulariser written with torch ops on the same logits (first step: the anchors are the detached means).
    Tolerance: the pair-form one of tests/test_gpu_diffaug.py for values that pass through the same kernels (1e-4 of the largest)."""
    from test_gpu_train_step import _setup
    lecam, ops, lib = _mods()
    from hr_viton_amd.losses import GANLoss
    opt, gen, Dn, x, seg, real, noise = _setup(seed=21, H=128, W=96, wmul=6.0)
    N, H, W = 2, 128, 96
    Dn.cuda().train()
    D2 = copy.deepcopy(Dn)
    g = torch.Generator().manual_seed(5)
    fake = (torch.rand(N, 3, H, W, generator=g) * 2 - 1).cuda()
    parse = torch.cat((seg.permute(0, 2, 3, 1), torch.zeros(N, H, W, 1)), dim=3).contiguous().cuda()
    lam = 0.5
    head = lecam.LeCam(lam)
    pf, pr = Dn.forward_pair(ops.Act(parse, CA), fake, real.cuda())
    la = head.d_losses(pf, pr)
    sum(la.values()).mean().backward()
    cg = GANLoss("hinge")
    pf2, pr2 = D2.forward_pair(ops.Act(parse, CA), fake, real.cuda())
    reg = 0
    for f_, r_ in zip(pf2, pr2):
        xf, xr = f_[-1], r_[-1]
        a_r, a_f = xr.detach().double().mean().float(), xf.detach().double().mean().float()
        reg = reg + ((xr - a_f) ** 2).mean() + ((xf - a_r) ** 2).mean()
    lb = {"D_Fake": cg(pf2, False, for_discriminator=True), "D_Real": cg(pr2, True, for_discriminator=True), "D_LeCam": lam * reg / len(pf2)}
    sum(lb.values()).mean().backward()
    torch.cuda.synchronize()
    for k in la:
        assert _rel(la[k], lb[k]) < 1e-4, (k, float(la[k].detach()), float(lb[k].detach()))
    assert float(la["D_LeCam"].detach()) > 0
    worst = 0.0
    scale = max(float(q.grad.abs().max()) for q in D2.parameters() if q.grad is not None)
    for (n_, p), (_, q) in zip(Dn.named_parameters(), D2.named_parameters()):
        assert (p.grad is None) == (q.grad is None), n_
        if p.grad is not None:
            err = float((p.grad.double() - q.grad.double()).abs().max()) / max(float(q.grad.abs().max()), 1e-3 * scale)
            worst = max(worst, err)
            assert err < 1e-4, (n_, err)
    with capsys.disabled():
        print("\n[dhead pair form] worst parameter-gradient error: %.2e" % worst)


def _build(seed=33):
    from test_gpu_train_step import _setup
    lecam, ops, lib = _mods()
    from hr_viton_amd import gen_train
    from hr_viton_amd.optim import Adam
    opt, gen, Dn, x, seg, real, noise = _setup(seed=seed, wmul=6.0)          # 2 x 256 x 128
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


def _snapshot(gen, Dn):
    torch.cuda.synchronize()
    sd = {"G." + k: v.detach().cpu().clone() for k, v in gen.state_dict().items()}
    sd.update({"D." + k: v.detach().cpu().clone() for k, v in Dn.state_dict().items()})
    return sd


def _eager(steps, head):
    lecam, ops, lib = _mods()
    from hr_viton_amd import pipeline
    from hr_viton_amd.losses import GANLoss, L1Loss
    opt, gen, Dn, og, od, inputs, nz = _build()
    kw = {} if head is None else {"lecam": head}
    for _ in range(steps):
        losses, _ = pipeline.generator_train_step(opt, gen, Dn, GANLoss("hinge"), L1Loss(), None, og, od, inputs["x"],
                                                  ops.Act(inputs["parse7"], 7), inputs["im"], noise=nz[0], noise_d=nz[1], **kw)
    return _snapshot(gen, Dn), {k: float(v.detach()) for k, v in losses.items()}


def test_weight_zero_leaves_three_train_steps_bit_identical():
    lecam, ops, lib = _mods()
    plain, lp = _eager(3, None)
    head = lecam.LeCam(0.0)
    stats, ls = _eager(3, head)
    for k in plain:
        assert torch.equal(plain[k], stats[k]), k
    assert ls["D_LeCam"] == 0.0 and set(ls) == set(lp) | {"D_LeCam"}
    s = head.scalars()
    assert s["count"] == 3 and len(s["r_t_avg"]) == 2 and all(-1.0 <= v <= 1.0 for v in s["r_t_avg"])


# ---------------------------------------------------------------------------------------------------------------
# 8. capture
# ---------------------------------------------------------------------------------------------------------------
def test_graphed_iteration_with_the_head_follows_the_eager_sequence_across_start():
    """Three eager warm-up iterations + two replays of graph.GraphedTrainStep(lecam=) end in the bits of five eager iterations,
    anchors and count included; start = 4, so lambda_eff switches on between the two replays, decided on the device."""
    lecam, ops, lib = _mods()
    from hr_viton_amd.graph import GraphedTrainStep
    from hr_viton_amd.losses import GANLoss, L1Loss
    mk = lambda: lecam.LeCam(0.25, 0.5, start=4)      # noqa: E731
    head_e = mk()
    want, want_losses = _eager(5, head_e)
    before, before_losses = _eager(4, mk())
    assert before_losses["D_LeCam"] == 0.0 and want_losses["D_LeCam"] > 0.0          # the crossing is at the fifth iteration
    head_g = mk()
    opt, gen, Dn, og, od, inputs, nz = _build()
    gs = GraphedTrainStep(opt, gen, Dn, GANLoss("hinge"), L1Loss(), None, og, od, inputs, noise=nz[0], noise_d=nz[1], warmup=3,
                          lecam=head_g)
    for _ in range(2):
        losses_g, _ = gs(inputs)
    got = _snapshot(gen, Dn)
    for k in want:
        assert torch.equal(want[k], got[k]), k
    for k, v in want_losses.items():
        assert float(losses_g[k]) == v, (k, float(losses_g[k]), v)
    assert torch.equal(head_e.stats().cpu().view(torch.int64), head_g.stats().cpu().view(torch.int64))
    assert head_g.scalars()["count"] == 5


# ---------------------------------------------------------------------------------------------------------------
# 9. the script
# ---------------------------------------------------------------------------------------------------------------
GEN_ARGV = ["--synthetic", "-b", "2", "--fine_height", "256", "--fine_width", "192", "--num_upsampling_layers", "more", "--ngf", "8",
            "--ndf", "8", "--tocg_ngf", "8", "--max_steps", "2", "--num_test_visualize", "0", "--no_vgg_loss", "--display_count", "1",
            "--lpips_count", "1000", "--save_count", "1000"]


def test_train_generator_with_and_without_the_flags(tmp_path, capsys):
    import train_generator as tg
    lecam, ops, lib = _mods()

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
    flags = ["--lecam", "0.3", "--lecam_start", "1", "--lecam_decay", "0.9"]
    names_a, sd_a, out_a = run("a", flags)
    assert (count(names_a, "dhead_reduce"), count(names_a, "dhead_finalize"), count(names_a, "dhead_grad")) == (2, 2, 2), \
        [n for n in names_a if n.startswith("dhead")]
    vals = [float(v) for v in re.findall(r"(?:G_loss|G_adv_loss|D_loss|D_fake_loss|D_real_loss|D_lecam): (\S+?),?(?:\s|$)", out_a)]
    assert len(vals) == 12 and all(v == v and abs(v) < 1e6 for v in vals), out_a
    assert len(re.findall(r"r_t: -?\d\.\d+/-?\d\.\d+", out_a)) == 2, out_a
    for sd in sd_a.values():
        assert all(bool(torch.isfinite(v).all()) for v in sd.values() if v.is_floating_point())
    saved = torch.load(str(tmp_path / "ck" / "a" / "lecam_final.pth"), map_location="cpu")
    fresh = lecam.LeCam(0.3, 0.9, 1)
    fresh.load_state_dict(saved)                 # strict
    assert saved["count"] == 2 and len(saved["anchor_real"]) == 2 and bool((saved["anchor_real"] != 0).all())
    # a resumed run continues count and anchors
    run("r", flags + ["--max_steps", "1", "--lecam_checkpoint", str(tmp_path / "ck" / "a" / "lecam_final.pth")])
    resumed = torch.load(str(tmp_path / "ck" / "r" / "lecam_final.pth"), map_location="cpu")
    assert resumed["count"] == 3
    assert not torch.equal(resumed["anchor_real"], saved["anchor_real"])
    assert bool(torch.isfinite(resumed["anchor_real"]).all()) and bool(torch.isfinite(resumed["anchor_fake"]).all())
    # without the flags: no such launch, the option line it always printed, and two runs end in the same bits
    names_p, sd_p, out_p = run("p", [])
    names_q, sd_q, out_q = run("q", [])
    assert not [n for n in names_p + names_q if "dhead" in n]
    assert "lecam" not in out_p and "r_t" not in out_p
    for which in ("gen", "dis"):
        assert list(sd_p[which]) == list(sd_q[which])
        for k, v in sd_p[which].items():
            w = sd_q[which][k]
            assert torch.equal(v.view(torch.int32), w.view(torch.int32)) if v.dtype == torch.float32 else torch.equal(v, w), (which, k)
    assert any(not torch.equal(sd_a["dis"][k], sd_p["dis"][k]) for k in sd_p["dis"] if sd_p["dis"][k].is_floating_point())
