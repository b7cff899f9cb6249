"""GPU: one generator step and one discriminator step of train_generator.py:279-360 on the HIP
path (module-level autograd Functions with hand-written backward plans) against torch autograd
over the oracle on the CPU: loss values and EVERY parameter gradient."""
from argparse import Namespace

import pytest
import torch
import torch.nn.functional as F

from conftest import diag_path
from oracle import hrviton_oracle as O

pytestmark = pytest.mark.gpu


def _rel(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-12)).item()


def _setup(seed=0, H=256, W=128, N=2, wmul=25.0):
    import hr_viton_amd  # noqa: F401
    from hr_viton_amd.network_generator import MultiscaleDiscriminator, SPADEGenerator
    opt = Namespace(cuda=True, norm_G="spectralaliasinstance", gen_semantic_nc=7, ngf=8, num_upsampling_layers="most",
                    fine_height=H, fine_width=W, ndf=8, norm_D="spectralinstance", n_layers_D=3, num_D=2,
                    no_ganFeat_loss=False)
    torch.manual_seed(seed)
    gen = SPADEGenerator(opt, 9)
    gen.init_weights("xavier", 0.02)
    D = MultiscaleDiscriminator(opt)
    D.init_weights("xavier", 0.02)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for n_, p in list(gen.named_parameters()) + list(D.named_parameters()):
            if n_.endswith("noise_scale"):
                p.copy_(0.2 * torch.randn(p.shape, generator=g))
            elif n_.endswith("weight") or n_.endswith("weight_orig"):
                p.mul_(wmul)
            elif n_.endswith("bias"):
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
    x = torch.rand(N, 9, H, W, generator=g) * 2 - 1
    lab = torch.randint(0, 7, (N, 1, H // 16, W // 16), generator=g).repeat_interleave(16, 2).repeat_interleave(16, 3)
    seg = torch.zeros(N, 7, H, W).scatter_(1, lab, 1.0)
    real = torch.rand(N, 3, H, W, generator=g) * 2 - 1
    noise = {}
    for j, name in enumerate(gen._blocks()):
        h, w = gen.sh << j, gen.sw << j
        k = 3 if getattr(gen, name).learned_shortcut else 2
        noise[name] = [torch.randn(N, w, h, 1, generator=g) for _ in range(k)]
    return opt, gen, D, x, seg, real, noise


def _oracle_sd(mod):
    return {k: v.detach().clone().requires_grad_(v.dtype.is_floating_point and not k.endswith(("weight_u", "weight_v")))
            for k, v in mod.state_dict().items()}


def _compare_grads(mod, sd, tol, what):
    """Per-parameter max-abs error relative to max(|oracle grad| of that parameter, 1e-3 x the largest
    gradient magnitude of the whole module): gradients that are analytically ~0 (a bias in front of an
    InstanceNorm) are pure round-off on both sides and are held to the module-level scale."""
    import os
    rows = []
    gmax = max((sd[n].grad.abs().max().item() for n, _ in mod.named_parameters() if sd[n].grad is not None), default=1.0)
    for name, p in mod.named_parameters():
        want = sd[name].grad
        if want is None:
            assert p.grad is None or p.grad.abs().max() == 0, f"{what}: {name} has a gradient but the oracle has none"
            continue
        assert p.grad is not None, f"{what}: {name} got no gradient"
        aerr = (p.grad.detach().cpu() - want).abs().max().item()
        rows.append((aerr / max(want.abs().max().item(), 1e-3 * gmax), aerr, want.abs().max().item(), name))
    rows.sort(reverse=True)
    with open(diag_path("grad_diag_" + what.split()[0] + ".txt"), "w") as f:
        f.write(f"# {what}: rel_err abs_err |want|max name   (global max grad {gmax:.3e})\n")
        for r in rows:
            f.write("%.3e %.3e %.3e %s\n" % r)
    assert rows[0][0] < tol, f"{what}: worst gradient mismatch {rows[:5]}"


def test_generator_step_matches_oracle_autograd():
    import hr_viton_amd  # noqa: F401
    from hr_viton_amd.losses import GANLoss, L1Loss
    opt, gen, D, x, seg, real, noise = _setup()
    sd_g, sd_d = _oracle_sd(gen), _oracle_sd(D)
    # ---------------- oracle: train_generator.py:279-314 (no VGG term here) ----------------
    O.SN_TRAIN["on"], O.SN_TRAIN["uv"] = True, {}
    try:
        fake = O.spade_generator_forward(sd_g, x, seg, opt.fine_height, opt.fine_width, "most", noise=noise)
        pred = O.gen_discriminator_forward(sd_d, torch.cat([torch.cat([seg, fake], 1), torch.cat([seg, real], 1)], 0))
    finally:
        O.SN_TRAIN["on"] = False
    pf, pr = O.split_fake_real(pred)
    l_gan = O.hinge_loss(pf, True, False)
    l_feat = O.feat_match_loss(pf, pr, 10.0)
    (l_gan + l_feat).backward()
    # ---------------- HIP ----------------
    gen.cuda().train()
    D.cuda().train()
    crit_gan, crit_feat = GANLoss("hinge"), L1Loss()
    xc, sc, rc = x.cuda(), seg.cuda(), real.cuda()
    out = gen(xc, sc, noise=noise)
    assert _rel(out, fake) < 2e-4
    pred_h = D(torch.cat([torch.cat([sc, out], 1), torch.cat([sc, rc], 1)], 0))
    pf_h = [[t[: t.size(0) // 2] for t in p] for p in pred_h]
    pr_h = [[t[t.size(0) // 2:] for t in p] for p in pred_h]
    g_gan = crit_gan(pf_h, True, for_discriminator=False)
    g_feat = 0
    for i in range(2):
        for j in range(len(pf_h[i]) - 1):
            g_feat = g_feat + crit_feat(pf_h[i][j], pr_h[i][j].detach()) * 10.0 / 2
    assert abs(g_gan.item() - l_gan.item()) < 1e-4 * max(1.0, abs(l_gan.item()))
    assert abs(g_feat.item() - l_feat.item()) < 1e-4 * max(1.0, abs(l_feat.item()))
    (g_gan + g_feat).mean().backward()
    _compare_grads(gen, sd_g, 1e-2, "generator")   # sign() of the L1 feature-matching term amplifies round-off
    _compare_grads(D, sd_d, 1e-2, "discriminator (through the G loss)")
    # the power iteration updated the spectral-norm buffers like the reference does
    u_w, v_w = O.SN_TRAIN["uv"]["up_0.conv_0"]
    assert _rel(gen.up_0.conv_0.weight_u, u_w) < 1e-4 and _rel(gen.up_0.conv_0.weight_v, v_w) < 1e-4


def test_discriminator_step_matches_oracle_autograd():
    import hr_viton_amd  # noqa: F401
    from hr_viton_amd.losses import GANLoss
    opt, gen, D, x, seg, real, noise = _setup(seed=3)
    sd_d = _oracle_sd(D)
    g = torch.Generator().manual_seed(9)
    fake = torch.rand(real.shape, generator=g) * 2 - 1          # stands for the no_grad generator output (:327-330)
    inp = torch.cat([torch.cat([seg, fake], 1), torch.cat([seg, real], 1)], 0)
    O.SN_TRAIN["on"], O.SN_TRAIN["uv"] = True, {}
    try:
        pred = O.gen_discriminator_forward(sd_d, inp)
    finally:
        O.SN_TRAIN["on"] = False
    pf, pr = O.split_fake_real(pred)
    l_d = O.hinge_loss(pf, False, True) + O.hinge_loss(pr, True, True)
    l_d.backward()
    D.cuda().train()
    crit = GANLoss("hinge")
    pred_h = D(inp.cuda())
    pf_h = [[t[: t.size(0) // 2] for t in p] for p in pred_h]
    pr_h = [[t[t.size(0) // 2:] for t in p] for p in pred_h]
    loss = crit(pf_h, False, for_discriminator=True) + crit(pr_h, True, for_discriminator=True)
    assert abs(loss.item() - l_d.item()) < 1e-4 * max(1.0, abs(l_d.item()))
    loss.mean().backward()
    _compare_grads(D, sd_d, 1e-4, "discriminator step")


def test_vgg_loss_value_and_input_gradient():
    """VGGLoss (networks.py:235-251) forward + backward through x vs autograd over the oracle."""
    import hr_viton_amd  # noqa: F401
    from hr_viton_amd.vgg import VGGLoss
    torch.manual_seed(2)
    crit = VGGLoss(Namespace(cuda=False))
    sd = {k: v.detach().clone() for k, v in crit.vgg.state_dict().items()}
    g = torch.Generator().manual_seed(3)
    x = (torch.rand(2, 3, 64, 48, generator=g) * 2 - 1).requires_grad_()
    y = torch.rand(2, 3, 64, 48, generator=g) * 2 - 1
    want = O.vgg_loss(sd, x, y)
    (want * 10.0).backward()
    crit.cuda()
    xc = x.detach().cuda().requires_grad_()
    got = crit(xc, y.cuda())
    assert abs(got.item() - want.item()) < 1e-5 * max(1.0, abs(want.item()))
    (got * 10.0).backward()
    err = (xc.grad.cpu() - x.grad).abs().max().item() / x.grad.abs().max().item()
    assert err < 2e-2, err      # sign() gradients of the L1 terms flip on round-off-level differences
    feats = crit.vgg(y.cuda())
    for a, b in zip(feats, O.vgg19_features(sd, y)):
        assert _rel(a, b) < 1e-4


def test_mixed_precision_vgg_loss_batches_x_and_y_bit_identically(monkeypatch):
    """Mixed precision with a fresh target: x and y run through VGG19 as ONE batch of 2 N (13 launches instead of 26), the
    backward over the x half.  Per-image convolutions, pools and taps are independent of the batch they sit in, so loss and
    input gradient are bit-identical to the two separate passes (HRV_VGG_BATCH=0) -- and within the bf16 tolerance of the oracle."""
    import hr_viton_amd  # noqa: F401
    from hr_viton_amd import train_ops as T
    from hr_viton_amd.vgg import VGGLoss
    torch.manual_seed(2)
    crit = VGGLoss(Namespace(cuda=False))
    sd = {k: v.detach().clone() for k, v in crit.vgg.state_dict().items()}
    g = torch.Generator().manual_seed(3)
    # 192 x 192: every VGG level picks the SAME kernel for 2 images (the separate passes) and for 4 (the batch) -- 288 / 576 tiles of
    # 16 x 16 pixels at full resolution (conv_p2.hip from 192 tiles up), 72 / 144 and fewer below it (the generic tiles).  At a size
    # where doubling the batch crosses that threshold the two forms run different kernels on one level and agree to reassociation only
    x = (torch.rand(2, 3, 192, 192, generator=g) * 2 - 1).requires_grad_()
    y = torch.rand(2, 3, 192, 192, generator=g) * 2 - 1
    want = O.vgg_loss(sd, x, y)
    want.backward()
    crit.cuda()
    T.MMA_BF16[0] = True
    try:
        res = {}
        for flag in ("1", "0"):
            monkeypatch.setenv("HRV_VGG_BATCH", flag)
            crit.vgg._ycache = None
            xc = x.detach().cuda().requires_grad_()
            got = crit(xc, y.cuda().clone())
            got.backward()
            torch.cuda.synchronize()
            res[flag] = (got.detach().clone(), xc.grad.clone())
        assert torch.equal(res["1"][0], res["0"][0]) and torch.equal(res["1"][1], res["0"][1])
        assert abs(res["1"][0].item() - want.item()) < 2e-3 * max(1.0, abs(want.item()))
        cos = F.cosine_similarity(res["1"][1].cpu().flatten(), x.grad.flatten(), dim=0).item()
        assert cos > 0.99, cos
    finally:
        T.MMA_BF16[0] = False


def test_train_generator_script_small_run(tmp_path):
    """The drop-in train_generator.py loop (frozen tocg -> glue -> G step -> D step -> fused Adam) for a few
    steps on a small configuration: finite losses, parameters move, checkpoints are written and reload."""
    import sys
    sys.path.insert(0, str(tmp_path))
    import train_generator as tg
    argv = ["--name", "t", "--synthetic", "-b", "2", "--fine_height", "512", "--fine_width", "384", "--ngf", "8", "--ndf", "8",
            "--tocg_ngf", "16", "--max_steps", "3", "--display_count", "1", "--save_count", "3",
            "--checkpoint_dir", str(tmp_path), "--occlusion"]
    tg.main(argv)
    import hr_viton_amd  # noqa: F401
    from hr_viton_amd.network_generator import SPADEGenerator
    sd = torch.load(str(tmp_path / "t" / "gen_step_000003.pth"), map_location="cpu")
    opt = tg.get_opt(argv)
    torch.manual_seed(0)
    g0 = SPADEGenerator(opt, 9)
    g0.load_state_dict(sd, strict=True)
    assert all(torch.isfinite(v).all() for v in sd.values() if v.is_floating_point())
    fresh = SPADEGenerator(opt, 9)
    fresh.init_weights("xavier", 0.02)
    moved = sum(float((sd[k] - v).abs().max()) > 0 for k, v in fresh.state_dict().items() if k.endswith("conv_0.weight_orig"))
    assert moved > 0


def test_mixed_precision_generator_step_against_the_oracle():
    """--fp16 (train_ops.MMA_BF16): the generator half of one training iteration on the bf16 matrix cores against torch
    autograd over the ORACLE (oracle.step_check.compare_generator_step, the comparison tests/test_gpu_fullsize.py and
    bench.py's parity block run at 512x384 / 2x1024x768) -- not against this package's own fp32 engine, which the same
    call holds to the north-star tolerance.  256x128, ngf = 16: image, every loss term, every sizeable parameter gradient's
    cosine, within the stated bf16 tolerance (operands carry 8 mantissa bits)."""
    import os
    from oracle import step_check
    rep = step_check.compare_generator_step(256, 128, 16, 16, 2, seed=5, mixed=(False, True), cpu_threads=min(os.cpu_count() or 1, 16),
                                            table_path=diag_path("grad_parity_gen_256x128_ngf16.txt"))
    with open(diag_path("step_parity_gen_256x128_ngf16.txt"), "w") as f:
        f.write(repr(rep) + "\n")
    f32, b16 = rep[False], rep[True]
    assert f32["image_max_rel_err"] < 1e-3 and all(v < 1e-3 for v in f32["loss_rel_err"].values()) and f32["grad_worst_rel_err"] < 2e-2, f32
    # stated bf16 tolerance (operands carry 8 mantissa bits), at about twice what this small, noisy configuration measures
    # -- image mean-abs 3.1e-3 / max 5.9e-2 of the range, loss terms <= 2.0e-4, median gradient error 1.9e-2, worst cosine
    # 0.883 (head_0.conv_1, 24 convolutions below the loss: sign() of the L1 feature-matching term turns operand rounding
    # into flipped gradient elements, and a 16-channel level averages few of them); the bench resolution holds 1.1e-3 /
    # 0.998 against 3e-3 / 0.99 (tests/test_gpu_fullsize.py)
    assert b16["image_mean_abs_err"] < 6e-3 and b16["image_max_rel_err"] < 0.12, b16
    assert all(v < 2e-3 for v in b16["loss_rel_err"].values()), b16
    assert b16["grad_min_cosine"] > 0.85 and b16["grad_median_rel_err"] < 0.04, b16
    assert b16["image_mean_abs_err"] > 1e-7          # the bf16 path really ran



def test_split_discriminator_path_equals_sliced_path():
    """D(x, split=True) (zero-copy fake / real halves, half-batch backward when only the fake half carries a
    gradient) against the reference-style `pred = D(x); pred_fake = t[:N]` composition: same losses, same
    generator gradients, same discriminator gradients in the D step."""
    import hr_viton_amd  # noqa: F401
    from hr_viton_amd.losses import GANLoss, L1Loss

    def run(split):
        opt, gen, D, x, seg, real, noise = _setup(seed=5)
        gen.cuda().train()
        D.cuda().train()
        segc, realc = seg.cuda(), real.cuda()
        fake = gen(x.cuda(), segc, noise=noise)
        both = torch.cat([torch.cat([segc, fake], 1), torch.cat([segc, realc], 1)], 0)
        if split:
            pf, pr = D(both, split=True)
        else:
            pred = D(both)
            pf = [[t[: t.size(0) // 2] for t in p] for p in pred]
            pr = [[t[t.size(0) // 2:] for t in p] for p in pred]
        l = GANLoss("hinge")(pf, True, for_discriminator=False)
        for i in range(2):
            for j in range(len(pf[i]) - 1):
                l = l + L1Loss()(pf[i][j], pr[i][j].detach()) * 10.0 / 2
        l.mean().backward()
        gg = {n: p.grad.detach().cpu().clone() for n, p in gen.named_parameters() if p.grad is not None}
        for p in D.parameters():
            p.grad = None
        # discriminator step on detached images: both halves carry a (hinge) gradient
        both_d = both.detach()
        if split:
            pf, pr = D(both_d, split=True)
        else:
            pred = D(both_d)
            pf = [[t[: t.size(0) // 2] for t in p] for p in pred]
            pr = [[t[t.size(0) // 2:] for t in p] for p in pred]
        ld = GANLoss("hinge")(pf, False, for_discriminator=True) + GANLoss("hinge")(pr, True, for_discriminator=True)
        ld.mean().backward()
        gd = {n: p.grad.detach().cpu().clone() for n, p in D.named_parameters() if p.grad is not None}
        return float(l.mean()), float(ld.mean()), gg, gd

    l0, d0, gg0, gd0 = run(False)
    l1, d1, gg1, gd1 = run(True)
    assert abs(l0 - l1) < 1e-5 * max(1.0, abs(l0)) and abs(d0 - d1) < 1e-5 * max(1.0, abs(d0))
    gm = max(v.abs().max().item() for v in gg0.values())
    for n in gg0:
        assert (gg0[n] - gg1[n]).abs().max() <= 1e-4 * max(gg0[n].abs().max().item(), 1e-3 * gm), n
    dm = max(v.abs().max().item() for v in gd0.values())
    for n in gd0:
        assert (gd0[n] - gd1[n]).abs().max() <= 1e-4 * max(gd0[n].abs().max().item(), 1e-3 * dm), n


def test_second_generator_iteration_on_the_flat_gradient_path():
    """pipeline.generator_train_step twice: in the second iteration every generator / discriminator gradient is
    produced directly in its slot of the fused Adam's flat buffer (spectral-norm dW_orig, SPADE gamma/beta slices,
    fused bias columns).  The oracle is synchronised to the HIP weights (incl. the power-iterated u, v) before that
    iteration and fed the same SPADE noise; compared: the generator-step losses and every generator gradient."""
    import hr_viton_amd  # noqa: F401
    from hr_viton_amd import gen_train, ops, pipeline
    from hr_viton_amd.losses import GANLoss, L1Loss
    from hr_viton_amd.optim import Adam
    opt, gen, D, x, seg, real, noise = _setup(seed=9, wmul=8.0)
    opt.lambda_feat, opt.lambda_vgg, opt.no_vgg_loss = 10.0, 10.0, True
    gen.cuda().train()
    D.cuda().train()
    og = Adam(gen.parameters(), lr=1e-4, betas=(0.0, 0.9))
    od = Adam(D.parameters(), lr=4e-4, betas=(0.0, 0.9))
    xc, realc = x.cuda(), real.cuda()
    parse7 = ops.to_nhwc(seg.cuda())
    blocks = list(noise.keys())
    real_randn = torch.randn
    fed = {}

    def feed_randn(*size, **kw):
        # SPADENorm noise draws (network_generator.py:104-107; one flat draw per generator forward, gen_train.noise_planes):
        # recorded so the oracle can replay them
        if len(size) == 1 and size[0] == gen_train.noise_elems(gen, x.shape[0]):
            z = real_randn(*size, **kw)
            fed.setdefault("z", []).append(z.detach().cpu())
            return z
        return real_randn(*size, **kw)

    cap = {}
    for it in range(2):
        fed.clear()
        # the weights (and u, v) this iteration starts from, on the CPU for the oracle
        sd_g, sd_d = ({k: v.detach().cpu().clone().requires_grad_(v.dtype.is_floating_point and not k.endswith(("weight_u", "weight_v")))
                       for k, v in m.state_dict().items()} for m in (gen, D))
        real_step = og.step

        def capture():
            cap.clear()
            cap.update({n: p.grad.detach().cpu().clone() for n, p in gen.named_parameters() if p.grad is not None})
            return real_step()

        og.step = capture
        torch.randn = feed_randn
        try:
            losses, _ = pipeline.generator_train_step(opt, gen, D, GANLoss("hinge"), L1Loss(), None, og, od, xc, parse7, realc)
        finally:
            torch.randn = real_randn
            og.step = real_step
    # oracle replay of the SECOND iteration's generator step
    assert len(fed["z"]) == 2 and list(blocks) == list(gen._blocks())   # (G-step forward, D-step no-grad forward)
    onoise = gen_train.noise_planes(gen, x.shape[0], fed["z"][0])       # the first draw belongs to the G-step forward
    O.SN_TRAIN["on"], O.SN_TRAIN["uv"] = True, {}
    try:
        fake = O.spade_generator_forward(sd_g, x, seg, opt.fine_height, opt.fine_width, "most", noise=onoise)
        pred = O.gen_discriminator_forward(sd_d, torch.cat([torch.cat([seg, fake], 1), torch.cat([seg, real], 1)], 0))
    finally:
        O.SN_TRAIN["on"] = False
    pf, pr = O.split_fake_real(pred)
    l_gan, l_feat = O.hinge_loss(pf, True, False), O.feat_match_loss(pf, pr, 10.0)
    (l_gan + l_feat).backward()
    assert abs(float(losses["GAN"]) - l_gan.item()) < 2e-4 * max(1.0, abs(l_gan.item()))
    assert abs(float(losses["GAN_Feat"]) - l_feat.item()) < 2e-4 * max(1.0, abs(l_feat.item()))
    p0 = gen.up_4.conv_0.weight_orig
    assert p0.grad is None or p0.grad.data_ptr() == p0._hrv_flat_grad.data_ptr()
    gmax = max(v.grad.abs().max().item() for v in sd_g.values() if v.grad is not None)
    rows = []
    for n, p in gen.named_parameters():
        w = sd_g[n].grad
        if w is None:
            continue
        rows.append(((cap[n] - w).abs().max().item() / max(w.abs().max().item(), 1e-3 * gmax), n))
    rows.sort(reverse=True)
    assert rows[0][0] < 1e-2, rows[:5]


@pytest.mark.parametrize("mixed", [False, True], ids=["fp32", "bf16"])
def test_batched_weight_packs_leave_the_iteration_bit_identical(mixed):
    """T.PackBatch: from the third iteration on every recorded weight pack of a plan comes from ONE
    hrv_conv2d_pack_weight_multi launch at the top of its forward.  Four iterations (same inputs, same injected SPADE
    noise) with and without batching end in bit-identical generator and discriminator weights, and the batched run did
    serve its convolutions from the batch (records exist, the multi launch ran once per plan forward).  Four iterations:
    the first records packs of parameters that the fused optimizer then MOVES (flat buffers) -- those records are dropped."""
    import hr_viton_amd  # noqa: F401
    from hr_viton_amd import gen_train, ops, pipeline
    from hr_viton_amd import train_ops as T
    from hr_viton_amd.losses import GANLoss, L1Loss
    from hr_viton_amd.optim import Adam

    def run(batching):
        opt, gen, D, x, seg, real, noise = _setup(seed=4, wmul=8.0)
        opt.lambda_feat, opt.lambda_vgg, opt.no_vgg_loss = 10.0, 10.0, True
        gen.cuda().train()
        D.cuda().train()
        og = Adam(gen.parameters(), lr=1e-3, betas=(0.0, 0.9))
        od = Adam(D.parameters(), lr=4e-3, betas=(0.0, 0.9))
        xc, realc, parse7 = x.cuda(), real.cuda(), ops.to_nhwc(seg.cuda())
        g = torch.Generator().manual_seed(77)
        old, oldm = T.PACK_BATCHING[0], T.MMA_BF16[0]
        T.PACK_BATCHING[0], T.MMA_BF16[0] = batching, mixed
        try:
            counts = []
            for _ in range(4):
                nz = [gen_train.noise_planes(gen, x.shape[0], torch.randn(gen_train.noise_elems(gen, x.shape[0]), generator=g))
                      for _ in range(2)]
                pipeline.generator_train_step(opt, gen, D, GANLoss("hinge"), L1Loss(), None, og, od, xc, parse7, realc,
                                              noise=nz[0], noise_d=nz[1])
                counts.append(tuple(len(p._pack_batch.bufs) for p in (gen._train_plan, D._train_plan)
                                    if getattr(p, "_pack_batch", None) is not None))
            # the fused optimizers move every parameter into their flat buffers at their first step: the records made
            # before that are dropped (they hold addresses of freed storages), and the set is stable afterwards
            assert counts[2] == counts[3], counts
        finally:
            T.PACK_BATCHING[0], T.MMA_BF16[0] = old, oldm
        torch.cuda.synchronize()
        sd = {"G." + k: v.detach().cpu().clone() for k, v in gen.state_dict().items()}
        sd.update({"D." + k: v.detach().cpu().clone() for k, v in D.state_dict().items()})
        stats = [(len(p._pack_batch.bufs), p._pack_batch.launches) for p in (gen._train_plan, D._train_plan)
                 if getattr(p, "_pack_batch", None) is not None]
        return sd, stats

    a, sa = run(True)
    b, sb = run(False)
    assert len(sa) == 2 and all(n > 4 and launches >= 5 for n, launches in sa), sa       # from the third iteration on
    assert all(n == 0 for n, _ in sb), sb
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("which", ["generator_step", "discriminator_step"])
def test_discriminator_pair_form_equals_the_concatenated_batch_form(which):
    """MultiscaleDiscriminator.forward_pair(parse, fake, real) -- the PatchGAN input of train_generator.py:283-295 assembled
    NHWC by hrv_concat_nhwc_nchw_f32 -- against discriminator(cat((cat((parse, fake), 1), cat((parse, real), 1)), 0),
    split=True) on the same weights and spectral-norm state: every output bit-identical, d(fake) and (discriminator
    step) every parameter gradient equal."""
    import copy
    import hr_viton_amd  # noqa: F401
    from hr_viton_amd import ops
    from hr_viton_amd.losses import GANLoss, L1Loss
    opt, gen, D, x, seg, real, noise = _setup(seed=21, H=128, W=96, wmul=6.0)
    D.cuda().train()
    D2 = copy.deepcopy(D)
    g = torch.Generator().manual_seed(5)
    fake = (torch.rand(2, 3, 128, 96, generator=g) * 2 - 1).cuda()
    realc, parse7 = real.cuda(), ops.to_nhwc(seg.cuda())
    cg, cf = GANLoss("hinge"), L1Loss()

    def losses(pf, pr):
        if which == "generator_step":
            tot = cg(pf, True, for_discriminator=False)
            for i in range(len(pf)):
                for j in range(len(pf[i]) - 1):
                    tot = tot + cf(pf[i][j], pr[i][j].detach()) * 10.0 / len(pf)
            return tot
        return cg(pf, False, for_discriminator=True) + cg(pr, True, for_discriminator=True)

    fa = fake.clone().requires_grad_(which == "generator_step")
    pf_a, pr_a = D.forward_pair(parse7, fa, realc)
    la = losses(pf_a, pr_a)
    la.sum().backward()
    fb = fake.clone().requires_grad_(which == "generator_step")
    pn = ops.to_nchw(parse7)
    pf_b, pr_b = D2(torch.cat((torch.cat((pn, fb), 1), torch.cat((pn, realc), 1)), 0), split=True)
    lb = losses(pf_b, pr_b)
    lb.sum().backward()
    for u, v in zip([t for s_ in pf_a + pr_a for t in s_], [t for s_ in pf_b + pr_b for t in s_]):
        assert torch.equal(u, v)
    assert torch.equal(la, lb)
    if which == "generator_step":
        assert torch.equal(fa.grad, fb.grad)
    else:
        for (n, p), (_, q) in zip(D.named_parameters(), D2.named_parameters()):
            assert (p.grad is None) == (q.grad is None), n
            if p.grad is not None:
                assert torch.equal(p.grad, q.grad), n


def test_graphed_training_iteration_is_bit_identical_to_eager():
    """graph.GraphedTrainStep: one train_generator.py iteration (G step, D step, VGG + feature-matching + hinge losses, both
    fused Adam updates with step count and learning rate on the device) captured as ONE hipGraph.  Three eager warm-up
    iterations + two replays end in bit-identical generator / discriminator weights, optimizer moments and step counts as
    five eager iterations from the same start -- including a learning-rate change between the replays (the scheduler's
    value reaches the captured iteration through push_lr) and the VGG target features (recomputed inside the graph)."""
    import hr_viton_amd  # noqa: F401
    from hr_viton_amd import gen_train, ops, pipeline
    from hr_viton_amd.graph import GraphedTrainStep
    from hr_viton_amd.losses import GANLoss, L1Loss
    from hr_viton_amd.optim import Adam
    from hr_viton_amd.vgg import VGGLoss

    def build():
        opt, gen, D, x, seg, real, noise = _setup(seed=31, wmul=6.0)          # 2 x 256 x 128
        opt.lambda_feat, opt.lambda_vgg, opt.no_vgg_loss = 10.0, 10.0, False
        gen.cuda().train()
        D.cuda().train()
        torch.manual_seed(77)
        vgg = VGGLoss(opt).cuda()
        og = Adam(gen.parameters(), lr=1e-3, betas=(0.0, 0.9), device_step=True)
        od = Adam(D.parameters(), lr=2e-3, betas=(0.0, 0.9), device_step=True)
        g = torch.Generator().manual_seed(5)
        n_el = gen_train.noise_elems(gen, x.shape[0])
        nz = [gen_train.noise_planes(gen, x.shape[0], torch.randn(n_el, generator=g).cuda()) for _ in range(2)]
        inputs = {"x": x.cuda(), "parse7": ops.to_nhwc(seg.cuda()).t, "im": real.cuda()}
        return opt, gen, D, vgg, og, od, inputs, nz

    def lr_at(it, o, base):
        for grp in o.param_groups:
            grp["lr"] = base * (0.5 if it >= 4 else 1.0)

    def snapshot(gen, D, og, od):
        torch.cuda.synchronize()
        sd = {"G." + k: v.detach().cpu().clone() for k, v in gen.state_dict().items()}
        sd.update({"D." + k: v.detach().cpu().clone() for k, v in D.state_dict().items()})
        for tag, o in (("og", og), ("od", od)):
            st = o._flat[0]
            sd[tag + ".m"], sd[tag + ".v"] = st["m"].detach().cpu().clone(), st["v"].detach().cpu().clone()
            sd[tag + ".step"] = st["step_dev"].detach().cpu().clone()
        return sd

    # ---- eager: five iterations
    opt, gen, D, vgg, og, od, inputs, nz = build()
    cg, cf = GANLoss("hinge"), L1Loss()
    for it in range(5):
        lr_at(it, og, 1e-3)
        lr_at(it, od, 2e-3)
        losses_e, _ = pipeline.generator_train_step(opt, gen, D, cg, cf, vgg, og, od, inputs["x"], ops.Act(inputs["parse7"], 7),
                                                    inputs["im"], noise=nz[0], noise_d=nz[1])
    want = snapshot(gen, D, og, od)
    want_losses = {k: float(v) for k, v in losses_e.items()}
    # ---- graph: three eager warm-up iterations inside the constructor, then two replays
    opt, gen, D, vgg, og, od, inputs, nz = build()
    gs = GraphedTrainStep(opt, gen, D, GANLoss("hinge"), L1Loss(), vgg, og, od, inputs, noise=nz[0], noise_d=nz[1], warmup=3)
    for it in (3, 4):
        lr_at(it, og, 1e-3)
        lr_at(it, od, 2e-3)
        losses_g, _ = gs(inputs)
        if it == 3:
            # an eager call that outgrows the shared split-K / weight-gradient workspace replaces the tensor; the graph
            # recorded the old address and must keep that memory to itself (graph.CaptureGuard) -- poison what a freed
            # workspace would have been recycled into
            dev = (str(inputs["x"].device), torch.cuda.current_stream().cuda_stream)      # (one scratch per device and stream)
            old = ops._WS[dev]
            new = ops._workspace(inputs["x"].device, 2 * old.numel() * 4 + 4096)
            assert new.data_ptr() != old.data_ptr() and any(t.data_ptr() == old.data_ptr() for t in gs._it.guard.keep)
            n_old = old.numel()
            del old
            new.fill_(float("nan"))
            junk = [torch.full((n_old,), float("nan"), device="cuda") for _ in range(3)]      # noqa: F841
    got = snapshot(gen, D, og, od)
    assert gs.replays == 2 and int(got["og.step"]) == 5 and int(got["od.step"]) == 5
    for k in want:
        assert torch.equal(want[k], got[k]), k
    for k, v in want_losses.items():
        assert float(losses_g[k]) == v, (k, float(losses_g[k]), v)
    assert int(og.state_dict()["state"][0]["step"]) == 5
    # a weight-pack batch of the captured plan dropping its buffers (a weight moved) makes the graph stale: loud, not silent
    from hr_viton_amd.ops import HrvError
    assert gs._it.guard.watch, "the captured iteration ran batched weight packs"
    gs._it.guard.watch[0][0]().reset()
    with pytest.raises(HrvError):
        gs(inputs)


@pytest.mark.parametrize("no_feat", [False, True])
def test_standalone_nlayer_discriminator_in_training_mode_equals_scale_0_of_the_multiscale_one(no_feat):
    """NLayerDiscriminator.forward called on its own in training mode (network_generator.py:278-289): the same plan, kernels and
    autograd Function as scale 0 of MultiscaleDiscriminator.forward -- features, d(input) and every parameter gradient
    bit-identical to the multi-scale run on a copy with the same weights and spectral-norm state (that path is held to the
    oracle by test_discriminator_step_matches_oracle_autograd)."""
    import copy
    import hr_viton_amd  # noqa: F401
    opt, gen, D, x, seg, real, noise = _setup(seed=33, H=128, W=96, wmul=6.0)
    D.no_ganFeat_loss = no_feat
    for d_ in D.children():
        d_.no_ganFeat_loss = no_feat
    D.cuda().train()
    D2 = copy.deepcopy(D)
    solo = D2.discriminator_0
    g = torch.Generator().manual_seed(9)
    inp = torch.cat((seg, torch.rand(2, 3, 128, 96, generator=g) * 2 - 1), 1).cuda()
    ia = inp.clone().requires_grad_(True)
    fa = D(ia)[0]                                   # scale 0 of the multi-scale forward: list of layer features (or [last])
    sum((f * f).mean() for f in fa).backward()
    ib = inp.clone().requires_grad_(True)
    fb = solo(ib)
    fb = [fb] if no_feat else fb
    assert len(fa) == len(fb) == (1 if no_feat else 4)
    sum((f * f).mean() for f in fb).backward()
    for u, v in zip(fa, fb):
        assert torch.equal(u, v)
    pa, pb = dict(D.discriminator_0.named_parameters()), dict(solo.named_parameters())
    for n in pa:
        assert pa[n].grad is not None and pb[n].grad is not None, n
        assert torch.equal(pa[n].grad, pb[n].grad), n
    # (d(input) of the multi-scale run also holds scale 1's share: none here -- the loss reads scale 0 only -- but its
    #  avg-pool backward still runs on a zero gradient, so compare values, not bits)
    assert torch.allclose(ia.grad, ib.grad, rtol=0, atol=0)
    # the spectral-norm state advanced alike
    for (n, a), (_, b) in zip(D.discriminator_0.named_buffers(), solo.named_buffers()):
        assert torch.equal(a, b), n


def test_weight_gradients_on_the_side_stream_leave_the_iteration_bit_identical(monkeypatch):
    """train_ops.wgrad_side (opt-in, HRV_WGRAD_SIDE=1): the weight gradients of every level run on a second stream next to the
    data-gradient chain -- forked per leaf, joined at the end of each backward Function and in front of the fused optimizer step.
    Same kernels on the same operands: four mixed-precision iterations end in bit-identical generator / discriminator weights
    and Adam moments with and without it (a missing fork / join / record_stream shows up here as a difference)."""
    import hr_viton_amd  # noqa: F401
    from hr_viton_amd import gen_train, ops, pipeline
    from hr_viton_amd import train_ops as T
    from hr_viton_amd.losses import GANLoss, L1Loss
    from hr_viton_amd.optim import Adam

    def run(side):
        monkeypatch.setenv("HRV_WGRAD_SIDE", "1" if side else "0")
        monkeypatch.setenv("HRV_WGRAD_SIDE_MAXPIX", "1000000000")
        opt, gen, D, x, seg, real, noise = _setup(seed=4, wmul=8.0)
        opt.lambda_feat, opt.lambda_vgg, opt.no_vgg_loss = 10.0, 10.0, True
        gen.cuda().train()
        D.cuda().train()
        og = Adam(gen.parameters(), lr=1e-3, betas=(0.0, 0.9))
        od = Adam(D.parameters(), lr=4e-3, betas=(0.0, 0.9))
        xc, realc, parse7 = x.cuda(), real.cuda(), ops.to_nhwc(seg.cuda())
        g = torch.Generator().manual_seed(77)
        oldm = T.MMA_BF16[0]
        T.MMA_BF16[0] = True
        forks0 = sum(1 for v in T._Side.pending.values())
        try:
            for _ in range(4):
                nz = [gen_train.noise_planes(gen, x.shape[0], torch.randn(gen_train.noise_elems(gen, x.shape[0]), generator=g))
                      for _ in range(2)]
                pipeline.generator_train_step(opt, gen, D, GANLoss("hinge"), L1Loss(), None, og, od, xc, parse7, realc,
                                              noise=nz[0], noise_d=nz[1])
        finally:
            T.MMA_BF16[0] = oldm
        torch.cuda.synchronize()
        sd = {"G." + k: v.detach().cpu().clone() for k, v in gen.state_dict().items()}
        sd.update({"D." + k: v.detach().cpu().clone() for k, v in D.state_dict().items()})
        for tag, o in (("og", og), ("od", od)):
            sd[tag + ".m"], sd[tag + ".v"] = o._flat[0]["m"].detach().cpu().clone(), o._flat[0]["v"].detach().cpu().clone()
        return sd, forks0

    a, _ = run(False)
    b, _ = run(True)
    assert T._Side.streams, "the side stream was never used"
    assert not any(T._Side.pending.values()), "a backward left weight gradients un-joined"
    for k in a:
        assert torch.equal(a[k], b[k]), k
