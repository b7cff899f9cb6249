"""GPU: training path of the condition generator (train_condition.py:113-286) on the HIP kernels --
kernel-level adjoints against torch autograd on the CPU, then one full tocg + D iteration (losses,
EVERY parameter gradient, BatchNorm running statistics, Adam update) against the oracle, which
tests/test_oracle_golden.py pins to the real reference's step."""
from argparse import Namespace

import os

import pytest
import torch
import torch.nn.functional as F

from conftest import diag_path
from oracle import hrviton_oracle as O

pytestmark = pytest.mark.gpu


def _close(name, got, want, tol):
    got, want = got.detach().float().cpu(), want.detach().float().cpu()
    assert got.shape == want.shape, (name, got.shape, want.shape)
    err = (got - want).abs().max().item()
    ref = want.abs().max().item()
    assert err <= tol * max(ref, 1e-6), f"{name}: max err {err:.3e} vs max|ref| {ref:.3e} (tol {tol})"


def _ops():
    import hr_viton_amd  # noqa: F401
    from hr_viton_amd import ops
    return ops


# ------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("C", [8, 13])
def test_batchnorm_train_forward_backward(C):
    """stats + finalize + affine_act (+ residual, ReLU) and bn_bwd vs nn.BatchNorm2d in training mode."""
    ops = _ops()
    from hr_viton_amd import train_ops as T
    g = torch.Generator().manual_seed(C)
    N, H, W = 3, 10, 6
    x = (torch.randn(N, C, H, W, generator=g) * 1.7 + 0.8).requires_grad_(True)
    res = torch.randn(N, C, H, W, generator=g)
    bn = torch.nn.BatchNorm2d(C)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(C, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(C, generator=g) * 0.3)
        bn.running_mean.copy_(torch.randn(C, generator=g) * 0.1)
        bn.running_var.copy_(torch.rand(C, generator=g) + 0.5)
    rm0, rv0 = bn.running_mean.clone(), bn.running_var.clone()
    bn.train()
    y = F.relu(bn(x) + res)
    dy = torch.randn(y.shape, generator=g)
    y.backward(dy)
    xa = ops.to_nhwc(x.detach().cuda())
    rm, rv = rm0.cuda(), rv0.cuda()
    w, b = bn.weight.detach().cuda(), bn.bias.detach().cuda()
    st = T.bn_train_stats(xa, w, b, bn.eps, 0.1, rm, rv)
    out = T.affine_act(xa, st.scale, st.shift, ops.ACT_RELU, ops.to_nhwc(res.cuda()))
    _close("bn_out", ops.to_nchw(out), y, 2e-6)
    _close("running_mean", rm, bn.running_mean, 1e-6)
    _close("running_var", rv, bn.running_var, 1e-6)
    d = ops.to_nhwc(dy.cuda())
    T.act_bwd_(d, out, ops.ACT_RELU, 0.0)
    dg, db = torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
    dx = T.bn_bwd(d, xa, st, dg, db)
    _close("bn_dx", ops.to_nchw(dx), x.grad, 2e-5)
    _close("bn_dgamma", dg, bn.weight.grad, 2e-5)
    _close("bn_dbeta", db, bn.bias.grad, 2e-5)


@pytest.mark.parametrize("case", [("x2", 8, (6, 5), None, 2.0), ("size_x8", 4, (4, 3), (32, 24), None),
                                  ("size_odd", 12, (5, 7), (13, 9), None), ("down", 4, (12, 8), (5, 3), None)],
                         ids=lambda c: c[0])
def test_resize_bilinear_adjoint(case):
    ops = _ops()
    from hr_viton_amd import train_ops as T
    name, C, (H, W), size, sf = case
    g = torch.Generator().manual_seed(len(name))
    x = torch.randn(2, C, H, W, generator=g, requires_grad=True)
    y = F.interpolate(x, size=size, scale_factor=sf, mode="bilinear", align_corners=False)
    dy = torch.randn(y.shape, generator=g)
    y.backward(dy)
    Ho, Wo = y.shape[2], y.shape[3]
    rh, rw = (1 / sf, 1 / sf) if sf else (H / Ho, W / Wo)
    dx = T.resize_bilinear_bwd(ops.to_nhwc(dy.cuda()), H, W, rh, rw)
    _close("resize_bwd", ops.to_nchw(dx), x.grad, 2e-6)
    # dense 2-channel (flow) variant + accumulate
    d2 = dy[:, :2].permute(0, 2, 3, 1).contiguous().cuda()
    got = T.resize_bilinear_bwd_dense(d2, H, W, rh, rw)
    x2 = torch.randn(2, 2, H, W, generator=g, requires_grad=True)
    F.interpolate(x2, size=size, scale_factor=sf, mode="bilinear", align_corners=False).backward(dy[:, :2])
    _close("resize_bwd_flow", got.permute(0, 3, 1, 2), x2.grad, 2e-6)


def _smooth(g, N, C, H, W, f=4):
    lo = torch.rand(N, C, H // f, W // f, generator=g) * 2 - 1
    return F.interpolate(lo, scale_factor=f, mode="bilinear", align_corners=False)


@pytest.mark.parametrize("case", [("per_pixel", 8, 8, 6, 1.5), ("tiled", 24, 20, 18, 1.5), ("tiled_c40", 40, 12, 20, 0.7),
                                  ("tiled_window_overflow", 16, 24, 20, 9.0)], ids=lambda c: c[0])
def test_flow_warp_adjoint(case):
    """d_src (atomic scatter; >= 16 channels: LDS-privatised 16x16 tiles with a 24x24 source window, direct global
    atomics for tiles whose samples do not fit it) and d_flow_prev (coordinate gradient through normalise + x2
    upsample) of the fused warp vs autograd through the oracle's composition (networks.py:133-135)."""
    ops = _ops()
    from hr_viton_amd import train_ops as T
    g = torch.Generator().manual_seed(5)
    _, C, fh, fw, amp = case
    N = 2
    Ho, Wo = 2 * fh, 2 * fw
    src = _smooth(g, N, C, Ho, Wo).requires_grad_(True)
    flow = (torch.randn(N, fh, fw, 2, generator=g) * amp).requires_grad_(True)   # some samples leave the image
    nx, ny = (Wo / 2 - 1.0) / 2.0, (Ho / 2 - 1.0) / 2.0
    fup = O.resize_bilinear(flow.permute(0, 3, 1, 2), scale_factor=2).permute(0, 2, 3, 1)
    fn = torch.cat([fup[..., 0:1] / nx, fup[..., 1:2] / ny], 3)
    out = O.grid_sample_bilinear_border(src, fn + O.make_grid(N, Ho, Wo))
    dout = torch.randn(out.shape, generator=g)
    out.backward(dout)
    sa = ops.to_nhwc(src.detach().cuda())
    warped, fup_d = ops.flow_warp(sa, flow.detach().cuda().contiguous(), Ho, Wo, 0.5, 0.5, nx, ny)
    _close("warp_fwd", ops.to_nchw(warped), out, 1e-5)
    dsrc = ops.Act(torch.zeros_like(sa.t), C)
    dflow = torch.empty_like(fup_d)
    T.flow_warp_bwd(sa, fup_d, nx, ny, ops.to_nhwc(dout.cuda()), dsrc, dflow, False)
    _close("warp_dsrc", ops.to_nchw(dsrc), src.grad, 2e-5)
    dprev = T.resize_bilinear_bwd_dense(dflow, fh, fw, 0.5, 0.5)
    _close("warp_dflow", dprev, flow.grad, 2e-4)


def test_functional_ops_match_torch():
    """grid_sample / interpolate / softmax / cross_entropy2d / tv_loss: values and gradients."""
    import hr_viton_amd  # noqa: F401
    from hr_viton_amd import functional as HF
    g = torch.Generator().manual_seed(11)
    N, H, W = 2, 16, 12
    # grid_sample (3 + 1 channels, explicit grid partly outside the image)
    img = _smooth(g, N, 3, H, W).requires_grad_(True)
    grid = (O.make_grid(N, H, W) + 0.3 * torch.randn(N, H, W, 2, generator=g)).requires_grad_(True)
    ref = F.grid_sample(img, grid, padding_mode="border", align_corners=False)
    dref = torch.randn(ref.shape, generator=g)
    ref.backward(dref)
    ic, gc = img.detach().cuda().requires_grad_(True), grid.detach().cuda().requires_grad_(True)
    got = HF.grid_sample(ic, gc, padding_mode="border")
    got.backward(dref.cuda())
    _close("gs_fwd", got, ref, 1e-5)
    _close("gs_dinput", ic.grad, img.grad, 2e-5)
    _close("gs_dgrid", gc.grad, grid.grad, 2e-4)
    # interpolate: flow-shaped 2-channel tensor to a x8 size
    fl = torch.randn(N, 2, 4, 3, generator=g, requires_grad=True)
    r = F.interpolate(fl, size=(32, 24), mode="bilinear")
    dr = torch.randn(r.shape, generator=g)
    r.backward(dr)
    fc = fl.detach().cuda().requires_grad_(True)
    gi = HF.interpolate(fc, size=(32, 24), mode="bilinear")
    gi.backward(dr.cuda())
    _close("interp_fwd", gi, r, 2e-6)
    _close("interp_bwd", fc.grad, fl.grad, 2e-6)
    # interpolate(mode='nearest', size=): torch's legacy nearest (train_condition.py:242 under --upsample nearest) -- integer and
    # non-integer ratios, up and down; the forward is an index selection (bit-exact), the adjoint a sum of selected elements
    for (h, w), (ho, wo) in (((4, 3), (32, 24)), ((5, 4), (10, 12)), ((6, 8), (17, 13)), ((16, 12), (5, 7)), ((8, 6), (1024, 768))):
        fl = torch.randn(N, 2, h, w, generator=g, requires_grad=True)
        r = F.interpolate(fl, size=(ho, wo), mode="nearest")
        dr = torch.randn(r.shape, generator=g)
        r.backward(dr)
        fc = fl.detach().cuda().requires_grad_(True)
        gi = HF.interpolate(fc, size=(ho, wo), mode="nearest")
        gi.backward(dr.cuda())
        assert torch.equal(gi.detach().cpu(), r.detach()), (h, w, ho, wo)
        _close("nearest_bwd", fc.grad, fl.grad, 1e-5 if ho * wo > 100000 else 2e-6)
    # softmax / cross entropy over 13 channels
    x = (torch.randn(N, 13, H, W, generator=g) * 3).requires_grad_(True)
    tgt = torch.randint(0, 13, (N, H, W), generator=g)
    sm = torch.softmax(x, 1)
    dsm = torch.randn(sm.shape, generator=g)
    sm.backward(dsm)
    xc = x.detach().cuda().requires_grad_(True)
    smc = HF.softmax(xc, dim=1)
    smc.backward(dsm.cuda())
    _close("softmax", smc, sm, 2e-6)
    _close("softmax_bwd", xc.grad, x.grad, 2e-5)
    x.grad = None
    ce = O.cross_entropy2d(x, tgt)
    (ce * 3.0).backward()
    xc2 = x.detach().cuda().requires_grad_(True)
    cec = HF.cross_entropy2d(xc2, tgt.cuda())
    (cec * 3.0).backward()
    assert abs(cec.item() - ce.item()) < 2e-6 * max(1.0, abs(ce.item()))
    _close("ce_bwd", xc2.grad, x.grad, 2e-5)
    # TV of a flow
    f = torch.randn(N, 9, 7, 2, generator=g, requires_grad=True)
    tv = O.tv_loss(f)
    (tv * 2.0).backward()
    fc2 = f.detach().cuda().requires_grad_(True)
    tvc = HF.tv_loss(fc2)
    (tvc * 2.0).backward()
    assert abs(tvc.item() - tv.item()) < 2e-6 * max(1.0, abs(tv.item()))
    _close("tv_bwd", fc2.grad, f.grad, 1e-6)


def test_lsgan_loss_matches_oracle():
    import hr_viton_amd  # noqa: F401
    from hr_viton_amd.networks import GANLoss
    g = torch.Generator().manual_seed(3)
    preds = [[torch.randn(2, 1, 9, 7, generator=g, requires_grad=True)], [torch.randn(2, 1, 5, 4, generator=g, requires_grad=True)]]
    for real in (True, False):
        want = O.lsgan_loss(preds, real)
        for p in preds:
            p[0].grad = None
        want.backward()
        pc = [[p[0].detach().cuda().requires_grad_(True)] for p in preds]
        got = GANLoss(use_lsgan=True)(pc, real)
        got.backward()
        assert abs(got.item() - want.item()) < 1e-6 * max(1.0, want.item())
        for a, b in zip(pc, preds):
            _close("lsgan_grad", a[0].grad, b[0].grad, 1e-5)


# ----------------------------------------------------------------------------- the full iteration
def _compare_grads(mod, sd, tol, what):
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


def _vgg_pair(seed=5):
    """Random-weight VGG19 for both sides (torchvision's pretrained weights are unavailable offline)."""
    import hr_viton_amd  # noqa: F401
    from hr_viton_amd.vgg import VGGLoss
    torch.manual_seed(seed)
    crit = VGGLoss(Namespace(cuda=False))
    sd = {k: v.detach().clone() for k, v in crit.vgg.state_dict().items()}
    return crit, sd


@pytest.mark.parametrize("with_vgg,comp,occl,edge", [(False, "warp_grad", False, "no_edge"), (True, "warp_grad", False, "no_edge"),
                                                     (False, "detach", True, "no_edge"),
                                                     (False, "no_composition", False, "no_edge"),
                                                     (False, "warp_grad", False, "weighted")],
                         ids=["novgg", "vgg", "detach_occlusion", "no_composition", "edgeaware_weighted_addlast"])
def test_condition_training_iteration_matches_oracle(with_vgg, comp, occl, edge):
    """train_condition.py:136-286 (--Ddownx2 --lasttvonly --interflowloss) on the HIP path vs the oracle:
    the eight loss terms, every tocg / D parameter gradient, running statistics, one Adam update."""
    import hr_viton_amd  # noqa: F401
    from hr_viton_amd import networks, pipeline
    from hr_viton_amd.losses import L1Loss
    from hr_viton_amd.optim import Adam
    from oracle.recipes import condstep_build
    opt, tocg, D, batch = condstep_build(networks.ConditionGenerator, networks.define_D)
    opt.lasttvonly, opt.interflowloss, opt.occlusion, opt.clothmask_composition = True, True, occl, comp
    opt.edgeawaretv, opt.add_lasttv = edge, edge != "no_edge"
    opt.tvlambda, opt.CElamda, opt.GANlambda, opt.no_GAN_loss = 2.0, 10.0, 1.0, False
    crit_vgg, sd_vgg = _vgg_pair() if with_vgg else (None, None)
    sd_g = {k: v.detach().clone().requires_grad_(v.is_floating_point() and "running_" not in k)
            for k, v in tocg.state_dict().items()}
    sd_d = {k: v.detach().clone().requires_grad_(True) for k, v in D.state_dict().items()}
    r = O.condition_train_losses(sd_g, sd_d, sd_vgg, batch, occlusion=occl, composition=comp, edgeawaretv=edge,
                                 add_lasttv=edge != "no_edge")
    r["loss_G"].backward(retain_graph=True)
    g_grads = {k: (None if v.grad is None else v.grad.clone()) for k, v in sd_g.items()}
    for v in sd_d.values():
        v.grad = None
    r["loss_D"].backward()
    # ---------------- HIP ----------------
    tocg.cuda().train()
    D.cuda().train()
    if crit_vgg is not None:
        crit_vgg.vgg.cuda()
    rm_before = tocg.ClothEncoder[0].block[1].running_mean.detach().cpu().clone()
    w_before = {n: p.detach().cpu().clone() for n, p in tocg.named_parameters()}
    opt_g = Adam(tocg.parameters(), lr=0.0002, betas=(0.5, 0.999))
    opt_d = Adam(D.parameters(), lr=0.0002, betas=(0.5, 0.999))
    grads_g, grads_d = {}, {}
    # capture the gradients between backward() and step(): wrap the optimiser steps
    step_g, step_d = opt_g.step, opt_d.step

    def sg():
        grads_g.update({n: p.grad.detach().clone() for n, p in tocg.named_parameters() if p.grad is not None})
        return step_g()

    def sdd():
        grads_d.update({n: p.grad.detach().clone() for n, p in D.named_parameters() if p.grad is not None})
        return step_d()

    opt_g.step, opt_d.step = sg, sdd
    cb = {k: v.cuda() for k, v in batch.items()}
    losses = pipeline.condition_train_step(opt, tocg, D, L1Loss(), crit_vgg, networks.GANLoss(use_lsgan=True), opt_g,
                                           opt_d, cb)
    for k in ("l1", "vgg", "tv", "ce", "g_gan", "loss_G", "d_fake", "d_real", "loss_D"):
        want, got = float(r[k].detach()), float(losses[k].detach())
        assert abs(got - want) < 1e-4 * max(1.0, abs(want)), (k, got, want)

    class _G:   # adapters: _compare_grads walks named_parameters() and reads .grad
        def __init__(self, mod, grads):
            self.mod, self.grads = mod, grads

        def named_parameters(self):
            for n, p in self.mod.named_parameters():
                yield n, Namespace(grad=self.grads.get(n))

    class _W:
        def __init__(self, g):
            self.grad = g

    # sign() of the L1 terms and floor() flips of the warps make G's gradients noisy: 5e-3 scale-aware (measured 4.6e-4)
    _compare_grads(_G(tocg, grads_g), {k: _W(g_grads[k]) for k in sd_g}, 5e-3,
                   ("tocg_vgg step" if with_vgg else "tocg step") if (comp == "warp_grad" and edge == "no_edge")
                   else f"tocg_{comp}_{edge} step")
    _compare_grads(_G(D, grads_d), {k: _W(v.grad) for k, v in sd_d.items()}, 5e-4,
                   ("tocgD_vgg step" if with_vgg else "tocgD step") if (comp == "warp_grad" and edge == "no_edge")
                   else f"tocgD_{comp}_{edge} step")
    # running statistics: momentum 0.1 on the oracle's recorded batch statistics
    mean, var_unb = r["bn_stats"]["ClothEncoder.0.block.1"]
    _close("running_mean", tocg.ClothEncoder[0].block[1].running_mean, 0.9 * rm_before + 0.1 * mean, 1e-5)
    assert int(tocg.out_layer.block[1].num_batches_tracked) == 1
    # one Adam step (betas 0.5/0.999, lr 2e-4) on the oracle's gradient: |dw| = lr wherever the gradient is not ~0
    name = "PoseEncoder.2.block.0.weight"
    gref = g_grads[name]
    big = gref.abs() > 1e-3 * gref.abs().max()
    dw = dict(tocg.named_parameters())[name].detach().cpu() - w_before[name]
    assert torch.allclose(dw[big], -0.0002 * torch.sign(gref[big]), atol=2e-6)


def test_condition_generator_train_mode_no_grad_and_eval_agree_with_oracle():
    """`with torch.no_grad(): tocg(...)` in training mode (train_condition.py:298-299) runs the batch-statistics
    forward without a tape; eval mode keeps using the running statistics."""
    import hr_viton_amd  # noqa: F401
    from hr_viton_amd import networks
    from oracle.recipes import condstep_build
    opt, tocg, D, batch = condstep_build(networks.ConditionGenerator, networks.define_D)
    sd = {k: v.detach().clone() for k, v in tocg.state_dict().items()}
    in1 = torch.cat([batch["cloth"], batch["cloth_mask"]], 1)
    in2 = torch.cat([batch["parse_agnostic"], batch["densepose"]], 1)
    O.BN_TRAIN["on"], O.BN_TRAIN["stats"] = True, {}
    try:
        with torch.no_grad():
            fl, seg, wc, wcm = O.tocg_forward(sd, in1, in2)
    finally:
        O.BN_TRAIN["on"] = False
    tocg.cuda().train()
    with torch.no_grad():
        gfl, gseg, gwc, gwcm = tocg(in1.cuda(), in2.cuda())
    for a, b in zip(gfl, fl):
        _close("flow", a, b, 1e-4)
    _close("seg", gseg, seg, 1e-4)
    _close("warped_c", gwc, wc, 5e-4)
    _close("warped_cm", gwcm, wcm, 5e-4)


def test_rejection_flow_matches_oracle():
    """get_norm_const.py / test_condition.py: eval-mode tocg + D logits, odds, rejection score, misalign mask."""
    import hr_viton_amd  # noqa: F401
    from hr_viton_amd import networks, rejection
    from oracle.recipes import condstep_build
    opt, tocg, D, batch = condstep_build(networks.ConditionGenerator, networks.define_D)
    opt.clothmask_composition = "warp_grad"
    sd_g = {k: v.detach().clone() for k, v in tocg.state_dict().items()}
    sd_d = {k: v.detach().clone() for k, v in D.state_dict().items()}
    with torch.no_grad():
        lr, lf, seg = O.rejection_logits(sd_g, sd_d, batch)
    tocg.cuda().eval()
    D.cuda().eval()
    cb = {k: v.cuda() for k, v in batch.items()}
    glr, glf = rejection.segmap_logits(opt, tocg, D, cb)
    _close("logit_real", glr, lr, 1e-4)
    _close("logit_fake", glf, lf, 1e-4)
    want_const = max((l / (1 - l)) for l in torch.cat([lr, lf]).tolist())
    got_const = rejection.get_const(opt, [cb], tocg, D)
    assert abs(got_const - want_const) < 1e-3 * max(1.0, abs(want_const))
    score, misalign, gseg, _, wcm1 = rejection.rejection_scores(opt, tocg, D, cb, got_const)
    _close("score", score, (lf / (1 - lf)) / want_const, 1e-3)
    _close("fake_segmap", gseg, seg, 1e-4)
    assert misalign.shape == (2, 1, 128, 96) and misalign.min() >= 0


def test_three_training_iterations_against_the_oracle():
    """Three consecutive train_condition.py iterations on the HIP path (from the second one on the gradients are
    produced straight in the fused Adam's flat buffer; BatchNorm running statistics carry over).  Free-running
    trajectories of two fp32 implementations separate quickly under Adam (its update is ~lr*sign(g): elements
    whose gradient is round-off noise around zero step the other way, and the warps' floor() flips feed that
    back), so each iteration is compared at the SAME weights: the oracle is re-synchronised to the HIP weights,
    then takes its own torch.optim.Adam step with its own (continuing) moments.  Checked per iteration: both
    losses, every tocg gradient, and the weights after the step."""
    import hr_viton_amd  # noqa: F401
    from hr_viton_amd import networks, pipeline
    from hr_viton_amd.losses import L1Loss
    from hr_viton_amd.optim import Adam
    from oracle.recipes import condstep_build
    opt, tocg, D, batch0 = condstep_build(networks.ConditionGenerator, networks.define_D)
    opt.lasttvonly, opt.interflowloss, opt.occlusion, opt.clothmask_composition = True, True, False, "warp_grad"
    opt.tvlambda, opt.CElamda, opt.GANlambda, opt.no_GAN_loss = 2.0, 10.0, 1.0, False
    g = torch.Generator().manual_seed(7)
    batches = []
    for s_ in range(3):      # vary the images, keep the label maps
        b = dict(batch0)
        for k in ("cloth", "densepose", "parse_cloth"):
            b[k] = (batch0[k] + 0.2 * F.interpolate(torch.randn(2, 3, 16, 12, generator=g), scale_factor=8, mode="bilinear")
                    ).clamp(-1, 1)
        batches.append(b)
    sd_g = {k: v.detach().clone().requires_grad_(v.is_floating_point() and "running_" not in k)
            for k, v in tocg.state_dict().items()}
    sd_d = {k: v.detach().clone().requires_grad_(True) for k, v in D.state_dict().items()}
    og = torch.optim.Adam([v for v in sd_g.values() if v.requires_grad], lr=2e-4, betas=(0.5, 0.999))
    od = torch.optim.Adam(list(sd_d.values()), lr=2e-4, betas=(0.5, 0.999))
    tocg.cuda().train()
    D.cuda().train()
    hg = Adam(tocg.parameters(), lr=2e-4, betas=(0.5, 0.999))
    hd = Adam(D.parameters(), lr=2e-4, betas=(0.5, 0.999))
    crit_gan = networks.GANLoss(use_lsgan=True)
    for it, b in enumerate(batches):
        with torch.no_grad():                      # same starting point for this iteration
            for k, v in tocg.state_dict().items():
                sd_g[k].copy_(v.cpu())
            for k, v in D.state_dict().items():
                sd_d[k].copy_(v.cpu())
        sd_g_before = {k: v.detach().clone().requires_grad_(v.requires_grad) for k, v in sd_g.items()}
        sd_d_before = {k: v.detach().clone() for k, v in sd_d.items()}
        r = O.condition_train_losses(sd_g, sd_d, None, b)
        og.zero_grad()
        od.zero_grad()
        r["loss_G"].backward(retain_graph=True)
        want_g = {k: v.grad.clone() for k, v in sd_g.items() if v.grad is not None}
        og.step()
        od.zero_grad()
        r["loss_D"].backward()
        od.step()
        cap = {}
        real_step = hg.step

        def capture():
            cap.update({n: p.grad.detach().cpu().clone() for n, p in tocg.named_parameters() if p.grad is not None})
            return real_step()

        hg.step = capture
        losses = pipeline.condition_train_step(opt, tocg, D, L1Loss(), None, crit_gan, hg, hd,
                                               {k: v.cuda() for k, v in b.items()})
        hg.step = real_step
        if it > 0:      # the in-place path: the gradient IS its slot of the optimizer's flat buffer
            p0 = tocg.conv1[1].bias
            assert p0.grad is not None and p0.grad.data_ptr() == p0._hrv_flat_grad.data_ptr()
        for k in ("loss_G", "loss_D"):
            assert abs(float(losses[k].detach()) - float(r[k].detach())) < 1e-4 * max(1.0, abs(float(r[k].detach()))), (it, k)
        gmax = max(v.abs().max().item() for v in want_g.values())
        errs = sorted(((cap[k] - w).abs().max().item() / max(w.abs().max().item(), 1e-3 * gmax), k) for k, w in want_g.items())
        diag = diag_path("grad_diag_tocg_3iter.txt")
        with open(diag, "a" if it else "w") as f:
            f.write(f"# iteration {it}: relative gradient error (max-abs / max|want|), worst 8 of {len(errs)}; median "
                    f"{errs[len(errs) // 2][0]:.2e}\n" + "".join(f"{e:.3e} {k}\n" for e, k in errs[-8:]))
        # The gradient of this loss is a DISCONTINUOUS function of the forward values: sign() of the L1 / TV terms,
        # ReLU masks and the floor() of the warp coordinates are decisions, and a parameter gradient is a sum of ~n
        # signed per-pixel terms that largely cancel, so ONE flipped decision moves it by ~1/sqrt(n) (measured on the
        # oracle alone, tools/diag/cond_step_sensitivity.py and profiles/r02_cond_step_sensitivity.txt: a relative
        # input perturbation of 1e-6 flips 2 ReLU / 6 floor / 8 sign decisions and moves the median parameter
        # gradient by 8e-4; 1e-5 moves it by 4e-3..1.2e-2, worst entry up to 1e-1).  Two fp32 implementations whose
        # flows agree to ~3e-5 px sit exactly there (1e-5 moves the oracle's flows by 2.5e-5 px).  So the bound is
        # calibrated per iteration on the oracle itself: its own gradient change under two 1e-5 input perturbations.
        cal_med, cal_worst = 0.0, 0.0
        for ps in (0, 1):
            gp = torch.Generator().manual_seed(1000 + 10 * it + ps)
            bp = dict(b)
            for k in ("cloth", "densepose"):
                bp[k] = b[k] * (1 + 1e-5 * torch.randn(b[k].shape, generator=gp))
            sd_p = {k: v.detach().clone().requires_grad_(v.requires_grad) for k, v in sd_g_before.items()}
            rp = O.condition_train_losses(sd_p, {k: v.detach() for k, v in sd_d_before.items()}, None, bp)
            rp["loss_G"].backward()
            ep = sorted((sd_p[k].grad - w).abs().max().item() / max(w.abs().max().item(), 1e-3 * gmax)
                        for k, w in want_g.items())
            cal_med, cal_worst = max(cal_med, ep[len(ep) // 2]), max(cal_worst, ep[-1])
        with open(diag, "a") as f:
            f.write(f"# iteration {it}: oracle under 1e-5 input perturbations: median {cal_med:.2e} worst {cal_worst:.2e}\n")
        assert errs[len(errs) // 2][0] < 2 * cal_med + 1e-4, (it, errs[len(errs) // 2], cal_med)
        assert errs[-1][0] < 2 * cal_worst + 1e-3, (it, errs[-1], cal_worst)
        sd_h = tocg.state_dict()
        off = tot = 0
        for k, v in sd_g.items():
            if v.requires_grad:
                d = (sd_h[k].detach().cpu() - v.detach()).abs()
                off += (d > 2e-5).sum().item()
                tot += d.numel()
        assert off / tot < 5e-3, (it, off, tot)     # a tenth of one Adam step; the rest are sign flips of ~0 gradients
        mean, var_unb = r["bn_stats"]["SegDecoder.4.block.4"]
        _close("running_var", sd_h["SegDecoder.4.block.4.running_var"],
               0.9 * sd_g["SegDecoder.4.block.4.running_var"] + 0.1 * var_unb, 1e-4)


def test_discriminator_dropout_and_spectral_variants_match_oracle():
    """--Ddropout (the reference README's training command) and --spectral of the tocg discriminator: one
    condition-training iteration with the dropout keep-masks recorded from the oracle run and replayed on the HIP
    path (gen_train.DROP_MASKS); losses and all D gradients."""
    import hr_viton_amd  # noqa: F401
    from hr_viton_amd import gen_train, networks, pipeline
    from hr_viton_amd.losses import L1Loss
    from hr_viton_amd.optim import Adam
    from oracle.recipes import condstep_build

    def define_D(**kw):
        kw.update(Ddropout=True, spectral=True)
        return networks.define_D(**kw)

    opt, tocg, D, batch = condstep_build(networks.ConditionGenerator, define_D)
    assert any(isinstance(m, torch.nn.Dropout) for m in D.modules()) and any(k.endswith("weight_orig") for k in D.state_dict())
    opt.lasttvonly, opt.interflowloss, opt.occlusion, opt.clothmask_composition = True, False, False, "warp_grad"
    opt.tvlambda, opt.CElamda, opt.GANlambda, opt.no_GAN_loss = 2.0, 10.0, 1.0, False
    sd_g = {k: v.detach().clone().requires_grad_(v.is_floating_point() and "running_" not in k)
            for k, v in tocg.state_dict().items()}
    sd_d = {k: v.detach().clone().requires_grad_(v.is_floating_point() and not k.endswith(("weight_u", "weight_v")))
            for k, v in D.state_dict().items()}
    gm = torch.Generator().manual_seed(17)
    rec = {"g": [], "f": [], "r": []}

    def drawer(key):
        def f(shape):
            m = (torch.rand(shape, generator=gm) < 0.5).float() * 2.0
            rec[key].append(m)
            return m
        return f

    O.SN_TRAIN["on"], O.SN_TRAIN["uv"] = True, {}
    try:
        r = O.condition_train_losses(sd_g, sd_d, None, batch, interflowloss=False,
                                     drop_masks={k: drawer(k) for k in rec})
    finally:
        O.SN_TRAIN["on"] = False
    r["loss_G"].backward(retain_graph=True)
    for v in sd_d.values():
        v.grad = None
    r["loss_D"].backward()
    tocg.cuda().train()
    D.cuda().train()
    og = Adam(tocg.parameters(), lr=2e-4, betas=(0.5, 0.999))
    od = Adam(D.parameters(), lr=2e-4, betas=(0.5, 0.999))
    grads_d = {}
    step_d = od.step

    def sdd():
        grads_d.update({n: p.grad.detach().cpu().clone() for n, p in D.named_parameters() if p.grad is not None})
        return step_d()

    od.step = sdd
    gen_train.DROP_MASKS[:] = rec["g"] + [torch.cat([a, b], 0) for a, b in zip(rec["f"], rec["r"])]
    try:
        losses = pipeline.condition_train_step(opt, tocg, D, L1Loss(), None, networks.GANLoss(use_lsgan=True), og, od,
                                               {k: v.cuda() for k, v in batch.items()})
    finally:
        assert not gen_train.DROP_MASKS, "every recorded mask must have been consumed"
        gen_train.DROP_MASKS[:] = []
    for k in ("g_gan", "d_fake", "d_real", "loss_G", "loss_D"):
        want, got = float(r[k].detach()), float(losses[k].detach())
        assert abs(got - want) < 2e-4 * max(1.0, abs(want)), (k, got, want)
    dmax = max(v.grad.abs().max().item() for v in sd_d.values() if v.grad is not None)
    for n, gq in grads_d.items():
        w = sd_d[n].grad
        assert (gq - w).abs().max().item() < 2e-3 * max(w.abs().max().item(), 1e-3 * dmax), n
    # eval mode: dropout is the identity (test_condition.py / get_norm_const.py use D.eval())
    D.eval()
    with torch.no_grad():
        a = D(torch.randn(1, 33, 64, 48, device="cuda"))
        b = D(torch.randn(1, 33, 64, 48, device="cuda") * 0 + 0.1)
    assert a[0][0].shape == b[0][0].shape


def test_g_d_separate_ordering_uses_the_updated_generator():
    """--G_D_seperate (train_condition.py:287-310): the D step sees fake maps of the generator AFTER its Adam
    step, recomputed in training mode under no_grad and WITHOUT the cloth-mask composition.  Oracle: G step with
    torch Adam, forward of the updated weights, LSGAN terms."""
    import hr_viton_amd  # noqa: F401
    from hr_viton_amd import networks, pipeline
    from hr_viton_amd.losses import L1Loss
    from hr_viton_amd.optim import Adam
    from oracle.recipes import condstep_build
    opt, tocg, D, batch = condstep_build(networks.ConditionGenerator, networks.define_D)
    opt.lasttvonly, opt.interflowloss, opt.occlusion, opt.clothmask_composition = True, False, False, "warp_grad"
    opt.tvlambda, opt.CElamda, opt.GANlambda, opt.no_GAN_loss, opt.G_D_seperate = 2.0, 10.0, 1.0, False, True
    sd_g = {k: v.detach().clone().requires_grad_(v.is_floating_point() and "running_" not in k)
            for k, v in tocg.state_dict().items()}
    sd_d = {k: v.detach().clone().requires_grad_(True) for k, v in D.state_dict().items()}
    og = torch.optim.Adam([v for v in sd_g.values() if v.requires_grad], lr=2e-4, betas=(0.5, 0.999))
    r = O.condition_train_losses(sd_g, sd_d, None, batch, interflowloss=False)
    og.zero_grad()
    r["loss_G"].backward()
    og.step()
    in1 = torch.cat([batch["cloth"], batch["cloth_mask"]], 1)
    in2 = torch.cat([batch["parse_agnostic"], batch["densepose"]], 1)
    O.BN_TRAIN["on"], O.BN_TRAIN["stats"] = True, {}
    try:
        with torch.no_grad():
            _, seg_new, _, _ = O.tocg_forward(sd_g, in1, in2)
    finally:
        O.BN_TRAIN["on"] = False
    soft = torch.softmax(seg_new, 1)
    with torch.no_grad():
        want_f = O.lsgan_loss(O.tocg_discriminator_forward(sd_d, torch.cat((in1, in2, soft), 1), 2, 3, True), False)
        want_r = O.lsgan_loss(O.tocg_discriminator_forward(sd_d, torch.cat((in1, in2, batch["parse"]), 1), 2, 3, True), True)
    tocg.cuda().train()
    D.cuda().train()
    hg = Adam(tocg.parameters(), lr=2e-4, betas=(0.5, 0.999))
    hd = Adam(D.parameters(), lr=2e-4, betas=(0.5, 0.999))
    losses = pipeline.condition_train_step(opt, tocg, D, L1Loss(), None, networks.GANLoss(use_lsgan=True), hg, hd,
                                           {k: v.cuda() for k, v in batch.items()})
    assert abs(float(losses["d_fake"].detach()) - float(want_f)) < 2e-3 * max(1.0, float(want_f))
    assert abs(float(losses["d_real"].detach()) - float(want_r)) < 2e-4 * max(1.0, float(want_r))
    # and it differs from the default ordering's D loss (pre-update fake maps)
    assert abs(float(r["d_fake"].detach()) - float(want_f)) > 1e-6
    assert int(tocg.out_layer.block[1].num_batches_tracked) == 2     # two training-mode forwards


@pytest.mark.parametrize("wf,ol,up", [("encoder", "conv", "bilinear"), ("encoder", "relu", "bilinear"), ("T1", "conv", "bilinear"),
                                      ("T1", "relu", "nearest")])
def test_condition_training_iteration_of_the_tocg_variants_matches_oracle(wf, ol, up):
    """train_condition.py --warp_feature encoder / --out_layer conv (networks.py:46-61,142-144): the decoder's third source is the
    cloth-encoder feature warped by the same upsampled flow as T1 (a second consumer of that flow and of E1 on the tape), and the
    logits come out of ResBlock + Conv2d 1x1.  One iteration on the HIP path against torch autograd over the oracle (pinned to the
    reference by tests/golden/tocg_encoder_conv_ngf8_96x64.pt): loss terms, every tocg / D parameter gradient."""
    import hr_viton_amd  # noqa: F401
    from hr_viton_amd import networks, pipeline
    from hr_viton_amd.losses import L1Loss
    from hr_viton_amd.optim import Adam
    from oracle.recipes import condstep_build
    opt, tocg, D, batch = condstep_build(networks.ConditionGenerator, networks.define_D, warp_feature=wf, out_layer=ol)
    opt.lasttvonly, opt.interflowloss, opt.occlusion, opt.clothmask_composition = True, True, False, "warp_grad"
    opt.edgeawaretv, opt.add_lasttv = "no_edge", False
    opt.tvlambda, opt.CElamda, opt.GANlambda, opt.no_GAN_loss = 2.0, 10.0, 1.0, False
    opt.upsample = up          # train_condition.py:104,242: how the inter-flow loss resizes the intermediate flows to the image size
    sd_g = {k: v.detach().clone().requires_grad_(v.is_floating_point() and "running_" not in k) for k, v in tocg.state_dict().items()}
    sd_d = {k: v.detach().clone().requires_grad_(True) for k, v in D.state_dict().items()}
    r = O.condition_train_losses(sd_g, sd_d, None, batch, occlusion=False, composition="warp_grad", edgeawaretv="no_edge",
                                 add_lasttv=False, warp_feature=wf, out_layer=ol, upsample=up)
    r["loss_G"].backward(retain_graph=True)
    g_grads = {k: (None if v.grad is None else v.grad.clone()) for k, v in sd_g.items()}
    for v in sd_d.values():
        v.grad = None
    r["loss_D"].backward()
    tocg.cuda().train()
    D.cuda().train()
    opt_g = Adam(tocg.parameters(), lr=0.0002, betas=(0.5, 0.999))
    opt_d = Adam(D.parameters(), lr=0.0002, betas=(0.5, 0.999))
    grads_g, grads_d = {}, {}
    step_g, step_d = opt_g.step, opt_d.step

    def sg():
        grads_g.update({n: p.grad.detach().clone() for n, p in tocg.named_parameters() if p.grad is not None})
        return step_g()

    def sdd():
        grads_d.update({n: p.grad.detach().clone() for n, p in D.named_parameters() if p.grad is not None})
        return step_d()

    opt_g.step, opt_d.step = sg, sdd
    losses = pipeline.condition_train_step(opt, tocg, D, L1Loss(), None, networks.GANLoss(use_lsgan=True), opt_g, opt_d,
                                           {k: v.cuda() for k, v in batch.items()})
    for k in ("l1", "tv", "ce", "g_gan", "loss_G", "d_fake", "d_real", "loss_D"):
        want, got = float(r[k].detach()), float(losses[k].detach())
        assert abs(got - want) < 1e-4 * max(1.0, abs(want)), (k, got, want)

    class _G:
        def __init__(self, mod, grads):
            self.mod, self.grads = mod, grads

        def named_parameters(self):
            for n, p in self.mod.named_parameters():
                yield n, Namespace(grad=self.grads.get(n))

    class _W:
        def __init__(self, g):
            self.grad = g

    # the tocg gradient is discontinuous in its inputs (sign() of the L1 terms, floor() of the warps, ReLU masks): ONE flipped
    # decision moves every parameter gradient upstream of it by ~1e-2 of its scale (measured: encoder+conv 7e-5 -- no flip --,
    # encoder+relu 6e-3, T1+conv 1.4e-2 on these seeds; the default configuration's tests sit at 5e-4 .. 5e-3), so the bound per
    # parameter is 3e-2 and the DIRECTION over all parameters is held to 0.9998
    _compare_grads(_G(tocg, grads_g), {k: _W(g_grads[k]) for k in sd_g}, 3e-2, f"tocg_{wf}_{ol}_{up} step")
    names = [k for k in sd_g if g_grads[k] is not None and k in grads_g]
    a_ = torch.cat([grads_g[k].detach().cpu().flatten() for k in names])
    b_ = torch.cat([g_grads[k].flatten() for k in names])
    assert float(F.cosine_similarity(a_, b_, dim=0)) > 0.9998
    # (D reads the tocg outputs: a flipped decision there reaches D's gradient through its input -- measured 1.5e-2 on one layer of
    #  the encoder+relu case, <= 1.5e-3 elsewhere)
    _compare_grads(_G(D, grads_d), {k: _W(v.grad) for k, v in sd_d.items()}, 3e-2, f"tocgD_{wf}_{ol}_{up} step")
    dn = [k for k, v in sd_d.items() if v.grad is not None and k in grads_d]
    assert float(F.cosine_similarity(torch.cat([grads_d[k].detach().cpu().flatten() for k in dn]),
                                     torch.cat([sd_d[k].grad.flatten() for k in dn]), dim=0)) > 0.9998
    # every parameter of the variant's extra pieces got a gradient
    if ol == "conv":
        assert "out_layer.1.weight" in grads_g and "out_layer.0.block.0.weight" in grads_g


@pytest.mark.parametrize("wf", ["T1", "encoder"])
def test_condition_generator_training_forward_with_nearest_upsampling_matches_oracle(wf):
    """ConditionGenerator.forward(opt, input1, input2, upsample='nearest') in training mode (networks.py:98,130-133,150): T1 / T2 and the
    flows are up-sampled by selection (ops.resize_nearest / its gather-form adjoint; the warp kernel reads the pre-up-sampled flow at
    ratio 1).  Outputs and every parameter gradient of a loss over all four outputs against torch autograd over the oracle with
    batch-statistics BatchNorm (the oracle's nearest mode is pinned to the real reference by tests/golden/tocg_encoder_conv_...)."""
    import hr_viton_amd  # noqa: F401
    from hr_viton_amd import networks
    from oracle.recipes import condstep_build
    opt, tocg, _D, batch = condstep_build(networks.ConditionGenerator, networks.define_D, warp_feature=wf)
    input1 = torch.cat([batch["cloth"], batch["cloth_mask"]], 1)
    input2 = torch.cat([batch["parse_agnostic"], batch["densepose"]], 1)
    sd = {k: v.detach().clone().requires_grad_(v.is_floating_point() and "running_" not in k) for k, v in tocg.state_dict().items()}
    g = torch.Generator().manual_seed(3)
    O.BN_TRAIN["on"], O.BN_TRAIN["stats"] = True, {}
    try:
        wf_, ws_, wc_, wm_ = O.tocg_forward(sd, input1, input2, wf, "relu", "nearest")
    finally:
        O.BN_TRAIN["on"] = False
    def smooth_like(t):      # low-frequency loss weights: a white-noise weight on a warped image turns ONE flipped floor() cell of the
        if t.dim() == 4 and t.shape[2] >= 16 and t.shape[3] >= 16:      # (NCHW images; the [N,h,w,2] flows keep white noise)
            lo = torch.randn(t.shape[0], t.shape[1], t.shape[2] // 8, t.shape[3] // 8, generator=g)
            return F.interpolate(lo, size=t.shape[2:], mode="bilinear", align_corners=False)
        return torch.randn(t.shape, generator=g)
    ws = [smooth_like(t) for t in list(wf_) + [ws_, wc_, wm_]]
    (sum((f * w).sum() for f, w in zip(wf_, ws[:5])) + (ws_ * ws[5]).sum() + (wc_ * ws[6]).sum() + (wm_ * ws[7]).sum()).backward()
    tocg.cuda().train()
    gf, gs, gc, gm = tocg(opt, input1.cuda(), input2.cuda(), upsample="nearest")
    for i, (a, b) in enumerate(zip(gf, wf_)):
        _close(f"flow{i}", a, b.detach(), 2e-5)
    _close("seg", gs, ws_.detach(), 2e-5)
    _close("warped_c", gc, wc_.detach(), 2e-4)
    (sum((f * w.cuda()).sum() for f, w in zip(gf, ws[:5])) + (gs * ws[5].cuda()).sum() + (gc * ws[6].cuda()).sum() +
     (gm * ws[7].cuda()).sum()).backward()

    class _W:
        def __init__(self, g_):
            self.grad = g_
    # forward outputs agree to 2e-5 (above); the gradient is discontinuous in the sampling coordinates (floor() cells of six to ten warps):
    # measured worst parameter 3.7e-3 (encoder) with these smooth weights -- 8.8e-2 with white-noise weights, where ONE flipped cell
    # shows -- so 3e-2 per parameter and the DIRECTION over all parameters tightly
    _compare_grads(tocg, {k: _W(v.grad) for k, v in sd.items()}, 3e-2, f"tocg_nearest_{wf} fwd-bwd")
    names = [n for n, p in tocg.named_parameters() if p.grad is not None and sd[n].grad is not None]
    a_ = torch.cat([dict(tocg.named_parameters())[n].grad.detach().cpu().flatten() for n in names])
    b_ = torch.cat([sd[n].grad.flatten() for n in names])
    assert float(F.cosine_similarity(a_, b_, dim=0)) > 0.9995
