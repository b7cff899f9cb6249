"""GPU: the validation passes of the training scripts (csrc/validate.hip, hr_viton_amd.metrics / eval_models / validate, and the
val/iou and test/LPIPS plumbing of train_condition.py / train_generator.py) against the float64 restatements of
tests/validate_cases.py and against compositions of parts that have their own tests."""
import ctypes as C
from argparse import Namespace

import pytest
import torch
import torch.nn as nn

import validate_cases as VC

pytestmark = pytest.mark.gpu

POISON = 0x5A5A5A5A5A5A5A5A


def _pkg():
    import hr_viton_amd  # noqa: F401
    from hr_viton_amd import _lib, glue, metrics, validate
    return _lib, glue, metrics, validate


def _counts(seg, cm, label, comp, out=None):
    _, _, metrics, _ = _pkg()
    return metrics.seg_iou_counts(seg.cuda(), None if cm is None else cm.cuda(), label.cuda(), comp, out=out).cpu()


# ----------------------------------------------------------------------------------------- seg_iou_counts
@pytest.mark.parametrize("comp", VC.COMPOSITIONS)
def test_iou_counts_equal_float64_small(comp):
    """3 x 37 x 29: no multiple of the wave or the block, several blocks per sample"""
    _, seed, N, h, w = VC.SMALL
    seg, cm, label = VC.iou_inputs(seed, N, h, w)
    want = VC.iou_counts64(seg, cm, label, comp)
    got = _counts(seg, cm, label, comp)
    print(comp, got.tolist())
    assert got.dtype == torch.int64 and torch.equal(got, want), (got, want)


def test_iou_counts_single_pixel():
    seg, cm, label = VC.iou_inputs(0, 1, 1, 1)
    for comp in VC.COMPOSITIONS:
        assert VC.margin64(seg, cm, comp) > VC.MARGIN
        assert torch.equal(_counts(seg, cm, label, comp), VC.iou_counts64(seg, cm, label, comp)), comp
    assert torch.equal(_counts(seg, None, label, "no_composition"), VC.iou_counts64(seg, cm, label, "no_composition"))


def test_iou_counts_equal_float64_at_the_workload_size():
    """2 x 256 x 192 (192 blocks per sample), the three compositions; the seed's margins are checked in test_validate_cpu.py"""
    _, seed, N, h, w = VC.LARGE
    seg, cm, label = VC.iou_inputs(seed, N, h, w)
    sg, cg, lg = seg.cuda(), cm.cuda(), label.cuda()
    _, _, metrics, _ = _pkg()
    for comp in VC.COMPOSITIONS:
        want = VC.iou_counts64(seg, cm, label, comp)
        got = metrics.seg_iou_counts(sg, cg, lg, comp).cpu()
        print(comp, got.tolist())
        assert torch.equal(got, want), (comp, got, want)


def test_iou_counts_tie_hand_and_perfect_cases():
    seg, cm, label = VC.tie_case()                      # p == 0.5 exactly in fp32: not counted
    assert _counts(seg, cm, label, "warp_grad").tolist() == [[1, 1, 2]]
    assert _counts(seg, cm, label, "no_composition").tolist() == [[1, 1, 2]]
    seg, label, cm_keep, cm_drop = VC.hand_case()
    assert _counts(seg, cm_keep, label, "warp_grad").tolist() == [[1, 1, 2]]
    assert _counts(seg, cm_drop, label, "warp_grad").tolist() == [[0, 0, 2]]
    assert _counts(seg, cm_drop, label, "detach").tolist() == [[0, 0, 2]]
    assert _counts(seg, cm_drop, label, "no_composition").tolist() == [[1, 1, 2]]
    seg, cm, label = VC.perfect_case()
    got = _counts(seg, cm, label, "warp_grad")
    assert torch.equal(got, VC.iou_counts64(seg, cm, label, "warp_grad")) and torch.equal(got[:, 0], got[:, 2])
    _, _, metrics, _ = _pkg()
    assert torch.allclose(metrics.seg_iou(got), torch.ones(2, dtype=torch.float64), atol=1e-12)


def test_iou_counts_overwrite_their_rows_only_and_repeat():
    """a second call into the same buffer, pre-filled with garbage, gives the same counts (the entry zeroes, never accumulates);
    rows beyond N of an oversized buffer keep their poison; two runs are identical"""
    _, seed, N, h, w = VC.SMALL
    seg, cm, label = VC.iou_inputs(seed, N, h, w)
    want = VC.iou_counts64(seg, cm, label, "warp_grad")
    buf = torch.full((N + 2, 3), POISON, dtype=torch.int64, device="cuda")
    first = _counts(seg, cm, label, "warp_grad", out=buf)
    assert torch.equal(first, want)
    assert torch.equal(buf[:N].cpu(), want) and (buf[N:] == POISON).all()
    second = _counts(seg, cm, label, "warp_grad", out=buf)          # onto the first call's counts
    assert torch.equal(second, want) and (buf[N:] == POISON).all()
    buf[:N] = -12345
    assert torch.equal(_counts(seg, cm, label, "warp_grad", out=buf), want)
    assert torch.equal(_counts(seg, cm, label, "warp_grad"), _counts(seg, cm, label, "warp_grad"))


# ----------------------------------------------------------------------------------------- fused LPIPS input
def _scaling():
    return (C.c_float * 3)(*VC.SHIFT), (C.c_float * 3)(*VC.SCALE)


def _prep_fused(a, b, size=VC.OUT_SIZE):
    _lib, _, _, _ = _pkg()
    from hr_viton_amd.ops import _stream
    N, _, H, W = a.shape
    sh, sc = _scaling()
    out = torch.full((2 * N, size[0], size[1], 4), float("nan"), device="cuda")
    _lib.check(_lib.load().hrv_lpips_prep_resize_nchw_f32(a.data_ptr(), b.data_ptr(), N, H, W, size[0], size[1], 0, sh, sc,
                                                          out.data_ptr(), _stream()), "hrv_lpips_prep_resize_nchw_f32")
    return out


def _prep_unfused(a, b, size=VC.OUT_SIZE):
    _lib, glue, _, _ = _pkg()
    from hr_viton_amd.ops import _stream
    N = a.shape[0]
    sh, sc = _scaling()
    out = torch.full((2 * N, size[0], size[1], 4), float("nan"), device="cuda")
    for i, t in enumerate((a, b)):
        r = glue.resize_nchw(t, size, "bilinear")
        _lib.check(_lib.load().hrv_lpips_prep_nchw_f32(r.data_ptr(), N, size[0], size[1], 0, sh, sc, out[i * N:].data_ptr(),
                                                       _stream()), "hrv_lpips_prep_nchw_f32")
    return out


@pytest.mark.parametrize("N", VC.RESIZE_N)
@pytest.mark.parametrize("H,W", VC.RESIZE_SIZES)
def test_fused_lpips_input_is_bit_identical_and_within_the_fp32_margin(H, W, N):
    """hrv_lpips_prep_resize_nchw_f32 == glue.resize_nchw + hrv_lpips_prep_nchw_f32 bit for bit, and within 4x the error torch's
    fp32 CPU path (F.interpolate + scaling) shows against the float64 restatement on the same case.
    Measured on an MI355X over these ten cases (max abs error against float64): the kernel 7.4e-8 .. 3.4e-7, torch fp32 7.4e-8 ..
    3.4e-7; equal in nine, 3.24e-7 against 3.12e-7 at 1 x 131 x 77."""
    a, b = VC.resize_inputs(N, H, W)
    fused = _prep_fused(a.cuda(), b.cuda())
    assert torch.equal(fused, _prep_unfused(a.cuda(), b.cuda()))
    want = torch.cat([VC.prep_resized64(a), VC.prep_resized64(b)], 0)
    ref32 = torch.cat([VC.prep_resized_torch_f32(a), VC.prep_resized_torch_f32(b)], 0)
    err_torch = (ref32.double() - want).abs().max().item()
    err = (fused.cpu().double() - want).abs().max().item()
    print(f"{N}x{H}x{W}: kernel {err:.3e}, torch fp32 {err_torch:.3e}")
    assert err_torch > 0 and err <= 4 * err_torch, (err, err_torch)
    assert (fused[..., 3] == 0).all()


def test_forward_resized_equals_forward_of_the_resizes():
    _, glue, _, _ = _pkg()
    from hr_viton_amd.eval_models import PerceptualLoss
    torch.manual_seed(0)
    model = PerceptualLoss(model="net-lin", net="alex", use_gpu=True)
    with torch.no_grad():
        for k in range(5):          # positive lin weights, as the trained ones are: the distance is not a cancelling sum
            getattr(model.net, f"lin{k}").model[1].weight.abs_()
    for N, H, W in ((2, 256, 192), (1, 131, 77)):
        a, b = VC.resize_inputs(N, H, W)
        a, b = a.cuda(), b.cuda()
        got = model.forward_resized(a, b)
        want = model.forward(glue.resize_nchw(a, (128, 128)), glue.resize_nchw(b, (128, 128)))
        assert got.shape == (N, 1, 1, 1) and torch.isfinite(got).all() and (got > 0).all()
        assert torch.equal(got, want)
        assert torch.equal(model.net.forward_resized(a, b), model.net.forward(glue.resize_nchw(a, (128, 128)),
                                                                              glue.resize_nchw(b, (128, 128))))


# ----------------------------------------------------------------------------------------- condition_validation_iou
def _state(m):
    return {k: v.detach().clone() for k, v in m.state_dict().items()}


def _assert_state_bitwise(m, before):
    after = m.state_dict()
    assert list(after) == list(before)
    for k, v in before.items():
        assert torch.equal(after[k], v), k


def test_condition_validation_iou_vs_float64_oracle():
    """Random-initialised ConditionGenerator (ngf 8, non-trivial running statistics), 2 batches of 2 x 128 x 96 against
    oracle.tocg_forward in eval mode in float64 -> composition -> softmax -> counts.  A network output carries fp32 error, so
    elements whose float64 probability lies within tau = 8 x max |p_gpu - p_64| of 0.5 are exempt: their share is at most 0.5 %,
    and per sample each count differs from the float64 count by at most the number of exempt elements.
    Measured on an MI355X: max |p_gpu - p_64| 3.9e-6 and 3.0e-6 over the two batches (tau 3.2e-5 and 2.4e-5), exempt elements per
    sample 1, 0, 2, 0 of 159744, every count equal to the float64 count."""
    _, _, _, V = _pkg()
    opt, m, batches = VC.tocg_case()
    sd_cpu = _state(m)
    m.cuda()
    assert m.training
    before = _state(m)
    gpu_batches = [{k: v.cuda() for k, v in b.items()} for b in batches]
    res = V.condition_validation_iou(opt, m, gpu_batches)
    assert m.training is True
    _assert_state_bitwise(m, before)
    assert res["items"] == 4 and res["counts"].shape == (4, 3)
    # the float64 reference and the GPU's own probabilities (for tau)
    m.eval()
    row, worst_dp = 0, 0.0
    for b, gb in zip(batches, gpu_batches):
        p64 = VC.tocg_probs_oracle(sd_cpu, b, "warp_grad")
        with torch.no_grad():
            cm = (gb["cloth_mask"] > 0.5).float()
            _, seg, _, wcm = m(torch.cat([gb["cloth"], cm], 1), torch.cat([gb["parse_agnostic"], gb["densepose"]], 1))
        p_gpu = VC.softmax64(VC.compose64(seg.cpu(), wcm.cpu(), "warp_grad"))
        tau, exempt, share = VC.exempt_stats(p_gpu, p64, b["parse"])
        worst_dp = max(worst_dp, tau / 8)
        want = VC.counts_from_probs(p64, b["parse"])
        got = res["counts"][row:row + want.shape[0]]
        print(f"tau {tau:.3e} exempt per sample {exempt.tolist()} share {share:.3e}\n got {got.tolist()}\nwant {want.tolist()}")
        assert share <= VC.EXEMPT_SHARE, share
        assert ((got - want).abs() <= exempt[:, None]).all(), (got, want, exempt)
        assert (want[:, 1] > 1000).all()            # the case is decisive: thousands of predictions per sample
        row += want.shape[0]
    m.train()
    assert worst_dp < 1e-3, worst_dp                # fp32 network error, not a different function
    want_iou = float(VC.iou64(res["counts"]).mean())
    assert res["iou"] == pytest.approx(want_iou, rel=1e-12) and 0.0 <= res["iou"] <= 1.0
    # max_items: the first three samples only
    part = V.condition_validation_iou(opt, m, gpu_batches, max_items=3)
    assert part["items"] == 3 and torch.equal(part["counts"], res["counts"][:3])
    # a pass that raises midway still leaves the module in train mode and untouched
    bad = dict(gpu_batches[1])
    bad["densepose"] = bad["densepose"][:, :, :100]
    with pytest.raises(Exception):
        V.condition_validation_iou(opt, m, [gpu_batches[0], bad])
    assert m.training is True
    _assert_state_bitwise(m, before)


# ----------------------------------------------------------------------------------------- generator_validation_lpips
def _generator_case():
    import hr_viton_amd  # noqa: F401
    from hr_viton_amd.eval_models import PerceptualLoss
    from hr_viton_amd.network_generator import SPADEGenerator
    from hr_viton_amd.networks import ConditionGenerator
    import train_generator as tg
    H, W, N = 256, 192, 2
    opt = Namespace(cuda=True, warp_feature="T1", out_layer="relu", norm_G="spectralaliasinstance", gen_semantic_nc=7, ngf=8,
                    num_upsampling_layers="more", fine_height=H, fine_width=W, occlusion=True, GT=False,
                    clothmask_composition="warp_grad")
    torch.manual_seed(0)
    tocg = ConditionGenerator(opt, 4, 16, 13, ngf=8, norm_layer=nn.BatchNorm2d)
    gen = SPADEGenerator(opt, 9)
    gen.init_weights("xavier", 0.02)
    with torch.no_grad():
        for fc in tocg.flow_conv:
            fc.weight.mul_(4.0)
        for n_, p in gen.named_parameters():
            if n_.endswith("noise_scale"):
                p.normal_(0, 0.1)
            elif n_.endswith("weight") or n_.endswith("weight_orig"):
                p.mul_(30.0)
    model = PerceptualLoss(model="net-lin", net="alex", use_gpu=True)
    with torch.no_grad():
        for k in range(5):
            getattr(model.net, f"lin{k}").model[1].weight.abs_()
    tocg.cuda().eval()
    gen.cuda().train()
    g = torch.Generator().manual_seed(7)
    noise = {}
    for j, name in enumerate(gen._blocks()):
        h, w = gen.sh << j, gen.sw << j
        k = 3 if getattr(gen, name).learned_shortcut else 2
        noise[name] = [torch.randn(N, w, h, 1, generator=g).cuda() for _ in range(k)]
    batches = [tg.synthetic_batch(opt, N, 40 + i, "cuda") for i in range(2)]
    return opt, tocg, gen, model, noise, batches


def test_generator_validation_lpips_is_the_composition_of_its_parts():
    """ngf 8, 2 batches of 2 x 256 x 192, injected noise, random LPIPS weights: the mean equals, to 1e-6 relative, make_generator_inputs
    -> eval forward with the same noise -> glue.resize_nchw -> PerceptualLoss.forward; the generator's state (spectral-norm u
    included: a pass run in train mode would advance it) is bitwise unchanged and the module is back in train mode."""
    _, glue, _, V = _pkg()
    from hr_viton_amd.pipeline import make_generator_inputs
    opt, tocg, gen, model, noise, batches = _generator_case()
    before, before_t = _state(gen), _state(tocg)
    assert any(k.endswith("weight_u") for k in before)
    res = V.generator_validation_lpips(opt, tocg, gen, model, batches, noise=noise)
    assert gen.training is True and tocg.training is False
    _assert_state_bitwise(gen, before)
    _assert_state_bitwise(tocg, before_t)
    assert res["items"] == 4 and res["distances"].shape == (4,)
    gen.eval()
    want = []
    for b in batches:
        x, parse7 = make_generator_inputs(opt, tocg, b)
        out = gen(x, parse7, noise=noise)
        want.append(model.forward(glue.resize_nchw(b["image"], (128, 128)), glue.resize_nchw(out, (128, 128))).reshape(-1))
    gen.train()
    want = torch.cat(want).cpu()
    mean = float(want.double().mean())
    print("LPIPS per item", res["distances"].tolist(), "mean", res["lpips"])
    assert mean > 0 and torch.isfinite(want).all()
    assert res["lpips"] == pytest.approx(mean, rel=1e-6)
    assert torch.allclose(res["distances"], want, rtol=1e-6, atol=0)
    # per-batch noise and max_items
    part = V.generator_validation_lpips(opt, tocg, gen, model, batches, noise=[noise, noise], max_items=3)
    assert part["items"] == 3 and torch.allclose(part["distances"], want[:3], rtol=1e-6, atol=0)
    # without injected noise the pass draws its own, as the reference does: finite, and the state still does not move
    free = V.generator_validation_lpips(opt, tocg, gen, model, batches[:1])
    assert free["items"] == 2 and torch.isfinite(free["distances"]).all()
    _assert_state_bitwise(gen, before)
    assert gen.training is True


# ----------------------------------------------------------------------------------------- scripts
def test_train_generator_script_logs_one_lpips_record(tmp_path, capsys):
    import train_generator as tg
    _, _, _, V = _pkg()
    from hr_viton_amd.network_generator import SPADEGenerator
    argv = ["--name", "t", "--synthetic", "-b", "2", "--fine_height", "512", "--fine_width", "384", "--ngf", "8", "--ndf", "8",
            "--tocg_ngf", "16", "--max_steps", "2", "--display_count", "1", "--checkpoint_dir", str(tmp_path / "ck"),
            "--tensorboard_dir", str(tmp_path / "tb"), "--occlusion", "--lpips_count", "2", "--val_items", "3"]
    tg.main(argv)
    recs = V.read_scalars(str(tmp_path / "tb" / "t"))
    assert len(recs) == 1 and recs[0]["tag"] == "test/LPIPS" and recs[0]["step"] == 2
    assert recs[0]["value"] == recs[0]["value"] and abs(recs[0]["value"]) < float("inf")
    out = capsys.readouterr()
    assert f"LPIPS{recs[0]['value']}" in out.out and "RANDOMLY initialised AlexNet" in out.err
    opt = tg.get_opt(argv)
    sd = torch.load(str(tmp_path / "ck" / "t" / "gen_model_final.pth"), map_location="cpu")
    SPADEGenerator(opt, 9).load_state_dict(sd, strict=True)
    assert all(torch.isfinite(v).all() for v in sd.values() if v.is_floating_point())
    assert (tmp_path / "ck" / "t" / "dis_model_final.pth").exists()


def test_train_condition_script_logs_one_iou_record(tmp_path):
    import train_condition as tc
    _, _, _, V = _pkg()
    from hr_viton_amd.networks import ConditionGenerator
    argv = ["--name", "t", "--synthetic", "-b", "2", "--ngf", "8", "--max_steps", "2",
            "--display_count", "1", "--Ddownx2", "--lasttvonly", "--interflowloss", "--checkpoint_dir", str(tmp_path / "ck"),
            "--tensorboard_dir", str(tmp_path / "tb"), "--val_count", "2", "--val_items", "4"]
    tc.main(argv)
    recs = V.read_scalars(str(tmp_path / "tb" / "t"))
    assert len(recs) == 1 and recs[0]["tag"] == "val/iou" and recs[0]["step"] == 2
    assert 0.0 <= recs[0]["value"] <= 1.0
    opt = tc.get_opt(argv)
    sd = torch.load(str(tmp_path / "ck" / "t" / "tocg_final.pth"), map_location="cpu")
    ConditionGenerator(opt, 4, 16, 13, ngf=8, norm_layer=nn.BatchNorm2d).load_state_dict(sd, strict=True)
    assert int(sd["out_layer.block.1.num_batches_tracked"]) == 2          # two training steps; the pass added none


def test_default_counts_leave_no_scalar_record(tmp_path):
    import train_condition as tc
    _, _, _, V = _pkg()
    import train_generator as tg
    argv = ["--name", "t", "--synthetic", "-b", "2", "--ngf", "8", "--max_steps", "2", "--no_vgg_loss",
            "--checkpoint_dir", str(tmp_path / "ck"), "--tensorboard_dir", str(tmp_path / "tb")]
    tc.main(argv)
    assert V.read_scalars(str(tmp_path / "tb" / "t")) == [] and not (tmp_path / "tb").exists()
    tg.main(["--name", "g", "--synthetic", "-b", "1", "--fine_height", "256", "--fine_width", "192", "--num_upsampling_layers", "more",
             "--ngf", "8", "--ndf", "8", "--tocg_ngf", "8", "--max_steps", "1", "--no_vgg_loss",
             "--checkpoint_dir", str(tmp_path / "ck"), "--tensorboard_dir", str(tmp_path / "tb")])
    assert V.read_scalars(str(tmp_path / "tb" / "g")) == [] and not (tmp_path / "tb").exists()
