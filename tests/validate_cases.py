"""Case tables and float64 restatements for the validation passes (hr_viton_amd.validate, csrc/validate.hip), shared by
tests/test_validate_cpu.py and tests/test_gpu_validate.py.  Written from the definitions, not from the reference's text:

* IoU counts: ``pred = softmax_c(seg * mask) > 0.5`` over 13 channels, mask = ones but for channel 3 (``cm > 0.5`` under 'detach',
  ``cm`` under 'warp_grad'); per sample I = #(pred and label == 1), S_pred = #pred, S_true = #(label == 1);
  IoU = (I + 1e-7) / (S_pred + S_true - I + 1e-7).
* LPIPS input: bilinear resampling with ``align_corners=False``, no antialiasing -- source coordinate ``(d + 0.5) * (in / out) - 0.5``
  clamped at 0, the two neighbours clamped at the edge -- then ``(v - shift) / scale`` per channel, NHWC with a zero 4th channel.

A case is exact (the GPU test may demand equality of the counts) when, in float64, no softmax value lies within MARGIN of 0.5:
fp32 evaluation of a 13-term softmax is off by a few 1e-7, far inside the margin.
"""
import functools

import torch

COMPOSITIONS = ("no_composition", "detach", "warp_grad")
MARGIN = 1e-5
SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)

# (name, seed, N, h, w): seed 0 at 3x37x29 keeps 3.5e-4 / 7.2e-5 / 3.0e-4 (no_composition / detach / warp_grad) from 0.5; seed 1
# comes within 1.8e-6 and is not used.  At 2x256x192 (1.28 M values per composition) seed 0 fails the condition, as do most seeds;
# 2266 is the first of 0..2999 that holds it for all three compositions (1.01e-5 / 1.24e-5 / 1.28e-5; fp32 softmax is off by a few
# 1e-7).  tests/test_validate_cpu.py checks the condition for the recorded seeds.
SMALL = ("small", 0, 3, 37, 29)
LARGE = ("large", 2266, 2, 256, 192)

# fused LPIPS input: (H, W) -> 128x128; exact .5 taps / the workload / mixed down-up sampling with clamped edges / identity / 1x1
RESIZE_SIZES = ((1024, 768), (256, 192), (131, 77), (128, 128), (1, 1))
RESIZE_N = (1, 3)
OUT_SIZE = (128, 128)


# --------------------------------------------------------------------------------------------- IoU
def compose64(seg, cm, composition):
    """seg * cloth_mask in float64 (the products are those of the fp32 inputs, exact in float64)."""
    s = seg.double().clone()
    if composition == "detach":
        s[:, 3:4] = s[:, 3:4] * (cm > 0.5).double()
    elif composition == "warp_grad":
        s[:, 3:4] = s[:, 3:4] * cm.double()
    else:
        assert composition == "no_composition", composition
    return s


def softmax64(x):
    e = torch.exp(x - x.max(dim=1, keepdim=True).values)
    return e / e.sum(dim=1, keepdim=True)


def counts_from_probs(p, label, strict=True):
    """int64 [N,3] = (intersection, sum_pred, sum_true) per sample"""
    pred = (p > 0.5) if strict else (p >= 0.5)
    truth = label == 1
    N = p.shape[0]
    return torch.stack([(pred & truth).reshape(N, -1).sum(1), pred.reshape(N, -1).sum(1), truth.reshape(N, -1).sum(1)], 1).long()


def iou_counts64(seg, cm, label, composition, strict=True, composed=True):
    """The restatement.  ``strict=False`` (>= instead of >) and ``composed=False`` (composition dropped) are the mutants the CPU
    test must be able to tell apart."""
    s = compose64(seg, cm, composition if composed else "no_composition")
    return counts_from_probs(softmax64(s), label, strict)


def iou64(counts):
    c = counts.double()
    return (c[:, 0] + 1e-7) / (c[:, 1] + c[:, 2] - c[:, 0] + 1e-7)


def margin64(seg, cm, composition):
    """closest approach of a float64 softmax value to 0.5"""
    return float((softmax64(compose64(seg, cm, composition)) - 0.5).abs().min())


@functools.lru_cache(maxsize=None)
def iou_inputs(seed, N, h, w):
    """The recipe: seg = 4 * randn, cm = rand, then the labels -- half of the pixels (a coin per pixel) take the argmax of the
    warp_grad-composed logits, the rest a uniform class; one-hot fp32."""
    g = torch.Generator().manual_seed(seed)
    seg = 4 * torch.randn(N, 13, h, w, generator=g)
    cm = torch.rand(N, 1, h, w, generator=g)
    coin = torch.rand(N, 1, h, w, generator=g) < 0.5
    rnd = torch.randint(0, 13, (N, 1, h, w), generator=g)
    top = compose64(seg, cm, "warp_grad").argmax(dim=1, keepdim=True)
    idx = torch.where(coin, top, rnd)
    label = torch.zeros(N, 13, h, w).scatter_(1, idx, 1.0)
    return seg, cm, label


def tie_case():
    """1x13x1x2: at pixel 0 channels 2 and 7 hold equal logits and the rest -200, so both probabilities are exactly 0.5 in fp32 and
    in float64 (exp(-200) vanishes against 1) and '>' counts neither, '>=' both; at pixel 1 channel 4 wins outright.  Labels: pixel 0
    -> channel 2, pixel 1 -> channel 4."""
    seg = torch.full((1, 13, 1, 2), -200.0)
    seg[0, 2, 0, 0] = seg[0, 7, 0, 0] = 1.5
    seg[0, 4, 0, 1] = 3.0
    cm = torch.ones(1, 1, 1, 2)
    label = torch.zeros(1, 13, 1, 2)
    label[0, 2, 0, 0] = 1.0
    label[0, 4, 0, 1] = 1.0
    return seg, cm, label


def hand_case():
    """1x13x1x2 worked by hand; the logits are logarithms of weights, so a probability is weight / sum of weights.
    Pixel 0 weights: channel 3 -> 36, the other twelve -> 1 each: p3 = 36/48 = 0.75 (pred), the rest 1/48.
    Pixel 1 weights: channel 0 -> 5, channel 5 -> 5, the rest -> 1 each: p0 = p5 = 5/21 < 0.5, no prediction.
    Labels: pixel 0 -> channel 3, pixel 1 -> channel 0.  Counts: I = 1, S_pred = 1, S_true = 2; IoU = 1/2.
    Under 'warp_grad' with cm = 0 at pixel 0 the channel-3 logit becomes 0 (weight 1): 13 equal weights, no prediction: I = 0,
    S_pred = 0, S_true = 2; IoU = 1e-7 / (2 + 1e-7)."""
    w = torch.ones(1, 13, 1, 2, dtype=torch.float64)
    w[0, 3, 0, 0] = 36.0
    w[0, 0, 0, 1] = w[0, 5, 0, 1] = 5.0
    seg = w.log().float()
    label = torch.zeros(1, 13, 1, 2)
    label[0, 3, 0, 0] = 1.0
    label[0, 0, 0, 1] = 1.0
    cm_keep = torch.ones(1, 1, 1, 2)
    cm_drop = torch.tensor([0.0, 1.0]).view(1, 1, 1, 2)
    return seg, label, cm_keep, cm_drop


def perfect_case(N=2, h=9, w=7, seed=3):
    """every pixel predicts its label with a wide margin: IoU is 1 up to the 1e-7 terms"""
    g = torch.Generator().manual_seed(seed)
    idx = torch.randint(0, 13, (N, 1, h, w), generator=g)
    label = torch.zeros(N, 13, h, w).scatter_(1, idx, 1.0)
    seg = torch.randn(N, 13, h, w, generator=g) + 12.0 * label
    cm = torch.ones(N, 1, h, w)          # channel 3 must survive the composition
    return seg, cm, label


# --------------------------------------------------------------------------------------------- fused LPIPS input
def _axis64(out_size, in_size):
    d = torch.arange(out_size, dtype=torch.float64)
    src = ((d + 0.5) * (in_size / out_size) - 0.5).clamp_min(0.0)
    i0 = src.floor().long().clamp_max(in_size - 1)
    i1 = (i0 + 1).clamp_max(in_size - 1)
    lam = (src - i0.double()).clamp(0.0, 1.0)
    return i0, i1, lam


def prep_resized64(x, size=OUT_SIZE):
    """fp32 NCHW [N,3,H,W] -> float64 NHWC [N,Ho,Wo,4]: bilinear (align_corners=False, no antialias), ScalingLayer, zero channel 3"""
    xd = x.double()
    N, C, H, W = xd.shape
    y0, y1, ly = _axis64(size[0], H)
    x0, x1, lx = _axis64(size[1], W)
    ly = ly.view(1, 1, -1, 1)
    lx = lx.view(1, 1, 1, -1)
    top = xd[:, :, y0][:, :, :, x0] * (1 - lx) + xd[:, :, y0][:, :, :, x1] * lx
    bot = xd[:, :, y1][:, :, :, x0] * (1 - lx) + xd[:, :, y1][:, :, :, x1] * lx
    r = top * (1 - ly) + bot * ly
    shift = torch.tensor(SHIFT, dtype=torch.float32).double().view(1, 3, 1, 1)     # the module holds fp32 constants
    scale = torch.tensor(SCALE, dtype=torch.float32).double().view(1, 3, 1, 1)
    v = ((r - shift) / scale).permute(0, 2, 3, 1)
    return torch.cat([v, torch.zeros_like(v[..., :1])], dim=3)


def prep_resized_torch_f32(x, size=OUT_SIZE):
    """torch's fp32 CPU path for the same thing: the yardstick whose error against the float64 restatement sets the limit"""
    import torch.nn.functional as F
    r = F.interpolate(x, size=size, mode="bilinear", align_corners=False)
    shift = torch.tensor(SHIFT, dtype=torch.float32).view(1, 3, 1, 1)
    scale = torch.tensor(SCALE, dtype=torch.float32).view(1, 3, 1, 1)
    v = ((r - shift) / scale).permute(0, 2, 3, 1)
    return torch.cat([v, torch.zeros_like(v[..., :1])], dim=3)


@functools.lru_cache(maxsize=None)
def resize_inputs(N, H, W):
    g = torch.Generator().manual_seed(1000 + 7 * N + H + W)
    return (torch.rand(N, 3, H, W, generator=g) * 2 - 1, torch.rand(N, 3, H, W, generator=g) * 2 - 1)


# --------------------------------------------------------------------------------------------- the passes
TOCG_CASE = dict(seed=0, ngf=8, N=2, H=128, W=96, batches=2)
EXEMPT_SHARE = 0.005          # at most 0.5 % of the N * 13 * h * w elements may lie within tau of 0.5


def tocg_case():
    """A random-initialised ConditionGenerator (ngf 8) in train mode with non-trivial BatchNorm running statistics and an output
    layer scaled up so that the softmax is decisive at many pixels (a fresh network predicts 1/13 everywhere and the counts would
    be trivially zero), plus two train_condition.py-shaped batches of 2 x 128 x 96.  Returns (opt, module on the CPU, batches)."""
    from argparse import Namespace
    import torch.nn as nn
    import hr_viton_amd  # noqa: F401
    from hr_viton_amd.networks import ConditionGenerator
    import train_condition as tc
    c = TOCG_CASE
    opt = Namespace(cuda=True, warp_feature="T1", out_layer="relu", clothmask_composition="warp_grad", fine_height=c["H"],
                    fine_width=c["W"])
    torch.manual_seed(c["seed"])
    m = ConditionGenerator(opt, 4, 16, 13, ngf=c["ngf"], norm_layer=nn.BatchNorm2d)
    g = torch.Generator().manual_seed(c["seed"] + 1)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, nn.BatchNorm2d):
                mod.running_mean.copy_(torch.randn(mod.running_mean.shape, generator=g) * 0.1)
                mod.running_var.copy_(torch.rand(mod.running_var.shape, generator=g) + 0.5)
                mod.num_batches_tracked.fill_(5)
        for fc in m.flow_conv:
            fc.weight.mul_(4.0)
        m.out_layer.block[4].weight.mul_(12.0)
        m.out_layer.block[4].bias.copy_(torch.randn(13, generator=g) * 2.0)
    m.train()
    batches = [{k: v for k, v in tc.synthetic_batch(opt, c["N"], 500 + i, "cpu").items()} for i in range(c["batches"])]
    return opt, m, batches


def tocg_probs_oracle(sd, batch, composition, dtype=torch.float64):
    """softmax(fake_segmap * cloth_mask) of the ORACLE's eval-mode forward in ``dtype`` (float64: the reference of the GPU test)"""
    from oracle import hrviton_oracle as O
    sdd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
    cm = (batch["cloth_mask"] > 0.5).to(dtype)
    i1 = torch.cat([batch["cloth"].to(dtype), cm], 1)
    i2 = torch.cat([batch["parse_agnostic"].to(dtype), batch["densepose"].to(dtype)], 1)
    with torch.no_grad():
        _, seg, _, wcm = O.tocg_forward(sdd, i1, i2)
    return softmax64(compose64(seg, wcm, composition))


def exempt_stats(p_test, p64, label):
    """tau = 8 x the largest |p_test - p64|; the exempt elements (|p64 - 0.5| <= tau), their count per sample and their share"""
    tau = 8.0 * float((p_test.double() - p64).abs().max())
    exempt = (p64 - 0.5).abs() <= tau
    per_sample = exempt.reshape(exempt.shape[0], -1).sum(1)
    return tau, per_sample, float(exempt.double().mean())
