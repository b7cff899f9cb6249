"""Integer-operand cases for the bf16 matrix-core kernels (tests/test_gpu_exact_integer.py; needs no GPU).

Small integers stored in bf16 multiply exactly in fp32, and while every partial sum stays an integer far below 2^24 an fp32
accumulator holds the exact value in ANY summation order -- tile shape, chunking and split-K cannot change a bit.  So the
reference is the same convolution in float64 on the CPU and the comparison is torch.equal; where the kernel stores bf16 the
expected value is the float64 result rounded to nearest-even (odd integers in [256, 512) are exact ties).

Every case keeps its worst-case |sum| (``bound``: K x max|a| x max|b| + the epilogue's addends) at or below 2^20.

Operand ranges (``pick_m``): a sum of K products of independent integers uniform on [-m, m] has standard deviation
sqrt(K) * m (m + 1) / 3.  The ranges aim at ~316 (K * (m (m + 1) / 3)^2 >= 1e5), so that a zero-mean result lies at or above 256
-- where bf16 has fewer mantissa bits than the integer has digits -- for ~40 % of the outputs, and forward cases add an integer
bias around +300, which moves a narrower result into [256, 512).  tests/test_exact_cases_cpu.py checks on the references alone
that every bf16-stored output of every case has >= 1 % exact ties and >= 10 % values with |v| >= 256."""
from functools import lru_cache

import torch
import torch.nn.functional as F

LIMIT = 2 ** 20
BIAS0 = 300


def int_tensor(shape, lo, hi, generator):
    """Integer-valued fp32 in [lo, hi] (|values| <= 256 convert to bf16 exactly)."""
    assert max(abs(lo), abs(hi)) <= 256
    return torch.randint(lo, hi + 1, tuple(shape), generator=generator).to(torch.float32)


def bound(K, amax, bmax, extra=0):
    """Worst-case |sum| of K products plus the epilogue's addends; asserts the case's headroom (2^20 of fp32's 2^24)."""
    b = K * amax * bmax + extra
    assert b <= LIMIT, (K, amax, bmax, extra, b)
    return b


def pick_m(K):
    m = 1
    while K * (m * (m + 1) / 3.0) ** 2 < 1e5 and m < 15:
        m += 1
    return m


def to_bf16_rne(t64):
    """float64 -> bf16, round-to-nearest-even on the fp32 bit pattern (the values here are exact in fp32)."""
    f = t64.to(torch.float32)
    assert torch.equal(f.to(torch.float64), t64.to(torch.float64)), "reference value is not exact in fp32"
    u = f.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    u = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    u = torch.where(u >= 0x8000, u - 0x10000, u).to(torch.int16)
    return u.view(torch.bfloat16)


def _low16(t64):
    f = t64.to(torch.float32).contiguous()
    return f.view(torch.int32).to(torch.int64) & 0xFFFF


def tie_share(ref64):
    """Fraction of the reference outputs that lie exactly half-way between two bf16 values."""
    return float((_low16(ref64) == 0x8000).double().mean())


def big_share(ref64):
    return float((ref64.abs() >= 256).double().mean())


def _nchw(t):
    return t.permute(0, 3, 1, 2).to(torch.float64)


def _act(y, act, slope):
    if act == "relu":
        return F.relu(y)
    if act == "lrelu":
        assert slope in (0.5, 0.25)
        return F.leaky_relu(y, slope)
    assert act in (None, "none")
    return y


def _epilogue(y, bias, residual, res_after_mask, act, slope, mask, mask_slope):
    """act(y + bias [+ residual]) [* (mask > 0 ? 1 : mask_slope)] [+ residual behind the mask]; NCHW float64 in, NHWC out."""
    if bias is not None:
        y = y + bias.to(torch.float64).view(1, -1, 1, 1)
    if residual is not None and not res_after_mask:
        y = y + _nchw(residual)
    y = _act(y, act, slope)
    if mask is not None:
        assert mask_slope in (0.0, 0.5, 0.25)
        m = _nchw(mask)
        y = y * torch.where(m > 0, torch.ones_like(m), torch.full_like(m, mask_slope))
    if residual is not None and res_after_mask:
        y = y + _nchw(residual)
    return y.permute(0, 2, 3, 1).contiguous()


def ref_conv64(x, w, bias=None, stride=1, padding=1, residual=None, res_after_mask=False, act=None, slope=0.5, mask=None,
               mask_slope=0.0):
    """float64 CPU convolution of an NHWC ``x`` with an OIHW ``w`` and the kernels' epilogue; NHWC float64."""
    y = F.conv2d(_nchw(x), w.to(torch.float64), None, stride=stride, padding=padding)
    return _epilogue(y, bias, residual, res_after_mask, act, slope, mask, mask_slope)


def ref_conv_transpose64(dy, w, stride=1, padding=1, output_padding=0, bias=None, residual=None, res_after_mask=False, act=None,
                         slope=0.5, mask=None, mask_slope=0.0):
    """float64 CPU data gradient (F.conv_transpose2d over the forward layer's OIHW ``w``) and the kernels' epilogue."""
    y = F.conv_transpose2d(_nchw(dy), w.to(torch.float64), None, stride=stride, padding=padding, output_padding=output_padding)
    return _epilogue(y, bias, residual, res_after_mask, act, slope, mask, mask_slope)


def _bias(C, g, off=BIAS0):
    return off + int_tensor((C,), -8, 8, g)


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31))


# ---------------------------------------------------------------------------------------------------------------
# generic engine (conv_f32.hip, bf16 tiles): (name, cfg, Cin, Cout, k, N, H, W, out_bf16, act, res, wscale, sigma)
# cfg None: the tile conv_dispatch picks (the probe).  17 / 18: patch tiles (3x3 over C % 128 == 0).
# ---------------------------------------------------------------------------------------------------------------
ENGINE = ([("probe_default", None, 80, 64, 3, 2, 33, 47, False, None, None, 1.0, None)] +
          [(f"cfg{c}", c, 80, 96, 3, 2, 17, 20, c % 2 == 0, "lrelu", "bf16" if c % 4 == 0 else None, 1.0, None) for c in range(8, 16)] +
          [("cfg9_1x1", 9, 144, 64, 1, 2, 17, 20, True, None, None, 1.0, None),
           ("cfg8_sigma", 8, 80, 128, 3, 2, 17, 20, True, "relu", None, 4.0, 2.0),
           ("cfg9_sigma_f32", 9, 32, 36, 3, 2, 33, 47, False, None, "f32", 0.5, 0.25),
           # column counts off the 4-channel granule: the scalar epilogues (gather tile, eight-wave tile, patch tiles)
           ("cfg9_cout35", 9, 80, 35, 3, 2, 17, 20, False, "lrelu", None, 1.0, None),
           ("cfg12_cout35", 12, 80, 35, 3, 2, 17, 20, True, "relu", None, 1.0, None),
           ("cfg13_cout67", 13, 80, 67, 3, 2, 17, 20, False, None, None, 1.0, None),
           ("cfg17_cout125", 17, 128, 125, 3, 2, 17, 20, False, "relu", None, 1.0, None),
           ("cfg18_cout61", 18, 128, 61, 3, 2, 17, 20, True, "lrelu", None, 1.0, None),
           ("cfg17", 17, 128, 128, 3, 2, 17, 20, True, "relu", None, 1.0, None),
           ("cfg18_split", 18, 128, 192, 3, 2, 17, 20, True, "lrelu", "bf16", 2.0, 4.0),
           ("cfg18_f32", 18, 256, 64, 3, 2, 33, 47, False, None, None, 1.0, None),
           ("cfg18_wrap", 18, 128, 64, 3, 1, 250, 270, True, "relu", None, 1.0, None)])
ENGINE_SPLITK = (0, 2, 5)


@lru_cache(maxsize=None)
def engine(case):
    name, cfg, Cin, Cout, k, N, H, W, out_bf16, act, res, wscale, sigma = case
    g = _gen(Cin, Cout, k, H, W, len(name))
    K = k * k * Cin
    m = pick_m(K)
    f = wscale / (sigma or 1.0)
    xall = int_tensor((N, H, W, Cin + 16), -m, m, g)
    w = int_tensor((Cout, Cin, k, k), -m, m, g)
    b = _bias(Cout, g)
    r = int_tensor((N, H, W, Cout), -64, 64, g) if res else None
    ref = ref_conv64(xall[..., 16:], w * f, b, 1, k // 2, residual=r, act=act)
    return dict(xall=xall, coff=16, w=w, b=b, res=r, want={"out": ref}, bf16={"out": out_bf16},
                bound=bound(K, m, m * f, BIAS0 + 8 + (64 if res else 0)))


# ---------------------------------------------------------------------------------------------------------------
# conv_p2.hip
# ---------------------------------------------------------------------------------------------------------------
# (Cin, Cout, N, H, W, out_bf16, act, res): res None | "f32" | "bf16" (added in front of the activation)
P2_FWD = [(32, 36, 2, 33, 47, False, "relu", None), (80, 64, 2, 33, 47, True, "relu", None), (144, 80, 2, 17, 20, True, "relu", None),
          (272, 128, 2, 17, 20, False, "relu", None), (512, 128, 1, 17, 20, True, "relu", None), (64, 144, 1, 17, 20, False, "relu", None),
          (128, 272, 1, 17, 20, True, "relu", None), (96, 192, 1, 17, 20, True, "relu", None), (128, 256, 1, 17, 20, True, "relu", None),
          (48, 48, 2, 17, 20, True, "relu", None), (80, 32, 1, 33, 47, True, "relu", None), (32, 272, 2, 250, 270, True, "relu", None),
          (48, 36, 2, 17, 20, True, "relu", None), (32, 34, 1, 17, 20, False, "relu", None),
          (80, 64, 2, 17, 20, False, None, "f32"), (48, 32, 2, 17, 20, True, "lrelu", "f32"), (144, 128, 2, 17, 20, False, None, "bf16"),
          (80, 80, 2, 33, 47, True, "relu", "f32")]


@lru_cache(maxsize=None)
def p2_fwd(case):
    Cin, Cout, N, H, W, out_bf16, act, res = case
    g = _gen(Cin, Cout, H, W, 1)
    m = pick_m(9 * Cin)
    xall = int_tensor((N, H, W, Cin + 32), -m, m, g)
    w = int_tensor((Cout, Cin, 3, 3), -m, m, g)
    b = _bias(Cout, g)
    rall = int_tensor((N, H, W, Cout + 12), -64, 64, g) if res else None
    ref = ref_conv64(xall[..., 32:], w, b, residual=None if rall is None else rall[..., 4:4 + Cout], act=act)
    return dict(xall=xall, coff=32, w=w, b=b, rall=rall, rcoff=4, want={"out": ref}, bf16={"out": out_bf16},
                bound=bound(9 * Cin, m, m, BIAS0 + 8 + (64 if res else 0)))


# (Ck, Ccol, N, H, W, out_bf16, mask_slope or None, res): res None | "before" | "after" (res_after_mask: conv_dgrad's add_after)
P2_DGRAD = [(128, 64, 2, 33, 47, True, 0.0, None), (64, 128, 2, 17, 20, False, None, None), (64, 144, 1, 17, 20, True, 0.5, None),
            (32, 80, 1, 33, 47, True, 0.0, None), (32, 48, 2, 17, 20, True, None, None), (128, 272, 1, 17, 20, True, 0.0, None),
            (512, 64, 1, 17, 20, True, 0.0, None), (128, 64, 2, 17, 20, True, 0.0, "after"), (64, 80, 2, 17, 20, False, 0.0, "before"),
            (128, 64, 2, 17, 20, True, 0.0, "before"), (32, 272, 2, 250, 270, True, 0.0, None)]


@lru_cache(maxsize=None)
def p2_dgrad(case):
    Ck, Ccol, N, H, W, out_bf16, mslope, res = case
    g = _gen(Ck, Ccol, H, W, 2)
    m = pick_m(9 * Ck)
    dy = int_tensor((N, H, W, Ck), -m, m, g)
    w = int_tensor((Ck, Ccol, 3, 3), -m, m, g)
    mask = int_tensor((N, H, W, Ccol), -3, 3, g).clamp_min(0) if mslope is not None else None
    r = int_tensor((N, H, W, Ccol), -64, 64, g) if res else None
    ref = ref_conv_transpose64(dy, w, residual=r, res_after_mask=res == "after", mask=mask, mask_slope=mslope or 0.0)
    return dict(dy=dy, w=w, mask=mask, res=r, want={"out": ref}, bf16={"out": out_bf16}, bound=bound(9 * Ck, m, m, 64 if res else 0))


# (C, N, H, W, cs_mult, out_bf16): the pair data gradient over [dgamma | dbeta] into 128 channels, ReLU mask of actv
# (a 7th field: the column count where it is not the generator's 128 -- 272 columns are two 4-tile passes in one block + a tail launch)
P2_PAIR = [(80, 2, 33, 47, 3, True), (144, 1, 17, 20, 1, True), (32, 1, 17, 20, 1, False), (272, 1, 17, 20, 2, True),
           (16, 2, 250, 270, 1, True, 272)]
GB_DGRAD = [(80, 2, 33, 47, 3, True), (144, 1, 17, 20, 1, True), (32, 1, 33, 47, 1, False), (272, 1, 17, 20, 2, True),
            (64, 2, 17, 20, 1, True), (96, 1, 17, 20, 2, False), (32, 1, 250, 270, 1, True)]


@lru_cache(maxsize=None)
def pair_dgrad(case):
    C_, N, H, W, cs_mult, out_bf16 = case[:6]
    g = _gen(C_, H, W, cs_mult, 3)
    hid = case[6] if len(case) > 6 else 128
    m = pick_m(18 * C_)
    actv_all = int_tensor((N, H, W, hid * cs_mult), -3, 3, g).clamp_min(0)
    wg, wb = int_tensor((C_, hid, 3, 3), -m, m, g), int_tensor((C_, hid, 3, 3), -m, m, g)
    dgb = int_tensor((N, H, W, 2 * C_), -m, m, g)
    mask = actv_all[..., hid * (cs_mult - 1):]
    ref = ref_conv_transpose64(dgb, torch.cat([wg, wb], 0), mask=mask, mask_slope=0.0)
    return dict(actv_all=actv_all, coff=hid * (cs_mult - 1), wg=wg, wb=wb, dgb=dgb, want={"out": ref}, bf16={"out": out_bf16},
                bound=bound(18 * C_, m, m))


# the 3-channel image ends (VGG19 features.0 and its data gradient): (N, H, W)
P2_IMAGE = [(2, 35, 27)]


@lru_cache(maxsize=None)
def p2_image(case):
    N, H, W = case
    g = _gen(N, H, W, 4)
    m = pick_m(27)
    img = int_tensor((N, 3, H, W), -m, m, g)
    w = int_tensor((64, 3, 3, 3), -m, m, g)
    b = _bias(64, g)
    md = pick_m(9 * 64)
    wd = int_tensor((64, 3, 3, 3), -md, md, g)
    dy = int_tensor((N, H, W, 64), -md, md, g)
    x = img.permute(0, 2, 3, 1)
    return dict(img=img, w=w, b=b, wd=wd, dy=dy,
                want={"out": ref_conv64(x, w, b, act="relu"), "dx": ref_conv_transpose64(dy, wd)}, bf16={"out": True, "dx": False},
                bound=max(bound(27, m, m, BIAS0 + 8), bound(9 * 64, md, md)))


# ---------------------------------------------------------------------------------------------------------------
# spade_gb.hip forward: (C, N, H, W, cs_mult, rstd, noise, act, save)
# ---------------------------------------------------------------------------------------------------------------
GB_FWD = [(80, 2, 33, 47, 3, 1.0, True, "lrelu", True), (144, 2, 17, 20, 1, 2.0, True, None, False), (32, 1, 33, 47, 1, 1.0, False, "lrelu", True),
          (64, 1, 17, 20, 2, 2.0, True, "lrelu", True), (96, 1, 17, 20, 2, 1.0, True, None, True), (272, 1, 17, 20, 1, 2.0, False, "lrelu", False),
          (32, 1, 250, 270, 1, 1.0, True, "lrelu", True)]


def _modulate(N, H, W, C_, rstd, noise, act, gam, bet, g, xm, zm):
    """The SPADE epilogue on integers: act(((x + z * noise_scale) - 0) * rstd * (1 + gamma) + beta), NHWC float64."""
    x = int_tensor((N, H, W, C_), -xm, xm, g)
    z = int_tensor((N, W, H, 1), -zm, zm, g) if noise else None
    ns = int_tensor((C_,), -zm, zm, g) if noise else None
    xn = x.to(torch.float64)
    if noise:
        xn = xn + z.permute(0, 2, 1, 3).to(torch.float64) * ns.to(torch.float64)
    xn = xn * rstd
    out = _act((xn * (1 + gam) + bet).permute(0, 3, 1, 2), act, 0.5).permute(0, 2, 3, 1).contiguous()
    return x, z, ns, out, float(xn.abs().max())


@lru_cache(maxsize=None)
def gb_fwd(case):
    C_, N, H, W, cs_mult, rstd, noise, act, save = case
    g = _gen(C_, H, W, cs_mult, int(rstd), 5)
    hid = 128
    actv_all = int_tensor((N, H, W, hid * cs_mult), -3, 3, g).clamp_min(0)
    wg, wb = int_tensor((C_, hid, 3, 3), -3, 3, g), int_tensor((C_, hid, 3, 3), -3, 3, g)
    bg, bb = _bias(C_, g), _bias(C_, g)
    a = actv_all[..., hid * (cs_mult - 1):]
    gam, bet = ref_conv64(a, wg, bg), ref_conv64(a, wb, bb)
    x, z, ns, out, xmax = _modulate(N, H, W, C_, rstd, noise, act, gam, bet, g, 4, 2)
    gmax = bound(9 * hid, 3, 3, BIAS0 + 8)
    want, bf = {"out": out}, {"out": True}
    if save:
        want["g1p"], bf["g1p"] = 1 + gam, True
    return dict(actv_all=actv_all, coff=hid * (cs_mult - 1), wg=wg, wb=wb, bg=bg, bb=bb, x=x, z=z, ns=ns, want=want, bf16=bf,
                bound=bound(1, (4 + (4 if noise else 0)) * rstd, 1 + gmax, gmax))


# ---------------------------------------------------------------------------------------------------------------
# spade_fused.hip: (C, N, H, W, seg_shift, rstd, noise, act, save).  conv_shared over a 7-channel integer label map in {0, 1} with
# weights in [-3, 3] and a bias in [-4, 4]: |actv| <= 63 * 3 + 4 = 193, which bf16 holds exactly -- the second convolution's
# worst case 1152 * |actv| * |w| leaves no room under 2^20 for an actv beyond 256, so the saved actv is compared exactly but
# carries no tie / magnitude condition ("rounds": False).  The reference still rounds actv with to_bf16_rne as the kernel does.
# ---------------------------------------------------------------------------------------------------------------
FUSED = [(80, 2, 33, 47, 0, 1.0, True, "lrelu", True), (80, 2, 17, 20, 1, 2.0, False, None, False), (144, 1, 17, 20, 1, 1.0, True, "lrelu", True),
         (64, 1, 33, 47, 0, 2.0, False, "lrelu", True), (272, 1, 17, 20, 1, 1.0, True, None, True), (32, 1, 17, 20, 0, 1.0, True, "lrelu", False),
         (96, 1, 17, 20, 1, 2.0, False, "lrelu", True), (32, 2, 250, 270, 0, 1.0, True, "lrelu", True)]


@lru_cache(maxsize=None)
def fused(case):
    C_, N, H, W, shift, rstd, noise, act, save = case
    g = _gen(C_, H, W, shift, int(rstd), 6)
    seg = torch.zeros(N, H << shift, W << shift, 8)
    seg[..., :7] = int_tensor((N, H << shift, W << shift, 7), 0, 1, g)
    wsh, bsh = int_tensor((128, 7, 3, 3), -3, 3, g), int_tensor((128,), -4, 4, g)
    wg, wb = int_tensor((C_, 128, 3, 3), -1, 1, g), int_tensor((C_, 128, 3, 3), -1, 1, g)
    bg, bb = _bias(C_, g), _bias(C_, g)
    s = seg[:, ::(1 << shift), ::(1 << shift), :7]                  # nearest, power-of-two ratio
    amax = bound(63, 1, 3, 4)
    actv = to_bf16_rne(ref_conv64(s, wsh, bsh, act="relu")).to(torch.float64)
    gam, bet = ref_conv64(actv, wg, bg), ref_conv64(actv, wb, bb)
    x, z, ns, out, xmax = _modulate(N, H, W, C_, rstd, noise, act, gam, bet, g, 1, 1)
    gmax = bound(9 * 128, amax, 1, BIAS0 + 8)
    want, bf, rounds = {"out": out}, {"out": True}, {"out": True}
    if save:
        want.update(g1p=1 + gam, actv=actv)
        bf.update(g1p=True, actv=True)
        rounds.update(g1p=True, actv=False)
    return dict(seg=seg, wsh=wsh, bsh=bsh, wg=wg, wb=wb, bg=bg, bb=bb, x=x, z=z, ns=ns, want=want, bf16=bf, rounds=rounds,
                bound=bound(1, (1 + (1 if noise else 0)) * rstd, 1 + gmax, gmax))


# ---------------------------------------------------------------------------------------------------------------
# conv_s2.hip (4x4 stride 2 pad 2)
# ---------------------------------------------------------------------------------------------------------------
# (Cin, Cout, N, H, W, out_bf16, act, wscale, sigma)
S2_FWD = [(64, 128, 2, 35, 27, False, None, 1.0, None), (32, 64, 2, 33, 25, True, "lrelu", 4.0, 2.0), (128, 256, 1, 35, 27, True, None, 1.0, None),
          (64, 192, 1, 33, 25, False, "lrelu", 1.0, 0.5), (32, 64, 2, 498, 538, True, "lrelu", 1.0, None)]


@lru_cache(maxsize=None)
def s2_fwd(case):
    Cin, Cout, N, H, W, out_bf16, act, wscale, sigma = case
    g = _gen(Cin, Cout, H, W, 7)
    m = pick_m(16 * Cin)
    f = wscale / (sigma or 1.0)
    xall = int_tensor((N, H, W, Cin + 8), -m, m, g)
    w = int_tensor((Cout, Cin, 4, 4), -m, m, g)
    b = _bias(Cout, g)
    ref = ref_conv64(xall[..., 8:], w * f, b, 2, 2, act=act)
    assert tuple(ref.shape[1:3]) == (H // 2 + 1, W // 2 + 1)
    return dict(xall=xall, coff=8, w=w, b=b, want={"out": ref}, bf16={"out": out_bf16}, bound=bound(16 * Cin, m, m * f, BIAS0 + 8))


# (Ck, Cph, N, H, W, out_bf16, extra): the forward layer maps Cph -> Ck over H x W; extra: "none" | "mask" | "both" | "res32"
S2_DGRAD = [(128, 64, 2, 35, 27, True, "both"), (64, 32, 2, 33, 25, True, "mask"), (128, 64, 1, 33, 25, False, "none"),
            (256, 128, 1, 35, 27, True, "res32"), (64, 32, 2, 498, 538, True, "both")]


@lru_cache(maxsize=None)
def s2_dgrad(case):
    Ck, Cph, N, H, W, out_bf16, extra = case
    g = _gen(Ck, Cph, H, W, 8)
    Hy, Wy = H // 2 + 1, W // 2 + 1
    m = pick_m(4 * Ck)                      # every dX pixel receives 2 x 2 of the 4 x 4 taps
    dy = int_tensor((N, Hy, Wy, Ck), -m, m, g)
    w = int_tensor((Ck, Cph, 4, 4), -m, m, g)
    xin = int_tensor((N, H, W, Cph), -3, 3, g) if extra in ("both", "mask") else None
    tap = int_tensor((N, H, W, Cph), -64, 64, g) if extra in ("both", "res32") else None
    ref = ref_conv_transpose64(dy, w, 2, 2, (H - 2 * (Hy - 1), W - 2 * (Wy - 1)), residual=tap, mask=xin, mask_slope=0.5)
    assert tuple(ref.shape[1:3]) == (H, W)
    return dict(dy=dy, w=w, xin=xin, tap=tap, want={"out": ref}, bf16={"out": out_bf16}, bound=bound(4 * Ck, m, m, 64 if tap is not None else 0))


# (Cin, Cout, N, H, W, split3): the 2x2 form over the space-to-depth image (even H, W); split3: [hi | lo | hi] operands, fp32 out
S2_CELLS = [(10, 64, 2, 34, 26, False), (3, 64, 1, 66, 34, False), (12, 64, 2, 34, 26, True)]
S2_SPLIT3_FWD = [(64, 128, 2, 35, 27)]


@lru_cache(maxsize=None)
def s2_cells(case):
    Cin, Cout, N, H, W, split3 = case
    g = _gen(Cin, Cout, H, W, 9)
    m = pick_m(16 * Cin)
    Cq = (Cin + 3) // 4 * 4
    x = int_tensor((N, Cin, H, W), -m, m, g)
    w = int_tensor((Cout, Cin, 4, 4), -m, m, g)
    b = _bias(Cout, g)
    xs = torch.zeros(N, H // 2, W // 2, 2, 2, Cq)                  # channel (dy*2+dx)*Cq + c of cell (cy, cx) = pixel (2cy+dy, 2cx+dx)
    xs[..., :Cin] = x.view(N, Cin, H // 2, 2, W // 2, 2).permute(0, 2, 4, 3, 5, 1)
    w2 = torch.zeros(Cout, 2, 2, Cq, 2, 2)
    w2[:, :, :, :Cin] = w.view(Cout, Cin, 2, 2, 2, 2).permute(0, 3, 5, 1, 2, 4)
    ref = ref_conv64(x.permute(0, 2, 3, 1), w, b, 2, 2, act=None if split3 else "lrelu")
    return dict(xs=xs.view(N, H // 2, W // 2, 4 * Cq).contiguous(), w2=w2.view(Cout, 4 * Cq, 2, 2).contiguous(), b=b, Cq=Cq,
                want={"out": ref}, bf16={"out": not split3}, bound=bound(16 * Cin, m, m, BIAS0 + 8))


@lru_cache(maxsize=None)
def s2_split3_fwd(case):
    Cin, Cout, N, H, W = case
    g = _gen(Cin, Cout, H, W, 10)
    m = pick_m(16 * Cin)
    x = int_tensor((N, H, W, Cin), -m, m, g)
    w = int_tensor((Cout, Cin, 4, 4), -m, m, g)
    b = _bias(Cout, g)
    return dict(x=x, w=w, b=b, want={"out": ref_conv64(x, w, b, 2, 2)}, bf16={"out": False}, bound=bound(16 * Cin, m, m, BIAS0 + 8))


# ---------------------------------------------------------------------------------------------------------------
# weight gradients (fp32 results): (name, kernel family the plan must pick, cin, cout, k, stride, pad, N, H, W, wide, accumulate, mixed)
# |dy|, |x| <= 2: the reduction runs over N * Ho * Wo pixels.
# ---------------------------------------------------------------------------------------------------------------
WGRAD = [("class0", "conv_wgrad_tr_kernel[class 0]", 128, 160, 3, 1, 1, 2, 70, 72, False, False, True),
         ("class1", "conv_wgrad_tr_kernel[class 1]", 80, 32, 3, 1, 1, 2, 70, 72, True, True, True),
         ("class2", "conv_wgrad_tr_kernel[class 2]", 32, 32, 3, 1, 1, 2, 70, 72, False, False, True),
         ("class3", "conv_wgrad_tr_kernel[class 3]", 80, 32, 1, 1, 0, 2, 70, 72, False, False, True),
         ("class4", "conv_wgrad_tr_kernel[class 4]", 144, 64, 3, 1, 1, 2, 70, 72, False, False, True),
         ("class5", "conv_wgrad_tr_kernel[class 5]", 64, 128, 3, 1, 1, 2, 70, 72, True, False, True),
         ("class6", "conv_wgrad_tr_kernel[class 6]", 272, 64, 3, 1, 1, 2, 70, 72, False, True, True),
         ("class7", "conv_wgrad_tr_kernel[class 7]", 256, 64, 3, 1, 1, 2, 70, 72, False, False, True),
         ("class8_2x2", "conv_wgrad_tr_kernel[class 8]", 48, 64, 2, 1, 1, 2, 70, 72, False, False, True),
         ("s2", "conv_wgrad_s2_kernel", 64, 128, 4, 2, 2, 2, 129, 131, False, False, True),
         ("s2_c2", "conv_wgrad_s2_kernel", 128, 256, 4, 2, 2, 2, 129, 131, False, False, True),
         ("fallback_528", "conv_wgrad_kernel[bf16 stored]", 528, 64, 3, 1, 1, 2, 34, 36, False, True, True),
         ("fp32", "conv_wgrad_kernel[fp32]", 16, 24, 3, 1, 1, 2, 33, 47, False, True, False)]


@lru_cache(maxsize=None)
def wgrad(case):
    name, kernel, cin, cout, k, stride, pad, N, H, W, wide, accumulate, mixed = case
    g = _gen(cin, cout, k, H, W, 11)
    x = int_tensor((N, H, W, cin), -2, 2, g)
    if k == 2:                                  # the space-to-depth image's zero border: a 'same' 2x2 layer, pad 1 on top / left
        x[:, -1] = 0
        x[:, :, -1] = 0
        Ho, Wo = H, W
        xp = F.pad(_nchw(x), (1, 0, 1, 0))
        p_ref = 0
    else:
        Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
        xp, p_ref = _nchw(x), pad
    dy = int_tensor((N, Ho, Wo, cout), -2, 2, g)
    dw = torch.nn.grad.conv2d_weight(xp, (cout, cin, k, k), _nchw(dy).contiguous(), stride=stride, padding=p_ref)
    db = dy.to(torch.float64).sum((0, 1, 2))
    dw0 = int_tensor((cout, cin, k, k), -64, 64, g) if accumulate else None
    db0 = int_tensor((cout,), -64, 64, g) if accumulate else None
    if accumulate:
        dw, db = dw + dw0, db + db0
    return dict(x=x, dy=dy, dw0=dw0, db0=db0, want={"dw": dw, "db": db}, bf16={"dw": False, "db": False},
                bound=bound(N * Ho * Wo, 2, 2, 64 if accumulate else 0))


# ---------------------------------------------------------------------------------------------------------------
# thin_conv.hip and conv_cout1.hip at the shapes of their own tests: forward and data gradient
# ---------------------------------------------------------------------------------------------------------------
THIN = [(80, 32, 3, 2, 180, 200)]            # (cin, cout, k, N, H, W): bf16 source, bias + LeakyReLU 0.5, bf16 out; dgrad fp32
COUT1 = [(256, 4, 2, 3, 35, 27)]             # (Cin, K, pad, N, H, W): fp32 tensors


@lru_cache(maxsize=None)
def thin(case):
    cin, cout, k, N, H, W = case
    g = _gen(cin, cout, k, H, W, 12)
    m, md = pick_m(k * k * cin), pick_m(k * k * cout)
    x = int_tensor((N, H, W, cin), -m, m, g)
    w = int_tensor((cout, cin, k, k), -m, m, g)
    b = _bias(cout, g)
    wd = int_tensor((cout, cin, k, k), -md, md, g)
    dy = int_tensor((N, H, W, cout), -md, md, g)
    return dict(x=x, w=w, b=b, wd=wd, dy=dy,
                want={"out": ref_conv64(x, w, b, 1, k // 2, act="lrelu"), "dx": ref_conv_transpose64(dy, wd, 1, k // 2)},
                bf16={"out": True, "dx": False}, bound=max(bound(k * k * cin, m, m, BIAS0 + 8), bound(k * k * cout, md, md)))


@lru_cache(maxsize=None)
def cout1(case):
    Cin, K, pad, N, H, W = case
    g = _gen(Cin, K, pad, H, W, 13)
    m = pick_m(K * K * Cin)
    x = int_tensor((N, H, W, Cin), -m, m, g)
    w = int_tensor((1, Cin, K, K), -m, m, g)
    b = _bias(1, g)
    Ho, Wo = H + 2 * pad - K + 1, W + 2 * pad - K + 1
    dy = int_tensor((N, Ho, Wo, 1), -8, 8, g)
    add = int_tensor((N, H, W, Cin), -64, 64, g)
    return dict(x=x, w=w, b=b, dy=dy, add=add,
                want={"out": ref_conv64(x, w, b, 1, pad), "dx": ref_conv_transpose64(dy, w, 1, pad, residual=add)},
                bf16={"out": False, "dx": False}, bound=max(bound(K * K * Cin, m, m, BIAS0 + 8), bound(K * K, 8, m, 64)))


TABLES = {"engine": (ENGINE, engine), "p2_fwd": (P2_FWD, p2_fwd), "p2_dgrad": (P2_DGRAD, p2_dgrad), "p2_pair": (P2_PAIR, pair_dgrad),
          "p2_image": (P2_IMAGE, p2_image), "gb_fwd": (GB_FWD, gb_fwd), "gb_dgrad": (GB_DGRAD, pair_dgrad), "fused": (FUSED, fused),
          "s2_fwd": (S2_FWD, s2_fwd), "s2_dgrad": (S2_DGRAD, s2_dgrad), "s2_cells": (S2_CELLS, s2_cells),
          "s2_split3_fwd": (S2_SPLIT3_FWD, s2_split3_fwd), "wgrad": (WGRAD, wgrad), "thin": (THIN, thin), "cout1": (COUT1, cout1)}


# The case of each persistent kernel with more 16 x 16 tiles than resident blocks (2 per CU: 512 on the MI355X), so that a block
# loops over several tiles (below that count these kernels hand every block ONE (tile, pass) unit and the loop never wraps):
# family -> (case, N, tile-grid height, tile-grid width).  conv_s2 tiles its output (forward) / one phase of dX (data gradient).
WRAP = {"p2_fwd": (P2_FWD[11], 2, 250, 270), "p2_dgrad": (P2_DGRAD[-1], 2, 250, 270), "p2_pair": (P2_PAIR[-1], 2, 250, 270),
        "fused": (FUSED[-1], 2, 250, 270), "s2_fwd": (S2_FWD[-1], 2, 250, 270), "s2_dgrad": (S2_DGRAD[-1], 2, 249, 269),
        "gb_fwd": (GB_FWD[-1], 1, 250, 270), "gb_dgrad": (GB_DGRAD[-1], 1, 250, 270)}      # (spade_gb: one block per CU)


def wrap_tiles(fam):
    _, N, Ht, Wt = WRAP[fam]
    return N * ((Ht + 15) // 16) * ((Wt + 15) // 16)


def case_id(case):
    return "-".join(str(v) for v in case)
