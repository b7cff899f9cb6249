"""Case tables and float64 restatements for the R1 phase (hr_viton_amd.r1, csrc/r1.hip): the InstanceNorm tangent and its adjoint
through torch.autograd (create_graph=True), the closed form the kernels evaluate, and the whole penalty on the oracle's
MultiscaleDiscriminator with spectral norm in eval mode (u, v constants)."""
from argparse import Namespace

import torch
import torch.nn.functional as F

from oracle import hrviton_oracle as O

EPS = 1e-5
SLOPE = 0.2
KSLOPE = float(torch.tensor(0.2, dtype=torch.float32))      # the slope the kernels take (a C float), exactly
MIN_PREACT = 1e-6      # no LeakyReLU decision of an end-to-end case may be closer to 0 than this in float64

# ---- the two InstanceNorm launches: N = 2; C, H x W, channel offset inside a wider tensor ------------------------------------
KERNEL_N = 2
KERNEL_CASES = {"c%d_%dx%d_off%d" % (C, H, W, off): (C, H, W, off)
                for C in (5, 8, 64) for (H, W) in ((1, 1), (3, 5), (17, 13), (33, 37)) for off in (0, 4)}

# ---- r1_seed: Ca + Cb = 10 in Cp = 12 -------------------------------------------------------------------------------------
SEED_CA, SEED_CB, SEED_CP = 7, 3, 12
SEED_CASES = {"n%d_%dx%d" % (N, H, W): (N, H, W) for N in (1, 3) for (H, W) in ((1, 1), (3, 5), (33, 25))}

# ---- the phase: D of ndf = 8, spectral norm on --------------------------------------------------------------------------------
PHASE_CASES = {"d1_2x64x48": dict(num_D=1, N=2, H=64, W=48, seed=11), "d2_2x64x48": dict(num_D=2, N=2, H=64, W=48, seed=12),
               "d1_1x32x24": dict(num_D=1, N=1, H=32, W=24, seed=13), "d2_1x32x24": dict(num_D=2, N=1, H=32, W=24, seed=14)}
GAMMA, INTERVAL = 10.0, 4


def case_seed(name: str) -> int:
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(name)) % 100003


def kernel_inputs(name: str):
    """(c, t, df, cin) float32 NHWC [N, H, W, C] of one kernel case (gaussian; the channels have different means and spreads)."""
    C, H, W, _ = KERNEL_CASES[name]
    g = torch.Generator().manual_seed(case_seed(name))
    shape = (KERNEL_N, H, W, C)
    spread = 0.5 + torch.rand(1, 1, 1, C, generator=g) * 2.0
    shift = torch.randn(1, 1, 1, C, generator=g)
    c = torch.randn(shape, generator=g) * spread + shift
    return c, torch.randn(shape, generator=g), torch.randn(shape, generator=g), torch.randn(shape, generator=g)


def _norm(c):
    mu = c.mean(dim=(1, 2), keepdim=True)
    r = (((c - mu) ** 2).mean(dim=(1, 2), keepdim=True) + EPS) ** -0.5
    return mu, r, (c - mu) * r


def lrelu_mask(y, slope=SLOPE):
    return torch.where(y > 0, torch.ones_like(y), torch.full_like(y, slope))


def closed_form(c, t, df, dtype, cin=None, mask=None, stats=None):
    """The closed form of include/hrviton_hip.h evaluated by torch in ``dtype`` on NHWC operands.  ``mask``: lrelu'(y) decided
    elsewhere (the float64 run), so that an fp32 evaluation rounds the arithmetic and not the decision.  ``stats``: (mean, rstd)
    [N, C] as the launches receive them (they are OPERANDS of the kernels: fp32, from the statistics pass of the forward);
    default: taken from ``c`` in ``dtype``."""
    c, t, df = c.to(dtype), t.to(dtype), df.to(dtype)
    P = c.shape[1] * c.shape[2]
    mu, r, y = _norm(c)
    if stats is not None:
        mu, r = (s.to(dtype)[:, None, None, :] for s in stats)
        y = (c - mu) * r
    m = lrelu_mask(y, KSLOPE) if mask is None else mask.to(dtype)
    q = m * df
    mean = lambda a: a.mean(dim=(1, 2), keepdim=True)  # noqa: E731
    sums = torch.stack([a.sum(dim=(1, 2)) for a in (q, t, y * q, y * t, q * t)], dim=-1)      # [N, C, 5]
    mq, mt, myq, myt = mean(q), mean(t), mean(y * q), mean(y * t)
    ydot = r * (t - mt - y * myt)
    tbar = r * (q - mq - y * myq)
    A = (q * t).sum(dim=(1, 2), keepdim=True) - P * mq * mt
    B = P * myq * myt
    w = q * myt + t * myq
    mw, myw = mq * myt + mt * myq, 2 * myq * myt
    cbar = -(r * r / P) * (A - B) * y - r * r * (w - mw - y * myw)
    if cin is not None:
        cbar = cbar + cin.to(dtype)
    return dict(sums=sums, tbar=tbar, cbar=cbar, fdot=m * ydot, y=y, mask=m)


def check_stats(c, mean, rstd):
    """(mean, rstd) [N, C] fp32 as the statistics pass of the forward hands them to the launches, against float64 statistics of ``c``
    (eps the fp32 value the pass takes).  The pass sums d = c - c[pixel 0] and d^2 in fp32 over slabs of at most 128 pixels -- fewer than
    256 additions per partial, rows included -- and finishes in fp64 with one rounding of each result, so with u = 2^-24
        |mean - mean64| <= u (256 mean|d| + |mean64|),   |var - var64| <= 256 u (mean d^2 + 2 |mean d| mean|d|),
        |rstd - rstd64| <= rstd64 (|var - var64| / (2 (var64 + eps)) + u)."""
    u = 2.0 ** -24
    eps = float(torch.tensor(EPS, dtype=torch.float32))
    c = c.double()
    d = c - c[:, :1, :1, :]
    mean64 = c.mean(dim=(1, 2))
    var64 = ((c - mean64[:, None, None, :]) ** 2).mean(dim=(1, 2))
    rstd64 = (var64 + eps) ** -0.5
    mad, md, md2 = d.abs().mean(dim=(1, 2)), d.mean(dim=(1, 2)).abs(), (d * d).mean(dim=(1, 2))
    tol_mean = u * (256 * mad + mean64.abs())
    tol_rstd = rstd64 * (256 * u * (md2 + 2 * md * mad) / (2 * (var64 + eps)) + u)
    assert bool(((mean.double() - mean64).abs() <= tol_mean).all()), float(((mean.double() - mean64).abs() / tol_mean.clamp_min(1e-300)).max())
    assert bool(((rstd.double() - rstd64).abs() <= tol_rstd).all()), float(((rstd.double() - rstd64).abs() / tol_rstd).max())


def autograd_form(c, t, df):
    """float64 torch.autograd: fdot = J_f(c) t by the double-backward construction, then (tbar, cbar) = d <fdot, df> / d (t, c)."""
    c = c.double().requires_grad_()
    t = t.double().requires_grad_()
    f = F.leaky_relu(_norm(c)[2], KSLOPE)
    u = torch.zeros_like(f, requires_grad=True)
    jt_u, = torch.autograd.grad(f, c, u, create_graph=True)            # J^T u, linear in u
    fdot, = torch.autograd.grad(jt_u, u, t, create_graph=True)         # J t
    tbar, cbar = torch.autograd.grad((fdot * df.double()).sum(), (t, c))
    return dict(fdot=fdot.detach(), tbar=tbar, cbar=cbar)


# ---------------------------------------------------------------------------------------------------------------
# r1_seed
# ---------------------------------------------------------------------------------------------------------------
def seed_restated(d_in: torch.Tensor, Ca: int, Cb: int, gamma: float):
    """d_in float32 [N,H,W,Cp] -> (v float32, sums float64 [N], penalty float32, loss float32) as the header defines them."""
    N = d_in.shape[0]
    img = d_in[..., Ca:Ca + Cb]
    v = torch.zeros_like(d_in)
    v[..., Ca:Ca + Cb] = img * (torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(N), dtype=torch.float32))
    sums = (img.double() ** 2).sum(dim=(1, 2, 3))
    pen = sums.sum() / N
    return v, sums, pen.float(), (0.5 * float(torch.tensor(gamma, dtype=torch.float32)) * pen).float()


# ---------------------------------------------------------------------------------------------------------------
# the phase
# ---------------------------------------------------------------------------------------------------------------
def build_d(num_D: int, seed: int, wmul: float = 6.0):
    """The tiny MultiscaleDiscriminator of tests/test_gpu_train_step.py (ndf = 8, spectral norm on), on the CPU."""
    import hr_viton_amd  # noqa: F401
    from hr_viton_amd.network_generator import MultiscaleDiscriminator
    opt = Namespace(cuda=True, gen_semantic_nc=7, ndf=8, norm_D="spectralinstance", n_layers_D=3, num_D=num_D, no_ganFeat_loss=False)
    torch.manual_seed(seed)
    D = MultiscaleDiscriminator(opt)
    D.init_weights("xavier", 0.02)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for n_, p in D.named_parameters():
            if n_.endswith("weight") or n_.endswith("weight_orig"):
                p.mul_(wmul)
            elif n_.endswith("bias"):
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
    return D


def phase_inputs(case: dict):
    """(parse one-hot [N,7,H,W], real [N,3,H,W]) float32"""
    g = torch.Generator().manual_seed(case["seed"] + 100)
    N, H, W = case["N"], case["H"], case["W"]
    lab = torch.randint(0, 7, (N, 1, H // 8, W // 8), generator=g).repeat_interleave(8, 2).repeat_interleave(8, 3)
    parse = torch.zeros(N, 7, H, W).scatter_(1, lab, 1.0)
    return parse, torch.rand(N, 3, H, W, generator=g) * 2 - 1


def _sd(D, dtype):
    return {k: v.detach().clone().to(dtype).requires_grad_(not k.endswith(("weight_u", "weight_v")))
            for k, v in D.state_dict().items() if v.dtype.is_floating_point}


def _param_grads(loss, sd, names):
    ps = [sd[n] for n in names]
    gs = torch.autograd.grad(loss, ps, allow_unused=True)
    return {n: (torch.zeros_like(p) if g is None else g).detach() for n, p, g in zip(names, ps, gs)}


def penalty_autograd(D, parse, real, gamma, scale, num_D, dtype=torch.float64):
    """The penalty as its definition: g = d(sum_n S_n)/d(real) with create_graph=True through the ORACLE's discriminator, then the
    gradient of scale * gamma / 2 * mean_n ||g_n||^2.  Returns {'D_R1', 'r1_penalty', 'g' (the input gradient), 'grads': {name: tensor}}."""
    sd = _sd(D, dtype)
    names = [n for n, _ in D.named_parameters()]
    x = real.to(dtype).requires_grad_()
    pred = O.gen_discriminator_forward(sd, torch.cat([parse.to(dtype), x], 1), num_D=num_D)
    S = sum(p[-1].mean(dim=(1, 2, 3)) for p in pred) / num_D
    g, = torch.autograd.grad(S.sum(), x, create_graph=True)
    pen = (g ** 2).sum(dim=(1, 2, 3)).mean()
    return {"D_R1": float(0.5 * gamma * pen.detach()), "r1_penalty": float(pen.detach()), "g": g.detach(),
            "grads": _param_grads(scale * 0.5 * gamma * pen, sd, names)}


def _conv(x, w, b, stride):
    return F.conv2d(x, w, b, stride=stride, padding=2)


def pair_forward(sd, inp, tin, num_D, n_layers=3):
    """(S [N], Sdot [N], smallest |pre-activation| of any LeakyReLU) of the discriminator and of its tangent along ``tin``, written
    out layer by layer: the tangent convolutions carry NO bias, InstanceNorm's tangent is the closed form."""
    S = Sdot = 0
    closest = float("inf")
    for d in range(num_D):
        p = "discriminator_%d" % d
        w = sd[p + ".model0.0.weight"]
        c, tc = _conv(inp, w, sd[p + ".model0.0.bias"], 2), _conv(tin, w, None, 2)
        closest = min(closest, float(c.detach().abs().min()))
        h, t = F.leaky_relu(c, SLOPE), lrelu_mask(c.detach()) * tc
        for n in range(1, n_layers):
            w = O._sn_weight(sd, "%s.model%d.0.0" % (p, n))
            c, tc = _conv(h, w, None, 2), _conv(t, w, None, 2)
            mu = c.mean(dim=(2, 3), keepdim=True)
            r = (((c - mu) ** 2).mean(dim=(2, 3), keepdim=True) + EPS) ** -0.5
            y = (c - mu) * r
            closest = min(closest, float(y.detach().abs().min()))
            ydot = r * (tc - tc.mean(dim=(2, 3), keepdim=True) - y * (y * tc).mean(dim=(2, 3), keepdim=True))
            h, t = F.leaky_relu(y, SLOPE), lrelu_mask(y.detach()) * ydot
        w = sd["%s.model%d.0.weight" % (p, n_layers)]
        S = S + _conv(h, w, sd["%s.model%d.0.bias" % (p, n_layers)], 1).mean(dim=(1, 2, 3)) / num_D
        Sdot = Sdot + _conv(t, w, None, 1).mean(dim=(1, 2, 3)) / num_D
        inp = F.avg_pool2d(inp, kernel_size=3, stride=2, padding=[1, 1], count_include_pad=False)
        tin = F.avg_pool2d(tin, kernel_size=3, stride=2, padding=[1, 1], count_include_pad=False)
    return S, Sdot, closest


def penalty_tangent(D, parse, real, gamma, scale, num_D, dtype=torch.float64):
    """The same gradients by the identity the phase uses: grad_theta P = gamma grad_theta sum_n <g_n, sg(g_n) / N>, the inner
    product taken as the tangent pass of pair_forward (no bias in a tangent convolution: the bias gradients get nothing from the
    tangent path).  Also returns 'closest', the smallest |pre-activation| of the run."""
    sd = _sd(D, dtype)
    names = [n for n, _ in D.named_parameters()]
    N = real.shape[0]
    x = real.to(dtype).requires_grad_()
    inp = torch.cat([parse.to(dtype), x], 1)
    S, _, closest = pair_forward(sd, inp, torch.zeros_like(inp), num_D)
    g, = torch.autograd.grad(S.sum(), x)
    pen = (g ** 2).sum(dim=(1, 2, 3)).mean()
    v = torch.cat([torch.zeros_like(parse, dtype=dtype), g.detach() / N], 1)
    _, Sdot, _ = pair_forward(sd, inp.detach(), v, num_D)
    return {"D_R1": float(0.5 * gamma * pen), "r1_penalty": float(pen), "closest": closest,
            "grads": _param_grads(scale * gamma * Sdot.sum(), sd, names)}
