"""Cases and restatements of DiffAugment inside the PatchGAN input assembly (csrc/diffaug.hip, hr_viton_amd/diffaug.py; the
transform is defined in include/hrviton_hip.h).  Pure CPU torch / numpy: tests/test_diffaug_cases_cpu.py holds the restatements
against a pure-Python decode and torch's float64 autograd, tests/test_gpu_diffaug.py holds the kernels against the restatements.

The integer decisions (shift, box) are decoded in fp32 with truncation toward zero, as the kernel decodes them, so restatement and
kernel agree to the bit on WHERE every pixel comes from; the color arithmetic is float64 here."""
import struct
from fractions import Fraction

import numpy as np
import torch

COLOR, TRANSLATION, CUTOUT = 1, 2, 4
GEOMETRY = TRANSLATION | CUTOUT
ALL = COLOR | GEOMETRY
SLOTS, BLOCK = 128, 256          # HRV_DIFFAUG_SLOTS partial sums per sample, threads per block
# (N, H, W): one pixel row of blocks | odd extents, 3HW = 663: sample 1 starts on a 4-byte boundary only | several blocks a sample |
# 129 * 97 = 12513 pixels: 3HW / 4 = 9384 groups + a tail of 3, more than one block per slot row
SHAPES = [(1, 8, 8), (2, 17, 13), (3, 64, 48), (2, 129, 97)]
POW2_SHAPES = [(1, 8, 8), (2, 16, 32)]      # HW a power of two: the exact color cases
TOP = 1.0 - 2.0 ** -24          # the largest fp32 below 1
EPS = 2.0 ** -24


# ------------------------------------------------------------------ decode
def _f32(x) -> np.float32:
    return np.float32(x)


def shift(u, extent: int) -> int:
    S = (extent + 4) // 8
    return min(int(_f32(u) * _f32(2 * S + 1)), 2 * S) - S


def box(u, extent: int):
    c = extent // 2
    odd = c % 2
    o = min(int(_f32(u) * _f32(extent + 1 - odd)), extent - odd)
    return max(o - c // 2, 0), min(o - c // 2 + c, extent)


def decode(urow, flags: int, H: int, W: int):
    """(beta, s, k) as np.float32 and (ty, tx, y0, y1, x0, x1) as ints, of one row of uniforms; identities for what the policy lacks"""
    urow = np.asarray(urow, dtype=np.float32)
    beta, s, k = _f32(0), _f32(1), _f32(1)
    if flags & COLOR:
        beta, s, k = urow[0] - _f32(0.5), _f32(2) * urow[1], urow[2] + _f32(0.5)
    ty = tx = y0 = y1 = x0 = x1 = 0
    if flags & TRANSLATION:
        ty, tx = shift(urow[3], H), shift(urow[4], W)
    if flags & CUTOUT:
        (y0, y1), (x0, x1) = box(urow[5], H), box(urow[6], W)
    return (beta, s, k), (ty, tx, y0, y1, x0, x1)


def _round_f32(q: Fraction) -> Fraction:
    """q rounded to the nearest fp32 (ties to even), without numpy: q = (24-bit value) x (small integer) is exact as a double"""
    d = q.numerator / q.denominator
    assert Fraction(d) == q
    return Fraction(struct.unpack("f", struct.pack("f", d))[0])


def decode_geom_py(urow, flags: int, H: int, W: int):
    """the same six integers from integers and fractions only"""
    def sh(u, extent):
        S = (extent + 4) // 8
        return min(int(_round_f32(Fraction(float(u)) * (2 * S + 1))), 2 * S) - S

    def bx(u, extent):
        c = extent // 2
        odd = c % 2
        o = min(int(_round_f32(Fraction(float(u)) * (extent + 1 - odd))), extent - odd)
        return max(o - c // 2, 0), min(o - c // 2 + c, extent)
    ty, tx = (sh(urow[3], H), sh(urow[4], W)) if flags & TRANSLATION else (0, 0)
    (y0, y1), (x0, x1) = (bx(urow[5], H), bx(urow[6], W)) if flags & CUTOUT else ((0, 0), (0, 0))
    return ty, tx, y0, y1, x0, x1


# ------------------------------------------------------------------ the forced table
def forced_rows(H: int, W: int, seed: int = 0):
    """[(name, row of 8)]: identity color and shift; t = -S, 0, +S on each axis, +S through u = TOP; the box overhanging each of the
    four borders; u = 1.0 on the four geometric entries; random rows.  TOP * n never rounds up to n in fp32 (n * 2^-24 is at least
    half an ulp below n), so TOP lands in the last bin WITHOUT the clamp; the clamp is what keeps a u of exactly 1.0 -- outside
    torch.rand's range, but a caller may inject it -- inside the image, and the 'clamp' row is the one that exercises it."""
    mid = [0.5] * 7 + [0.0]

    def row(**kw):
        r = list(mid)
        for k, v in kw.items():
            r[int(k[1:])] = v
        return r
    rows = [("identity", row())]
    for ny, uy in (("-S", 0.0), ("0", 0.5), ("+S", TOP)):
        for nx, ux in (("-S", 0.0), ("0", 0.5), ("+S", TOP)):
            if (ny, nx) != ("0", "0"):
                rows.append((f"t=({ny},{nx})", row(u3=uy, u4=ux)))
    Sy, Sx = (H + 4) // 8, (W + 4) // 8
    rows.append(("t=+S unclamped", row(u3=(2 * Sy + 0.5) / (2 * Sy + 1), u4=(2 * Sx + 0.5) / (2 * Sx + 1))))
    rows += [("box top", row(u5=0.0)), ("box bottom", row(u5=TOP)), ("box left", row(u6=0.0)), ("box right", row(u6=TOP)),
             ("box corner", row(u5=TOP, u6=0.0)), ("clamp", row(u3=1.0, u4=1.0, u5=1.0, u6=1.0))]
    g = torch.Generator().manual_seed(1000 + seed)
    for i in range(4):
        rows.append((f"random{i}", torch.rand(8, generator=g).tolist()))
    return [(n, np.asarray(r, dtype=np.float32)) for n, r in rows]


def batches(rows, N: int):
    """the table as [N, 8] tensors (the last one wraps around)"""
    out = []
    for i in range(0, len(rows), N):
        pick = [rows[(i + j) % len(rows)] for j in range(N)]
        out.append(([n for n, _ in pick], torch.from_numpy(np.stack([r for _, r in pick]))))
    return out


# ------------------------------------------------------------------ data
def gauss_inputs(N, H, W, seed, Ca=7):
    """(parse [N,H,W,8] with a zero pad channel, fake, real [N,3,H,W]) Gaussian; the parse map too, so that a wrong pixel shows"""
    g = torch.Generator().manual_seed(seed)
    parse = torch.randn(N, H, W, 8, generator=g)
    parse[..., Ca:] = 0
    return parse, torch.randn(N, 3, H, W, generator=g), torch.randn(N, 3, H, W, generator=g) * 0.5 + 0.25


def int_image(N, H, W, seed):
    """integers in [-8, 8] whose per-sample sum is a multiple of 3HW / 4 (HW a multiple of 4), so that the mean is a multiple of 1/4:
    with s = 1 and k, beta powers of two every intermediate of the color transform is exact in fp32"""
    assert (H * W) % 4 == 0
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-8, 9, (N, 3, H, W), generator=g).double()
    q = 3 * H * W // 4
    for n in range(N):
        x[n, 0, 0, 0] -= float(int(x[n].sum().item()) % q)
    return x.float()


def int_values(shape, seed, lo=-64, hi=64):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def mean_ref(img: torch.Tensor) -> torch.Tensor:
    """fp32 [N]: the float64 sum of a sample over 3HW, rounded once"""
    return (img.double().sum(dim=(1, 2, 3)) / float(img[0].numel())).float()


# ------------------------------------------------------------------ restatements
def _maps(geom, H, W):
    """V [H,W] over destinations, and the (clamped) source rows / columns of every destination"""
    ty, tx, y0, y1, x0, x1 = geom
    ys, xs = torch.arange(H)[:, None], torch.arange(W)[None, :]
    sy, sx = ys + ty, xs + tx
    inside = (sy >= 0) & (sy < H) & (sx >= 0) & (sx < W)
    inbox = (ys >= y0) & (ys < y1) & (xs >= x0) & (xs < x1)
    return inside & ~inbox, sy.clamp(0, H - 1).expand(H, W), sx.clamp(0, W - 1).expand(H, W)


def valid_map(urow, flags, H, W) -> torch.Tensor:
    return _maps(decode(urow, flags, H, W)[1], H, W)[0]


def forward_ref(parse: torch.Tensor, Ca: int, img: torch.Tensor, u: torch.Tensor, flags: int, mean=None) -> torch.Tensor:
    """float64 [N,H,W,12].  ``mean``: the per-sample image means the color term uses (None: the float64 mean of ``img``,
    differentiable).  Masked destinations are SELECTED to zero: a NaN behind them does not show."""
    N, _, H, W = img.shape
    img64, out = img.double(), []
    for n in range(N):
        (beta, s, k), geom = decode(u[n].numpy(), flags, H, W)
        V, sy, sx = _maps(geom, H, W)
        x = img64[n][:, sy, sx]                                   # [3,H,W] gathered
        if flags & COLOR:
            kd, sd, M = float(k), float(s), (img64[n].mean() if mean is None else mean[n].double())
            x = kd * sd * x + kd * (1.0 - sd) * x.mean(dim=0, keepdim=True) + (1.0 - kd) * M + float(beta)
        pad = torch.zeros(H, W, 12 - Ca - 3, dtype=torch.float64)
        row = torch.cat((parse[n].double()[sy, sx][..., :Ca], x.permute(1, 2, 0), pad), dim=2)
        out.append(torch.where(V[..., None], row, torch.zeros((), dtype=torch.float64)))
    return torch.stack(out)


def forward_bound(Ca: int, img: torch.Tensor, u: torch.Tensor, flags: int, mean: torch.Tensor) -> torch.Tensor:
    """[N,H,W,12]: 8 * 2^-24 * (k s |x| + k |1 - s| |m| + |1 - k| |M| + |beta|) on the image channels of unmasked destinations, 0
    elsewhere (and 0 everywhere without color: a pure gather).  At most 7 fp32 roundings, each of a partial result no larger than
    that sum; M comes from an fp64 accumulation."""
    N, _, H, W = img.shape
    b = torch.zeros(N, H, W, 12, dtype=torch.float64)
    if not flags & COLOR:
        return b
    for n in range(N):
        (beta, s, k), geom = decode(u[n].numpy(), flags, H, W)
        V, sy, sx = _maps(geom, H, W)
        x = img[n].double()[:, sy, sx]
        kd, sd = float(k), float(s)
        t = (kd * sd * x.abs() + kd * abs(1.0 - sd) * x.mean(dim=0, keepdim=True).abs() + abs(1.0 - kd) * abs(float(mean[n]))
             + abs(float(beta)))
        b[n, :, :, Ca:Ca + 3] = torch.where(V[..., None], 8.0 * EPS * t.permute(1, 2, 0), torch.zeros((), dtype=torch.float64))
    return b


def _selected(g: torch.Tensor, Ca: int, urow, flags, H, W):
    V, _, _ = _maps(decode(urow, flags, H, W)[1], H, W)
    return torch.where(V[..., None], g[..., Ca:Ca + 3].double(), torch.zeros((), dtype=torch.float64))      # [H,W,3]


def gsum_ref(g: torch.Tensor, Ca: int, u: torch.Tensor, flags: int) -> torch.Tensor:
    """float64 [N]: the selected gradient summed over destinations and the three image channels"""
    N, H, W, _ = g.shape
    return torch.stack([_selected(g[n], Ca, u[n].numpy(), flags, H, W).sum() for n in range(N)])


def _backward_terms(g, Ca, u, flags):
    N, H, W, _ = g.shape
    for n in range(N):
        (beta, s, k), geom = decode(u[n].numpy(), flags, H, W)
        ty, tx = geom[0], geom[1]
        G = _selected(g[n], Ca, u[n].numpy(), flags, H, W)
        ys, xs = torch.arange(H)[:, None], torch.arange(W)[None, :]
        dy, dx = ys - ty, xs - tx
        inside = ((dy >= 0) & (dy < H) & (dx >= 0) & (dx < W))[..., None]
        Gd = torch.where(inside, G[dy.clamp(0, H - 1).expand(H, W), dx.clamp(0, W - 1).expand(H, W)], torch.zeros((), dtype=torch.float64))
        kd, sd = float(k), float(s)
        yield n, Gd.permute(2, 0, 1), G.sum(), kd, sd


def backward_ref(g: torch.Tensor, Ca: int, u: torch.Tensor, flags: int) -> torch.Tensor:
    """float64 [N,3,H,W]: d_img[c, y', x'] = k s G_c(dst) + (k (1 - s) / 3) sum_c' G_c'(dst) + ((1 - k) / (3 H W)) sum G"""
    N, H, W, _ = g.shape
    out = torch.zeros(N, 3, H, W, dtype=torch.float64)
    for n, Gd, S, kd, sd in _backward_terms(g, Ca, u, flags):
        out[n] = Gd
        if flags & COLOR:
            out[n] = kd * sd * Gd + (kd * (1.0 - sd) / 3.0) * Gd.sum(dim=0, keepdim=True) + ((1.0 - kd) / (3.0 * H * W)) * S
    return out


def backward_bound(g: torch.Tensor, Ca: int, u: torch.Tensor, flags: int) -> torch.Tensor:
    """the forward's bound on the backward's own terms; 0 without color"""
    N, H, W, _ = g.shape
    b = torch.zeros(N, 3, H, W, dtype=torch.float64)
    if not flags & COLOR:
        return b
    for n, Gd, S, kd, sd in _backward_terms(g, Ca, u, flags):
        b[n] = 8.0 * EPS * (kd * sd * Gd.abs() + (kd * abs(1.0 - sd) / 3.0) * Gd.sum(dim=0, keepdim=True).abs()
                            + (abs(1.0 - kd) / (3.0 * H * W)) * abs(float(S)))
    return b
