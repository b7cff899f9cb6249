"""Exact-operand cases for the sampling family: the fused flow warp and its adjoint (csrc/sample.hip flow_warp_kernel, csrc/
cond_train.hip flow_warp_bwd_kernel / flow_warp_dsrc_tiled_kernel), grid_sample with an explicit grid and its backward, the bilinear
and nearest resizes and their adjoints (resize_bilinear_kernel, resize_bwd_kernel<4> / <1>, the resize_nearest_nhwc kernels, glue.hip
resize_planes_kernel).  Shared by tests/test_sample_exact_cases_cpu.py (the conditions, proved on the references alone) and tests/
test_gpu_sample_exact.py (the kernels against these references).  Needs no GPU and imports nothing of the project.

The references are float64 and written from the formulas: torch's area_pixel_compute_source_index (align_corners=False), the legacy
nearest index min(floor(dst * scale), in - 1) with a float scale, and grid_sample(bilinear, border, align_corners=False) with
clip_coordinates_set_grad (the coordinate gradient is zero where the unclamped position is <= 0 or >= size - 1).  The resizes are
matrices (out = Ry x Rx^T, adjoint = Ry^T dy Rx), the sampler is a gather with an index_add scatter as its adjoint.

WHY THE COMPARISONS ARE torch.equal
  * torch.linspace(-1, 1, n) has the step 2 / (n - 1), a power of two for n = 2^k + 1 (17, 33).  With such an output extent, a
    power-of-two normaliser and a dyadic flow, gx = fx / norm + lin, ix = ((gx + 1) * W - 1) / 2 for ANY integer W, the clamps, the
    floor, the four weights and their products are the same numbers in fp32 and float64 (every intermediate is a dyadic number of
    far fewer than 24 bits).  `coords` / `taps` below take the dtype as an argument; the CPU test runs them in both and compares
    bit for bit.  Exact border hits ix == 0 / ix == W - 1 need a power-of-two W (ix = 0 <=> (gx + 1) * W = 1), so the cases that
    place them sample a 32x16 or 16x32 source; there the flow is solved from the wanted position: gx = (2 ix + 1) / W - 1.
  * With integer source and gradient values every product and every partial sum of the forward, of d_src and of d_flow is a
    multiple of one dyadic step; while sum |term| stays at or below 2^22 steps (`bound`), fp32 holds every partial sum exactly in
    ANY order of addition -- per pixel, LDS-privatised, atomics.  The d_flow epilogue gix * mx * (W / 2) / norm stays dyadic.
  * grid_sample with an explicit grid: grid values are multiples of 2^-6, so ix is a multiple of 2^-7 for any W.
  * Bilinear resizes at a ratio whose fp32 source positions equal the float64 ones (x2, x4, x8, /2, and every pair of the sweep
    for which every fp32 tap weight is the float64 one) are exact for integer data; `resize_is_exact` decides it from the two
    sets of taps and the same 2^22 rule (1 -> 13 is not exact: both taps meet on the one pixel and l0 + l1 rounds).  The nearest resizes are selections and sums of selected integers: always exact.

DERIVED BOUNDS (u = 2^-24; a rounding of a value of magnitude <= M costs at most M * u)
  * warp on contract (an even output extent: the base grid is not dyadic).  lin = 1 - step * k costs 3 u (step, product, sum);
    gx = fx / norm + lin costs G u and gx + 1 costs (G + 1) u with G = max |gx|; the product with W costs (G + 1) W u, the - 1
    another (G + 1) W u; the halving is exact.  delta = ((2 G + 4) W u + 2 (G + 1) W u) / 2  (`warp_delta`).  Clamps are
    1-Lipschitz.  Bilinear interpolation is continuous across cells, so a floor that flips costs nothing extra, and
    |out32 - out64| <= delta_x * Lx + delta_y * Ly + 8 u * max |src|, where Lx, Ly are the largest differences of adjacent source
    pixels in the 5x5 block of pixels around the sample's cell (a superset of the 3x3 cells around it) and 8 u covers the
    roundings of the four products and their sum (`interp_bound`).
  * bilinear resize off the dyadic ratios.  s = r * (dst + 0.5) - 0.5: r costs in * u (it multiplies at most out ~ in / r), the
    product and the difference in * u each, l0 = 1 - l1 another u: delta = (3 in + 1) u (`resize_delta`).  The forward is bounded
    like the warp.  The adjoint sums dy over a support: every weight moves by at most delta (the hat function is 1-Lipschitz, a
    flipped floor included), so with B the 0/1 support |s - i| <= 1,
    |d dx| <= delta_y B_y^T |dy| R_x + delta_x R_y^T |dy| B_x + delta_y delta_x B_y^T |dy| B_x + (K + 2) u R_y^T |dy| R_x + u |old|
    with K the number of support terms of the element (`resize_adjoint_bound`).
  Largest fraction of a bound that the fp32 restatement uses over the cases (tests/test_sample_exact_cases_cpu.py asserts <= 0.5
  and prints them): warp on contract 0.16, resize forward 0.26, resize adjoint 0.28.
  The kernels on gfx950 (printed by tests/test_gpu_sample_exact.py): 0.16, 0.25, 0.22.

CHANNEL PADDING THAT IS WRITTEN: the Act entry points run over Cp = C rounded up to 4 channels, so channels [C, Cp) of an output
slice are written.  Every Act of these cases has C % 4 == 0, so there is no such padding here and everything outside a slice must
keep its poison."""
from collections import namedtuple
from functools import lru_cache

import torch

F64, F32 = torch.float64, torch.float32
U = 2.0 ** -24
LIMIT = 2 ** 22
WT, WB, WCH = 16, 24, 16            # output tile edge, source window edge, channels per block of the LDS-privatised scatter


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def ints(g, shape, lo, hi):
    """integers in [lo, hi] as float64"""
    return torch.randint(lo, hi + 1, shape, generator=g).to(F64)


# ---------------------------------------------------------------------------------------------------------------
# comparison functions (the GPU test and the fault-injection test use these, nothing else)
# ---------------------------------------------------------------------------------------------------------------
def check_equal(got, want, what):
    got, want = got.detach().cpu().to(F64), want.to(F64)
    assert got.shape == want.shape, f"{what}: shape {tuple(got.shape)} != {tuple(want.shape)}"
    bad = got != want
    if bool(bad.any()):
        k = torch.nonzero(bad)[0].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ, first at {k}: "
                             f"{got[tuple(k)].item()!r} != {want[tuple(k)].item()!r}")


def check_bounded(got, want, bnd, what):
    """|got - want| <= bnd element by element -> the largest |error| / bound (0 / 0 counts as 0)"""
    got, want = got.detach().cpu().to(F64), want.to(F64)
    assert got.shape == want.shape, f"{what}: shape {tuple(got.shape)} != {tuple(want.shape)}"
    bnd = bnd.to(F64).expand_as(want)
    err = (got - want).abs()
    bad = ~(err <= bnd)                                   # (a NaN fails)
    if bool(bad.any()):
        k = torch.nonzero(bad)[0].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements out of bound, first at {k}: |error| "
                             f"{err[tuple(k)].item():.3e} > {bnd[tuple(k)].item():.3e}")
    frac = torch.where(bnd > 0, err / bnd.clamp_min(1e-300), torch.zeros_like(err))
    return float(frac.max()) if frac.numel() else 0.0


def check_outside(wide_after, wide_before, coff, C, what):
    """everything outside channels [coff, coff + C) is bit-identical to before"""
    m = torch.ones(wide_before.shape[-1], dtype=torch.bool)
    m[coff:coff + C] = False
    a, b = wide_after.detach().cpu()[..., m], wide_before.detach().cpu()[..., m]
    assert torch.equal(a, b), f"{what}: {int((a != b).sum())} elements outside the slice changed"


# ---------------------------------------------------------------------------------------------------------------
# the 2^22 rule
# ---------------------------------------------------------------------------------------------------------------
def finest_step(*tensors):
    """the largest 2^-k of which every element of every tensor is an integer multiple"""
    k = 0
    for t in tensors:
        t = t.to(F64).reshape(-1)
        t = t[t != 0]
        while t.numel() and bool((torch.round(t * 2.0 ** k) != t * 2.0 ** k).any()):
            k += 1
            assert k <= 60, "operand is not dyadic"
    return 2.0 ** -k


def units(abs_sum, step):
    """the largest sum |term| in steps"""
    return float(abs_sum.max()) / step if abs_sum.numel() else 0.0


def bound(parts, what):
    """``parts``: {name: (sum |term| per output element, step)}.  Asserts the 2^22 rule for each -> {name: units}"""
    res = {}
    for name, (s, step) in parts.items():
        res[name] = units(s, step)
        assert res[name] <= LIMIT, f"{what} {name}: {res[name]:.3g} steps of {step} exceed 2^22"
    return res


# ---------------------------------------------------------------------------------------------------------------
# the sampler: grid_sample(bilinear, border, align_corners=False) at un-normalised positions
# ---------------------------------------------------------------------------------------------------------------
def linspace_m1_1(n, dtype):
    """torch.linspace(-1, 1, n): first half from the start, second half from the end (the same in both dtypes)"""
    i = torch.arange(n, dtype=dtype)
    step = torch.tensor(2.0, dtype=dtype) / torch.tensor(float(max(n - 1, 1)), dtype=dtype) if n > 1 else torch.tensor(0.0, dtype=dtype)
    return torch.where(i < n // 2, -1.0 + step * i, 1.0 - step * (n - 1 - i))


def unnormalise(g, size, dtype):
    return ((g.to(dtype) + 1.0) * float(size) - 1.0) / 2.0


def coords(flow_up, H, W, norm_x, norm_y, dtype):
    """flow_up [N, Ho, Wo, 2] -> (ix, iy) [N, Ho, Wo] before the clamp: base grid + normalised flow, un-normalised"""
    f = flow_up.to(dtype)
    Ho, Wo = f.shape[1], f.shape[2]
    gx = f[..., 0] / norm_x + linspace_m1_1(Wo, dtype)[None, None, :]
    gy = f[..., 1] / norm_y + linspace_m1_1(Ho, dtype)[None, :, None]
    return unnormalise(gx, W, dtype), unnormalise(gy, H, dtype)


Taps = namedtuple("Taps", "ix iy x0 y0 wx0 wx1 wy0 wy1 vx1 vy1 mx my")


def taps(ix, iy, H, W, strict_mask=False):
    """clamp to the border, floor, weights; mx / my: clip_coordinates_set_grad.  ``strict_mask``: the injected fault < / > for <= / >="""
    if strict_mask:
        mx = ((ix >= 0) & (ix <= W - 1)).to(ix.dtype)
        my = ((iy >= 0) & (iy <= H - 1)).to(iy.dtype)
    else:
        mx = ((ix > 0) & (ix < W - 1)).to(ix.dtype)
        my = ((iy > 0) & (iy < H - 1)).to(iy.dtype)
    cx, cy = ix.clamp(0, W - 1), iy.clamp(0, H - 1)
    x0f, y0f = torch.floor(cx), torch.floor(cy)
    x0, y0 = x0f.long(), y0f.long()
    return Taps(cx, cy, x0, y0, (x0f + 1.0) - cx, cx - x0f, (y0f + 1.0) - cy, cy - y0f, x0 + 1 < W, y0 + 1 < H, mx, my)


def same_taps(a, b):
    """every field of the fp32 taps equals the float64 one bit for bit"""
    return all(torch.equal(x.to(F64), y.to(F64)) for x, y in zip(a, b))


def _four(t):
    """the four taps: (dy, dx, weight, valid)"""
    one = torch.ones_like(t.vx1)
    return [(0, 0, t.wx0 * t.wy0, one), (0, 1, t.wx1 * t.wy0, t.vx1), (1, 0, t.wx0 * t.wy1, t.vy1), (1, 1, t.wx1 * t.wy1, t.vx1 & t.vy1)]


def _gather(src, n_idx, y, x):
    return src[n_idx, y, x]                     # [N, Ho, Wo, C]


def sample(src, t, dout=None, old_dsrc=None, drop_tap=None, absolute=False):
    """src [N, H, W, C] float64, t: Taps (any dtype: the weights are taken to float64) -> dict(out, dsrc, gix, giy).  ``drop_tap``
    (0..3): the injected fault.  ``absolute``: sums of |term| instead (for `bound`)."""
    N, H, W, Cc = src.shape
    n_idx = torch.arange(N)[:, None, None].expand_as(t.x0)
    A = (lambda v: v.abs()) if absolute else (lambda v: v)
    out = torch.zeros(t.x0.shape + (Cc,), dtype=F64)
    vals = []
    for k, (dy, dx, w, ok) in enumerate(_four(t)):
        y, x = (t.y0 + dy).clamp_max(H - 1), (t.x0 + dx).clamp_max(W - 1)
        v = _gather(src, n_idx, y, x) * ok[..., None].to(F64)
        vals.append(v)
        if k != drop_tap:
            out += A(v) * w.to(F64)[..., None]
    res = {"out": out}
    if dout is None:
        return res
    dsrc = torch.zeros(N * H * W, Cc, dtype=F64) if old_dsrc is None else A(old_dsrc.to(F64)).reshape(N * H * W, Cc).clone()
    for k, (dy, dx, w, ok) in enumerate(_four(t)):
        if k == drop_tap:
            continue
        y, x = (t.y0 + dy).clamp_max(H - 1), (t.x0 + dx).clamp_max(W - 1)
        flat = ((n_idx * H + y) * W + x).reshape(-1)
        dsrc.index_add_(0, flat, (A(dout) * (w.to(F64) * ok.to(F64))[..., None]).reshape(-1, Cc))
    v00, v01, v10, v11 = vals
    wx0, wx1, wy0, wy1 = (q.to(F64)[..., None] for q in (t.wx0, t.wx1, t.wy0, t.wy1))
    if absolute:
        tx = (v01.abs() + v00.abs()) * wy0 + (v11.abs() + v10.abs()) * wy1
        ty = (v10.abs() + v00.abs()) * wx0 + (v11.abs() + v01.abs()) * wx1
    else:
        tx = (v01 - v00) * wy0 + (v11 - v10) * wy1
        ty = (v10 - v00) * wx0 + (v11 - v01) * wx1
    res.update(dsrc=dsrc.view(N, H, W, Cc), gix=(A(dout) * tx).sum(-1), giy=(A(dout) * ty).sum(-1))
    return res


def warp_reference(src, flow_up, norm_x, norm_y, dout=None, old_dsrc=None, old_dflow=None, dtype=F64, **fault):
    """the warp at a given flow_up and its adjoint.  dflow [N, Ho, Wo, 2] = gi * mask * (size / 2) / norm (+ old)"""
    N, H, W, _ = src.shape
    t = taps(*coords(flow_up, H, W, norm_x, norm_y, dtype), H, W, strict_mask=fault.get("strict_mask", False))
    r = sample(src, t, dout, old_dsrc, drop_tap=fault.get("drop_tap"))
    if dout is not None:
        d = torch.stack([r["gix"] * t.mx.to(F64) * (W * 0.5) / norm_x, r["giy"] * t.my.to(F64) * (H * 0.5) / norm_y], -1)
        r["dflow"] = d if old_dflow is None else d + old_dflow.to(F64)
    r["taps"] = t
    return r


def warp_bound(src, flow_up, norm_x, norm_y, dout, old_dsrc, old_dflow, what):
    """the 2^22 rule for every sum of an exact warp case"""
    N, H, W, _ = src.shape
    t = taps(*coords(flow_up, H, W, norm_x, norm_y, F64), H, W)
    a = sample(src, t, dout, old_dsrc, absolute=True)
    w_step = finest_step(*[w for _, _, w, _ in _four(t)], old_dsrc if old_dsrc is not None else torch.zeros(1))
    g_step = finest_step(t.wx0, t.wx1, t.wy0, t.wy1)
    dfx, dfy = a["gix"] * (W * 0.5) / norm_x, a["giy"] * (H * 0.5) / norm_y
    old = torch.zeros(1) if old_dflow is None else old_dflow.abs()
    f_step = min(g_step * finest_step(torch.tensor([W * 0.5 / norm_x, H * 0.5 / norm_y])), finest_step(old))
    return bound({"out": (a["out"], w_step), "dsrc": (a["dsrc"], w_step), "gi": (torch.maximum(a["gix"], a["giy"]), g_step),
                  "dflow": (torch.maximum(dfx, dfy) + old.max(), f_step)}, what)


# ---------------------------------------------------------------------------------------------------------------
# the LDS-privatised scatter, as the kernel documents it: 16x16 output tiles, a 24x24 source window around the bounding box of the
# tile's taps (the +1 taps count wherever they are in range, whatever their weight), direct adds for a tile that does not fit
# ---------------------------------------------------------------------------------------------------------------
Tile = namedtuple("Tile", "n ty tx x_lo x_hi y_lo y_hi fits live")


def tiles(t):
    N, Ho, Wo = t.x0.shape
    res = []
    for n in range(N):
        for ty in range(-(-Ho // WT)):
            for tx in range(-(-Wo // WT)):
                ys, xs = slice(ty * WT, min(Ho, ty * WT + WT)), slice(tx * WT, min(Wo, tx * WT + WT))
                x0, y0 = t.x0[n, ys, xs], t.y0[n, ys, xs]
                x1, y1 = x0 + t.vx1[n, ys, xs].long(), y0 + t.vy1[n, ys, xs].long()
                b = (int(x0.min()), int(x1.max()), int(y0.min()), int(y1.max()))
                res.append(Tile(n, ty, tx, *b, b[1] - b[0] < WB and b[3] - b[2] < WB, x0.numel()))
    return res


def tiled_dsrc_model(H, W, t, dout, old_dsrc, fault=None):
    """d_src by tiles and windows, in float64 from the taps given.  Faults: "cell" (`fits` decided with <= so that a 25-cell box
    is taken into a 24-cell window row: its last column lands on the next row's first cell), "flush_row" (the flush stops one
    window row early)"""
    N, Ho, Wo = t.x0.shape
    Cc = dout.shape[-1]
    dsrc = old_dsrc.to(F64).clone()
    four = _four(t)
    cells = WB * WB + 1                                   # one plane of the window per channel, an odd stride between planes
    for tl in tiles(t):
        ys, xs = slice(tl.ty * WT, min(Ho, tl.ty * WT + WT)), slice(tl.tx * WT, min(Wo, tl.tx * WT + WT))
        dx_, dy_ = tl.x_hi - tl.x_lo, tl.y_hi - tl.y_lo
        fits = (dx_ <= WB and dy_ <= WB) if fault == "cell" else tl.fits
        for c0 in range(0, Cc, WCH):
            nch = min(WCH, Cc - c0)
            plane = torch.arange(nch) * cells
            win = torch.zeros((nch + 2) * cells, dtype=F64)          # (a cell past its plane lands in the next channel's)
            for dy, dx, w, ok in four:
                y, x = t.y0[tl.n, ys, xs] + dy, t.x0[tl.n, ys, xs] + dx
                term = (dout[tl.n, ys, xs, c0:c0 + nch] * (w[tl.n, ys, xs].to(F64) * ok[tl.n, ys, xs].to(F64))[..., None]).reshape(-1, nch)
                keep = ok[tl.n, ys, xs].reshape(-1)
                y, x = y.reshape(-1)[keep], x.reshape(-1)[keep]
                if fits:
                    win.index_add_(0, (((y - tl.y_lo) * WB + (x - tl.x_lo))[:, None] + plane[None, :]).reshape(-1), term[keep].reshape(-1))
                else:
                    dsrc[tl.n].view(H * W, Cc)[:, c0:c0 + nch].index_add_(0, y * W + x, term[keep])
            if fits:
                wh = dy_ + 1 - (1 if fault == "flush_row" else 0)
                for cy in range(wh):
                    for cx in range(dx_ + 1):
                        dsrc[tl.n, tl.y_lo + cy, tl.x_lo + cx, c0:c0 + nch] += win[plane + cy * WB + cx]
    return dsrc


# ---------------------------------------------------------------------------------------------------------------
# group 1: warp adjoint, exact
# ---------------------------------------------------------------------------------------------------------------
Geom = namedtuple("Geom", "Ho Wo H W norm_x norm_y")
G_TALL = Geom(33, 17, 32, 16, 4.0, 8.0)         # power-of-two source: positions are placed; the long axis (32) is y
G_WIDE = Geom(17, 33, 16, 32, 8.0, 4.0)         # the long axis is x
G_OTHER = Geom(17, 33, 33, 24, 4.0, 8.0)        # source of another, non-power-of-two extent
G_SAME = Geom(33, 17, 33, 17, 2.0, 4.0)         # source extent == output extent

WarpCase = namedtuple("WarpCase", "name geom pattern C N")
WARP_BWD_CASES = (
    [WarpCase(f"tall-{p}-c16", G_TALL, p, 16, 2 if p == "corner" else 1) for p in ("smooth", "spread", "bb23", "bb24", "corner", "edges")]
    + [WarpCase(f"wide-{p}-c16", G_WIDE, p, 16, 1) for p in ("spread", "bb23", "bb24", "edges")]
    + [WarpCase(f"tall-edges-c{c}", G_TALL, "edges", c, 1) for c in (4, 12, 24, 40, 68)]
    + [WarpCase(f"tall-spread-c{c}", G_TALL, "spread", c, 1) for c in (24, 40, 68)]
    + [WarpCase("other-quarters-c4", G_OTHER, "quarters", 4, 2), WarpCase("other-quarters-c40", G_OTHER, "quarters", 40, 1),
       WarpCase("same-quarters-c12", G_SAME, "quarters", 12, 1), WarpCase("same-quarters-c16", G_SAME, "quarters", 16, 2)])


def _positions(pattern, g, n):
    """wanted (ix, iy) [Ho, Wo] before the clamp, multiples of 1/32, for a power-of-two source.  ``long``: the 32-pixel axis."""
    Ho, Wo, H, W = g.Ho, g.Wo, g.H, g.W
    ho, wo = torch.arange(Ho, dtype=F64)[:, None].expand(Ho, Wo), torch.arange(Wo, dtype=F64)[None, :].expand(Ho, Wo)
    ix, iy = wo * (W - 1) / (Wo - 1), ho * (H - 1) / (Ho - 1)          # 15/16 or 31/32 of the output index: every tile fits
    if pattern == "smooth":
        return ix + 0.0, iy + 0.0
    long_y = H > W
    pos, k = (iy, ho) if long_y else (ix, wo)
    pos = pos.clone()
    first = k < WT                                                       # the tiles of the first row / column of tiles
    if pattern == "spread":                                              # tile 0 spans 31 source pixels, its neighbours fit
        pos[first] = (2.0 * k)[first] + 0.5
    elif pattern in ("bb23", "bb24"):                                    # floor 2 .. 24, +1 tap at 25: difference 23
        pos[first] = (2.0 + 1.5 * k)[first]
        if pattern == "bb24":                                            # lane 15: floor 25, +1 tap at 26: difference 24
            pos[k == WT - 1] = 25.5
    elif pattern == "corner":
        return (torch.full_like(ix, -5.0), torch.full_like(iy, -3.0)) if n == 0 else (torch.full_like(ix, W + 4.0), torch.full_like(iy, H + 2.5))
    elif pattern == "edges":
        ix, iy = ix + 0.125, iy + 0.25
        iy = iy.clone()
        ix = ix.clone()
        iy[0], iy[1], iy[2], iy[3] = 0.0, H - 1.0, -2.0, H + 1.0
        for r in range(4, 10):
            iy[r] = float(r * 3 % (H - 2) + 1)                            # interior integers
        ix[:, 0], ix[:, 1], ix[:, 2], ix[:, 3] = 0.0, W - 1.0, -1.5, W + 0.25
        for c in range(4, 7):
            ix[:, c] = float(c * 5 % (W - 2) + 1)
        return ix.clamp(-4, W + 3), iy.clamp(-4, H + 3)
    else:
        raise ValueError(pattern)
    return (ix, pos) if long_y else (pos, iy)


@lru_cache(maxsize=None)
def warp_bwd_case(name):
    """operands (float64, CPU) of one case: src, flow_up, dout, old_dsrc, old_dflow -- integers except the flow"""
    c = next(x for x in WARP_BWD_CASES if x.name == name)
    g, seed = c.geom, sum(map(ord, name))
    rnd = _gen(seed)
    if c.pattern == "quarters":                 # the flow itself: multiples of 1/4, one in eight far outside
        f = ints(rnd, (c.N, g.Ho, g.Wo, 2), -24, 24) / 4.0
        far = torch.randint(0, 8, (c.N, g.Ho, g.Wo, 2), generator=rnd) == 0
        flow = torch.where(far, f * 8.0, f)
    else:
        fl = []
        for n in range(c.N):
            ix, iy = _positions(c.pattern, g, n)
            gx, gy = (2.0 * ix + 1.0) / g.W - 1.0, (2.0 * iy + 1.0) / g.H - 1.0
            fl.append(torch.stack([(gx - linspace_m1_1(g.Wo, F64)[None, :]) * g.norm_x, (gy - linspace_m1_1(g.Ho, F64)[:, None]) * g.norm_y], -1))
        flow = torch.stack(fl)
    dlim = 1 if c.pattern == "corner" else 2    # 561 samples pile up on one cell
    return dict(case=c, src=ints(rnd, (c.N, g.H, g.W, c.C), -8, 8), flow_up=flow, dout=ints(rnd, (c.N, g.Ho, g.Wo, c.C), -dlim, dlim),
                old_dsrc=ints(rnd, (c.N, g.H, g.W, c.C), -4, 4), old_dflow=ints(rnd, (c.N, g.Ho, g.Wo, 2), -4, 4))


def warp_case_taps(d, dtype=F64):
    g = d["case"].geom
    return taps(*coords(d["flow_up"], g.H, g.W, g.norm_x, g.norm_y, dtype), g.H, g.W)


def edge_census(ix, iy, H, W):
    """counts over unclamped positions: the four exact borders, interior integers per axis, strictly interior samples"""
    inx, iny = (ix > 0) & (ix < W - 1), (iy > 0) & (iy < H - 1)
    return dict(total=ix.numel(), x_lo=int((ix == 0).sum()), x_hi=int((ix == W - 1).sum()), y_lo=int((iy == 0).sum()),
                y_hi=int((iy == H - 1).sum()), x_int=int((inx & (ix == ix.round())).sum()), y_int=int((iny & (iy == iy.round())).sum()),
                interior=int((inx & iny).sum()))


def add_census(a, b):
    return {k: a[k] + b[k] for k in a}


# ---------------------------------------------------------------------------------------------------------------
# the resizes as matrices
# ---------------------------------------------------------------------------------------------------------------
def bilinear_taps(out_size, in_size, ratio, dtype=F64):
    """(i0, i1, l0, l1, s) of area_pixel_compute_source_index (align_corners=False), evaluated in ``dtype``.  i1 == i0 at the far
    border and wherever in == 1: the two weights then meet on one pixel, each with its own rounding"""
    r = torch.tensor(ratio, dtype=dtype)
    s = (r * (torch.arange(out_size, dtype=dtype) + 0.5) - 0.5).clamp_min(0)
    i0 = s.long().clamp_max(in_size - 1)
    i1 = i0 + (i0 < in_size - 1).long()
    l1 = (s - i0.to(dtype)).clamp(0, 1)
    return i0, i1, 1.0 - l1, l1, s


def same_bilinear_taps(out_size, in_size, ratio):
    """the fp32 taps and weights equal the float64 ones bit for bit"""
    return all(torch.equal(a.to(F64), b.to(F64)) for a, b in zip(bilinear_taps(out_size, in_size, ratio, F32)[:4],
                                                                 bilinear_taps(out_size, in_size, ratio, F64)[:4]))


def bilinear_matrix(out_size, in_size, ratio, dtype=F64, with_pos=False):
    """R [out, in] of those taps, returned in float64"""
    i0, i1, l0, l1, s = bilinear_taps(out_size, in_size, ratio, dtype)
    R = torch.zeros(out_size, in_size, dtype=F64)
    o = torch.arange(out_size)
    R.index_put_((o, i0), l0.to(F64), accumulate=True)
    R.index_put_((o, i1), l1.to(F64), accumulate=True)
    return (R, s.to(F64)) if with_pos else R


def nearest_matrix(out_size, in_size):
    """S [out, in]: legacy nearest, min(floor(dst * scale), in - 1) with scale = (float) in / out"""
    scale = torch.tensor(float(in_size), dtype=F32) / torch.tensor(float(out_size), dtype=F32)
    idx = torch.floor(torch.arange(out_size, dtype=F32) * scale).long().clamp_max(in_size - 1)
    S = torch.zeros(out_size, in_size, dtype=F64)
    S[torch.arange(out_size), idx] = 1.0
    return S


def resize_fwd(x, Ry, Rx):
    """x [N, H, W, C] -> [N, Ho, Wo, C]"""
    return torch.einsum("oi,nijc,qj->noqc", Ry, x.to(F64), Rx)


def resize_adj(dy, Ry, Rx):
    """dy [N, Ho, Wo, C] -> [N, H, W, C]"""
    return torch.einsum("oi,noqc,qj->nijc", Ry, dy.to(F64), Rx)


def resize_delta(in_size):
    return (3 * in_size + 1) * U


def support(out_size, in_size, ratio):
    """B [out, in]: |s - i| <= 1, where a weight may be non-zero in either arithmetic"""
    _, s = bilinear_matrix(out_size, in_size, ratio, with_pos=True)
    return ((s[:, None] - torch.arange(in_size, dtype=F64)[None, :]).abs() <= 1.0).to(F64)


def resize_is_exact(Ho, H, rh, Wo, W, rw, abs_terms, adjoint):
    """every fp32 tap weight equals the float64 one (tap by tap, not merged into the matrix: where both taps meet on one pixel the sum
    l0 + l1 is rounded in fp32), and sum |term| (``abs_terms``: [N, H, W, C], or [N, Ho, Wo, C] of the adjoint) obeys the 2^22 rule"""
    if not (same_bilinear_taps(Ho, H, rh) and same_bilinear_taps(Wo, W, rw)):
        return False
    ty, tx = bilinear_taps(Ho, H, rh), bilinear_taps(Wo, W, rw)
    step = finest_step(ty[2], ty[3]) * finest_step(tx[2], tx[3]) * finest_step(abs_terms)
    Ry, Rx = bilinear_matrix(Ho, H, rh), bilinear_matrix(Wo, W, rw)
    return units((resize_adj if adjoint else resize_fwd)(abs_terms.abs(), Ry, Rx), step) <= LIMIT


def _slopes(x):
    """largest |difference| of adjacent pixels in the 5x5 block around each pixel: (Ly, Lx) [N, H, W, C]"""
    N, H, W, Cc = x.shape
    p = x.permute(0, 3, 1, 2)
    dy_, dx_ = torch.zeros_like(p), torch.zeros_like(p)
    if H > 1:
        dy_[:, :, :-1] = (p[:, :, 1:] - p[:, :, :-1]).abs()
    if W > 1:
        dx_[:, :, :, :-1] = (p[:, :, :, 1:] - p[:, :, :, :-1]).abs()
    pool = lambda t: torch.nn.functional.max_pool2d(t, 5, 1, 2).permute(0, 2, 3, 1)
    return pool(dy_), pool(dx_)


def interp_bound(x, y0, x0, delta_y, delta_x):
    """|out32 - out64| of a bilinear interpolation of x [N, H, W, C] at positions with floor (y0, x0) [N, Ho, Wo], each coordinate
    off by at most delta"""
    Ly, Lx = _slopes(x.to(F64))
    n_idx = torch.arange(x.shape[0])[:, None, None].expand_as(y0)
    return delta_y * Ly[n_idx, y0, x0] + delta_x * Lx[n_idx, y0, x0] + 8 * U * float(x.abs().max())


def resize_fwd_bound(x, Ho, Wo, rh, rw, addend=None):
    N, H, W, _ = x.shape
    _, sy = bilinear_matrix(Ho, H, rh, with_pos=True)
    _, sx = bilinear_matrix(Wo, W, rw, with_pos=True)
    y0 = sy.long().clamp_max(H - 1)[None, :, None].expand(N, Ho, Wo)
    x0 = sx.long().clamp_max(W - 1)[None, None, :].expand(N, Ho, Wo)
    b = interp_bound(x, y0, x0, resize_delta(H), resize_delta(W))
    return b if addend is None else b + U * (float(x.abs().max()) + addend.abs().to(F64))


def resize_adjoint_bound(dy, H, W, rh, rw, old=None):
    N, Ho, Wo, _ = dy.shape
    Ry, Rx, By, Bx = bilinear_matrix(Ho, H, rh), bilinear_matrix(Wo, W, rw), support(Ho, H, rh), support(Wo, W, rw)
    a, dly, dlx = dy.abs().to(F64), resize_delta(H), resize_delta(W)
    K = By.sum(0)[:, None] * Bx.sum(0)[None, :]
    b = (dly * resize_adj(a, By, Rx) + dlx * resize_adj(a, Ry, Bx) + dly * dlx * resize_adj(a, By, Bx)
         + (K[None, :, :, None] + 2) * U * resize_adj(a, Ry, Rx))
    return b if old is None else b + U * (old.abs().to(F64) + resize_adj(a, Ry, Rx))


def out_range_f32(i, in_size, out_size, r):
    """the candidate range the gather adjoint documents: outputs o with src(o) in (i - 1, i + 1), one of slack on either side, in
    fp32; everything from 0 for i == 0 and up to out - 1 for i >= in - 1"""
    r = torch.tensor(r, dtype=F32)
    a = (torch.tensor(float(i), dtype=F32) - 0.5) / r - 0.5
    b = (torch.tensor(float(i), dtype=F32) + 1.5) / r - 0.5
    lo, hi = int(torch.floor(a)) - 1, int(torch.ceil(b)) + 1
    if i == 0:
        lo = 0
    if i >= in_size - 1:
        hi = out_size - 1
    return max(lo, 0), min(hi, out_size - 1)


def gather_matrix(out_size, in_size, ratio, fault=None):
    """R^T restricted to each input's candidate range, weights in fp32 -> [out, in].  Faults: "lo" / "hi" shorten the range by one"""
    R = bilinear_matrix(out_size, in_size, ratio, F32).clone()
    for i in range(in_size):
        lo, hi = out_range_f32(i, in_size, out_size, ratio)
        lo, hi = lo + (fault == "lo"), hi - (fault == "hi")
        R[:lo, i] = 0
        R[hi + 1:, i] = 0
    return R


INS, OUTS = (1, 2, 3, 5, 8, 12), (1, 2, 3, 4, 7, 13, 24, 33, 96)
SIZE_PAIRS = [(i, o, i / o) for i in INS for o in OUTS]
SCALED_PAIRS = [(2, 3, 1 / 1.5), (8, 12, 1 / 1.5), (12, 18, 1 / 1.5), (2, 5, 1 / 2.5), (8, 20, 1 / 2.5)]     # ratio = 1 / scale_factor
ALL_PAIRS = SIZE_PAIRS + SCALED_PAIRS
DYADIC_PAIRS = [(5, 10, 0.5), (3, 12, 0.25), (2, 16, 0.125), (12, 6, 2.0), (3, 24, 0.125), (8, 4, 2.0)]          # x2, x4, x8, /2


def sweep():
    """[(pair in H, pair in W)]: every pair once on each axis, different pairs on the two axes of a launch"""
    n = len(ALL_PAIRS)
    return [(ALL_PAIRS[k], ALL_PAIRS[(k * 7 + 5) % n]) for k in range(n)]


def dyadic_sweep():
    n = len(DYADIC_PAIRS)
    return [(DYADIC_PAIRS[k], DYADIC_PAIRS[(k + 1 + k % 2) % n]) for k in range(n)]


@lru_cache(maxsize=None)
def resize_case(hp, wp, C, N=2):
    """integer operands of one size pair: x, addend (forward), dy, old (adjoint)"""
    (H, Ho, _), (W, Wo, _) = hp, wp
    g = _gen(H * 1009 + Ho * 31 + W * 7 + Wo + C)
    return dict(x=ints(g, (N, H, W, C), -8, 8), addend=ints(g, (N, Ho, Wo, C), -8, 8), dy=ints(g, (N, Ho, Wo, C), -2, 2),
                old=ints(g, (N, H, W, C), -4, 4))


# ---------------------------------------------------------------------------------------------------------------
# groups 2 and 3: warp forward through the x2 flow up-sampling (rh = rw = 0.5)
# ---------------------------------------------------------------------------------------------------------------
FwdCase = namedtuple("FwdCase", "name Ho Wo fh fw H W C norm_x norm_y N")
WARP_FWD_EXACT = [FwdCase("33x17-from-32x16", 33, 17, 17, 9, 32, 16, 8, 4.0, 8.0, 2), FwdCase("17x33-from-33x24", 17, 33, 9, 17, 33, 24, 4, 4.0, 4.0, 1),
                  FwdCase("33x33-from-17x33", 33, 33, 17, 17, 17, 33, 12, 8.0, 2.0, 1)]
WARP_FWD_CONTRACT = [FwdCase("32x24-from-32x24", 32, 24, 16, 12, 32, 24, 8, 4.0, 8.0, 2), FwdCase("16x48-from-17x40", 16, 48, 8, 24, 17, 40, 4, 8.0, 4.0, 1)]


@lru_cache(maxsize=None)
def warp_fwd_case(c):
    g = _gen(c.Ho * 100 + c.Wo)
    flow = ints(g, (c.N, c.fh, c.fw, 2), -6, 6) / 2.0
    src = ints(g, (c.N, c.H, c.W, c.C), -8, 8)
    fup = resize_fwd(flow, bilinear_matrix(c.Ho, c.fh, 0.5), bilinear_matrix(c.Wo, c.fw, 0.5))
    return dict(flow=flow, src=src, flow_up=fup, ref=warp_reference(src, fup, c.norm_x, c.norm_y))


def warp_delta(flow_up, size, norm):
    G = float(flow_up.abs().max()) / norm + 1.0
    return ((2 * G + 4) * size * U + 2 * (G + 1) * size * U) / 2


def warp_fwd_bound(c, d):
    t = d["ref"]["taps"]
    return interp_bound(d["src"], t.y0, t.x0, warp_delta(d["flow_up"][..., 1], c.H, c.norm_y), warp_delta(d["flow_up"][..., 0], c.W, c.norm_x))


# ---------------------------------------------------------------------------------------------------------------
# group 4: grid_sample with an explicit grid (NCHW)
# ---------------------------------------------------------------------------------------------------------------
GridCase = namedtuple("GridCase", "name N C H W Ho Wo placed")
GRID_CASES = [GridCase("13x7-to-9x11-c3", 2, 3, 13, 7, 9, 11, False), GridCase("8x8-to-17x5-c1", 1, 1, 8, 8, 17, 5, True),
              GridCase("8x8-to-17x5-c4", 2, 4, 8, 8, 17, 5, True)]


@lru_cache(maxsize=None)
def grid_case(c):
    """inp [N, C, H, W], grid [N, Ho, Wo, 2] (multiples of 2^-6), dout [N, C, Ho, Wo]; the float64 reference with it"""
    g = _gen(c.H * 10 + c.C)
    if c.placed:                                   # a power-of-two source: positions by the flat index of the sample
        k = torch.arange(c.N * c.Ho * c.Wo).view(c.N, c.Ho, c.Wo)
        ix = ints(g, (c.N, c.Ho, c.Wo), 1, 8 * (c.W - 1) - 1) / 8.0
        iy = ints(g, (c.N, c.Ho, c.Wo), 1, 8 * (c.H - 1) - 1) / 8.0
        sel = k % 10
        ix = torch.where(sel == 0, torch.zeros_like(ix), ix)
        ix = torch.where(sel == 1, torch.full_like(ix, c.W - 1.0), ix)
        iy = torch.where(sel == 2, torch.zeros_like(iy), iy)
        iy = torch.where(sel == 3, torch.full_like(iy, c.H - 1.0), iy)
        ix = torch.where(sel == 4, (k // 10 % (c.W - 2) + 1).to(F64), ix)
        iy = torch.where(sel == 5, (k // 10 % (c.H - 2) + 1).to(F64), iy)
        ix = torch.where(sel == 6, torch.where(k % 20 == 6, torch.full_like(ix, -1.25), torch.full_like(ix, c.W + 0.5)), ix)
        iy = torch.where(sel == 6, torch.where(k % 20 == 6, torch.full_like(iy, c.H + 2.0), torch.full_like(iy, -0.75)), iy)
        grid = torch.stack([(2 * ix + 1) / c.W - 1, (2 * iy + 1) / c.H - 1], -1)
    else:
        grid = ints(g, (c.N, c.Ho, c.Wo, 2), -80, 80) / 64.0      # one in five beyond the border
    inp, dout = ints(g, (c.N, c.C, c.H, c.W), -8, 8), ints(g, (c.N, c.C, c.Ho, c.Wo), -2, 2)
    return dict(inp=inp, grid=grid, dout=dout, ref=grid_reference(inp, grid, dout))


def grid_taps(c, grid, dtype=F64):
    return taps(unnormalise(grid[..., 0], c.W, dtype), unnormalise(grid[..., 1], c.H, dtype), c.H, c.W)


def grid_reference(inp, grid, dout, dtype=F64, **fault):
    N, Cc, H, W = inp.shape
    t = taps(unnormalise(grid[..., 0], W, dtype), unnormalise(grid[..., 1], H, dtype), H, W, strict_mask=fault.get("strict_mask", False))
    r = sample(inp.permute(0, 2, 3, 1), t, dout.permute(0, 2, 3, 1), drop_tap=fault.get("drop_tap"))
    return dict(out=r["out"].permute(0, 3, 1, 2), din=r["dsrc"].permute(0, 3, 1, 2),
                dgrid=torch.stack([r["gix"] * t.mx.to(F64) * (W * 0.5), r["giy"] * t.my.to(F64) * (H * 0.5)], -1), taps=t)


def grid_bound(c, d):
    t = grid_taps(c, d["grid"])
    a = sample(d["inp"].permute(0, 2, 3, 1), t, d["dout"].permute(0, 2, 3, 1), absolute=True)
    w_step, g_step = finest_step(*[w for _, _, w, _ in _four(t)]), finest_step(t.wx0, t.wx1, t.wy0, t.wy1)
    return bound({"out": (a["out"], w_step), "din": (a["dsrc"], w_step),
                  "dgrid": (torch.maximum(a["gix"] * c.W * 0.5, a["giy"] * c.H * 0.5), g_step * 0.5)}, c.name)
