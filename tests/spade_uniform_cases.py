"""Cases and the pure-Python reference of the SPADE tile classifier (csrc/spade_tiles.hip); needs no GPU.  Shared by
tests/test_spade_tiles_cpu.py (the rule itself, on the reference alone) and tests/test_gpu_spade_uniform.py (the kernel's lists
against the reference; the fused forward with the tile plan against the forward without it).

The rule.  Level image H x W, label map [N, H << shift, W << shift, 8] bf16, 16x16-pixel tiles in the order of patch_tiles(N, H, W)
(image, tile row, tile column).  A tile is LIGHT with class k when
  * its 20x20 patch (the tile + the 2-pixel halo of the two stacked 3x3s) lies wholly inside the H x W image,
  * the 400 sampled label vectors (y << shift, x << shift) are bitwise equal, and
  * that vector is channel k = bf16 1.0 (0x3F80), every other channel all-zero bits.
Every other tile is heavy.  Of the light tiles of each class the lowest-numbered one is its REPRESENTATIVE: it goes to the heavy
list with the flag (k + 1) << 24.  Both lists ascend; together they hold every tile once."""
from functools import lru_cache

import torch

import exact_cases as E

ONE = 0x3F80          # bf16 1.0

# (H, W, seg_shift): N = 2 everywhere
SHAPES = [(64, 48, 0), (72, 56, 0), (64, 48, 1)]
MAPS = ["one_class", "edge2", "edge3", "multihot", "speckle", "random"]


def bits(seg_bf16):
    """bf16 [N, Hs, Ws, 8] -> its 16-bit patterns as int64"""
    return seg_bf16.contiguous().view(torch.int16).to(torch.int64) & 0xFFFF


def classify(seg_bf16, shift, N, H, W):
    """The reference.  Returns dict(cls=[class or -1 per tile], heavy=[entries], light=[entries], rep=[tile or -1] * 8)."""
    b = bits(seg_bf16)[:, ::(1 << shift), ::(1 << shift), :]
    assert tuple(b.shape) == (N, H, W, 8), (b.shape, N, H, W)
    ty, tx = (H + 15) // 16, (W + 15) // 16
    cls = []
    for n in range(N):
        for r in range(ty):
            for c in range(tx):
                y0, x0 = 16 * r, 16 * c
                k = -1
                if y0 >= 2 and x0 >= 2 and y0 + 18 <= H and x0 + 18 <= W:
                    p = b[n, y0 - 2:y0 + 18, x0 - 2:x0 + 18, :].reshape(400, 8)
                    v = p[0]
                    if bool((p == v).all()):
                        ones = [e for e in range(8) if int(v[e]) == ONE]
                        if len(ones) == 1 and all(int(v[e]) == 0 for e in range(8) if e != ones[0]):
                            k = ones[0]
                cls.append(k)
    rep = [-1] * 8
    for t, k in enumerate(cls):
        if k >= 0 and rep[k] < 0:
            rep[k] = t
    heavy, light = [], []
    for t, k in enumerate(cls):
        if k < 0:
            heavy.append(t)
        elif rep[k] == t:
            heavy.append(t | ((k + 1) << 24))
        else:
            light.append(t | (k << 24))
    return dict(cls=cls, heavy=heavy, light=light, rep=rep)


def tile_index(N, H, W, n, y0, x0):
    ty, tx = (H + 15) // 16, (W + 15) // 16
    return (n * ty + y0 // 16) * tx + x0 // 16


def _onehot(labels):
    """int64 [N, H, W] -> bf16 [N, H, W, 8] one-hot"""
    return torch.nn.functional.one_hot(labels, 8).to(torch.bfloat16)


@lru_cache(maxsize=None)
def label_map(name, H, W, shift):
    """bf16 [2, H << shift, W << shift, 8].  Built on the LEVEL grid and repeated (1 << shift)-fold, so the sampled pixels are the
    level's; "speckle" then changes full-resolution pixels at odd coordinates only (never sampled when shift > 0).

    Image 0 is class 1 throughout in every map but "random": its first interior tile, (16, 16), is the representative of class 1, so
    a class-1 tile of image 1 that the rule leaves light is ON the light list."""
    g = torch.Generator().manual_seed(1000 + 7 * H + W + shift)
    lab = torch.ones(2, H, W, dtype=torch.int64)
    f = 1 << shift
    if name == "one_class":
        lab[1] = 3                              # two classes that both have light tiles
    elif name == "edge2":
        lab[1, 33:, :] = 2                      # tile (16, 16): rows 16..31, patch rows 14..33 -- row 33 is 2 pixels outside: heavy
    elif name == "edge3":
        lab[1, 34:, :] = 2                      # row 34 is 3 pixels outside the tile and outside its patch: light
    elif name == "random":
        lab = torch.randint(0, 7, (2, H, W), generator=g)
    seg = _onehot(lab)
    if name == "multihot":
        seg[1, :40, :, 2] = 1.0                 # uniform two-hot tiles (channels 1 and 2) in the upper part of image 1 ...
        seg[1, 40:, :, 1] = 2.0                 # ... uniform value-2.0 tiles below (72 x 56: tiles (48, 16) and (48, 32))
    seg = seg.repeat_interleave(f, 1).repeat_interleave(f, 2).contiguous()
    if name == "speckle":
        sp = torch.rand(2, (H << shift) // 2, (W << shift) // 2, generator=g) < 0.3
        odd = seg[:, 1::2, 1::2, :]
        odd[sp] = _onehot(torch.tensor(2))      # class 2 at odd full-resolution coordinates
    return seg


# ---------------------------------------------------------------------------------------------------------------
# the forward: (H, W, shift, map, C).  C = 32: bf16 x (NTP 2); 64: fp32 x (NTP 4); 80: x = cat(up2(lo 64), hi 16) (NTP 5 with tail)
# ---------------------------------------------------------------------------------------------------------------
WIDTHS = [32, 64, 80]
FORWARD = [(H, W, s, m, C) for (H, W, s) in SHAPES for m in MAPS for C in WIDTHS]
# more tiles (2 x 17 x 16 = 544) than the blocks the fused kernel keeps resident (two per CU): a block walks several entries of
# the heavy list -- below that count every block gets one (tile, pass) unit
WRAP = [(272, 256, 0, "one_class", 64), (272, 256, 0, "edge3", 80)]


@lru_cache(maxsize=None)
def weights(C):
    g = torch.Generator().manual_seed(4242 + C)
    r = lambda *s: torch.randn(*s, generator=g)      # noqa: E731
    return dict(wsh=r(128, 7, 3, 3) * 0.3, bsh=r(128) * 0.1, wg=r(C, 128, 3, 3) * 0.05, wb=r(C, 128, 3, 3) * 0.05, bg=r(C) * 0.1, bb=r(C) * 0.1,
                ns=r(C) * 0.2)


@lru_cache(maxsize=None)
def inputs(H, W, C):
    """x (N = 2; C = 80: the (lo, hi) pair of the up-sampled source), z [N, W, H, 1], mean / rstd [N, C]"""
    g = torch.Generator().manual_seed(99 + 3 * H + W + C)
    r = lambda *s: torch.randn(*s, generator=g)      # noqa: E731
    x = (r(2, H // 2, W // 2, 64), r(2, H, W, 16)) if C == 80 else r(2, H, W, C)
    return dict(x=x, z=r(2, W, H, 1), mean=r(2, C) * 0.1, rstd=torch.rand(2, C, generator=g) + 0.5)


# ---------------------------------------------------------------------------------------------------------------
# exact-integer form (exact_cases.py: integer operands, float64 reference, torch.equal) of two of the cases:
# (H, W, shift, map, C, rstd, noise, act, save)
# ---------------------------------------------------------------------------------------------------------------
EXACT = [(72, 56, 0, "one_class", 64, 1.0, True, "lrelu", True), (64, 48, 1, "edge3", 32, 2.0, False, None, True)]


@lru_cache(maxsize=None)
def exact(case):
    H, W, shift, name, C_, rstd, noise, act, save = case
    N = 2
    g = E._gen(C_, H, W, shift, int(rstd), 14)
    seg = label_map(name, H, W, shift).to(torch.float32)
    wsh, bsh = E.int_tensor((128, 7, 3, 3), -3, 3, g), E.int_tensor((128,), -4, 4, g)
    wg, wb = E.int_tensor((C_, 128, 3, 3), -1, 1, g), E.int_tensor((C_, 128, 3, 3), -1, 1, g)
    bg, bb = E._bias(C_, g), E._bias(C_, g)
    s = seg[:, ::(1 << shift), ::(1 << shift), :7]
    amax = E.bound(9, 1, 3, 4)                   # a one-hot map: one channel per tap
    actv = E.to_bf16_rne(E.ref_conv64(s, wsh, bsh, act="relu")).to(torch.float64)
    gam, bet = E.ref_conv64(actv, wg, bg), E.ref_conv64(actv, wb, bb)
    x, z, ns, out, xmax = E._modulate(N, H, W, C_, rstd, noise, act, gam, bet, g, 1, 1)
    gmax = E.bound(9 * 128, amax, 1, E.BIAS0 + 8)
    want = {"out": out}
    if save:
        want.update(g1p=1 + gam, actv=actv)
    return dict(seg=seg, wsh=wsh, bsh=bsh, wg=wg, wb=wb, bg=bg, bb=bb, x=x, z=z, ns=ns, want=want,
                bound=E.bound(1, (1 + (1 if noise else 0)) * rstd, 1 + gmax, gmax))


def case_id(case):
    return "-".join(str(v) for v in case)
