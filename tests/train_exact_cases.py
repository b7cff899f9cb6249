"""Exact cases for the HBM-bound training kernels that carry a reduction, a routing decision or an edge rule: the losses, the
pools, the 2x2 down-sum and add_slice of csrc/train.hip, and the BatchNorm training kernels, channel softmax, 2-D cross entropy
and flow TV of csrc/cond_train.hip.  Shared by tests/test_train_exact_cases_cpu.py (the conditions the comparisons rest on, proved
on the references alone) and tests/test_gpu_train_exact.py (the kernels against these references).  Pure CPU torch / numpy;
imports nothing of the project.

The principle (the one of exact_cases.py and norm_exact_cases.py).  Operands are small integers, or small multiples of 1/2 or
1/4.  The per-channel mean / rstd / scale of the BatchNorm backward are supplied by the test: mean dyadic, rstd a power of two,
pad channels zero.  Every term a kernel sums is then a multiple of one granule 2^-k, and while sum |term| stays at or below 2^22
granules an fp32 accumulator holds every partial sum exactly, in ANY order (``bound`` asserts it per case): block shape,
unrolling, partial rows, grid-stride trips and fma contraction cannot change a bit.  So

  * outputs that are exact are compared with torch.equal; bf16-stored outputs with round-to-nearest-even of the exact value, on
    the bit pattern (odd integers in [256, 512) are exact ties);
  * the references are written from the formulas in the kernels' header comments, not from autograd (torch splits the gradient
    0.5 / 0.5 at a hinge tie; the documented rule is g = [x > -1] and g = -[x < 1]; a max pool hands the whole gradient to the
    FIRST maximum in the order (0,0), (0,1), (1,0), (1,1));
  * what cannot be exact -- dx of the BatchNorm backward (s / M is not dyadic), the outputs of bn_finalize (a double finalize,
    rounded once), the TV gradient and loss (1 / count is not dyadic) -- is held to a bound derived from the roundings of its
    formula, never to a measured tolerance.

What this pins is the VALUE of each output.  It does not pin the order of any sum, the block counts, the caps, or which of the
vector and scalar paths serves an element: the geometry mirrors below exist so that the CPU test can show that the tables reach
every path of the kernels as they are, not to constrain them.

Seeded defects (``defect=`` of the references): variants of the references that restate one plausible kernel fault each; the CPU
test shows that every one of them changes the expected output of at least one case of its family."""
from collections import namedtuple
from functools import lru_cache

import numpy as np
import torch

from exact_cases import _gen, int_tensor, tie_share, to_bf16_rne  # noqa: F401  (re-exported for the two tests)

LIMIT = 2 ** 22
U = 2.0 ** -24            # half an ulp of fp32, relative
NAN = float("nan")
POISON = 1.5e4            # exact in bf16 and fp32; marks everything around an operand slice


def bound(terms, granule=1.0, extra=0.0, dims=None):
    """sum |term| (over ``dims``; everything by default) + ``extra``, in granules: asserts that every term is a multiple of
    the granule and that the sum stays at or below LIMIT, and returns the largest sum."""
    t = terms.double() / granule
    assert bool((t == t.round()).all()), "a term is not a multiple of its granule"
    s = t.abs().sum() if dims is None else t.abs().sum(dims)
    b = float(torch.as_tensor(s).max()) + abs(extra) / granule
    assert b <= LIMIT, (b, LIMIT)
    return b


def f32(v):
    """a Python float rounded to fp32 (what a float argument of the C ABI carries), widened again"""
    return float(np.float32(v))


def within_one_ulp(got32, ref64):
    """bool per element: got is the float64 value rounded to fp32, or one of that value's two fp32 neighbours"""
    r = ref64.to(torch.float32)
    inf = torch.full_like(r, float("inf"))
    return (got32 == r) | (got32 == torch.nextafter(r, inf)) | (got32 == torch.nextafter(r, -inf))


def trunc_bf16(t64):
    """float64 -> bf16 by dropping the low 16 bits of the fp32 pattern (the seeded defect of a bf16 store)"""
    f = t64.to(torch.float32).contiguous()
    return ((f.view(torch.int32) >> 16).to(torch.int16)).view(torch.bfloat16)


def store_bf16(t64, defect=None):
    return trunc_bf16(t64) if defect == "trunc_bf16" else to_bf16_rne(t64)


def bits(t):
    """integer view for bit-pattern comparisons (bf16 -> int16, fp32 -> int32)"""
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


# ---------------------------------------------------------------------------------------------------------------
# losses (loss_kernel<AB> + loss_final_kernel): loss = lscale * sum l, grad = gscale * dl/da
#   0 L1 |a-b|, g = sign(a-b) ; 1 max(1+a, 0), g = [a > -1] ; 2 max(1-a, 0), g = -[a < 1] ; 3 -a, g = -1 ; 4 (a-b)^2, g = 2 (a-b)
#   RELU_MASK: a = ReLU(pre), g = 0 where not a > 0 ; GRAD_BF16: the gradient is stored as bf16
# ---------------------------------------------------------------------------------------------------------------
L1, HINGE_FAKE, HINGE_REAL, NEG_MEAN, MSE = 0, 1, 2, 3, 4
RELU_MASK, GRAD_BF16 = 16, 32
LOSS_BLOCK, LOSS_BLOCK_CAP = 256, 1024
LOSS_N = [1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 262143, 262144, 262145, 1048575, 1048576, 1048577, 1048583,
          2 * 1048576 + 7]
LOSS0 = 37.0              # the old value of loss_out where a variant accumulates

LossVariant = namedtuple("LossVariant", "mode relu bf16 shift with_b want_grad accumulate lscale gscale grad_bf16")
LossGeo = namedtuple("LossGeo", "nb vec one_pass vec_trips tail_start tail_trips")


def loss_vec(v):
    """the entry points' ``vec``: every operand pointer 16-byte (fp32) / 8-byte (bf16) aligned.  The operands are views
    buf[s : s + n] of an aligned buffer, s the shift in elements, so one element of shift takes the scalar path"""
    return int(v.shift[0] == 0 and (v.shift[1] == 0 or not v.with_b))


def loss_geometry(n, vec):
    """mirror of the launch: nb blocks of 256 threads; ``one_pass`` elements per trip of the grid on the path that serves the
    bulk, the trips of the 4-element loop, where the scalar tail loop starts and how many trips it takes"""
    nb = min(-(-n // LOSS_BLOCK), LOSS_BLOCK_CAP)
    per = nb * LOSS_BLOCK
    n4 = n // 4 if vec else 0
    return LossGeo(nb, vec, per * 4 if vec else per, -(-n4 // per), 4 * n4, -(-(n - 4 * n4) // per))


def loss_variants(n):
    """every mode x storage type on the 16-byte path and on one shifted view (a, b, or both, rotating), b=None on every other
    variant of the modes that take none, and want_grad / accumulate / the two scales rotating; then the ReLU mask"""
    k = LOSS_N.index(n)
    out = []
    for mode in range(5):
        for bf in (False, True):
            for shift in ((0, 0), [(1, 0), (0, 1), (1, 1)][k % 3]):
                with_b = mode in (L1, MSE) or k % 2 == 0
                out.append(LossVariant(mode, False, bf, shift, with_b, k % 5 != 4, k % 3 == 1, 2.0 ** (k % 4 - 2), 2.0 ** (k % 3 - 1), False))
                k += 1
    for mode in (L1, MSE, NEG_MEAN):
        for bf in (False, True):
            shift = [(0, 0), (1, 0), (0, 1), (1, 1)][k % 4]
            out.append(LossVariant(mode, True, bf, shift, mode != NEG_MEAN, True, k % 2 == 0, 2.0 ** (k % 4 - 2), 2.0 ** (k % 3 - 1), False))
            k += 1
    return out


def loss_kind(v):
    return "relu" if v.relu else ("diff" if v.mode in (L1, MSE) else "hinge")


@lru_cache(maxsize=6)
def loss_operands(n, kind):
    """(a, b) fp32, integer valued (bf16 holds them too), with constructed values at a known share of the positions:
    diff: b == a at i % 7 == 0 (d == 0 for L1);  hinge: a == -1 at i % 5 == 0 and +1 at i % 5 == 1 (both kinks);
    relu: a == +0 at i % 4 == 0 and -0.0 at i % 4 == 1 (a is a ReLU output: >= +0 or -0.0)"""
    g = _gen(n, {"diff": 1, "hinge": 2, "relu": 3}[kind], 41)
    m = 3 if n <= 2 ** 18 + 1 else 1              # (the sum of the largest sizes has to stay under 2^22)
    i = torch.arange(n)
    one = torch.ones(n)
    if kind == "diff":
        a, b = int_tensor((n,), -m, m, g), int_tensor((n,), -m, m, g)
        b = torch.where(i % 7 == 0, a, b)
    elif kind == "hinge":
        a, b = int_tensor((n,), -m - 1, m + 1, g), int_tensor((n,), -m, m, g)
        a = torch.where(i % 5 == 0, -one, torch.where(i % 5 == 1, one, a))
    else:
        a, b = int_tensor((n,), 0, m + 1, g), int_tensor((n,), 0, m + 1, g)
        a = torch.where(i % 4 == 0, 0.0 * one, torch.where(i % 4 == 1, -0.0 * one, a))
    return a, b


def loss_ref(a, b, v, defect=None, dtype=torch.float64):
    """-> dict(loss [1] (the value of loss_out afterwards), grad [n] or None, terms [n]).  ``dtype`` float32: the fp32
    restatement (same formulas, torch's own summation order)"""
    n = a.numel()
    x = a.to(dtype)
    y = b.to(dtype) if (b is not None and v.with_b) else torch.zeros(n, dtype=dtype)
    if v.mode == L1:
        d = x - y
        l, g = d.abs(), torch.sign(d)
    elif v.mode == HINGE_FAKE:
        l, g = (1 + x).clamp_min(0), ((x >= -1) if defect == "hinge_ge" else (x > -1)).to(dtype)
    elif v.mode == HINGE_REAL:
        l, g = (1 - x).clamp_min(0), -((x <= 1) if defect == "hinge_ge" else (x < 1)).to(dtype)
    elif v.mode == NEG_MEAN:
        l, g = -x, -torch.ones(n, dtype=dtype)
    else:
        d = x - y
        l, g = d * d, 2 * d
    g = g * v.gscale
    if v.relu:
        g = torch.where((x >= 0) if defect == "relu_ge" else (x > 0), g, torch.zeros_like(g))
    keep = torch.ones(n, dtype=torch.bool)
    if defect == "drop_tail":
        keep[n - 1] = False
    one_pass = loss_geometry(n, loss_vec(v)).one_pass
    if defect == "skip_second_trip" and n > one_pass:
        keep[one_pass] = False
    old = LOSS0 if (v.accumulate and defect != "ignore_accumulate") else 0.0
    loss = (v.lscale * torch.where(keep, l, torch.zeros_like(l)).sum() + old).reshape(1)
    grad = None
    if v.want_grad:
        grad = torch.where(keep, g, torch.full_like(g, NAN))      # (an element the kernel skips keeps the NaN it was handed)
        if v.grad_bf16:
            grad = torch.where(keep, store_bf16(g.double(), defect), torch.full((n,), NAN, dtype=torch.bfloat16))
    return dict(loss=loss, grad=grad, terms=l)


def loss_bound(a, b, v):
    r = loss_ref(a, b, v)
    return bound(r["terms"], 1.0, LOSS0 / v.lscale if v.accumulate else 0.0)


# the bf16 gradient: only MSE produces a value that rounds.  a even in [256, 320], b odd in [-63, -1] (bf16 holds both): d = a - b odd
# in [257, 383], gscale = 0.5: g = d, an exact tie.  "dense": every position; "sparse": every 64th, the others in [-1, 1] (the sum
# of d^2 has to stay under 2^22: 24 dense elements, or 16 among 1024).  n % 4 == 0 (the wrapper drops grad_bf16 otherwise).
LOSS_BF16_GRAD = [(4, "dense"), (12, "dense"), (24, "dense"), (1024, "sparse")]
LOSS_BF16_GRAD_VARIANTS = [LossVariant(MSE, False, True, s, True, True, acc, ls, 0.5, True)
                           for s, acc, ls in (((0, 0), False, 0.25), ((1, 0), True, 1.0))]


@lru_cache(maxsize=None)
def loss_bf16_grad_operands(n, kind):
    g = _gen(n, 43)
    a = 256.0 + 2.0 * int_tensor((n,), 0, 32, g)
    b = -(2.0 * int_tensor((n,), 0, 31, g) + 1.0)
    if kind == "sparse":
        tie = torch.arange(n) % 64 == 0
        a, b = torch.where(tie, a, int_tensor((n,), -1, 1, g)), torch.where(tie, b, int_tensor((n,), -1, 1, g))
    assert torch.equal(a.bfloat16().float(), a) and torch.equal(b.bfloat16().float(), b)
    return a, b


# ---------------------------------------------------------------------------------------------------------------
# 2x2 max pool: windows constructed by pattern
# ---------------------------------------------------------------------------------------------------------------
GRID_CAP = 4096 * 256     # threads of the capped grid of the per-channel-group kernels: more groups than this take a second trip
PATTERNS = ["all_equal", "pair01", "pair02", "pair03", "pair12", "pair13", "pair23", "max0", "max1", "max2", "max3",
            "zeros", "neg_zeros", "mixed_zeros", "negzero_pos", "random", "negative"]
_MAXPOS = [(0, 1, 2, 3), (0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3), (0,), (1,), (2,), (3,)]


def to_windows(x):
    """[N, 2Ho, 2Wo, C] -> [N, Ho, Wo, 4, C], position 2 * dy + dx: the scan order (0,0), (0,1), (1,0), (1,1)"""
    N, H, W, C = x.shape
    return x.reshape(N, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(N, H // 2, W // 2, 4, C)


def from_windows(w):
    N, Ho, Wo, _, C = w.shape
    return w.reshape(N, Ho, Wo, 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(N, 2 * Ho, 2 * Wo, C)


@lru_cache(maxsize=None)
def pool_case(N, H, W, C, negative):
    """x [N, H, W, C] (integers in [-6, 6] and -0.0: fp32 and bf16 hold them), the pattern of every (window, channel), and dy
    [N, H/2, W/2, C]: non-zero integers, so that a gradient that goes to the wrong position shows.  ``negative``: with the
    all-negative windows a bf16-stored or ReLU-gated x cannot have"""
    g = _gen(N, H, W, C, 51 + int(negative))
    Ho, Wo = H // 2, W // 2
    P = len(PATTERNS) if negative else len(PATTERNS) - 1
    pat = ((torch.arange(N * Ho * Wo * C) * 7 + 3) % P).view(N, Ho, Wo, 1, C)        # every pattern at a share of 1 / P
    ishi = torch.zeros(len(PATTERNS), 4, dtype=torch.bool)
    for p, pos in enumerate(_MAXPOS):
        ishi[p, list(pos)] = True
    hi = int_tensor((N, Ho, Wo, 1, C), 2, 6, g).expand(N, Ho, Wo, 4, C)
    low = int_tensor((N, Ho, Wo, 4, C), 0, 1, g)
    w = torch.where(ishi[pat.squeeze(3)].permute(0, 1, 2, 4, 3), hi, low)
    pos = torch.arange(4).view(1, 1, 1, 4, 1)
    zero, negz = torch.zeros(()), -torch.zeros(())
    name = PATTERNS.index
    w = torch.where(pat == name("zeros"), zero, w)
    w = torch.where(pat == name("neg_zeros"), negz, w)
    w = torch.where(pat == name("mixed_zeros"), torch.where((pos == 0) | (pos == 3), negz, zero), w)
    w = torch.where((pat == name("negzero_pos")) & (pos % 2 == 0), negz, torch.where((pat == name("negzero_pos")) & (pos == 1), hi, w))
    w = torch.where(pat == name("random"), int_tensor((N, Ho, Wo, 4, C), 0, 6, g), w)
    if negative:
        w = torch.where(pat == name("negative"), int_tensor((N, Ho, Wo, 4, C), -6, -1, g), w)
    dy = int_tensor((N, Ho, Wo, C), 1, 64, g) * (2 * int_tensor((N, Ho, Wo, C), 0, 1, g) - 1)
    return dict(x=from_windows(w).contiguous(), pat=pat.squeeze(3), dy=dy)


def maxpool_ref(x):
    return to_windows(x).double().max(3).values


def maxpool_bwd_ref(x, dy, relu, defect=None):
    """dx [N, H, W, C] float64: the first maximum of a window in scan order takes dy, the other three are written as 0;
    ``relu``: nothing passes a window whose maximum is not > 0"""
    w = to_windows(x).double()
    m = w.max(3, keepdim=True).values
    eq = w == m                                                    # (-0.0 == +0.0, as in the kernel's float compare)
    if defect == "last_max":
        take = eq & (eq.flip(3).cumsum(3).flip(3) == 1)
    else:
        take = eq & (eq.cumsum(3) == 1)
    if relu:
        take = take & ((m >= 0) if defect == "gate_ge" else (m > 0))
    return from_windows(torch.where(take, dy.double().unsqueeze(3), torch.zeros(())))


# (entry point, x bf16, dy / dx bf16, relu)
MAXPOOL_BWD_ENTRIES = [("hrv_maxpool2x2_bwd_nhwc_f32", False, False, False), ("hrv_maxpool2x2_bwd_relu_nhwc_f32", False, False, True),
                       ("hrv_maxpool2x2_bwd_relu_nhwc_xbf16", True, False, True), ("hrv_maxpool2x2_bwd_relu_nhwc_bf16", True, True, True)]
POOL_SHAPES = {False: [(1, 2, 2, 4), (2, 6, 10, 12)], True: [(1, 2, 2, 8), (2, 6, 10, 16)]}     # by "x is bf16": (N, H, W, C)
# the second grid-stride trip: a tile (N, H, W, C) repeated (rh, rw) times on the device; the reference is the tile's, repeated
MAXPOOL_BIG = {"hrv_maxpool2x2_bwd_relu_nhwc_f32": ((1, 10, 16, 4), (205, 128)),
               "hrv_maxpool2x2_bwd_relu_nhwc_bf16": ((1, 38, 16, 8), (27, 128))}


def groups(N, H, W, C):
    return N * H * W * (C // 4)


# ---------------------------------------------------------------------------------------------------------------
# avg_pool2d(3, s2, p1, count_include_pad=False) backward, 2x2 down-sum, add_slice
# ---------------------------------------------------------------------------------------------------------------
# (N, H, W, C, accumulate, sliced)
AVG_CASES = [(2, h, w, 8, i % 2 == 1, i % 3 != 0) for i, (h, w) in enumerate(
    [(1, 1), (1, 2), (2, 1), (2, 2), (3, 3), (3, 4), (4, 3), (4, 5), (5, 4), (5, 7), (7, 8), (8, 7), (8, 8), (2, 3), (7, 5)])] + \
    [(1, 2, 2, 4, False, False), (2, 7, 5, 12, True, True)]
AVG_BIG = ((1, 27, 32, 4), (19, 16), (1025, 1024))       # dy tile, repeats, (H, W) of dx: 1025 * 1024 groups > GRID_CAP


def avg_out(H):
    return (H + 2 - 3) // 2 + 1


def avg_big_dy():
    return 36.0 * int_tensor(AVG_BIG[0], -8, 8, _gen(*AVG_BIG[0], 64))


@lru_cache(maxsize=None)
def avg_case(N, H, W, C, accumulate):
    g = _gen(N, H, W, C, 61)
    dy = 36.0 * int_tensor((N, avg_out(H), avg_out(W), C), -8, 8, g)      # dy / count is an integer for count 1, 2, 3, 4, 6, 9
    return dict(dy=dy, dx0=int_tensor((N, H, W, C), -64, 64, g) if accumulate else None)


def avgpool_bwd_ref(dy, H, W, dx0=None, defect=None, dtype=torch.float64):
    """dx[h, w] = sum over the (<= 4) windows that contain (h, w) of dy[ho, wo] / count(ho, wo), count = the window's pixels
    inside the image"""
    N, Ho, Wo, C = dy.shape
    assert (Ho, Wo) == (avg_out(H), avg_out(W))

    def cnt(n_out, n_in):
        o = torch.arange(n_out)
        return (torch.minimum(2 * o + 1, torch.tensor(n_in - 1)) - torch.clamp(2 * o - 1, min=0) + 1).to(dtype)
    count = cnt(Ho, H).view(1, Ho, 1, 1) * cnt(Wo, W).view(1, 1, Wo, 1)
    if defect == "count9":
        count = torch.full_like(count, 9.0)
    q = dy.to(dtype) / count
    dx = torch.zeros(N, H, W, C, dtype=dtype)
    for dh in (-1, 0, 1):
        h0, h1 = (1 if dh < 0 else 0), min(Ho - 1, (H - 1 - dh) // 2)
        for dw in (-1, 0, 1):
            w0, w1 = (1 if dw < 0 else 0), min(Wo - 1, (W - 1 - dw) // 2)
            if h1 >= h0 and w1 >= w0:
                dx[:, 2 * h0 + dh:2 * h1 + dh + 1:2, 2 * w0 + dw:2 * w1 + dw + 1:2] += q[:, h0:h1 + 1, w0:w1 + 1]
    if dx0 is not None and defect != "ignore_accumulate":
        dx = dx + dx0.to(dtype)
    return dx


# (N, Hl, Wl, C, accumulate): 2 stores bf16 -- four values in [64, 127], sums in [256, 508], the odd ones exact ties
DOWNSUM_CASES = [(1, 1, 1, 4, 0), (2, 3, 5, 12, 0), (2, 3, 5, 12, 1), (1, 4, 6, 8, 1), (1, 1, 1, 8, 2), (2, 3, 5, 16, 2), (1, 4, 6, 8, 2)]


@lru_cache(maxsize=None)
def downsum_case(N, Hl, Wl, C, accumulate):
    g = _gen(N, Hl, Wl, C, accumulate, 62)
    lo, hi = (64, 127) if accumulate == 2 else (-8, 8)
    return dict(dhi=int_tensor((N, 2 * Hl, 2 * Wl, C), lo, hi, g), dlo0=int_tensor((N, Hl, Wl, C), -64, 64, g) if accumulate == 1 else None)


def downsum_ref(dhi, dlo0=None, defect=None, dtype=torch.float64):
    """dlo[n, h, w] = the sum of the 2x2 block of dhi (+ dlo0)"""
    N, H, W, C = dhi.shape
    d = dhi.to(dtype)
    if defect == "row_offset":              # the second row read one pixel to the right (flat pixel index + 1, clamped)
        flat = d.reshape(-1, C)
        sh = torch.cat([flat[1:], flat[-1:]]).view(N, H, W, C)
        s = d[:, 0::2, 0::2] + d[:, 0::2, 1::2] + sh[:, 1::2, 0::2] + sh[:, 1::2, 1::2]
    else:
        s = to_windows(d).sum(3)
    if dlo0 is not None and defect != "ignore_accumulate":
        s = s + dlo0.to(dtype)
    return s


# (N, H, W, C, bf16, accumulate): the bf16 sums a + out0 with both in [128, 255] lie in [256, 510], the odd ones exact ties
ADD_CASES = [(1, 1, 1, 4, False, False), (2, 3, 5, 12, False, True), (2, 3, 5, 12, False, False), (1, 1, 1, 8, True, True),
             (2, 3, 5, 16, True, True), (2, 3, 5, 16, True, False)]


@lru_cache(maxsize=None)
def add_case(N, H, W, C, bf16, accumulate):
    g = _gen(N, H, W, C, int(bf16), int(accumulate), 63)
    lo, hi = (128, 255) if bf16 else (-64, 64)
    return dict(a=int_tensor((N, H, W, C), lo, hi, g), out0=int_tensor((N, H, W, C), lo, hi, g))


def add_ref(a, out0, accumulate, defect=None, dtype=torch.float64):
    return a.to(dtype) + out0.to(dtype) if (accumulate and defect != "ignore_accumulate") else a.to(dtype)


# ---------------------------------------------------------------------------------------------------------------
# BatchNorm backward: s1[c] = sum dy, s2[c] = sum dy * (x - mean[c]) * rstd[c] (partial rows, then a double sum), dbeta (+)= s1,
# dgamma (+)= s2, dx (+)= scale * (dy - s1 / M - xhat * (s2 / M))
# ---------------------------------------------------------------------------------------------------------------
BN_ROWS, BN_ROW_PIXELS, BN_THREADS = 256, 1024, 256
BNCase = namedtuple("BNCase", "N H W C sliced dx_acc dgb_acc reps")        # reps: the operands are a tile of H / reps rows, repeated
BN_BWD = [BNCase(1, 1, 1, 4, False, False, False, 1), BNCase(2, 9, 10, 13, True, True, True, 1), BNCase(1, 32, 32, 12, True, False, False, 1),
          BNCase(1, 40, 50, 12, False, True, False, 1), BNCase(1, 50, 50, 12, True, False, True, 1), BNCase(1, 25, 40, 4, True, True, False, 1),
          BNCase(1, 500, 600, 4, False, False, True, 1), BNCase(2, 9, 10, 256, True, False, False, 1), BNCase(1, 5, 7, 1024, False, True, False, 1),
          BNCase(1, 3, 5, 1040, True, False, True, 1), BNCase(1, 1025, 1024, 4, False, False, False, 25)]
BNGeo = namedtuple("BNGeo", "nb PB C4 GB R idle trips last_trip blocks")


def bn_id(c):
    return f"{c.N}x{c.H}x{c.W}x{c.C}" + ("-sliced" if c.sliced else "") + ("-dxacc" if c.dx_acc else "") + ("-dgbacc" if c.dgb_acc else "")


def bn_geometry(npix, C):
    """mirror of hrv_bn_bwd_nhwc_f32 / bn_bwd_partial_kernel: nb partial rows of PB pixels, GB channel groups x R pixel rows per
    block with ``idle`` threads, ``trips`` of the g0 loop with ``last_trip`` live groups in the last one, and per block its pixel
    range with, per thread row r, (iterations of the four-chain loop, pixels left to the remainder loop)"""
    C4 = (C + 3) // 4
    nb = max(1, min(-(-npix // BN_ROW_PIXELS), BN_ROWS))
    PB = -(-npix // nb)
    GB = min(C4, BN_THREADS)
    R = BN_THREADS // GB
    blocks = []
    for b in range(nb):
        p0, p1 = b * PB, min(b * PB + PB, npix)
        rows = []
        for r in range(R):
            px, it = p0 + r, 0
            while px + 3 * R < p1:
                px, it = px + 4 * R, it + 1
            rows.append((it, max(0, -(-(p1 - px) // R))))
        blocks.append((p0, p1, rows))
    trips = -(-C4 // GB)
    return BNGeo(nb, PB, C4, GB, R, BN_THREADS - R * GB, trips, C4 - (trips - 1) * GB, blocks)


@lru_cache(maxsize=None)
def bn_case(c):
    """operands over Cp = ceil4(C) channels (the kernels read and write whole groups of 4: the pad channels of dy / x hold data
    like any other, mean / rstd / scale are zero there) and the float64 reference"""
    g = _gen(c.N, c.H, c.W, c.C, 71)
    Cp = (c.C + 3) // 4 * 4
    Ht = c.H // c.reps
    assert Ht * c.reps == c.H
    npix = c.N * c.H * c.W
    big = npix > 4096
    m = 1 if big else 4
    dy, x = int_tensor((c.N, Ht, c.W, Cp), -m, m, g), int_tensor((c.N, Ht, c.W, Cp), -m, m, g)
    live = (torch.arange(Cp) < c.C).float()
    mean = int_tensor((Cp,), -2, 2, g) * 0.5 * live
    rstd = 2.0 ** int_tensor((Cp,), -1, 0 if big else 1, g) * live
    scale = int_tensor((Cp,), -4, 4, g) * 0.5 * rstd
    d = dict(dy=dy, x=x, mean=mean, rstd=rstd, scale=scale, Cp=Cp, npix=npix,
             dx0=int_tensor((c.N, Ht, c.W, Cp), -8, 8, g) if c.dx_acc else None,
             dg0=int_tensor((c.C,), -64, 64, g) if c.dgb_acc else None, db0=int_tensor((c.C,), -64, 64, g) if c.dgb_acc else None)
    d["ref"] = bn_sums_ref(c, d)
    return d


def bn_terms(d, mean=None):
    """the two summed terms per element, float64 [pixels of the tile][Cp]"""
    Cp = d["Cp"]
    dy, x = d["dy"].double().reshape(-1, Cp), d["x"].double().reshape(-1, Cp)
    xh = (x - (d["mean"] if mean is None else mean).double()) * d["rstd"].double()
    return dy, dy * xh, xh


def bn_sums_ref(c, d, defect=None):
    """-> s1, s2 [Cp] float64 (what the workspace holds behind the partial rows), dgamma / dbeta [Cp]: NaN where the kernel must
    not write (c >= C)"""
    Cp = d["Cp"]
    mean = d["mean"]
    if defect == "g0_mean":           # the second trip of the g0 loop (channels from 4 * 256 on) reads the first trip's mean
        mean = torch.cat([mean[:1024], mean[:Cp - 1024]]) if Cp > 1024 else mean
    t1, t2, _ = bn_terms(d, mean)
    if defect == "drop_row_end":      # every partial row loses its last pixel
        assert c.reps == 1
        geo = bn_geometry(d["npix"], c.C)
        keep = torch.ones(d["npix"], dtype=torch.bool)
        keep[[p1 - 1 for _, p1, _ in geo.blocks]] = False
        t1, t2 = t1[keep], t2[keep]
    s1, s2 = t1.sum(0) * c.reps, t2.sum(0) * c.reps
    nan = torch.full((Cp,), NAN, dtype=torch.float64)
    wr = torch.arange(Cp) < (Cp if defect == "pad_leak" else c.C)
    old_g = torch.zeros(Cp, dtype=torch.float64)
    old_b = torch.zeros(Cp, dtype=torch.float64)
    if c.dgb_acc and defect != "ignore_accumulate":
        old_g[:c.C], old_b[:c.C] = d["dg0"].double(), d["db0"].double()
    return dict(s1=s1, s2=s2, dgamma=torch.where(wr, s2 + old_g, nan), dbeta=torch.where(wr, s1 + old_b, nan))


def bn_bound(c, d):
    """sum |term| per channel in granules of 1/4 (dy an integer, x - mean a multiple of 1/2, rstd >= 1/2), over all the
    repeats of the tile, with the old values"""
    t1, t2, _ = bn_terms(d)
    extra = 64.0 if c.dgb_acc else 0.0
    worst = max(bound(t1, 1.0, extra, dims=0) * c.reps, bound(t2, 0.25, extra, dims=0) * c.reps)
    assert worst <= LIMIT, (worst, LIMIT)
    return worst


def bn_dx_steps(d, dtype=torch.float64):
    """the kernel's expression sc * (d - s1 * invM - xh * (s2 * invM)) (+ old) step by step in ``dtype``, from the EXACT s1 / s2
    and the fp32 invM = 1 / (float) npix.  -> [t1, t2, p, a, b, v, out] over the tile [N, Ht, W, Cp], and the bracket
    |sc| * (|d| + |s1 invM| + |xh * s2 invM|) (float64)"""
    shape = d["dy"].shape
    dy, _, xh = bn_terms(d)
    invM = torch.tensor(float(np.float32(1.0) / np.float32(d["npix"])), dtype=dtype)
    s1, s2, sc = d["ref"]["s1"].to(dtype), d["ref"]["s2"].to(dtype), d["scale"].to(dtype)
    dy, xh = dy.to(dtype), xh.to(dtype)
    t1 = s1 * invM
    t2 = s2 * invM
    p = xh * t2
    a = dy - t1
    b = a - p
    v = sc * b
    out = v + d["dx0"].to(dtype).reshape(-1, d["Cp"]) if d["dx0"] is not None else v
    bracket = sc.double().abs() * (dy.double().abs() + (s1.double() * invM.double()).abs() + (xh.double() * s2.double() * invM.double()).abs())
    return [s.reshape(shape) for s in (t1.expand_as(dy), t2.expand_as(dy), p, a, b, v, out)], bracket.reshape(shape)


def bn_dx_bound(d):
    """2^-21 * (bracket + |old|) per element: the six roundings of the expression (s1 * invM, s2 * invM, the product with xhat,
    the two subtractions, the product with scale) and the one of the accumulation are at most half an ulp (2^-24, relative)
    each of a magnitude inside the bracket (+ |old|): seven halves of an ulp, taken as eight.  A contracted fma rounds less"""
    steps, bracket = bn_dx_steps(d)
    old = d["dx0"].double().abs() if d["dx0"] is not None else 0.0
    return steps[-1], 8 * U * (bracket + old)


def bn_dx_exact(d):
    """True where every step of the fp32 restatement equals its float64 value: the case makes dx exact (M a power of two) and a
    contracted fma cannot change it either (the unrounded product is then the rounded one)"""
    s64, _ = bn_dx_steps(d)
    s32, _ = bn_dx_steps(d, torch.float32)
    return all(torch.equal(a.double(), b) for a, b in zip(s32, s64))


def bn_dx_check(got, d, reps=1, what=""):
    """got [N, H, W, Cp] fp32 on the CPU -> worst |error| / bound"""
    ref, bnd = bn_dx_bound(d)
    if reps > 1:
        ref, bnd = ref.repeat(1, reps, 1, 1), bnd.repeat(1, reps, 1, 1)
    assert not bool(torch.isnan(got).any()), what
    err = (got.double() - ref).abs()
    ok = err <= bnd
    ratio = float((err / bnd.clamp_min(2.0 ** -60)).max())
    assert bool(ok.all()), f"{what} dx: {int((~ok).sum())} of {ok.numel()} beyond the bound, worst |error| / bound = {ratio:.3g}"
    return ratio


# ---------------------------------------------------------------------------------------------------------------
# bn_finalize: the per-sample (mean, rstd) folded over the batch in double, every output rounded once
# ---------------------------------------------------------------------------------------------------------------
# (N, C, nc_stride, HW, affine (gamma and beta), running statistics)
BN_FIN = [(1, 5, 8, 1, True, True), (1, 130, 136, 12, False, False), (2, 13, 16, 35, True, False), (2, 4, 7, 1, False, True),
          (5, 130, 131, 7, False, True), (5, 5, 8, 300, True, True)]
BN_EPS_IN, BN_EPS, BN_MOMENTUM = f32(1e-5), f32(1e-5), f32(0.1)


@lru_cache(maxsize=None)
def bn_fin_case(case):
    N, C, cs, HW, affine, running = case
    g = _gen(N, C, cs, HW, 72)
    rnd = lambda *s: torch.rand(*s, generator=g)
    d = dict(mean_nc=(rnd(N, cs) * 4 - 2), rstd_nc=0.5 + 1.5 * rnd(N, cs),
             gamma=(0.5 + rnd(C)) if affine else None, beta=(rnd(C) * 2 - 1) if affine else None,
             rm=(rnd(C) - 0.5) if running else None, rv=(0.5 + rnd(C)) if running else None)
    d["ref"] = bn_finalize_ref(case, d)
    return d


def bn_finalize_ref(case, d):
    """float64 restatement of bn_finalize_kernel's header: mean_c = avg_n mean_nc; var_c = avg_n (var_nc + mean_nc^2) - mean_c^2
    with var_nc = 1 / rstd_nc^2 - eps_in; scale = gamma * rstd, shift = beta - mean * scale; running <- (1 - momentum) * running +
    momentum * (mean | unbiased var; the biased one where N * HW == 1)"""
    N, C, cs, HW, affine, running = case
    m = d["mean_nc"][:, :C].double()
    r = d["rstd_nc"][:, :C].double()
    v = 1.0 / (r * r) - BN_EPS_IN
    mean = m.sum(0) / N
    msq = (v + m * m).sum(0) / N
    var = (msq - mean * mean).clamp_min(0.0)
    rs = 1.0 / torch.sqrt(var + BN_EPS)
    gm = d["gamma"].double() if affine else torch.ones(C, dtype=torch.float64)
    bt = d["beta"].double() if affine else torch.zeros(C, dtype=torch.float64)
    out = dict(mean=mean, rstd=rs, scale=gm * rs, shift=bt - mean * gm * rs, cancel=(mean * mean / var).max(),
               shift_cancel=((bt.abs() + (mean * gm * rs).abs()) / (bt - mean * gm * rs).abs()).max())
    if running:
        cnt = float(N) * float(HW)
        unb = var * cnt / (cnt - 1.0) if cnt > 1.0 else var
        out["rm"] = (1.0 - BN_MOMENTUM) * d["rm"].double() + BN_MOMENTUM * mean
        out["rv"] = (1.0 - BN_MOMENTUM) * d["rv"].double() + BN_MOMENTUM * unb
    return out


# ---------------------------------------------------------------------------------------------------------------
# affine_act: out = act(x * scale[c] + shift[c] (+ residual)); x, residual integers, scale halves, shift quarters: exact
# ---------------------------------------------------------------------------------------------------------------
ACT_NONE, ACT_RELU, ACT_LRELU = 0, 1, 2
# (N, H, W, C, act, residual, slope): the BatchNorm path uses ACT_NONE and ACT_RELU, with and without the residual
AFFINE_CASES = [(1, 1, 1, 4, ACT_NONE, False, 0.0), (2, 5, 7, 12, ACT_RELU, True, 0.0), (2, 5, 7, 12, ACT_RELU, False, 0.0),
                (2, 5, 7, 8, ACT_NONE, True, 0.0), (1, 3, 3, 16, ACT_LRELU, True, 0.5), (1, 33, 35, 1040, ACT_RELU, True, 0.0)]


@lru_cache(maxsize=None)
def affine_case(case):
    N, H, W, C, act, res, slope = case
    g = _gen(N, H, W, C, act, int(res), 73)
    return dict(x=int_tensor((N, H, W, C), -8, 8, g), scale=int_tensor((C,), -4, 4, g) * 0.5, shift=int_tensor((C,), -8, 8, g) * 0.25,
                res=int_tensor((N, H, W, C), -8, 8, g) if res else None)


def affine_ref(case, d, dtype=torch.float64):
    _, _, _, _, act, res, slope = case
    v = d["x"].to(dtype) * d["scale"].to(dtype) + d["shift"].to(dtype)
    if res:
        v = v + d["res"].to(dtype)
    if act == ACT_RELU:
        v = torch.where(v > 0, v, torch.zeros_like(v))
    elif act == ACT_LRELU:
        v = torch.where(v > 0, v, v * slope)
    return v


# ---------------------------------------------------------------------------------------------------------------
# cross entropy over NCHW logits: loss = mean over the valid pixels of logsumexp(x) - x[t]; grad = gscale * (softmax - onehot(t)),
# zero at ignored pixels (t outside [0, C)).  Structure: one maximal integer logit m in [-8, 8] per pixel, every other logit at
# most m - 128.  fp32 expf(t) is exactly 0 for t <= -104 (e^-104 < 2^-150, half the smallest denormal), so sum == 1, logf(1) == 0
# and the per-pixel loss is the integer m - x[t]; nothing here needs the accuracy of expf or logf.
# ---------------------------------------------------------------------------------------------------------------
EXPF_ZERO_BELOW = -104.0
IGNORE = 250
CE_BLOCKS = 512
# (N, C, H, W, all ignored)
CE_CASES = [(N, C, H, W, False) for C in (1, 2, 13, 64) for N in (1, 3) for H, W in ((1, 1), (15, 17), (1, 257))] + \
           [(3, 13, 15, 17, True), (3, 2, 1, 43691, False)]
CE_GSCALE = 0.5


@lru_cache(maxsize=None)
def ce_case(case):
    """x [N, C, H, W]; target by pixel index p: p % 8 in 0..3 the argmax, 4 another class (C > 1), 5 -> 250, 6 -> -1, 7 -> C"""
    N, C, H, W, all_ignored = case
    g = _gen(N, C, H, W, 81)
    am = torch.randint(0, C, (N, H, W), generator=g)
    m = int_tensor((N, 1, H, W), -8, 8, g)
    x = m - 128.0 - int_tensor((N, C, H, W), 0, 8, g)
    x = torch.where(torch.arange(C).view(1, C, 1, 1) == am.unsqueeze(1), m, x)
    other = (am + 1 + torch.randint(0, max(C - 1, 1), (N, H, W), generator=g)) % C
    p = torch.arange(N * H * W).view(N, H, W) % 8
    t = torch.where(p == 4, other, am)
    t = torch.where(p == 5, torch.tensor(IGNORE), torch.where(p == 6, torch.tensor(-1), torch.where(p == 7, torch.tensor(C), t)))
    if all_ignored:
        t = torch.where(p % 3 == 0, torch.tensor(IGNORE), torch.where(p % 3 == 1, torch.tensor(-1), torch.tensor(C)))
    return dict(x=x, t=t.to(torch.int64), am=am)


def ce_ref(x, t, gscale, defect=None):
    """-> dict(loss_sum, count (float64 scalars), mean (fp32 [1]: the double quotient rounded once, 0 without a valid pixel),
    grad [N, C, H, W] float64, terms).  General in the logits but for expf's underflow, which it restates"""
    N, C, H, W = x.shape
    xd = x.double()
    if defect == "sample_stride":            # logits of sample n read from n * HW instead of n * C * HW
        flat = xd.reshape(-1)
        idx = (torch.arange(N).view(N, 1, 1) * H * W + torch.arange(C).view(1, C, 1) * H * W + torch.arange(H * W).view(1, 1, -1))
        xd = flat[idx.reshape(-1)].view(N, C, H, W)
    m = xd.max(1, keepdim=True).values
    e = torch.where(xd - m <= EXPF_ZERO_BELOW, torch.zeros(()).double(), torch.exp(xd - m))
    s = e.sum(1, keepdim=True)
    valid = (t >= 0) & (t < C)
    tc = t.clamp(0, C - 1).unsqueeze(1)
    terms = torch.where(valid, (torch.log(s) + m - xd.gather(1, tc)).squeeze(1), torch.zeros(()).double())
    onehot = (torch.arange(C).view(1, C, 1, 1) == tc) & valid.unsqueeze(1)
    grad = gscale * (e / s - onehot.double())
    if defect != "ignored_grad":
        grad = torch.where(valid.unsqueeze(1), grad, torch.zeros(()).double())
    count = float(valid.numel() if defect == "count_ignored" else valid.sum())
    loss_sum = float(terms.sum())
    mean = np.float32(np.float64(loss_sum) / np.float64(count)) if count > 0 else np.float32(0.0)
    return dict(loss_sum=loss_sum, count=count, mean=torch.tensor([mean]), grad=grad, terms=terms, valid=valid)


# ---------------------------------------------------------------------------------------------------------------
# channel softmax: per pixel k logits equal and maximal, the rest at least 128 lower: y = fl(1 / k) or 0, exactly.  With integer
# dy the backward dx = y * (dy - sum dy * y) is exact for k a power of two
# ---------------------------------------------------------------------------------------------------------------
SOFTMAX_CASES = [(N, C, H, W) for C, N, (H, W) in ((1, 1, (1, 1)), (1, 3, (15, 17)), (2, 1, (15, 17)), (2, 3, (1, 257)), (4, 3, (15, 17)),
                                                    (13, 1, (1, 257)), (13, 3, (15, 17)), (64, 1, (15, 17)), (64, 3, (1, 257)), (64, 1, (1, 1)))]


@lru_cache(maxsize=None)
def softmax_case(case, pow2_only=False):
    N, C, H, W = case
    g = _gen(N, C, H, W, 82 + int(pow2_only))
    ks = sorted({k for k in (1, 2, 4, C) if k <= C and (not pow2_only or k & (k - 1) == 0)})
    k = torch.tensor(ks)[torch.arange(N * H * W) % len(ks)].view(N, 1, H, W)
    rank = torch.rand(N, C, H, W, generator=g).argsort(1).argsort(1)            # a random permutation of the channels per pixel
    top = rank < k
    m = int_tensor((N, 1, H, W), -8, 8, g)
    x = torch.where(top, m, m - 128.0 - int_tensor((N, C, H, W), 0, 8, g))
    y = torch.where(top, (torch.ones(()) / k.float()).expand(N, C, H, W), torch.zeros(()))      # fp32 division: fl(1 / k)
    dy = int_tensor((N, C, H, W), -8, 8, g)
    return dict(x=x, k=k, y=y, dy=dy)


def softmax_bwd_ref(y, dy, dtype=torch.float64):
    yd, dd = y.to(dtype), dy.to(dtype)
    return yd * (dd - (dd * yd).sum(1, keepdim=True))


# ---------------------------------------------------------------------------------------------------------------
# TV of a [N, H, W, 2] flow: loss = sy * sum |f[h+1] - f[h]| + sx * sum |f[w+1] - f[w]|, sy = 1 / (N (H-1) W 2), sx = 1 / (N H (W-1) 2)
# (fp32, as the entry point computes them); grad = the signs, scaled
# ---------------------------------------------------------------------------------------------------------------
TV_CASES = [(1, 2, 2), (2, 9, 7), (1, 2, 300), (1, 300, 2), (1, 513, 256)]          # the last: 2 * 513 * 256 values > 1024 * 256


def tv_scales(N, H, W):
    one, two = np.float32(1.0), np.float32(2.0)
    return (float(one / (np.float32(N) * np.float32(H - 1) * np.float32(W) * two)),
            float(one / (np.float32(N) * np.float32(H) * np.float32(W - 1) * two)))


@lru_cache(maxsize=None)
def tv_case(case):
    """integer flow; every third row repeats the one above and every fourth column the one to its left where p % 5 == 0: a
    constructed share of zero differences in both directions"""
    N, H, W = case
    g = _gen(N, H, W, 83)
    f = int_tensor((N, H, W, 2), -8, 8, g)
    for h in range(1, H):
        if h % 3 == 1:
            f[:, h, ::2] = f[:, h - 1, ::2]
    for w in range(1, W):
        if w % 4 == 1:
            f[:, ::2, w] = f[:, ::2, w - 1]
    return dict(f=f)


def tv_ref(f, dtype=torch.float64):
    """-> loss (scalar), grad [N, H, W, 2], sum |term|, number of terms.  float32: the kernel's expression in its own order of the
    four gradient terms (down, up, right, left), torch's order for the loss sum"""
    N, H, W, _ = f.shape
    sy, sx = (torch.tensor(s, dtype=dtype) for s in tv_scales(N, H, W))
    fd = f.to(dtype)
    dh, dw = fd[:, 1:] - fd[:, :-1], fd[:, :, 1:] - fd[:, :, :-1]
    ty, tx = dh.abs() * sy, dw.abs() * sx
    z = torch.zeros_like(fd)
    down, up, right, left = z.clone(), z.clone(), z.clone(), z.clone()
    down[:, :-1], up[:, 1:] = torch.sign(dh) * sy, torch.sign(dh) * sy
    right[:, :, :-1], left[:, :, 1:] = torch.sign(dw) * sx, torch.sign(dw) * sx
    grad = (((z - down) + up) - right) + left
    mag = ty.double().sum() + tx.double().sum()
    return dict(loss=ty.sum() + tx.sum(), grad=grad, mag=float(mag), T=ty.numel() + tx.numel(), sy=float(sy), sx=float(sx))


def tv_grad_bound(r):
    """3 u (2 sy + 2 sx): three additions of exact products (0 - a is exact), each within half an ulp of a partial sum that is at
    most 2 sy + 2 sx"""
    return 3 * U * (2 * r["sy"] + 2 * r["sx"])


def tv_loss_bound(r):
    """(T + 1) u sum |term|: T rounded products summed in any order"""
    return (r["T"] + 1) * U * r["mag"]
