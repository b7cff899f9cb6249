"""Dyadic-operand cases for the two-stage reductions behind every InstanceNorm / SPADE norm: the statistics (csrc/norm.hip) and the
normalisation backward (csrc/norm_bwd.hip).  Shared by tests/test_norm_exact_cases_cpu.py (the conditions the comparisons rest on,
proved on the references alone) and tests/test_gpu_norm_exact.py (the kernels against these references); needs no GPU.

Every operand is a small integer or a small multiple of 1/2 or 1/4, and mean / rstd of the backward are given by the caller, so
they are dyadic too (rstd a power of two).  Every term the kernels sum -- d and d^2 of the statistics, dnh and dnh * nh of the
backward -- is then a multiple of one granule 2^-k per (sample, channel), and while sum |term| over the whole sample stays at or
below 2^22 granules an fp32 accumulator holds every partial sum exactly, in ANY order: the slab rule, the rows in flight, the
unrolling and a future fusion cannot change a bit.  The finalize stages divide in double.  So

  * m1 = S1 / HW and m2 = S2 / HW of the backward are compared with torch.equal, dnh / dgamma / dbeta too (bf16 stores against
    round-to-nearest-even of the exact value): one pixel dropped or counted twice at a slab seam, or a wrong row in a finalize
    loop, cannot pass;
  * mean / rstd of the statistics are the correctly rounded fp32 value or, at a rounding boundary, its neighbour;
  * dx and the noise-scale gradient, which are not exact (m1, m2 are not dyadic), are held to bounds derived from the roundings
    of the formula (dx_check / dns_check below), never to a measured tolerance.

What this pins is the VALUE of each output.  It does not pin the order of the sums, the slab rule, or whether a sum takes dnh
before or after its bf16 store (dnh is exactly representable in bf16 in every case)."""
from collections import namedtuple
from functools import lru_cache

import torch

import norm_bwd_instance_cases as K
from exact_cases import _gen, int_tensor, tie_share, to_bf16_rne  # noqa: F401  (re-exported for the two tests)

# ---------------------------------------------------------------------------------------------------------------
# launch geometry: a mirror of norm_slabs / norm_chunks (csrc/hrv_common.h) and norm_tile (csrc/norm_bwd.hip)
# ---------------------------------------------------------------------------------------------------------------
NORM_GCAP = 64            # channel groups (of 4) per block
SLAB_PIXELS = 128         # a slab is at least this long ...
SLAB_CAP = 256            # ... until there would be more slabs than this (HRV_NORM_SLABS_MAX overrides it)
FIN_LANES_STATS, FIN_LANES_BWD = 64, 16     # lanes per (n, c) in instnorm_finalize_kernel / norm_bwd_finalize_kernel

Geo = namedtuple("Geo", "NB PB slabs last empty GB R idle chunks live_last walk")


def geometry(H, W, C, cap=None):
    """NB slabs of PB pixels (``slabs``: the length of each; ``last``: of the last one that holds pixels; ``empty``: how many hold
    none), GB channel groups x R pixel rows per block with ``idle`` threads past the last row, ``chunks`` blocks along the channels
    with ``live_last`` groups in the last one, and ``walk``: the most pixels one thread visits."""
    hw, c4 = H * W, C // 4
    cap = SLAB_CAP if cap is None or cap < 1 else cap
    nb = max(1, min(-(-hw // SLAB_PIXELS), cap))
    pb = -(-hw // nb)
    slabs = [max(0, min(pb, hw - b * pb)) for b in range(nb)]
    gb = min(c4, NORM_GCAP)
    r = 256 // gb
    chunks = -(-c4 // NORM_GCAP)
    return Geo(nb, pb, slabs, [s for s in slabs if s][-1], sum(s == 0 for s in slabs), gb, r, 256 - r * gb, chunks,
               c4 - (chunks - 1) * NORM_GCAP, -(-pb // r))


# (N, H, W, HRV_NORM_SLABS_MAX or None, C).  N = 2 at one small extent: the sample stride.  H and W even wherever the up-sampled
# source runs.
Extent = namedtuple("Extent", "N H W cap C")
ALL_C = [4, 12, 80, 256, 260, 1040]
SMALL = [(1, 4, 4, None), (2, 12, 11, None)]
LARGE = [Extent(1, 48, 43, None, 12), Extent(1, 96, 86, None, 8), Extent(1, 136, 242, None, 8), Extent(1, 164, 200, None, 12),
         Extent(1, 22, 20, 3, 12), Extent(1, 48, 44, 2, 8)]
GENERIC_AGAIN = [LARGE[0], LARGE[4]]          # every form once more with HRV_NORM_BWD_GENERIC=1


def ext_id(e):
    return f"{e.N}x{e.H}x{e.W}x{e.C}" + (f"-cap{e.cap}" if e.cap else "")


def wide(e):
    """the two smallest extents have the headroom for wide operands (|x| <= 16, mean in quarters): bf16 ties in dgamma"""
    return e.H * e.W <= 256


def up_channels(C):
    """channels of the low-resolution half of x = cat(up2(lo), hi) in the backward cases"""
    return C - (4 if C < 32 else 16)


def can_up(e):
    return e.H % 2 == 0 and e.W % 2 == 0 and e.C >= 8


# ---------------------------------------------------------------------------------------------------------------
# helpers: granules, headroom, rounding
# ---------------------------------------------------------------------------------------------------------------
LIMIT = 2 ** 22


def granule(t):
    """per (n, c) of an [N, H, W, C] float64 tensor: the largest 2^-k (k <= 20) every element is a multiple of"""
    N, C = t.shape[0], t.shape[-1]
    flat = t.reshape(N, -1, C)
    g = torch.zeros(N, C, dtype=torch.float64)
    for k in range(20, -1, -1):
        s = flat * 2.0 ** k
        ok = (s == s.round()).all(1)
        g = torch.where(ok, torch.full_like(g, 2.0 ** -k), g)
    assert bool((g > 0).all()), "a term is not a multiple of 2^-20"
    return g


def headroom(t):
    """max over (n, c) of sum |term| in granules: at or below LIMIT, every partial sum of the terms is exact in fp32 in any order"""
    N, C = t.shape[0], t.shape[-1]
    return float((t.abs().reshape(N, -1, C).sum(1) / granule(t)).max())


def bf16_exact(t64):
    f = t64.to(torch.float32)
    return torch.equal(f.double(), t64) and torch.equal(f.to(torch.bfloat16).double(), t64)


def needs_rounding_share(t64):
    f = t64.to(torch.float32)
    return float((f.to(torch.bfloat16).double() != t64).double().mean())


def f64_to_bf16_rne(t64):
    """float64 -> bf16, round-to-nearest-even on the float64 bit pattern (one rounding; values in bf16's normal range or zero)"""
    u = t64.contiguous().view(torch.int64)
    u = ((u + ((1 << 44) - 1) + ((u >> 45) & 1)) >> 45) << 45
    return u.view(torch.float64).to(torch.float32).to(torch.bfloat16)


def _up2(lo):
    return lo.repeat_interleave(2, 1).repeat_interleave(2, 2)


def _noise(z, ns):
    """z [N, W, H] (the noise map is stored transposed), ns [C] -> z[n, w, h] * ns[c] as [N, H, W, C] float64"""
    return z.double().permute(0, 2, 1).unsqueeze(-1) * ns.double()


def _halves(shape, m, g):
    return int_tensor(shape, -m, m, g) * 0.5


# ---------------------------------------------------------------------------------------------------------------
# statistics
# ---------------------------------------------------------------------------------------------------------------
EPS = float(torch.tensor(1e-5, dtype=torch.float32).double())      # the fp32 eps the entry points receive, widened
SHIFT_CASE = LARGE[0]        # x = 2048 + {-2..2}: exact in fp32, the shifted sums exact, the unshifted sum of x^2 not
STATS_EXTENTS = [Extent(N, H, W, cap, C) for N, H, W, cap in SMALL for C in ALL_C] + LARGE


def stats_up_splits(e):
    """channel counts of the low-resolution half in the up-sampled statistics: below and above one chunk's 256 channels where C allows"""
    if not can_up(e):
        return []
    return {8: [4], 12: [8], 80: [64], 256: [128], 260: [16, 256], 1040: [64, 512]}[e.C]


def stats_ref(v):
    """float64 (mean, rstd) [N, C] of v [N, H, W, C]: biased variance, two passes"""
    N, C = v.shape[0], v.shape[-1]
    f = v.reshape(N, -1, C)
    mean = f.mean(1)
    var = ((f - mean[:, None]) ** 2).mean(1)
    return mean, 1.0 / torch.sqrt(var + EPS)


@lru_cache(maxsize=None)
def stats_case(e, shifted=False):
    """x (fp32; bf16 holds it too unless ``shifted``), two noise terms (z_a, ns_a), (z_b, ns_b), and per noise choice the values v and
    their float64 statistics.  Channel ``const`` is constant under every noise choice: variance exactly 0, rstd = 1 / sqrt(eps)."""
    g = _gen(e.N, e.H, e.W, e.C, e.cap or 0, 21 + int(shifted))
    m = 2 if shifted or not wide(e) else 16
    x = int_tensor((e.N, e.H, e.W, e.C), -m, m, g) + (2048.0 if shifted else 0.0)
    const = e.C // 2
    x[..., const] = 1.0 + (2048.0 if shifted else 0.0)
    zm = 2 if wide(e) else 1
    z = [int_tensor((e.N, e.W, e.H), -zm, zm, g) for _ in range(2)]
    ns = [_halves((e.C,), 2 if wide(e) else 1, g) for _ in range(2)]
    for s in ns:
        s[const] = 0.0
    v = {"plain": x.double(), "a": x.double() + _noise(z[0], ns[0]), "b": x.double() + _noise(z[1], ns[1])}
    return dict(x=x, z=z, ns=ns, const=const, v=v, ref={k: stats_ref(t) for k, t in v.items()})


def stats_up_parts(case, up_c):
    """(lo, hi) whose cat(up2(lo), hi) replaces x: the low-resolution half takes x at the even pixels.  -> lo, hi, the float64
    values per noise choice and their statistics"""
    x = case["x"]
    lo, hi = x[:, ::2, ::2, :up_c].contiguous(), x[..., up_c:].contiguous()
    xf = torch.cat([_up2(lo), hi], -1).double()
    v = {"a": xf + _noise(case["z"][0], case["ns"][0]), "b": xf + _noise(case["z"][1], case["ns"][1])}
    return lo, hi, v, {k: stats_ref(t) for k, t in v.items()}


def within_one_ulp(got32, ref64):
    """bool per element: got is the float64 value rounded to fp32, or one of that value's two fp32 neighbours.  Derived: the sums
    are exact and the finalize runs in double, so the kernel rounds (almost) the true value once"""
    r = ref64.to(torch.float32)
    inf = torch.full_like(r, float("inf"))
    return (got32 == r) | (got32 == torch.nextafter(r, inf)) | (got32 == torch.nextafter(r, -inf))


def stats_check(got_mean, got_rstd, ref, what=""):
    """the assertion of the GPU test on one (mean, rstd) pair ([N, C] fp32 on the CPU)"""
    for name, got, want in (("mean", got_mean, ref[0]), ("rstd", got_rstd, ref[1])):
        assert not bool(torch.isnan(got).any()), (what, name)
        ok = within_one_ulp(got, want)
        bad = (~ok).nonzero()
        assert bool(ok.all()), f"{what} {name}: {len(bad)} of {ok.numel()} beyond one ulp, first (n, c) = {bad[0].tolist()}: " \
                               f"{float(got[tuple(bad[0])])!r} vs {float(want[tuple(bad[0])])!r}"


# ---------------------------------------------------------------------------------------------------------------
# backward
# ---------------------------------------------------------------------------------------------------------------
def _one_norm_operands(form, e, g):
    """the operands of ONE norm of ``form`` besides x (tests/norm_bwd_instance_cases.py: what each kind carries)"""
    N, H, W, C = e.N, e.H, e.W, e.C
    w = wide(e)
    o = {}
    # (wide: odd quarters, so that v - mean always carries the quarter and dgamma = dpre * nh needs more bits than bf16 has)
    o["mean"] = (2 * int_tensor((N, C), -4, 3, g) + 1) * 0.25 if w else _halves((N, C), 1, g)
    o["rstd"] = 2.0 ** (int_tensor((N, C), -2, 1 if w else 0, g))
    if form.kind != "inorm":
        o["z"] = int_tensor((N, W, H), -2, 2, g) if w else int_tensor((N, W, H), -1, 1, g)
        o["ns"] = _halves((C,), 2 if w else 1, g)
        o["g1p"] = int_tensor((N, H, W, C), 0, 8, g) * 0.25 if w else int_tensor((N, H, W, C), 0, 4, g) * 0.5
    dm = 15 if w else 2
    o["dout"] = int_tensor((N, H, W, C), -dm, dm, g)
    if form.kind != "spade":
        o["out"] = int_tensor((N, H, W, C), -3, 3, g)
        o["slope"] = 0.25 if w else 0.5
    return o


def norm_ref(x64, o):
    """float64, from the formulas above stage 1 of csrc/norm_bwd.hip:  v = x + z * ns;  nh = (v - mean) * rstd;
    dpre = dout * act'(out);  dnh = dpre * (1 + gamma);  dgamma = dpre * nh;  dbeta = dpre;  S1 = sum dnh;  S2 = sum dnh * nh"""
    v = x64 + (_noise(o["z"], o["ns"]) if "z" in o else 0.0)
    rs = o["rstd"].double()[:, None, None, :]
    nh = (v - o["mean"].double()[:, None, None, :]) * rs
    dpre = o["dout"].double()
    if "out" in o:
        dpre = dpre * torch.where(o["out"] > 0, 1.0, o["slope"]).double()
    dnh = dpre * o["g1p"].double() if "g1p" in o else dpre
    hw = x64.shape[1] * x64.shape[2]
    S1, S2 = dnh.sum((1, 2)), (dnh * nh).sum((1, 2))
    return dict(v=v, nh=nh, rs=rs, dpre=dpre, dnh=dnh, dgamma=dpre * nh, dbeta=dpre, S1=S1, S2=S2, hw=hw,
                m1=(S1 / hw).to(torch.float32), m2=(S2 / hw).to(torch.float32))


def dx_term(r, m1, m2):
    """float64 rstd * (dnh - m1 - nh * m2) with the given m1 / m2 [N, C] (the kernel's own fp32 values, widened), and the
    bracket rstd * (|dnh| + |m1| + |nh * m2|) its error bound scales with"""
    a1, a2 = m1.double()[:, None, None, :], m2.double()[:, None, None, :]
    return r["rs"] * (r["dnh"] - a1 - r["nh"] * a2), r["rs"] * (r["dnh"].abs() + a1.abs() + (r["nh"] * a2).abs())


DNS_ACCUMULATE = "norm_s_coarse"       # the form whose noise-scale gradient is accumulated into an old value


@lru_cache(maxsize=None)
def bwd_case(form_id, e):
    """operands and float64 reference of one form at one extent: x (or lo / hi), one norm ("a") or the two of a pair ("a", "b"),
    the old dx where the form accumulates, the old noise-scale gradient of DNS_ACCUMULATE"""
    form = next(c for c in K.CASES if c.id == form_id)
    idx = [c.id for c in K.CASES].index(form_id)
    g = _gen(e.N, e.H, e.W, e.C, e.cap or 0, 31 + idx)
    xm = 16 if wide(e) else 2
    d = dict(form=form)
    if form.up:
        assert can_up(e)
        uc = up_channels(e.C)
        d["lo"] = int_tensor((e.N, e.H // 2, e.W // 2, uc), -xm, xm, g)
        d["hi"] = int_tensor((e.N, e.H, e.W, e.C - uc), -xm, xm, g)
        x64 = torch.cat([_up2(d["lo"]), d["hi"]], -1).double()
    else:
        d["x"] = int_tensor((e.N, e.H, e.W, e.C), -xm, xm, g)
        x64 = d["x"].double()
    d["x64"] = x64
    d["norms"] = [_one_norm_operands(form, e, g) for _ in range(2 if form.pair else 1)]
    d["refs"] = [norm_ref(x64, o) for o in d["norms"]]
    d["dx0"] = int_tensor((e.N, e.H, e.W, e.C), -4, 4, g) if form.dx == "acc" else None
    d["dns0"] = int_tensor((e.C,), -4, 4, g) if form_id == DNS_ACCUMULATE else None       # (of norm "a")
    return d


def m_check(got_m1, got_m2, r, what=""):
    """m1 / m2 as the kernel left them in its workspace against (S / HW in float64).to(float32), bit for bit"""
    for name, got, want in (("m1", got_m1, r["m1"]), ("m2", got_m2, r["m2"])):
        bad = (got != want).nonzero()
        assert torch.equal(got, want), f"{what} {name}: {len(bad)} of {want.numel()} differ, first (n, c) = {bad[0].tolist()}: " \
                                       f"{float(got[tuple(bad[0])])!r} vs {float(want[tuple(bad[0])])!r}"


def dx_check(got, terms, old=None, bf16=False, what=""):
    """dx ([N, H, W, C] as stored, on the CPU) against the sum of ``terms`` [(float64 value, bracket)] (+ ``old``).  Bound, element
    by element: 2^-22 * (sum of the brackets + |old|) -- the three roundings of a term (dnh - m1, nh * m2, their difference; the
    product with rstd, a power of two, is exact) are at most half an ulp each of magnitudes inside the bracket, 2^-23 * bracket
    together, and the one add that joins two terms or the old value is another half ulp of their sum; doubled.  A bf16 dx lies
    between the roundings of the two ends.  -> worst |error| / bound"""
    ref = sum(t for t, _ in terms) + (old.double() if old is not None else 0.0)
    bound = 2.0 ** -22 * (sum(b for _, b in terms) + (old.double().abs() if old is not None else 0.0))
    assert not bool(torch.isnan(got.float()).any()), what
    if bf16:
        lo, hi, g = f64_to_bf16_rne(ref - bound).double(), f64_to_bf16_rne(ref + bound).double(), got.double()
        ok = (g >= lo) & (g <= hi)
        ratio = ((g - ref).abs() / torch.maximum((hi - ref).abs(), (lo - ref).abs()).clamp_min(2.0 ** -60)).max()
    else:
        err = (got.double() - ref).abs()
        ok = err <= bound
        ratio = (err / bound.clamp_min(2.0 ** -60)).max()
    assert bool(ok.all()), f"{what} dx: {int((~ok).sum())} of {ok.numel()} beyond the bound, worst |error| / bound = {float(ratio):.3g}"
    return float(ratio)


def dns_check(got, term, bracket, z, geo, old=None, what=""):
    """dnoise_scale [C] against float64 sum dx * z (+ ``old``).  Bound per channel: 2^-23 * (ceil(PB / R) + R + 2) * sum |dx * z|
    (the forward error of the kernel's longest fp32 chain: a thread's pixels, the R rows of its block, the store and the add into
    ``old``) + sum 2^-22 * bracket * |z| (the error carried in from dx).  -> worst |error| / bound"""
    zz = z.double().permute(0, 2, 1).unsqueeze(-1)
    ref = (term * zz).sum((0, 1, 2)) + (old.double() if old is not None else 0.0)
    mag = (term * zz).abs().sum((0, 1, 2)) + (old.double().abs() if old is not None else 0.0)
    bound = 2.0 ** -23 * (geo.walk + geo.R + 2) * mag + (2.0 ** -22 * bracket * zz.abs()).sum((0, 1, 2))
    err = (got.double() - ref).abs()
    ratio = float((err / bound.clamp_min(2.0 ** -60)).max())
    assert not bool(torch.isnan(got).any()) and bool((err <= bound).all()), \
        f"{what} dnoise_scale: {int((err > bound).sum())} of {err.numel()} beyond the bound, worst |error| / bound = {ratio:.3g}"
    return ratio


# ---------------------------------------------------------------------------------------------------------------
# which form runs where
# ---------------------------------------------------------------------------------------------------------------
def backward_runs():
    """[(form, extent, generic kernels forced)]: every form of norm_bwd_instance_cases.CASES at every extent it can run at (the
    up-sampled source needs even H, W and C >= 8), the channel counts crossed sparingly with the two smallest extents -- the
    channel chunking is norm_tile's, the same code under every form -- and every form again on the generic kernels at two extents"""
    runs = []
    for i, form in enumerate(K.CASES):
        for j, (N, H, W, cap) in enumerate(SMALL):
            cs = ALL_C[1:] if form.up else [ALL_C[(i + j) % 6], ALL_C[(i + j + 3) % 6]]
            runs += [(form, Extent(N, H, W, cap, c), False) for c in cs if not form.up or can_up(Extent(N, H, W, cap, c))]
        runs += [(form, e, False) for e in LARGE if not form.up or can_up(e)]
        runs += [(form, e, True) for e in GENERIC_AGAIN if not form.up or can_up(e)]
    return runs


def run_id(run):
    form, e, generic = run
    return f"{form.id}-{ext_id(e)}" + ("-generic" if generic else "")
