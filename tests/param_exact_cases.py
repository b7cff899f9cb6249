"""Exact cases for the kernels that run on the PARAMETERS of every training step: the spectral-norm family of csrc/train.hip
(gemv_rows / gemv_cols / normalize / dot_partial, the four sn_*_batched kernels, sn_grad), the per-step staging kernels
(spade_vec_prep, spade_vec_prep_multi, shared_taps_prep, shared_taps_grad, and tap_expand of csrc/glue.hip) and the element-wise
scale / tanh_bwd / act_bwd.  Shared by tests/test_param_exact_cases_cpu.py (the conditions the comparisons rest on, proved on the
references alone) and tests/test_gpu_param_exact.py (the kernels against these references).  Pure CPU torch / numpy; imports nothing
of the project.  The helpers (bound, LIMIT, POISON, bits, within_one_ulp, ...) are the ones of train_exact_cases.py.

Spectral forward on exact singular pairs.  p in Z^R and q in Z^K hold ones, twos and threes (zeros only where R or K is too small)
with p.p = 4^a and q.q = 4^b; E is an integer sum of outer products a_i b_i^T with a_i = p_j e_i - p_i e_j and b_i = q_l e_k - q_k e_l,
so E^T p = 0 and E q = 0; W = p q^T + E and u0 = p.  Then W^T u0 = 4^a q (norm 4^a 2^b), v = q / 2^b, W v = 2^b p, u = p / 2^a,
sigma = 2^(a+b), and a further iteration returns the same bits.  Every term a kernel sums is a multiple of one granule and
sum |term| stays at or below 2^22 granules (``bound`` asserts it per case and stage), so every partial sum is exact in fp32 in ANY
order; the norms are powers of two, whose square root and reciprocal are exact.  E has to cancel to zero: a skipped row group, a
dropped column quad or a wrong stride leaves a residue.

What cannot be exact (Gaussian operands) is held, stage by stage on the stage's actual inputs, to a bound derived from the stage's
formula (``gamma(n) * sum |term|`` for a sum of n products, two ulps each for the square root and the reciprocal), never to a
measured tolerance.

The staging kernels are index maps: operands carry distinct integer codes, the references are the index formulas of the header
comments, and everything is compared on the bit pattern.

What this pins is the VALUE of each output and the zero padding.  It does not pin the order of any sum, block counts, caps, or
which path serves an element: the geometry mirrors exist only so that the CPU test can show that the tables reach every path of the
kernels as they are.  Seeded defects (``defect=``) restate one plausible kernel fault each."""
from collections import namedtuple
from functools import lru_cache

import numpy as np
import torch

from train_exact_cases import LIMIT, NAN, POISON, U, _gen, bits, bound, f32, int_tensor, to_bf16_rne, within_one_ulp  # noqa: F401

GRID_CAP = 4096 * 256     # threads of grid_for's capped grid: more work items than this take a second grid-stride trip
SLACK = 1.0 + 2.0 ** -8   # the second-order terms of the derived bounds (every relative perturbation below is < 2^-8)


def grid_trips(total):
    """trips of a grid-stride loop over ``total`` items launched with grid_for(total) blocks of 256"""
    nb = max(1, min(-(-total // 256), 4096))
    return -(-total // (nb * 256))


def gamma(n):
    """n u / (1 - n u): the relative bound of a sum of n rounded products in any order (u = 2^-24)"""
    return n * U / (1.0 - n * U)


# ---------------------------------------------------------------------------------------------------------------
# 1. spectral forward: v <- normalize(W^T u), u <- normalize(W v) per iteration, sigma = u . (W v); normalize(x) = x * (1 / max(|x|, eps))
# ---------------------------------------------------------------------------------------------------------------
SN_EPS = f32(1e-12)
SN_MAX = 40
# (R, K).  K for gemv_cols_body: 4 one quad; 60 / 64 / 68 last block partial, full, one quad over; 81, 215 scalar path (K % 4 != 0)
# with a partial last quad; 576.  K for the 256-stride loops: 255, 256, 257, 516.  R: 1, 3, 15, 16, 17; 48 tail only, 49 row group 0
# takes the four-in-flight loop once; 63, 64, 65; 112, 113 (a second four-in-flight trip); 130, 257 (two 256-thread trips over R); 1024;
# 150: EVERY row group takes two four-in-flight trips and has tail rows behind them
SN_SHAPES = [(1, 4), (3, 60), (15, 64), (16, 68), (17, 81), (48, 215), (49, 576), (63, 255), (64, 256), (65, 257), (112, 516),
             (113, 64), (130, 216), (257, 60), (1024, 576), (24, 180), (113, 215), (130, 68), (150, 68)]
SN_SMALL = [(1, 4), (3, 60), (15, 64), (16, 68), (17, 81)] * 9          # 45 jobs: a second SN_MAX chunk of five
SN_ZERO = (17, 81)                                                      # the W = 0 case
SnGeo = namedtuple("SnGeo", "col_blocks last_block_cols vector quad_trips tail_rows scalar_partial row_trips norm_trips_K norm_trips_R")


def cols_row_plan(R):
    """mirror of the vector path of gemv_cols_body: per row group rg (16 of them) the rows each trip of the four-in-flight loop
    takes (``while r + 48 < R``) and the rows left to the 16-row tail loop"""
    plan = []
    for rg in range(16):
        r, quads = rg, []
        while r + 48 < R:
            quads.append([r, r + 16, r + 32, r + 48])
            r += 64
        plan.append((quads, list(range(r, R, 16))))
    return plan


def sn_geometry(R, K):
    plan = cols_row_plan(R)
    nb = -(-K // 64)
    return SnGeo(nb, K - 64 * (nb - 1), K % 4 == 0, [len(q) for q, _ in plan], [len(t) for _, t in plan], K % 4 != 0,
                 -(-K // 256), -(-K // 256), -(-R // 256))


def _squares(n, S):
    """(n1, n2, n3) with n1 + n2 + n3 = n and n1 + 4 n2 + 9 n3 = S, the fewest twos and threes; None where there is none"""
    D = S - n
    if D < 0:
        return None
    for n3 in range(D // 8, -1, -1):
        if (D - 8 * n3) % 3 == 0 and n3 + (D - 8 * n3) // 3 <= n:
            n2 = (D - 8 * n3) // 3
            return n - n2 - n3, n2, n3
    return None


def unit_vector(n, g):
    """integer x in Z^n with x.x = 4^a, a >= 1: ones, twos and threes at shuffled positions, zeros only where no such vector
    without them exists (n = 3: (2, 0, 0))"""
    for z in range(n):
        m = n - z
        for a in range(1, 8):
            c = _squares(m, 4 ** a)
            if c is not None and 4 ** a <= 9 * m:
                x = torch.cat([torch.full((k,), float(val)) for k, val in zip(c + (z,), (1, 2, 3, 0))])
                x = x[torch.randperm(n, generator=g)]
                assert float((x * x).sum()) == 4 ** a
                return x, a
    raise AssertionError(n)


@lru_cache(maxsize=None)
def sn_case(R, K, terms=40):
    """-> dict(p, q, a, b, E, W): W = p q^T + E [R, K], E of ``terms`` outer products on random index pairs"""
    g = _gen(R, K, 91)
    p, a = unit_vector(R, g)
    q, b = unit_vector(K, g)
    E = torch.zeros(R, K)
    if R > 1 and K > 1:
        i = torch.randint(0, R, (terms,), generator=g)
        j = (i + 1 + torch.randint(0, R - 1, (terms,), generator=g)) % R
        k = torch.randint(0, K, (terms,), generator=g)
        l = (k + 1 + torch.randint(0, K - 1, (terms,), generator=g)) % K
        s = 2.0 * torch.randint(0, 2, (terms,), generator=g) - 1.0
        for rows, cols, val in ((i, k, p[j] * q[l]), (i, l, -p[j] * q[k]), (j, k, -p[i] * q[l]), (j, l, p[i] * q[k])):
            E.index_put_((rows, cols), s * val, accumulate=True)
    W = torch.outer(p, q) + E
    assert not bool((E.t().double() @ p.double()).any()) and not bool((E.double() @ q.double()).any())
    return dict(p=p, q=q, a=a, b=b, E=E, W=W, R=R, K=K)


def _cols_mask(R, K, defect):
    """which products W[r][k] * x[r] the (seeded) gemv_cols sums"""
    m = torch.ones(R, K, dtype=torch.bool)
    if K % 4 == 0 and defect in ("cols_skip_tail", "cols_quad_early"):
        for quads, tail in cols_row_plan(R):
            lost = tail if defect == "cols_skip_tail" else (quads[-1] if quads else [])
            m[lost] = False
    if K % 4 != 0 and defect == "cols_scalar_partial":
        m[:, K - K % 4:] = False
    return m


def _normalize(x, eps, defect=None):
    nrm = torch.sqrt((x * x).sum())
    inv = 1.0 / (nrm if defect == "no_eps" else torch.clamp_min(nrm, eps))
    return x * inv


def sn_ref(W, u, v, iters, eps=SN_EPS, defect=None, first_block_lost=False):
    """float64 restatement of hrv_spectral_norm_f32 / hrv_spectral_norm_batched_f32.  -> dict(u, v, sigma [1], wv (what the scratch
    holds), u_keep, v_keep).  ``first_block_lost``: the job's first 64-column block of gemv_cols never ran (sn_find gave it to the
    previous job, where it is out of range): those columns keep the old v"""
    W64, u, v = W.double(), u.double().clone(), v.double().clone()
    R, K = W64.shape
    t = wv = None
    for _ in range(iters):
        t = (torch.where(_cols_mask(R, K, defect), W64, torch.zeros(())) * u.view(R, 1)).sum(0)
        if first_block_lost:
            t[:64] = v[:64]
        v = _normalize(t, eps, defect)
        wv = (W64[:, :256] if defect == "rows_one_trip" else W64) @ (v[:256] if defect == "rows_one_trip" else v)
        u = _normalize(wv, eps, defect)
    if iters == 0:
        wv = (W64[:, :256] if defect == "rows_one_trip" else W64) @ (v[:256] if defect == "rows_one_trip" else v)
    sigma = ((wv if (defect == "sigma_unnormalised" and iters) else u) * wv).sum().reshape(1)
    keep = defect == "keep_before_norm" and iters
    return dict(u=u, v=v, sigma=sigma, wv=wv, u_keep=wv if keep else u, v_keep=t if keep else v)


def sn_bounds(c, iters):
    """asserts, stage by stage, that every term summed is a multiple of the stage's granule and that sum |term| stays within LIMIT
    granules, for ``iters`` iterations from u0 = p, v0 = q; returns the largest sum in granules"""
    W, p, q, a, b = c["W"].double(), c["p"].double(), c["q"].double(), c["a"], c["b"]
    R, K = W.shape
    worst = 0.0
    u, v = p, q
    for it in range(iters):
        gu = 1.0 if it == 0 else 2.0 ** -a
        t = W.t() @ u
        worst = max(worst, bound(W * u.view(R, 1), gu, dims=0), bound(t * t, (4.0 ** a if it == 0 else 2.0 ** a) ** 2 * 1.0))
        v = t / torch.sqrt((t * t).sum())
        wv = W @ v
        worst = max(worst, bound(W * v.view(1, K), 2.0 ** -b, dims=1), bound(wv * wv, 4.0 ** b))
        u = wv / torch.sqrt((wv * wv).sum())
    wv = W @ v
    worst = max(worst, bound(W * v.view(1, K), 2.0 ** -b if iters else 1.0, dims=1),
                bound(u * wv, 2.0 ** (b - a) if iters else 4.0 ** b))
    return worst


def _sum32(terms, axis, rng):
    """fp32 sum along ``axis`` in a random sequential order"""
    t = np.take(terms, rng.permutation(terms.shape[axis]), axis=axis)
    return np.take(np.cumsum(t, axis=axis, dtype=np.float32), -1, axis=axis)


def sn_f32(W, u, v, iters, seed, eps=SN_EPS):
    """the iteration restated in numpy fp32, every sum in its own random order"""
    rng = np.random.default_rng(seed)
    W, u, v = (x.numpy().astype(np.float32) for x in (W, u, v))
    one, e = np.float32(1.0), np.float32(eps)

    def norm(x):
        return x * (one / max(np.sqrt(_sum32(x * x, 0, rng)), e))
    for _ in range(iters):
        v = norm(_sum32(W * u[:, None], 0, rng))
        wv = _sum32(W * v[None, :], 1, rng)
        u = norm(wv)
    wv = _sum32(W * v[None, :], 1, rng)
    return dict(u=torch.from_numpy(u), v=torch.from_numpy(v), sigma=torch.from_numpy(np.asarray([_sum32(u * wv, 0, rng)])), wv=torch.from_numpy(wv))


def sn_prefix(shapes):
    """mirror of the batched launch per SN_MAX chunk: [(first job, jobs, col_blk prefix, row_blk prefix, scratch offsets)]; the
    scratch offset runs on across the chunks"""
    out, off = [], 0
    for j0 in range(0, len(shapes), SN_MAX):
        ch = shapes[j0:j0 + SN_MAX]
        col, row, offs = [0], [0], []
        for R, K in ch:
            col.append(col[-1] + -(-K // 64))
            row.append(row[-1] + R)
            offs.append(off)
            off += R
        out.append((j0, len(ch), col, row, offs))
    return out


def sn_scratch_ref(shapes, wvs, defect=None):
    """what a NaN-filled scratch of sum(R) floats holds after the batched call: job j's W v at its running offset.
    defect ``chunk_scratch``: the second chunk's offsets start at the first chunk's again"""
    out = torch.full((sum(R for R, _ in shapes),), NAN, dtype=torch.float64)
    for ci, (j0, n, _, _, offs) in enumerate(sn_prefix(shapes)):
        base = offs[0] if (defect == "chunk_scratch" and ci) else 0
        for j in range(n):
            o = offs[j] - base
            out[o:o + shapes[j0 + j][0]] = wvs[j0 + j]
    return out


# ---------------------------------------------------------------------------------------------------------------
# 2. spectral forward on Gaussian operands: each stage against float64 on the stage's actual inputs
# ---------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def sn_gauss_case(R, K):
    g = _gen(R, K, 92)
    W = torch.randn(R, K, generator=g)
    u0, v0 = torch.randn(R, generator=g).double(), torch.randn(K, generator=g).double()
    return dict(W=W, u0=(u0 / u0.norm()).float(), v0=(v0 / v0.norm()).float())


def normalize_stage(M, x):
    """y = normalize(M x), M [m, n] and x [n] the fp32 operands the stage was handed -> (y float64, bound [m]).
    t_i = sum_k M_ik x_k is held to d_i = gamma(n) sum_k |M_ik x_k|.  s = sum t_i^2 over the computed t: m rounded products summed,
    relative gamma(m); its square root halves that and adds two ulps (4 u), the reciprocal two ulps (4 u), the final product one
    rounding (u); the computed norm also moves by at most |d|_2.  So
        |y_i - ref_i| <= d_i / |t| + |ref_i| (|d|_2 / |t| + gamma(m) / 2 + 9 u),   times SLACK for the second-order terms"""
    M64, x64 = M.double(), x.double()
    m, n = M64.shape
    t = M64 @ x64
    d = gamma(n) * (M64.abs() @ x64.abs())
    nt = float(t.norm())
    ref = t / nt
    return ref, SLACK * (d / nt + ref.abs() * (float(d.norm()) / nt + gamma(m) / 2 + 9 * U))


def sigma_stage(W, u, v):
    """sigma = u . (W v) on the fp32 u, v the kernel wrote -> (float64 value, bound): the rows of W v are held to
    d_r = gamma(K) sum_k |W_rk v_k|, the dot of R rounded products to gamma(R) sum_r |u_r (W v)_r|"""
    W64, u64, v64 = W.double(), u.double(), v.double()
    R, K = W64.shape
    wv = W64 @ v64
    d = gamma(K) * (W64.abs() @ v64.abs())
    return float(u64 @ wv), SLACK * float(u64.abs() @ d + gamma(R) * (u64 * wv).abs().sum())


def sn_gauss_check(d, u, v, sigma, what=""):
    """u, v, sigma (CPU fp32) after ONE iteration from (u0, v0) -> the used share of each stage's bound {"v", "u", "sigma"};
    asserts that none exceeds 1"""
    W = d["W"]
    shares = {}
    for name, got, (ref, bnd) in (("v", v, normalize_stage(W.t(), d["u0"])), ("u", u, normalize_stage(W, v))):
        assert not bool(torch.isnan(got).any()), f"{what} {name}: NaN"
        shares[name] = float(((got.double() - ref).abs() / bnd).max())
    ref, bnd = sigma_stage(W, u, v)
    shares["sigma"] = abs(float(sigma.double()) - ref) / bnd
    assert all(s <= 1.0 for s in shares.values()), f"{what}: |error| / bound = {shares}"
    return shares


# ---------------------------------------------------------------------------------------------------------------
# 3. spectral backward: dW_orig = (G - c u_r v_k) / sigma (+ old), c = <G, W_orig> / sigma
# ---------------------------------------------------------------------------------------------------------------
# R x K: 1, 255, 256, 257 elements; 135 200 (> 512 * 256: the second trip of dot_partial_kernel under its 512-block cap);
# 1 064 960 (> 4096 * 256: the second trip of sn_grad_kernel)
SG_SHAPES = [(1, 1), (15, 17), (16, 16), (1, 257), (130, 1040), (1024, 1040)]
SG_GAUSS = SG_SHAPES[:5]
SG_DOT = 6                 # <G, W> the exact tier steers to (where the entries of W allow it)


def sg_trips(R, K):
    """(trips of dot_partial_kernel under its 512-block cap, trips of sn_grad_kernel under grid_for's cap)"""
    n = R * K
    return -(-n // (min(-(-n // 256), 512) * 256)), grid_trips(n)


@lru_cache(maxsize=None)
def sg_case(R, K):
    """exact tier: W, u = p / 2^a, v = q / 2^b of family 1, sigma = 2^-(a+b+1), integer G with <G, W> steered to SG_DOT (a greedy
    walk over the positions adds at most +-2 to an element), integer old values.  Then c = <G, W> 2^(a+b+1), c u_r v_k =
    2 <G, W> p_r q_k and the result (G - 2 <G, W> p_r q_k) 2^(a+b+1) are integers far below 2^24"""
    c = sn_case(R, K)
    g = _gen(R, K, 93)
    W = c["W"]
    m = 2 if R * K <= 2 ** 18 else 1
    G = int_tensor((R, K), -m, m, g)
    if R * K > 2 ** 18:
        G = G * (torch.rand(R, K, generator=g) < 0.25)              # (sum |G W| has to stay under 2^22)
    res = SG_DOT - int((G.double() * W.double()).sum())
    Gf, Wf = G.view(-1), W.reshape(-1)
    for i in torch.randperm(R * K, generator=g).tolist():
        if res == 0:
            break
        w = int(Wf[i])
        step = max(-2, min(2, int(res / w))) if w else 0
        Gf[i] += step
        res -= step * w
    sigma = 2.0 ** -(c["a"] + c["b"] + 1)
    return dict(G=G, W=W, u=c["p"] / 2.0 ** c["a"], v=c["q"] / 2.0 ** c["b"], sigma=torch.tensor([sigma]),
                old=int_tensor((R, K), -64, 64, g), dot=float((G.double() * W.double()).sum()))


@lru_cache(maxsize=None)
def sg_gauss_case(R, K):
    g = _gen(R, K, 94)
    W, G, old = (torch.randn(R, K, generator=g) for _ in range(3))
    u, v = torch.randn(R, generator=g).double(), torch.randn(K, generator=g).double()
    u, v = (u / u.norm()).float(), (v / v.norm()).float()
    sigma = (u.double() @ (W.double() @ v.double())).abs().clamp_min(0.5).float().reshape(1)
    return dict(G=G, W=W, u=u, v=v, sigma=sigma, old=old)


def sg_ref(d, accumulate, defect=None):
    """float64: (G - c u_r v_k) / sigma (+ old)"""
    G, W, u, v, sg = d["G"].double(), d["W"].double(), d["u"].double(), d["v"].double(), float(d["sigma"])
    R, K = G.shape
    c = (G * W).sum() if defect == "c_not_divided" else (G * W).sum() / sg
    uv = torch.outer(u, v)
    if defect == "swap_uv":                 # u indexed with k and v with r (wrapped into range)
        uv = torch.outer(v[torch.arange(R) % K], u[torch.arange(K) % R])
    out = (G - c * uv) / sg
    return out + d["old"].double() if (accumulate and defect != "ignore_accumulate") else out


def sg_steps(d, assoc, dtype):
    """the kernel's expression step by step in ``dtype`` from the exact <G, W>: c = dot / sg, the product c u_r v_k as (c u) v
    (``assoc`` 0) or c (u v) (1), the difference, the division, the accumulation"""
    G, u, v, old = d["G"].to(dtype), d["u"].to(dtype), d["v"].to(dtype), d["old"].to(dtype)
    sg = d["sigma"].to(dtype)[0]
    dot = torch.tensor(float((d["G"].double() * d["W"].double()).sum()), dtype=dtype)
    c = dot / sg
    inner = (c * u).view(-1, 1) if assoc == 0 else torch.outer(u, v)
    t = inner * v.view(1, -1) if assoc == 0 else c * inner
    diff = G - t
    q = diff / sg
    return [c.reshape(1), inner, t, diff, q, q + old]


def sg_bound(d, accumulate):
    """-> (float64 reference, bound per element).  <G, W>: n products in fp32 partial sums folded in double, gamma(n) sum |G W|,
    one rounding to fp32 (u) and the division by sigma (two ulps, 4 u): dc = gamma(n) sum |G W| / sigma + 5 u |c|.  t = c u_r v_k
    two roundings, G - t one, the division two ulps, the accumulation one:
        (dc |u_r v_k| + 2 u |t| + u (|G| + |t|)) / sigma + 4 u |d| (+ u (|old| + |d|)),   times SLACK"""
    G, W, u, v, sg = d["G"].double(), d["W"].double(), d["u"].double(), d["v"].double(), float(d["sigma"])
    n = G.numel()
    c = float((G * W).sum()) / sg
    dc = gamma(n) * float((G * W).abs().sum()) / sg + 5 * U * abs(c)
    uv = torch.outer(u, v).abs()
    t = abs(c) * uv
    out = sg_ref(d, False)
    b = (dc * uv + 2 * U * t + U * (G.abs() + t)) / sg + 4 * U * out.abs()
    if accumulate:
        b = b + U * (d["old"].double().abs() + out.abs())
        out = out + d["old"].double()
    return out, SLACK * b


def sg_check(d, got, accumulate, what=""):
    """got [R, K] CPU fp32 -> the used share of the bound; asserts that it is at most 1"""
    ref, bnd = sg_bound(d, accumulate)
    assert not bool(torch.isnan(got).any()), f"{what}: NaN"
    share = float(((got.double() - ref).abs() / bnd).max())
    assert share <= 1.0, f"{what}: |error| / bound = {share:.3g}"
    return share


# ---------------------------------------------------------------------------------------------------------------
# 4. staging kernels: index maps on distinct integer codes
# ---------------------------------------------------------------------------------------------------------------
# (n, hid, c, cp): the real SPADE size with one and three norms; ...; 4 * 4096 * 72 = 1 179 648 outputs: a second trip
TAPS_CASES = [(1, 128, 7, 8), (3, 128, 7, 8), (4, 5, 3, 4), (2, 16, 8, 8), (1, 1, 1, 4), (2, 7, 13, 16), (4, 4096, 7, 8)]


@lru_cache(maxsize=2)
def taps_case(n, hid, c, cp):
    """ws [n][hid, c, 3, 3] and bs [n][hid]: distinct non-zero codes; dw [n * hid, 9 * cp] / db for the inverse map: codes in the live
    columns, POISON in the pad columns"""
    per = hid * c * 9
    ws = [(1 + i * per + torch.arange(per)).float().view(hid, c, 3, 3) for i in range(n)]
    bs = [(1 + n * per + i * hid + torch.arange(hid)).float() for i in range(n)]
    assert n * per + n * hid < 2 ** 24
    dw = torch.full((n * hid, 9, cp), POISON)
    dw[:, :, :c] = (2 ** 23 + torch.arange(n * hid * 9 * c)).float().view(n * hid, 9, c)
    return dict(ws=ws, bs=bs, dw=dw.view(n * hid, 9 * cp), db=(2 ** 22 + torch.arange(n * hid)).float())


def taps_prep_ref(ws, bs, cp, defect=None):
    """wt[(i * hid + o)][tap * cp + ch] = w_i[o][ch][tap] for ch < c, +0 in the pad columns; bt = the biases, concatenated"""
    hid, c = ws[0].shape[:2]
    wt = torch.full((len(ws) * hid, 9 * cp), NAN if defect == "pad_unwritten" else 0.0)
    for i, w in enumerate(ws):
        rows = wt[i * hid:(i + 1) * hid]
        if defect == "channel_major":
            rows[:, :9 * c] = w.reshape(hid, c * 9)
        else:
            rows.view(hid, 9, cp)[:, :, :c] = w.reshape(hid, c, 9).permute(0, 2, 1)
    return wt, torch.cat(bs)


def taps_grad_ref(dw, db, n, hid, c, cp, defect=None):
    """gw_i[o][ch][tap] = dw[(i * hid + o)][tap * cp + ch], gb_i = db[i * hid ..]"""
    if defect == "channel_major":
        g = dw[:, :9 * c].reshape(n, hid, c, 3, 3)
    else:
        g = dw.view(n, hid, 9, cp)[:, :, :, :c].permute(0, 1, 3, 2).reshape(n, hid, c, 3, 3)
    return [g[i].contiguous() for i in range(n)], list(db.view(n, hid))


VEC_C = [1, 3, 4, 5, 31, 32, 33, 63, 64, 65, 96, 100, 128, 130, 1024, 1040]
VEC_SPLIT = 32            # jobs per launch of the wrapper


def vec_sizes(C):
    return (C + 31) // 32 * 64, (C + 3) // 4 * 4


def vec_case(C, job=0):
    """gamma, beta, noise scale [C]: distinct non-zero codes, distinct between jobs"""
    i = torch.arange(C)
    return tuple((job * 4096 + 3 * i + k).float() for k in (1, 2, 3))


def vec_prep_ref(gamma_b, beta_b, ns, defect=None):
    """bc[64 g + l] = gamma[32 g + l] (l < 32) | beta[32 g + l - 32], zero where the channel is >= C; ns padded with zeros to ceil4(C)"""
    C = gamma_b.numel()
    ncols, Cp = vec_sizes(C)
    i = torch.arange(ncols)
    l, ch = i & 63, (i >> 6) * 32 + (i & 31)
    first, second = (beta_b, gamma_b) if defect == "halves_swapped" else (gamma_b, beta_b)
    pad = torch.tensor(NAN if defect == "no_zero_pad" else 0.0)
    chc = ch.clamp_max(C - 1)
    bc = torch.where(ch < C, torch.where(l < 32, first[chc], second[chc]), pad)
    return bc, torch.cat([ns, pad.expand(Cp - C)])


# tap_expand: out[n, h, w, t * Cp + c] = src[n, (h + kh - 1) << down, (w + kw - 1) << down, c], t = kh * 3 + kw, zero outside the image
# (bf16, Cp, down, N, H, W, sliced): H, W of the OUTPUT; the last two are one size past the cap of the grid (N H W 9 Cp / group > 4096 * 256)
TAP_CASES = [(False, 8, 0, 1, 1, 1, False), (False, 8, 0, 2, 2, 3, True), (False, 8, 1, 2, 5, 4, True), (False, 8, 2, 1, 5, 4, False),
             (True, 8, 0, 2, 2, 3, True), (True, 8, 1, 1, 1, 1, True), (True, 8, 2, 2, 5, 4, False), (True, 16, 0, 1, 5, 4, True),
             (True, 16, 1, 2, 2, 3, False), (True, 16, 2, 1, 1, 1, True), (False, 8, 0, 1, 243, 240, True), (True, 8, 1, 1, 342, 341, False)]


def tap_groups(case):
    bf16, Cp, down, N, H, W, _ = case
    return N * H * W * 9 * (Cp * (2 if bf16 else 4) // 16)


@lru_cache(maxsize=2)
def tap_source(case):
    """[N, H << down, W << down, Cp] in the storage type: non-zero codes, distinct within any window (fp32: 1 + index; bf16: the bit
    patterns 1 .. 0x7EFF in turn, all finite)"""
    bf16, Cp, down, N, H, W, _ = case
    shape = (N, H << down, W << down, Cp)
    idx = torch.arange(N * (H << down) * (W << down) * Cp)
    if bf16:
        return (1 + idx % 0x7EFF).to(torch.int16).view(torch.bfloat16).view(shape)
    assert idx.numel() < 2 ** 24
    return (1 + idx).float().view(shape)


def tap_expand_ref(src, down, H, W, defect=None):
    """-> [N, H, W, 9 * Cp] in the storage type of ``src``"""
    N, _, _, Cp = src.shape
    s = 1 if defect == "down_ignored" else 1 << down
    sub = src[:, ::s, ::s][:, :H, :W]
    if defect == "borders":                # the border reads the clamped neighbour instead of zero
        pad = sub[:, [0] + list(range(H)) + [H - 1]][:, :, [0] + list(range(W)) + [W - 1]]
    else:
        pad = torch.zeros(N, H + 2, W + 2, Cp, dtype=src.dtype)
        pad[:, 1:H + 1, 1:W + 1] = sub
    out = torch.empty(N, H, W, 9, Cp, dtype=src.dtype)
    for kh in range(3):
        for kw in range(3):
            out[:, :, :, (kw * 3 + kh) if defect == "khkw_swapped" else (kh * 3 + kw)] = pad[:, kh:kh + H, kw:kw + W]
    return out.view(N, H, W, 9 * Cp)


# ---------------------------------------------------------------------------------------------------------------
# 5. element-wise kernels
# ---------------------------------------------------------------------------------------------------------------
EW_N = [1, 3, 255, 256, 257, 1048575, 1048576, 1048577, 2 * 1048576 + 7]
SCALES = [(0.5, None), (3.0, None), (-2.0, 4.0), (0.25, -8.0), (5.0, 0.5)]        # (s_host, s_dev[0] or None)
ACT_RELU, ACT_LRELU = 1, 2
ACT_VARIANTS = [(ACT_RELU, 0.0), (ACT_LRELU, 0.25), (ACT_LRELU, 0.5)]


@lru_cache(maxsize=2)
def ew_operands(n):
    """x, dy: integers in [-64, 64]; y_tanh: multiples of 1/16 in [-1, 1] with +1, -1, +0, -0.0 at i % 8 == 0, 1, 2, 3;
    y_act: positive, negative, +0, -0.0 at i % 4 == 0, 1, 2, 3"""
    g = _gen(n, 95)
    i = torch.arange(n)
    x = int_tensor((n,), -64, 64, g)
    yt = int_tensor((n,), -16, 16, g) / 16.0
    for k, val in enumerate((1.0, -1.0, 0.0, -0.0)):
        yt = torch.where(i % 8 == k, torch.tensor(val), yt)
    mag = int_tensor((n,), 1, 8, g)
    ya = torch.where(i % 4 == 0, mag, torch.where(i % 4 == 1, -mag, torch.where(i % 4 == 2, torch.tensor(0.0), torch.tensor(-0.0))))
    return dict(x=x, dy=int_tensor((n,), -64, 64, g), y_tanh=yt, y_act=ya)


def scale_ref(x, s_host, s_dev, dtype=torch.float64):
    s = torch.tensor(s_host, dtype=dtype) * (torch.tensor(s_dev, dtype=dtype) if s_dev is not None else 1.0)
    return x.to(dtype) * s


def tanh_bwd_ref(dy, y, dtype=torch.float64):
    y = y.to(dtype)
    return dy.to(dtype) * (1.0 - y * y)


def act_bwd_ref(d, y, act, slope, defect=None, dtype=torch.float64):
    """d * (y > 0 ? 1 : (0 | slope)): the rule of dact"""
    pos = (y >= 0) if defect == "act_ge" else (y > 0)
    return d.to(dtype) * torch.where(pos, torch.tensor(1.0, dtype=dtype), torch.tensor(0.0 if act == ACT_RELU else slope, dtype=dtype))


def act_split(n):
    """n channel groups as npix pixels of C4 groups: C4 the largest divisor of n up to 32"""
    c4 = max(k for k in range(1, 33) if n % k == 0)
    return n // c4, c4
