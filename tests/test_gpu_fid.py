"""GPU: FID / KID on the HIP path -- the FID input kernel, pool modes 2 and 3, the fp64 matrix-core GEMM with both epilogues, the
moments, KID's subset sums, the changed blocks and the whole FID Inception-v3, and evaluate.py --fid end to end -- against the float64
restatements of tests/fid_cases.py.

Where a limit is not exact equality it comes from the reference side: the standard bound of a reordered dot product for the GEMM and
the moments, the error of torch's own fp32 CPU path against the same float64 restatement for the input kernel and the network.  Every
test prints its figures before it asserts.
"""
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fid_cases as Fc
import inception_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
U = 2.0 ** -53
SENTINEL = -7168.0
FACTOR = 4.0          # the block allowance of tests/test_gpu_inception.py


@pytest.fixture(scope="module")
def I():
    import hr_viton_amd  # noqa: F401
    from hr_viton_amd import inception
    return inception


@pytest.fixture(scope="module")
def S():
    import hr_viton_amd  # noqa: F401
    from hr_viton_amd import feat_stats
    return feat_stats


def _nhwc(x, cstride=None, coff=0, fill=0.0):
    from hr_viton_amd.ops import Act
    N, C, H, W = x.shape
    cs = C if cstride is None else cstride
    t = torch.full((N, H, W, cs), fill, dtype=torch.float32)
    t[..., coff:coff + C] = x.permute(0, 2, 3, 1)
    return Act(t.cuda(), C, coff)


def _nchw(a, c0=0, c=None):
    c = a.C - c0 if c is None else c
    return a.t[..., a.coff + c0:a.coff + c0 + c].permute(0, 3, 1, 2).cpu()


# ---------------------------------------------------------------------------------------------------------- the input kernel
def _prep(img_u8):
    from hr_viton_amd import _lib, ops
    x = torch.from_numpy(img_u8).cuda()
    N, H, W, _ = x.shape
    out = torch.full((N, 299, 299, 4), float("nan"), dtype=torch.float32, device="cuda")
    _lib.check(_lib.load().hrv_fid_prep_u8(x.data_ptr(), N, H, W, 299, 299, out.data_ptr(), ops._stream()), "hrv_fid_prep_u8")
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("H,W", Fc.PREP_SIZES, ids=lambda v: str(v))
def test_fid_prep_against_float64(I, N, H, W):
    rng = np.random.default_rng(H * 7 + W + N)
    img = rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
    want = Fc.prep64(img)
    torch_err = np.abs(Fc.prep_torch32(img).astype(np.float64) - want).max()
    got = _prep(img)
    err = np.abs(got[..., :3].astype(np.float64) - want).max()
    print(f"fid_prep {N}x{H}x{W}: kernel {err:.3e}, torch fp32 CPU F.interpolate {torch_err:.3e} against float64 (limit 2 x the latter)")
    assert got.shape == (N, 299, 299, 4) and (got[..., 3] == 0).all()
    assert err <= 2.0 * torch_err, (err, torch_err)


def _nearest_f32(q: Fraction) -> np.float32:
    """the fp32 nearest to a rational, decided in exact arithmetic"""
    c = np.float32(float(q))
    cands = [c, np.nextafter(c, np.float32(-np.inf)), np.nextafter(c, np.float32(np.inf))]
    return min(cands, key=lambda v: abs(Fraction(float(v)) - q))


def test_fid_prep_constant_images_are_exact(I):
    for c in (0, 1, 2, 85, 127, 128, 200, 254, 255):
        for H, W in ((5, 7), (300, 301)):
            got = _prep(np.full((1, H, W, 3), c, np.uint8))
            want = _nearest_f32(Fraction(2 * c, 255) - 1)
            assert (got[..., :3] == want).all(), (c, H, W, want, np.unique(got[..., :3]))


# ---------------------------------------------------------------------------------------------------------- pools
def _pool_case(N, H, W, C, seed, exact=False):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, C, H, W, generator=g) * (1.0 + 3.0 * torch.rand(1, C, 1, 1, generator=g))
    if exact:        # multiples of 2^-10 below 2^6: nine of them add exactly in double, in any order
        x = (x * 1024).round().clamp(-65535, 65535) / 1024
    return x


def _run_pool(I, x, mode, Ho, Wo):
    from hr_viton_amd.ops import Act
    N, C = x.shape[:2]
    src = _nhwc(x, cstride=C + 12, coff=4, fill=3.0e3)
    out = Act(torch.full((N, Ho, Wo, C + 20), SENTINEL, dtype=torch.float32, device="cuda"), C, 8)
    I.pool3x3(src, mode, out)
    torch.cuda.synchronize()
    full = out.t.cpu()
    assert (full[..., :8] == SENTINEL).all() and (full[..., 8 + C:] == SENTINEL).all()
    return _nchw(out)


@pytest.mark.parametrize("N,H,W,C", Fc.POOL_SHAPES)
def test_pool_max_same(I, N, H, W, C):
    x = _pool_case(N, H, W, C, H * 100 + W + 3)
    got = _run_pool(I, x, 3, H, W)
    assert torch.equal(got, F.max_pool2d(x, 3, 1, 1))
    dense = I.pool3x3(_nhwc(x), 3)
    assert dense.t.shape == (N, H, W, C) and torch.equal(_nchw(dense), got)
    # padding never wins, whatever the sign of the data
    assert torch.equal(_run_pool(I, -x.abs() - 1.0, 3, H, W), F.max_pool2d(-x.abs() - 1.0, 3, 1, 1))


@pytest.mark.parametrize("N,H,W,C", Fc.POOL_SHAPES)
def test_pool_avg_inside(I, N, H, W, C):
    x = _pool_case(N, H, W, C, H * 100 + W + 2)
    want = F.avg_pool2d(x.double(), 3, 1, 1, count_include_pad=False)
    got = _run_pool(I, x, 2, H, W)
    # at most nine additions and one division: at most 2 fp32 ulps of the float64 result (the criterion of the mode-1 test)
    ulp = torch.from_numpy(np.spacing(np.abs(want.float().numpy()))).double()
    worst = ((got.double() - want).abs() / ulp).max().item()
    print(f"avg-pool over the taps inside {N}x{H}x{W}x{C}: worst error {worst:.3f} ulp")
    assert worst <= 2.0, worst
    # a constant image stays constant up to the border: the divisor is the number of taps inside (4, 6, 9), not 9
    ones = _run_pool(I, torch.full((N, C, H, W), 3.0), 2, H, W)
    assert (ones == 3.0).all()


def test_pool_modes_0_and_1_keep_their_bits(I):
    """On inputs whose window sums are exact in double the two existing modes are determined bit for bit by their definition: the
    maximum, and the double sum divided by 9 rounded to fp32 once.  torch states both."""
    N, H, W, C = 3, 23, 38, 20
    x = _pool_case(N, H, W, C, 77, exact=True)
    want0 = F.max_pool2d(x, 3, 2)
    assert torch.equal(_run_pool(I, x, 0, *want0.shape[2:]), want0)
    want1 = F.avg_pool2d(x.double(), 3, 1, 1).float()
    assert torch.equal(_run_pool(I, x, 1, H, W), want1)
    # and mode 2 differs from mode 1 on the border only
    m2 = _run_pool(I, x, 2, H, W)
    assert torch.equal(m2[..., 1:-1, 1:-1], want1[..., 1:-1, 1:-1]) and not torch.equal(m2, want1)


def test_pool_bad_mode_raises(I):
    from hr_viton_amd import _lib, ops
    a = _nhwc(torch.zeros(1, 4, 9, 9))
    out = torch.zeros((1, 9, 9, 4), device="cuda")
    rc = _lib.load().hrv_pool3x3_nhwc_f32(a.t.data_ptr(), 1, 9, 9, 4, 4, 0, 4, out.data_ptr(), 4, 0, ops._stream())
    assert rc != 0 and b"mode 4" in _lib.load().hrv_last_error()


# ---------------------------------------------------------------------------------------------------------- fp64 GEMM
def _poly3(s, D):
    t = s / D + 1.0
    return (t * t) * t


def _operands(M, N, k, dtype, integer, seed):
    rng = np.random.default_rng(seed)
    if integer:
        A, B = rng.integers(-8, 9, (M, k)), rng.integers(-8, 9, (N, k))
    else:
        A, B = rng.standard_normal((M, k)) * (0.5 + rng.random((1, k))), rng.standard_normal((N, k)) + 0.25
    return A.astype(dtype), B.astype(dtype)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("M,N,k", Fc.GEMM_SHAPES, ids=lambda v: str(v))
def test_gemm_integer_operands_are_bit_exact(S, M, N, k, dtype):
    """|v| <= 8: every product and every partial sum is an integer below 2^53, so any summation order gives the same number"""
    A, B = _operands(M, N, k, dtype, True, M + N + k)
    s = A.astype(np.float64) @ B.astype(np.float64).T
    assert np.array_equal(s, np.rint(s))
    a, b = torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda()
    lin = S.gemm_nt(a, b, S.EPI_LINEAR, 0.375).cpu().numpy()
    assert lin.dtype == np.float64 and lin.shape == (M, N) and np.array_equal(lin, s * 0.375)
    # poly3 in the kernel's operation order: t = s / D + 1, (t * t) * t.  With k = 2048 = D the quotient is exact as well.
    got = S.poly_gram(a, b).cpu().numpy()
    assert np.array_equal(got, _poly3(s, float(k)))
    if k == 2048:
        assert np.array_equal(s / 2048.0 * 2048.0, s)
    assert np.array_equal(S.gemm_nt(a, b, S.EPI_POLY3, 2048.0).cpu().numpy(), _poly3(s, 2048.0))


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("M,N,k", Fc.GEMM_SHAPES, ids=lambda v: str(v))
def test_gemm_gaussian_operands_within_the_dot_product_bound(S, M, N, k, dtype):
    A, B = _operands(M, N, k, dtype, False, 3 * M + N + k)
    A64, B64 = A.astype(np.float64), B.astype(np.float64)
    s = A64 @ B64.T
    bound = 2.0 * k * U * (np.abs(A64) @ np.abs(B64).T)          # a reordered dot product of k terms
    a, b = torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda()
    lin = S.gemm_nt(a, b).cpu().numpy()
    e = np.abs(lin - s)
    print(f"gemm linear {M}x{N}x{k} {np.dtype(dtype).name}: worst error / bound {np.max(e / bound):.3e}")
    assert (e <= bound).all()
    # through the cube to first order: |d (s/D + 1)^3| = 3 (s/D + 1)^2 / D |ds|, plus 4 ulp for the epilogue's four operations
    want = _poly3(s, float(k))
    pb = 3.0 * (s / k + 1.0) ** 2 / k * bound + 4.0 * np.spacing(np.abs(want))
    got = S.poly_gram(a, b).cpu().numpy()
    pe = np.abs(got - want)
    print(f"gemm poly3  {M}x{N}x{k} {np.dtype(dtype).name}: worst error / bound {np.max(pe / pb):.3e}")
    assert (pe <= pb).all()
    # the symmetric form: one triangle mirrored, bitwise symmetric, the same numbers
    sym = S.gemm_nt(a, a, symmetric=True).cpu().numpy()
    assert np.array_equal(sym, sym.T) and np.array_equal(np.triu(sym), np.triu(S.gemm_nt(a, a).cpu().numpy()))
    # bit-identical from run to run
    assert np.array_equal(S.gemm_nt(a, b).cpu().numpy(), lin) and np.array_equal(S.poly_gram(a, b).cpu().numpy(), got)


def test_gemm_bad_arguments_raise(S):
    from hr_viton_amd._lib import HrvError
    a = torch.zeros(4, 8, device="cuda")
    with pytest.raises(HrvError):
        S.gemm_nt(a, torch.zeros(4, 9, device="cuda"))
    with pytest.raises(HrvError):
        S.gemm_nt(a, a.double())
    with pytest.raises(HrvError):
        S.gemm_nt(a.cpu(), a.cpu())
    with pytest.raises(HrvError):
        S.gemm_nt(a, torch.zeros(4, 8, device="cuda"), symmetric=True)
    with pytest.raises(HrvError):
        S.gemm_nt(a, a, S.EPI_POLY3, 0.0)


# ---------------------------------------------------------------------------------------------------------- moments
@pytest.mark.parametrize("n,D", Fc.MOMENT_SHAPES)
def test_moments_integer_features_are_exact(S, n, D):
    rng = np.random.default_rng(n + D)
    x = rng.integers(-8, 9, (n, D)).astype(np.int64)
    x[-1] += n * np.rint(x.sum(0) / n).astype(np.int64) - x.sum(0)          # column sums divisible by n
    assert (x.sum(0) % n == 0).all() and np.abs(x).max() < 2 ** 12
    mean, cov = S.moments(torch.from_numpy(x.astype(np.float32)).cuda())
    mean, cov = mean.cpu().numpy(), cov.cpu().numpy()
    m = x.sum(0) // n
    xc = (x - m).astype(np.float64)
    assert mean.dtype == np.float64 and np.array_equal(mean, m.astype(np.float64))
    assert cov.shape == (D, D) and np.array_equal(cov, (xc.T @ xc) * (1.0 / (n - 1)))          # covariance * (n - 1) is an integer
    assert np.array_equal(cov, cov.T)


@pytest.mark.parametrize("n,D", Fc.MOMENT_SHAPES)
def test_moments_gaussian_features(S, n, D):
    rng = np.random.default_rng(5 * n + D)
    x32 = (rng.standard_normal((n, D)) * (0.2 + rng.random((1, D))) + rng.standard_normal((1, D))).astype(np.float32)
    x = x32.astype(np.float64)
    feats = torch.from_numpy(x32).cuda()
    mean, cov = S.moments(feats)
    torch.cuda.synchronize()
    mean_np, cov_np = mean.cpu().numpy(), cov.cpu().numpy()
    want_mean, want_cov = x.mean(axis=0), np.cov(x, rowvar=False)
    me = np.abs(mean_np - want_mean)
    mb = 2.0 * n * U * np.abs(x).sum(axis=0) / n
    xc = np.abs(x - want_mean)
    cb = 2.0 * n * U * (xc.T @ xc) / (n - 1)
    ce = np.abs(cov_np - want_cov)
    print(f"moments {n}x{D}: mean error / bound {np.max(me / mb):.3e}, covariance error / bound {np.max(ce / cb):.3e}, "
          f"rank {np.linalg.matrix_rank(want_cov) if D <= 64 else min(n - 1, D)}")
    assert (me <= mb).all() and (ce <= cb).all()
    assert np.array_equal(cov_np, cov_np.T)
    mean2, cov2 = S.moments(feats)
    assert torch.equal(mean2, mean) and torch.equal(cov2, cov)


def test_moments_needs_two_rows(S):
    with pytest.raises(ValueError):
        S.moments(torch.zeros(1, 16, device="cuda"))
    from hr_viton_amd._lib import HrvError
    with pytest.raises(HrvError):
        S.moments(torch.zeros(4, 16, device="cuda", dtype=torch.float64))


# ---------------------------------------------------------------------------------------------------------- KID subset sums
def _perm_subsets(n, S_, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.permutation(n) for _ in range(S_)]).astype(np.int32)


KID_CASES = {"9-11-m5": (9, 11, Fc.SUBSETS_9_11_5_3), "11-9-m5": (11, 9, (Fc.SUBSETS_9_11_5_3[1], Fc.SUBSETS_9_11_5_3[0])),
             "9-9-m9": (9, 9, (_perm_subsets(9, 3, 1), _perm_subsets(9, 3, 2))), "11-11-m11": (11, 11, (_perm_subsets(11, 3, 3),
                                                                                                   _perm_subsets(11, 3, 4)))}


@pytest.mark.parametrize("case", list(KID_CASES))
def test_kid_subset_sums(S, case):
    nx, ny, (ix, iy) = KID_CASES[case]
    ix, iy = np.asarray(ix, np.int32), np.asarray(iy, np.int32)
    m = ix.shape[1]
    assert not np.array_equal(ix, np.sort(ix, axis=1))          # unsorted
    rng = np.random.default_rng(nx + ny)
    for integer in (True, False):
        if integer:
            Ks = [rng.integers(-1000, 1000, sh).astype(np.float64) for sh in ((nx, nx), (ny, ny), (nx, ny))]
        else:
            Ks = [rng.standard_normal(sh) * 10.0 ** rng.integers(-3, 4, sh) for sh in ((nx, nx), (ny, ny), (nx, ny))]
        dev = [torch.from_numpy(k).cuda() for k in Ks]
        got = S.kid_subset_sums(*dev, ix, iy)
        assert got.shape == (3, 3) and got.dtype == torch.float64
        got_np = got.cpu().numpy()
        # the reference sums what the kernel sums (the diagonal is left out, not subtracted) with math.fsum: exact
        import math
        want = np.empty((3, 3))
        mass = np.empty((3, 3))
        for s in range(3):
            subs = (Ks[0][np.ix_(ix[s], ix[s])], Ks[1][np.ix_(iy[s], iy[s])], Ks[2][np.ix_(ix[s], iy[s])])
            for w, sub in enumerate(subs):
                vals = sub[~np.eye(m, dtype=bool)] if w < 2 else sub.ravel()
                want[s, w], mass[s, w] = math.fsum(vals), math.fsum(np.abs(vals))
        if integer:
            assert np.array_equal(got_np, want)
            assert np.array_equal(want, Fc.subset_sums64(*Ks, ix, iy))
        else:
            e = np.abs(got_np - want)
            print(f"kid_subset_sums {case}: worst error / (m^2 u sum|K|) {np.max(e / (m * m * U * mass)):.3e}")
            assert (e <= m * m * U * mass).all()
        assert torch.equal(S.kid_subset_sums(*dev, torch.from_numpy(ix).cuda(), torch.from_numpy(iy)), got)
    from hr_viton_amd._lib import HrvError
    bad = ix.copy()
    bad[0, 0] = nx
    with pytest.raises(HrvError):
        S.kid_subset_sums(*dev, bad, iy)


# ---------------------------------------------------------------------------------------------------------- the network
@pytest.fixture(scope="module")
def ref():
    return K.reference_run(0)


@pytest.fixture(scope="module")
def net(I, ref):
    m = I.FIDInceptionV3()
    m.load_state_dict(Fc.fid_state_dict(ref["sd"]))
    return m.eval()


@pytest.mark.parametrize("name", Fc.CHANGED_BLOCKS)
def test_fid_block_branches(I, net, ref, name):
    """One block of each changed type on the input and with the allowance of tests/test_gpu_inception.py's block test: every branch
    slice against float64, bounded by 4 x the error of the fp32 CPU run of the same block."""
    x32 = ref["io"][name][0][:4].float()
    with torch.no_grad():
        want = Fc.BLOCK_FN[name](K._Run(ref["sd"], torch.float64), name, x32.double())
        cpu = Fc.BLOCK_FN[name](K._Run(ref["sd"], torch.float32), name, x32)
        plain = K.BLOCK_FN[name](K._Run(ref["sd"], torch.float64), name, x32.double())
    out = net.run_block(name, _nhwc(x32))
    torch.cuda.synchronize()
    assert out.C == sum(b.shape[1] for b in want) and (out.H, out.W) == tuple(want[0].shape[2:])
    off = 0
    for k, (w64, c32) in enumerate(zip(want, cpu)):
        got = _nchw(out, off, w64.shape[1])
        off += w64.shape[1]
        err = (got.double() - w64).abs().max().item()
        err_cpu = (c32.double() - w64).abs().max().item()
        print(f"FID {name} branch {k} [{w64.shape[1]} ch]: HIP {err:.3e}, torch fp32 CPU {err_cpu:.3e}, |ref| max {w64.abs().max().item():.3f}")
        assert err <= FACTOR * err_cpu, (name, k, err, err_cpu)
    # the case tells the two networks apart: torchvision's pooled branch is further away than the allowance
    gap = (plain[-1] - want[-1]).abs().max().item()
    assert gap > 10 * FACTOR * (cpu[-1].double() - want[-1]).abs().max().item(), gap


def test_fid_network_features(I, net, ref):
    """Pooled features of 4 images at 299 x 299 (where the input kernel's resize is the identity) on the calibrated weights: batch of
    4 and 4 singles against the float64 restatement.  The limit is twice what torch's fp32 CPU run of the restatement shows against
    float64, per image relative to the feature's norm."""
    img = ref["img"][:4]
    x64 = Fc.prep64(img)
    x32 = torch.from_numpy(x64.astype(np.float32)).permute(0, 3, 1, 2).contiguous()
    assert np.array_equal(x32.permute(0, 2, 3, 1).numpy().astype(np.float64), x64.astype(np.float32).astype(np.float64))
    with torch.no_grad():
        f64 = Fc.forward(ref["sd"], x32, torch.float64)
        f32 = Fc.forward(ref["sd"], x32, torch.float32).double()
    norm = f64.norm(dim=1)

    def rel(f):
        return ((f.double().cpu() - f64).norm(dim=1) / norm).max().item()

    dev = torch.from_numpy(img).cuda()
    batch = net.features_u8(dev)
    singles = torch.cat([net.features_u8(dev[i:i + 1]) for i in range(4)])
    bank = torch.full((6, 2048), SENTINEL, dtype=torch.float32, device="cuda")
    net.features_u8(dev, out=bank[1:5])
    torch.cuda.synchronize()
    assert batch.shape == (4, 2048) and batch.dtype == torch.float32
    cpu_err, err_b, err_s = rel(f32), rel(batch), rel(singles)
    vs = ((batch.double() - singles.double()).norm(dim=1).cpu() / norm).max().item()
    print(f"FID features, relative to the feature norm: torch fp32 CPU {cpu_err:.3e}, HIP batch of 4 {err_b:.3e}, HIP 4 singles "
          f"{err_s:.3e}, batch against singles {vs:.3e} (limit 2 x the first); feature norm {norm.min().item():.3f} .. "
          f"{norm.max().item():.3f}")
    assert cpu_err <= 1e-3, f"torch's own fp32 error {cpu_err} says the case is ill-chosen"
    assert err_b <= 2.0 * cpu_err and err_s <= 2.0 * cpu_err and vs <= 2.0 * cpu_err, (err_b, err_s, vs, cpu_err)
    # rows of a bank: the same bits, the neighbours untouched; repeat runs: the same bits
    assert torch.equal(bank[1:5], batch) and (bank[0] == SENTINEL).all() and (bank[5] == SENTINEL).all()
    assert torch.equal(net.features_u8(dev), batch)
    # images differ, and the features tell them apart
    assert (f64[0] - f64[1]).norm().item() > 1e-2 * norm.max().item()


# ---------------------------------------------------------------------------------------------------------- evaluate.py
def _fid_line(line):
    parts = line.split(" / ")
    assert len(parts) == 3 and parts[0].startswith("FID : ") and parts[1].startswith("KID_mean : ") and \
        parts[2].startswith("KID_std : "), line
    return float(parts[0][6:]), float(parts[1][11:]), float(parts[2][10:])


def test_evaluate_fid_end_to_end(I, tmp_path):
    from PIL import Image
    gt_dir, pr_dir = tmp_path / "gt", tmp_path / "pred"
    gt_dir.mkdir()
    pr_dir.mkdir()
    pr_names = Fc.write_pngs(pr_dir, 12, 21)
    gt_names = Fc.write_pngs(gt_dir, 14, 22)
    argv = ["--predict_dir", str(pr_dir), "--ground_truth_dir", str(gt_dir), "--fid_only", "--fid_random_init", "--kid_subsets", "4",
            "--kid_subset_size", "8", "--resolution", "1024", "-j", "0", "--fid_inception_weights", str(tmp_path / "none.pth")]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "evaluate.py")] + argv, capture_output=True, text=True, timeout=600,
                       cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "RANDOMLY initialised" in r.stderr and "plumbing only" in r.stdout
    lines = (pr_dir / "eval.txt").read_text().splitlines()
    assert len(lines) == 2 and lines[1] == "FID Inception weights : random init (plumbing only)" and not (pr_dir / "lpips.txt").exists()
    got = _fid_line(lines[0])
    # the host restatement, fed with features_u8 of the same images on the weights the script builds (torch.manual_seed(seed), then
    # the module)
    torch.manual_seed(0)
    net = I.FIDInceptionV3().eval()
    fp = net.features_u8(torch.from_numpy(Fc.read_images(pr_dir, pr_names)).cuda()).cpu().numpy()
    fg = net.features_u8(torch.from_numpy(Fc.read_images(gt_dir, gt_names)).cuda()).cpu().numpy()
    want = Fc.fid_kid64(fp, fg, 4, 8)
    print(f"evaluate.py --fid_only: {got}; host restatement {want}; SVD form of the distance {Fc.frechet_svd(fp, fg)!r}")
    for g, w in zip(got, want):
        assert np.isfinite(g) and abs(g - w) <= 1e-9 * abs(w), (got, want)
    assert got[0] > 0 and got[2] > 0
    # a second run appends an identical line (in this process: the same entry point)
    import importlib
    ev = importlib.import_module("evaluate")
    res = ev.main(argv)
    lines = (pr_dir / "eval.txt").read_text().splitlines()
    assert len(lines) == 4 and lines[2] == lines[0] and lines[3] == lines[1]
    assert (res["fid"], res["kid_mean"], res["kid_std"]) == got and res["fid_images"] == [12, 14]
    # --fid together with the paired metrics on 12 + 12 images: today's two lines plus the new one (and the labels of the random
    # initialisations)
    gt2, pr2 = tmp_path / "gt2", tmp_path / "pred2"
    gt2.mkdir()
    pr2.mkdir()
    for i, nm in enumerate(pr_names):
        Image.open(pr_dir / nm).save(pr2 / f"{i:05d}_00_{(i + 1) % 12:05d}_00.png")
        Image.open(gt_dir / gt_names[i]).convert("RGB").save(gt2 / f"{i:05d}_00.jpg", quality=95)
    res = ev.main(["--predict_dir", str(pr2), "--ground_truth_dir", str(gt2), "--fid", "--fid_random_init", "--kid_subsets", "4",
                   "--kid_subset_size", "8", "-j", "0", "--lpips_random_init", "--lpips_weights", str(tmp_path / "no.pth"),
                   "--alexnet_weights", str(tmp_path / "no2.pth"), "--inception_weights", str(tmp_path / "no3.pth"),
                   "--fid_inception_weights", str(tmp_path / "none.pth")])
    lines = (pr2 / "eval.txt").read_text().splitlines()
    assert len(lines) == 5, lines
    assert lines[0] == f"SSIM : {res['ssim']} / MSE : {res['mse']} / LPIPS : {res['lpips']}" and lines[1] == "IS_mean : nan / IS_std : nan"
    assert lines[2] == "LPIPS weights : random init (plumbing only)"          # (today's label of today's lines)
    assert _fid_line(lines[3]) == (res["fid"], res["kid_mean"], res["kid_std"])
    assert lines[4] == "FID Inception weights : random init (plumbing only)"
    assert len((pr2 / "lpips.txt").read_text().splitlines()) == 12 and 0.0 < res["ssim"] < 1.0 and np.isfinite(res["fid"])
