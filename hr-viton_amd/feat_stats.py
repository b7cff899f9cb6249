"""Statistics over banks of Inception features for FID and KID (evaluate.py ``--fid``): float64 matrix products on the MI355X's
matrix cores (csrc/feat_stats.hip, ``v_mfma_f64_16x16x4_f64``), the small rest on the host in float64 numpy.

Device (no CPU path; results are bit-identical from run to run):
  ``gemm_nt(A, B, epilogue, param)``   C[i, j] = epi(sum_k A[i, k] * B[j, k]); fp32 or fp64 operands, fp64 products and result
  ``moments(feats)``                   (mean [D], cov [D, D]) of fp32 features [n, D] -- ``np.mean(axis=0)``, ``np.cov(rowvar=False)``
  ``poly_gram(X, Y)``                  KID's kernel matrix ((x . y) / D + 1)^3, [nx, ny]
  ``kid_subset_sums(Kxx, Kyy, Kxy, ix, iy)``   per subset the three sums the unbiased MMD^2 needs, [S, 3]
Host:
  ``frechet_distance(mu1, S1, mu2, S2)``, ``kid_subsets(n_pred, n_gt, m, S)``, ``kid(sums, m)``
  ``fid_kid(feats_pred, feats_gt, subsets, subset_size)``   the whole of it from two device-resident feature banks
The eigen-decomposition of the Frechet distance stays on the host: two ``numpy.linalg.eigh`` of [D, D] per run.
"""
from __future__ import annotations

from typing import Tuple

import numpy as np
import torch

from . import _lib
from ._lib import HrvError
from .ops import _stream

EPI_LINEAR, EPI_POLY3 = 0, 1
KID_SEED = 2020          # torch-fidelity's rng seed of the subset draw
KID_SUBSETS, KID_SUBSET_SIZE = 100, 1000


def _operand(t, what: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dim() != 2 or t.dtype not in (torch.float32, torch.float64):
        raise HrvError(f"{what}: expected a 2-D fp32 or fp64 CUDA tensor")
    return t.detach().contiguous()


def gemm_nt(A: torch.Tensor, B: torch.Tensor, epilogue: int = EPI_LINEAR, param: float = 1.0,
            symmetric: bool = False) -> torch.Tensor:
    """C fp64 [M, N] = epi(A [M, K] @ B [N, K]^T) with fp64 products.  ``epilogue`` EPI_LINEAR: ``s * param``; EPI_POLY3:
    ``(s / param + 1)^3``.  ``symmetric`` (B is A): one triangle is computed and mirrored."""
    A, B = _operand(A, "gemm_nt(A)"), _operand(B, "gemm_nt(B)")
    if A.dtype != B.dtype or A.shape[1] != B.shape[1] or A.device != B.device:
        raise HrvError(f"gemm_nt: operands {tuple(A.shape)} {A.dtype} and {tuple(B.shape)} {B.dtype} do not match")
    if symmetric and (A.data_ptr() != B.data_ptr() or A.shape != B.shape):
        raise HrvError("gemm_nt: symmetric needs B to be A")
    M, K = A.shape
    N = B.shape[0]
    if min(M, N, K) < 1:
        raise HrvError(f"gemm_nt: empty operand ({M}, {N}, {K})")
    out = torch.empty((M, N), dtype=torch.float64, device=A.device)
    lib = _lib.load()
    _lib.check(lib.hrv_gemm_nt_f64(A.data_ptr(), B.data_ptr(), int(A.dtype == torch.float64), M, N, K, K, K, epilogue, float(param),
                                   int(symmetric), out.data_ptr(), N, _stream()), "hrv_gemm_nt_f64")
    return out


def _features(feats, what: str) -> torch.Tensor:
    if not isinstance(feats, torch.Tensor) or not feats.is_cuda or feats.dim() != 2 or feats.dtype != torch.float32:
        raise HrvError(f"{what}: expected fp32 CUDA features [n, D]")
    return feats.detach().contiguous()


def moments(feats: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(mean fp64 [D], cov fp64 [D, D]) of fp32 features [n, D]: the mean summed in fp64 in row order; the covariance as the product
    of the centred, transposed bank (fp64 [D, n]) with itself times 1 / (n - 1), bitwise symmetric."""
    x = _features(feats, "moments")
    n, D = x.shape
    if n < 2:
        raise ValueError(f"moments: the covariance needs at least 2 rows, got {n}")
    lib = _lib.load()
    mean = torch.empty(D, dtype=torch.float64, device=x.device)
    xt = torch.empty((D, n), dtype=torch.float64, device=x.device)
    _lib.check(lib.hrv_feat_mean_f64(x.data_ptr(), n, D, mean.data_ptr(), _stream()), "hrv_feat_mean_f64")
    _lib.check(lib.hrv_feat_center_t_f64(x.data_ptr(), mean.data_ptr(), n, D, xt.data_ptr(), _stream()), "hrv_feat_center_t_f64")
    return mean, gemm_nt(xt, xt, EPI_LINEAR, 1.0 / (n - 1), symmetric=True)


def poly_gram(X: torch.Tensor, Y: torch.Tensor) -> torch.Tensor:
    """KID's polynomial kernel (degree 3, gamma 1 / D, coef0 1) between the rows of X [nx, D] and Y [ny, D]: fp64 [nx, ny]."""
    if X.shape[1] != Y.shape[1]:
        raise HrvError(f"poly_gram: feature widths {X.shape[1]} and {Y.shape[1]} differ")
    same = X.data_ptr() == Y.data_ptr() and X.shape == Y.shape and X.is_contiguous() and Y.is_contiguous()
    return gemm_nt(X, Y, EPI_POLY3, float(X.shape[1]), symmetric=same)


def kid_subset_sums(Kxx: torch.Tensor, Kyy: torch.Tensor, Kxy: torch.Tensor, ix, iy) -> torch.Tensor:
    """fp64 [S, 3]: per subset s the off-diagonal sum of Kxx[ix[s]][:, ix[s]], that of Kyy[iy[s]][:, iy[s]], and the full sum of
    Kxy[ix[s]][:, iy[s]].  ix, iy: integer [S, m] row numbers, unsorted, without repeats inside a subset."""
    dev = Kxx.device
    for t, nm in ((Kxx, "Kxx"), (Kyy, "Kyy"), (Kxy, "Kxy")):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float64 or t.dim() != 2 or not t.is_contiguous():
            raise HrvError(f"kid_subset_sums({nm}): expected a contiguous 2-D fp64 CUDA tensor")
    nx, ny = Kxx.shape[0], Kyy.shape[0]
    if Kxx.shape != (nx, nx) or Kyy.shape != (ny, ny) or Kxy.shape != (nx, ny):
        raise HrvError(f"kid_subset_sums: Gram shapes {tuple(Kxx.shape)}, {tuple(Kyy.shape)}, {tuple(Kxy.shape)} do not fit")
    ix = torch.as_tensor(np.asarray(ix.cpu() if isinstance(ix, torch.Tensor) else ix), dtype=torch.int32)
    iy = torch.as_tensor(np.asarray(iy.cpu() if isinstance(iy, torch.Tensor) else iy), dtype=torch.int32)
    if ix.dim() != 2 or ix.shape != iy.shape or ix.numel() == 0:
        raise HrvError(f"kid_subset_sums: index arrays {tuple(ix.shape)} and {tuple(iy.shape)} must be one [S, m] shape")
    S, m = ix.shape
    if m > min(nx, ny) or int(ix.min()) < 0 or int(ix.max()) >= nx or int(iy.min()) < 0 or int(iy.max()) >= ny:
        raise HrvError(f"kid_subset_sums: subsets of {m} with rows outside [0, {nx}) / [0, {ny})")
    ixd, iyd = ix.contiguous().to(dev), iy.contiguous().to(dev)
    out = torch.empty((S, 3), dtype=torch.float64, device=dev)
    lib = _lib.load()
    _lib.check(lib.hrv_kid_subset_sums_f64(Kxx.data_ptr(), nx, Kyy.data_ptr(), ny, Kxy.data_ptr(), ixd.data_ptr(), iyd.data_ptr(), S, m,
                                           out.data_ptr(), _stream()), "hrv_kid_subset_sums_f64")
    return out


# ------------------------------------------------------------------------------------------------------------------ host, float64
def _np64(a) -> np.ndarray:
    return np.asarray(a.detach().cpu() if isinstance(a, torch.Tensor) else a, dtype=np.float64)


def frechet_distance(mu1, sigma1, mu2, sigma2) -> float:
    """|mu1 - mu2|^2 + tr S1 + tr S2 - 2 sum_i sqrt(max(l_i, 0)), l the eigenvalues of S1^(1/2) S2 S1^(1/2) -- the trace of
    sqrtm(S1 S2), which has the same spectrum, without a non-symmetric matrix square root: real by construction and stable when fewer
    rows than features make the covariances singular.  Two symmetric eigen-decompositions.  Eigenvalues below the resolution of the
    decomposition (width x machine epsilon x the largest eigenvalue) are rounding noise around zero and count as zero: their square
    roots would put noise of the order 1e-8 into the sum for every null direction."""
    mu1, mu2, s1, s2 = _np64(mu1).ravel(), _np64(mu2).ravel(), _np64(sigma1), _np64(sigma2)
    D = mu1.shape[0]
    if mu2.shape != (D,) or s1.shape != (D, D) or s2.shape != (D, D):
        raise ValueError(f"frechet_distance: shapes {mu1.shape}, {s1.shape}, {mu2.shape}, {s2.shape} do not fit")
    eps = D * np.finfo(np.float64).eps
    w, V = np.linalg.eigh((s1 + s1.T) * 0.5)
    w = np.where(w > eps * max(float(w[-1]), 0.0), w, 0.0)
    half = V * np.sqrt(w)                      # S1^(1/2) = half @ V.T; the spectrum sought is that of half.T @ S2 @ half
    M = half.T @ s2 @ half
    lam = np.linalg.eigvalsh((M + M.T) * 0.5)
    lam = np.where(lam > eps * max(float(lam[-1]), 0.0), lam, 0.0)
    diff = mu1 - mu2
    return float(diff @ diff + np.trace(s1) + np.trace(s2) - 2.0 * np.sqrt(lam).sum())


def kid_subsets(n_pred: int, n_gt: int, subset_size: int = KID_SUBSET_SIZE, subsets: int = KID_SUBSETS,
                seed: int = KID_SEED) -> Tuple[np.ndarray, np.ndarray]:
    """torch-fidelity's subset draw: ``rng = np.random.RandomState(2020)``, then per subset ``rng.choice(n_pred, m, replace=False)``
    followed by ``rng.choice(n_gt, m, replace=False)``.  Returns (ix, iy) int32 [subsets, m]."""
    if subset_size < 2 or subsets < 1:
        raise ValueError(f"kid_subsets: {subsets} subsets of {subset_size}")
    if subset_size > min(n_pred, n_gt):
        raise ValueError(f"kid_subsets: subset size {subset_size} exceeds a set ({n_pred} predictions, {n_gt} ground truths)")
    rng = np.random.RandomState(seed)
    ix = np.empty((subsets, subset_size), np.int32)
    iy = np.empty((subsets, subset_size), np.int32)
    for s in range(subsets):
        ix[s] = rng.choice(n_pred, subset_size, replace=False)
        iy[s] = rng.choice(n_gt, subset_size, replace=False)
    return ix, iy


def kid(sums, m: int) -> Tuple[float, float]:
    """(mean, std) over the subsets of the unbiased MMD^2 = sxx / (m (m - 1)) + syy / (m (m - 1)) - 2 sxy / m^2 from
    ``kid_subset_sums``' rows (sxx, syy, sxy)."""
    s = _np64(sums).reshape(-1, 3)
    mmd = s[:, 0] / (m * (m - 1)) + s[:, 1] / (m * (m - 1)) - 2.0 * s[:, 2] / (m * m)
    return float(np.mean(mmd)), float(np.std(mmd))


def fid_kid(feats_pred: torch.Tensor, feats_gt: torch.Tensor, subsets: int = KID_SUBSETS,
            subset_size: int = KID_SUBSET_SIZE) -> Tuple[float, float, float]:
    """(FID, KID mean, KID std) between two device-resident fp32 feature banks [n, D]."""
    ix, iy = kid_subsets(feats_pred.shape[0], feats_gt.shape[0], subset_size, subsets)
    mu1, s1 = moments(feats_pred)
    mu2, s2 = moments(feats_gt)
    fid = frechet_distance(mu1, s1, mu2, s2)
    sums = kid_subset_sums(poly_gram(feats_pred, feats_pred), poly_gram(feats_gt, feats_gt), poly_gram(feats_pred, feats_gt), ix, iy)
    return (fid, *kid(sums, subset_size))
