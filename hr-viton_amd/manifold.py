"""Nearest-neighbour manifold statistics over banks of Inception features (evaluate.py ``--prdc``): improved precision / recall
(Kynkaanniemi et al., NeurIPS 2019) and density / coverage (Naeem et al., ICML 2020) as Naeem et al.'s ``prdc`` computes them, in
float64 on squared Euclidean distances (csrc/manifold.hip; the dot products on ``v_mfma_f64_16x16x4_f64``).

Device (no CPU path; results are bit-identical from run to run):
  ``row_sqnorm(X)``                        |x_i|^2 of fp32 rows, fp64 [n]
  ``sqdist(X, Y, normX, normY, self_offset)``   max(0, |x_i|^2 + |y_j|^2 - 2 x_i . y_j), fp64 [nx, ny]; with ``self_offset`` >= 0 the
                                           entry (i, self_offset + i) is +inf
  ``row_kth(d, k)``                        the k-th smallest of every row, fp64 [rows]
  ``row_ball(d, r_col)``                   (#{j : d[i, j] < r_col[j]} int32 [rows], min_j d[i, j] fp64 [rows])
  ``knn_radii(X, k)``                      the squared distance of every row to its k-th nearest other row (own index excluded)
  ``prdc_parts(real, fake, k)``            the radii, ball counts and minima the four numbers are made of, as device tensors
Host:
  ``prdc(real, fake, k)``                  dict(precision, recall, density, coverage, k, n_real, n_fake)

With ``rR`` / ``rF`` the radii inside the real / fake bank: ``cntF[j] = #{i : d2(F_j, R_i) < rR[i]}``, precision the fraction of
``cntF > 0``, density ``sum cntF / (k nf)``; ``cntR[i] = #{j : d2(R_i, F_j) < rF[j]}``, recall the fraction of ``cntR > 0``; coverage
the fraction of ``min_j d2(R_i, F_j) < rR[i]``.  Every comparison is strict.  The left operand goes through in slabs of at most
``slab_rows`` rows, so the largest live distance block is ``slab_rows x n`` fp64.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import HrvError
from .ops import _stream

SLAB_ROWS = 4096


def kth_max() -> int:
    """the largest k ``row_kth`` serves (hrv_row_kth_max(): a compile-time constant of the library)"""
    return int(_lib.load().hrv_row_kth_max())


def _bank(t, what: str) -> torch.Tensor:
    """fp32 CUDA rows [n, D] with unit column stride; a row stride above D is passed on as the leading dimension"""
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dim() != 2 or t.dtype != torch.float32 or min(t.shape) < 1:
        raise HrvError(f"{what}: expected non-empty fp32 CUDA features [n, D]")
    t = t.detach()
    if t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        t = t.contiguous()
    return t


def _block(d, what: str) -> torch.Tensor:
    if not isinstance(d, torch.Tensor) or not d.is_cuda or d.dim() != 2 or d.dtype != torch.float64 or min(d.shape) < 1:
        raise HrvError(f"{what}: expected a non-empty 2-D fp64 CUDA tensor")
    d = d.detach()
    if d.stride(1) != 1 or (d.shape[0] > 1 and d.stride(0) < d.shape[1]):
        d = d.contiguous()
    return d


def _ld(t: torch.Tensor) -> int:
    return int(t.stride(0)) if t.shape[0] > 1 else int(t.shape[1])


def _vector(v, n: int, what: str) -> torch.Tensor:
    if not isinstance(v, torch.Tensor) or not v.is_cuda or v.dtype != torch.float64 or v.shape != (n,):
        raise HrvError(f"{what}: expected an fp64 CUDA vector of {n}")
    return v.detach().contiguous()


def row_sqnorm(X: torch.Tensor) -> torch.Tensor:
    """fp64 [n]: the sum of the squares of every fp32 row, squared and added in fp64"""
    x = _bank(X, "row_sqnorm")
    n, D = x.shape
    out = torch.empty(n, dtype=torch.float64, device=x.device)
    _lib.check(_lib.load().hrv_row_sqnorm_f64(x.data_ptr(), n, D, _ld(x), out.data_ptr(), _stream()), "hrv_row_sqnorm_f64")
    return out


def sqdist(X: torch.Tensor, Y: torch.Tensor, normX: Optional[torch.Tensor] = None, normY: Optional[torch.Tensor] = None,
           self_offset: int = -1) -> torch.Tensor:
    """fp64 [nx, ny]: squared Euclidean distances between the rows of X and of Y from their squared norms (computed here when not
    given) and fp64 dot products.  ``self_offset`` >= 0: X is the slab of Y that starts there, and every row's own entry is +inf."""
    x, y = _bank(X, "sqdist(X)"), _bank(Y, "sqdist(Y)")
    if x.shape[1] != y.shape[1] or x.device != y.device:
        raise HrvError(f"sqdist: banks {tuple(x.shape)} and {tuple(y.shape)} do not match")
    nx, D = x.shape
    ny = y.shape[0]
    nX = _vector(row_sqnorm(x) if normX is None else normX, nx, "sqdist(normX)")
    nY = _vector(row_sqnorm(y) if normY is None else normY, ny, "sqdist(normY)")
    out = torch.empty((nx, ny), dtype=torch.float64, device=x.device)
    _lib.check(_lib.load().hrv_sqdist_nt_f64(x.data_ptr(), y.data_ptr(), nx, ny, D, _ld(x), _ld(y), nX.data_ptr(), nY.data_ptr(),
                                             int(self_offset), out.data_ptr(), ny, _stream()), "hrv_sqdist_nt_f64")
    return out


def row_kth(d: torch.Tensor, k: int) -> torch.Tensor:
    """fp64 [rows]: the k-th smallest of every row (with multiplicity; +inf sorts last), 1 <= k <= min(kth_max(), n)"""
    d = _block(d, "row_kth")
    rows, n = d.shape
    out = torch.empty(rows, dtype=torch.float64, device=d.device)
    _lib.check(_lib.load().hrv_row_kth_f64(d.data_ptr(), rows, n, _ld(d), int(k), out.data_ptr(), _stream()), "hrv_row_kth_f64")
    return out


def row_ball(d: torch.Tensor, r_col: torch.Tensor, count: bool = True, minimum: bool = True
             ) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]:
    """(cnt int32 [rows], dmin fp64 [rows]): per row the number of entries strictly below their column's radius, and the row
    minimum; an output that is not asked for is None"""
    d = _block(d, "row_ball")
    rows, n = d.shape
    r = _vector(r_col, n, "row_ball(r_col)")
    if not (count or minimum):
        raise HrvError("row_ball: neither output asked for")
    cnt = torch.empty(rows, dtype=torch.int32, device=d.device) if count else None
    dmin = torch.empty(rows, dtype=torch.float64, device=d.device) if minimum else None
    _lib.check(_lib.load().hrv_row_ball_f64(d.data_ptr(), r.data_ptr(), rows, n, _ld(d), cnt.data_ptr() if count else None,
                                            dmin.data_ptr() if minimum else None, _stream()), "hrv_row_ball_f64")
    return cnt, dmin


# ------------------------------------------------------------------------------------------------------------------ the metric
def _check_k(k: int, slab_rows: int, *counts: int):
    if not isinstance(k, (int, np.integer)) or isinstance(k, bool) or not 1 <= k <= kth_max():
        raise ValueError(f"prdc: k={k!r} outside 1 .. {kth_max()}")
    if slab_rows < 1:
        raise ValueError(f"prdc: slab_rows={slab_rows}")
    for n in counts:
        if n < k + 1:
            raise ValueError(f"prdc: a bank of {n} rows is too short for k={k} (at least k + 1 rows)")


def _slabs(n: int, slab_rows: int):
    return [(s, min(s + slab_rows, n)) for s in range(0, n, slab_rows)]


def _radii(x: torch.Tensor, norm: torch.Tensor, k: int, slab_rows: int) -> torch.Tensor:
    out = torch.empty(x.shape[0], dtype=torch.float64, device=x.device)
    for s0, s1 in _slabs(x.shape[0], slab_rows):
        out[s0:s1] = row_kth(sqdist(x[s0:s1], x, norm[s0:s1], norm, self_offset=s0), k)
    return out


def knn_radii(X: torch.Tensor, k: int, slab_rows: int = SLAB_ROWS) -> torch.Tensor:
    """fp64 [n]: the squared distance from every row to its k-th nearest other row.  Only the row's own index is left out: a
    duplicate of it elsewhere counts, with distance 0."""
    x = _bank(X, "knn_radii")
    _check_k(k, slab_rows, x.shape[0])
    return _radii(x, row_sqnorm(x), int(k), int(slab_rows))


def prdc_parts(real: torch.Tensor, fake: torch.Tensor, k: int = 5, slab_rows: int = SLAB_ROWS) -> Dict[str, torch.Tensor]:
    """The device side of ``prdc``: dict(rR fp64 [nr], rF fp64 [nf], cntF int32 [nf], cntR int32 [nr], minR fp64 [nr])."""
    R, F = _bank(real, "prdc(real)"), _bank(fake, "prdc(fake)")
    if R.shape[1] != F.shape[1] or R.device != F.device:
        raise HrvError(f"prdc: banks {tuple(R.shape)} and {tuple(F.shape)} do not match")
    nr, nf = R.shape[0], F.shape[0]
    _check_k(k, slab_rows, nr, nf)
    k, slab_rows = int(k), int(slab_rows)
    nR, nF = row_sqnorm(R), row_sqnorm(F)
    if not bool((torch.isfinite(nR).all() & torch.isfinite(nF).all()).item()):      # the one read-back before the result
        raise ValueError("prdc: a feature bank holds a non-finite value (or a row whose squared norm overflows)")
    rR, rF = _radii(R, nR, k, slab_rows), _radii(F, nF, k, slab_rows)
    cntF = torch.empty(nf, dtype=torch.int32, device=R.device)
    cntR = torch.empty(nr, dtype=torch.int32, device=R.device)
    minR = torch.empty(nr, dtype=torch.float64, device=R.device)
    for s0, s1 in _slabs(nf, slab_rows):
        cntF[s0:s1] = row_ball(sqdist(F[s0:s1], R, nF[s0:s1], nR), rR, minimum=False)[0]
    for s0, s1 in _slabs(nr, slab_rows):
        cntR[s0:s1], minR[s0:s1] = row_ball(sqdist(R[s0:s1], F, nR[s0:s1], nF), rF)
    return {"rR": rR, "rF": rF, "cntF": cntF, "cntR": cntR, "minR": minR}


def prdc(real: torch.Tensor, fake: torch.Tensor, k: int = 5, slab_rows: int = SLAB_ROWS) -> dict:
    """dict(precision, recall, density, coverage, k, n_real, n_fake) between two device-resident fp32 feature banks [n, D]: ``real``
    the ground truths, ``fake`` the predictions."""
    p = prdc_parts(real, fake, k, slab_rows)
    cntF, cntR = p["cntF"].cpu().numpy().astype(np.int64), p["cntR"].cpu().numpy().astype(np.int64)
    minR, rR = p["minR"].cpu().numpy(), p["rR"].cpu().numpy()
    nr, nf = int(cntR.shape[0]), int(cntF.shape[0])
    return {"precision": float(np.count_nonzero(cntF > 0)) / nf, "recall": float(np.count_nonzero(cntR > 0)) / nr,
            "density": float(int(cntF.sum())) / (int(k) * nf), "coverage": float(np.count_nonzero(minR < rR)) / nr,
            "k": int(k), "n_real": nr, "n_fake": nf}
