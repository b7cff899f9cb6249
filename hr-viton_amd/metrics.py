"""Image-pair metrics of the reference's evaluate.py on the HIP path (csrc/metrics.hip).

``pair_stats(gt, pred)`` scores a batch of RGB uint8 pairs in one launch: the SSIM of their PIL gray images, exactly as
``skimage.metrics.structural_similarity(gt, pred, data_range=255, gaussian_weights=True, use_sample_covariance=False)``
computes it (evaluate.py:67), and the MSE of ``ToTensor(gt)`` against ``ToTensor(pred)`` (evaluate.py:78-80).
``structural_similarity`` is the single-pair form with skimage's name; it accepts only the parameter set evaluate.py uses.
``seg_iou_counts`` / ``seg_iou`` are train_condition.py's validation ``iou_metric`` (:18-36; csrc/validate.hip): the counts on the
device in one launch, the ratio on the host.
There is no CPU path: without libhrviton_hip.so these raise.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import HrvError
from .ops import _stream

MIN_SIZE = 11        # the 11-tap Gaussian window (sigma 1.5, truncate 3.5)


def _u8_cuda(x, what: str) -> torch.Tensor:
    t = torch.as_tensor(x) if not isinstance(x, torch.Tensor) else x
    if t.dtype != torch.uint8:
        raise HrvError(f"{what}: expected uint8 images, got {t.dtype}")
    if not t.is_cuda:
        t = t.to("cuda")
    return t.contiguous()


def _check_size(H: int, W: int):
    if H < MIN_SIZE or W < MIN_SIZE:
        raise ValueError(f"SSIM needs images of at least {MIN_SIZE}x{MIN_SIZE} (the Gaussian window), got {H}x{W}")


def pair_stats(gt_rgb_u8: torch.Tensor, pred_rgb_u8: torch.Tensor,
               valid: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(ssim[B], mse[B]) as float64 CUDA tensors for ``[B,H,W,3]`` (or one ``[H,W,3]``) uint8 CUDA tensors.  ``valid``: optional
    int32 [B]; pairs with 0 are skipped (both results 0)."""
    for t, n in ((gt_rgb_u8, "gt"), (pred_rgb_u8, "pred")):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.uint8:
            raise HrvError(f"pair_stats({n}): expected a uint8 CUDA tensor")
    if gt_rgb_u8.dim() == 3:
        gt_rgb_u8, pred_rgb_u8 = gt_rgb_u8[None], pred_rgb_u8[None]
    if gt_rgb_u8.shape != pred_rgb_u8.shape or gt_rgb_u8.dim() != 4 or gt_rgb_u8.shape[3] != 3:
        raise ValueError(f"pair_stats: expected two [B,H,W,3] tensors of one shape, got {tuple(gt_rgb_u8.shape)} and "
                         f"{tuple(pred_rgb_u8.shape)}")
    B, H, W, _ = gt_rgb_u8.shape
    _check_size(H, W)
    gt, pred = gt_rgb_u8.contiguous(), pred_rgb_u8.contiguous()
    dev = gt.device
    if valid is not None:
        valid = valid.to(device=dev, dtype=torch.int32).contiguous()
        assert valid.numel() == B
    lib = _lib.load()
    nbytes = lib.hrv_pair_stats_workspace_bytes(B, H, W)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    ssim = torch.empty(B, dtype=torch.float64, device=dev)
    mse = torch.empty(B, dtype=torch.float64, device=dev)
    _lib.check(lib.hrv_pair_stats_u8(gt.data_ptr(), pred.data_ptr(), None if valid is None else valid.data_ptr(), B, H, W,
                                     ws.data_ptr(), nbytes, ssim.data_ptr(), mse.data_ptr(), _stream()), "hrv_pair_stats_u8")
    return ssim, mse


def rgb_to_gray(rgb_u8: torch.Tensor) -> torch.Tensor:
    """PIL ``Image.convert('L')`` of a ``[..., 3]`` uint8 CUDA tensor (bit-exact)."""
    if not rgb_u8.is_cuda or rgb_u8.dtype != torch.uint8 or rgb_u8.shape[-1] != 3:
        raise HrvError("rgb_to_gray: expected a uint8 CUDA tensor [..., 3]")
    x = rgb_u8.contiguous()
    out = torch.empty(x.shape[:-1], dtype=torch.uint8, device=x.device)
    lib = _lib.load()
    _lib.check(lib.hrv_rgb_to_gray_u8(x.data_ptr(), out.numel(), out.data_ptr(), _stream()), "hrv_rgb_to_gray_u8")
    return out


def structural_similarity(im1, im2, *, data_range=255, gaussian_weights=True, use_sample_covariance=False, **kwargs) -> float:
    """skimage.metrics.structural_similarity for two 2-D uint8 images (numpy arrays or tensors) with the settings of
    evaluate.py:67 only; any other setting raises NotImplementedError."""
    if kwargs or data_range != 255 or gaussian_weights is not True or use_sample_covariance is not False:
        raise NotImplementedError("structural_similarity: only data_range=255, gaussian_weights=True, use_sample_covariance=False "
                                  f"(evaluate.py:67) is implemented on the HIP path (got extra {sorted(kwargs)})")
    a = torch.as_tensor(np.asarray(im1)) if not isinstance(im1, torch.Tensor) else im1
    b = torch.as_tensor(np.asarray(im2)) if not isinstance(im2, torch.Tensor) else im2
    if a.dim() != 2 or a.shape != b.shape:
        raise ValueError(f"structural_similarity: expected two 2-D images of one shape, got {tuple(a.shape)} and {tuple(b.shape)}")
    if a.dtype != torch.uint8 or b.dtype != torch.uint8:
        raise NotImplementedError("structural_similarity: uint8 images only")
    _check_size(*a.shape)
    # a gray image is an RGB image with three equal channels: PIL's luma weights sum to 65536, so the conversion returns it unchanged
    a3 = _u8_cuda(a, "im1")[..., None].expand(*a.shape, 3).contiguous()
    b3 = _u8_cuda(b, "im2")[..., None].expand(*b.shape, 3).contiguous()
    ssim, _ = pair_stats(a3, b3)
    return float(ssim[0].item())


COMPOSITIONS = {"no_composition": 0, "detach": 1, "warp_grad": 2}


def seg_iou_counts(fake_segmap: torch.Tensor, warped_cm: Optional[torch.Tensor], label: torch.Tensor,
                   composition: str = "warp_grad", out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The counts behind train_condition.py's ``iou_metric(softmax(fake_segmap * cloth_mask, 1), label)`` (:18-36, 344-356) as an
    int64 CUDA tensor [N,3]: per sample (intersection, sum_pred, sum_true) with ``pred = softmax > 0.5`` over all 13 channels and
    pixels.  fake_segmap: fp32 [N,13,h,w] raw logits; warped_cm: fp32 [N,1,h,w] (unused and optional under 'no_composition');
    label: fp32 one-hot [N,13,h,w].  ``out``: optional int64 CUDA buffer of at least N rows; rows [0, N) are overwritten (never
    accumulated onto), later rows are left alone."""
    if composition not in COMPOSITIONS:
        raise ValueError(f"seg_iou_counts: composition {composition!r} is none of {sorted(COMPOSITIONS)}")
    comp = COMPOSITIONS[composition]
    for t, n in ((fake_segmap, "fake_segmap"), (label, "label")) + (((warped_cm, "warped_cm"),) if comp else ()):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or t.dim() != 4:
            raise HrvError(f"seg_iou_counts({n}): expected a 4-D fp32 CUDA tensor")
    N, Cn, h, w = fake_segmap.shape
    if Cn != 13 or tuple(label.shape) != (N, 13, h, w):
        raise ValueError(f"seg_iou_counts: expected [N,13,h,w] logits and labels of one shape, got {tuple(fake_segmap.shape)} and "
                         f"{tuple(label.shape)}")
    if comp and tuple(warped_cm.shape) != (N, 1, h, w):
        raise ValueError(f"seg_iou_counts: warped_cm {tuple(warped_cm.shape)} is not [{N},1,{h},{w}]")
    seg, lab = fake_segmap.detach().contiguous(), label.detach().contiguous()
    cm = warped_cm.detach().contiguous() if comp else None
    if out is None:
        out = torch.empty((N, 3), dtype=torch.int64, device=seg.device)
    elif (not out.is_cuda or out.dtype != torch.int64 or out.dim() != 2 or out.shape[1] != 3 or out.shape[0] < N
          or not out.is_contiguous()):
        raise HrvError(f"seg_iou_counts(out): expected a contiguous int64 CUDA tensor [>={N},3]")
    lib = _lib.load()
    _lib.check(lib.hrv_seg_iou_nchw_f32(seg.data_ptr(), None if cm is None else cm.data_ptr(), lab.data_ptr(), N, h, w, comp,
                                        out.data_ptr(), _stream()), "hrv_seg_iou_nchw_f32")
    return out[:N]


def seg_iou(counts) -> torch.Tensor:
    """``(I + 1e-7) / (S_pred + S_true - I + 1e-7)`` per row of ``counts`` [N,3] = (I, S_pred, S_true), as a float64 CPU tensor [N].
    The reference evaluates the same expression in fp32 on tensors (train_condition.py:31-35); from exact integer counts in
    float64 the two agree to fp32 rounding."""
    c = torch.as_tensor(counts).detach().to("cpu", torch.float64).reshape(-1, 3)
    inter, union = c[:, 0], c[:, 1] + c[:, 2]
    return (inter + 1e-7) / (union - inter + 1e-7)
