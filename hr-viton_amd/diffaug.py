"""DiffAugment (Zhao et al., NeurIPS 2020: ``color,translation,cutout``) for the PatchGAN of train_generator.py, applied INSIDE the
kernels that assemble the discriminator's input (csrc/diffaug.hip; the transform is defined in include/hrviton_hip.h).

One row of uniforms ``u[n]`` (fp32 [N, 8], in [0, 1)) is shared by the parse map, the fake image and the real image of sample n: the
discriminator is conditional on the parse map, and the feature-matching loss compares fake and real features position by position,
so both halves must see the same transform.  The decision is taken on the device from ``u``; nothing is read back to the host, and
``torch.rand`` on the device is graph-safe, so the draw may live inside a captured iteration."""
from __future__ import annotations

from typing import Optional, Union

import torch

from . import _lib, ops
from . import train_ops as T
from .ops import Act, HrvError

POLICY_BITS = {"color": _lib.DIFFAUG_COLOR, "translation": _lib.DIFFAUG_TRANSLATION, "cutout": _lib.DIFFAUG_CUTOUT}


def parse_policy(policy: Union[str, int, None]) -> int:
    """'color,translation,cutout' (any subset, any order, blanks ignored) -> the HRV_DIFFAUG_* bits; an unknown name is an error."""
    if policy is None:
        return 0
    if isinstance(policy, int) and not isinstance(policy, bool):
        if not 0 <= policy <= sum(POLICY_BITS.values()):
            raise HrvError(f"DiffAugment: policy bits {policy} out of range")
        return policy
    if not isinstance(policy, str):
        raise HrvError(f"DiffAugment: policy must be a string like 'color,translation,cutout', got {type(policy).__name__}")
    bits = 0
    for name in policy.split(","):
        name = name.strip()
        if not name:
            continue
        if name not in POLICY_BITS:
            raise HrvError(f"DiffAugment: unknown policy '{name}' (known: {', '.join(POLICY_BITS)})")
        bits |= POLICY_BITS[name]
    return bits


class DiffAugment:
    """The policy of a run.  ``draw(N, device)`` returns the uniforms of one discriminator call."""

    def __init__(self, policy: Union[str, int]):
        self.flags = parse_policy(policy)
        self.names = [n for n, b in POLICY_BITS.items() if self.flags & b]

    @property
    def color(self) -> bool:
        return bool(self.flags & _lib.DIFFAUG_COLOR)

    def draw(self, N: int, device) -> torch.Tensor:
        return torch.rand((N, 8), dtype=torch.float32, device=device)

    def __repr__(self):
        return "DiffAugment(%r)" % ",".join(self.names)


def check_u(u: torch.Tensor, N: int, device, what: str) -> torch.Tensor:
    if not (isinstance(u, torch.Tensor) and tuple(u.shape) == (N, 8) and u.dtype == torch.float32 and u.device == device):
        raise HrvError(f"{what}: the uniforms must be an fp32 [{N}, 8] tensor on {device}")
    return u.contiguous()


class _DiffAugConcatFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, parse_t, Ca, img, u, flags, mean):
        N, _, H, W = img.shape
        out = torch.empty((N, H, W, 12), dtype=torch.float32, device=img.device)
        T.diffaug_concat(Act(parse_t, Ca), img, u, mean, flags, Act(out, Ca + 3))
        ctx.aug = (Ca, u, flags)
        return out

    @staticmethod
    def backward(ctx, g):
        Ca, u, flags = ctx.aug
        d_img = None
        if ctx.needs_input_grad[2]:
            ga = Act(g.contiguous(), Ca + 3)
            gsum = T.diffaug_gsum(ga, Ca, u, flags) if flags & _lib.DIFFAUG_COLOR else None
            d_img = T.diffaug_bwd(ga, Ca, u, gsum, flags)
        return None, None, d_img, None, None, None


def diffaug_concat(parse7: Act, img: torch.Tensor, u: torch.Tensor, policy: Union[str, int, DiffAugment],
                   mean: Optional[torch.Tensor] = None) -> Act:
    """augment(cat((parse7, img), channels)) as an NHWC activation [N,H,W,12] -- the stand-alone form of what
    ``MultiscaleDiscriminator.forward_pair(..., aug=...)`` does per half.  ``parse7``: the label-map activation (channel stride 8,
    no gradient), ``img``: fp32 NCHW [N,3,H,W] (differentiable), ``u``: [N,8] uniforms, ``mean``: the per-sample image means the
    color transform uses (default: computed here from ``img``)."""
    ops.require_cuda(img, "diffaug_concat")
    flags = policy.flags if isinstance(policy, DiffAugment) else parse_policy(policy)
    N = img.shape[0]
    if parse7.bf16 or parse7.coff != 0 or parse7.cstride != 8 or img.dtype != torch.float32 or img.dim() != 4 or img.shape[1] != 3:
        raise HrvError("diffaug_concat: serves the PatchGAN shape only (fp32 parse map with channel stride 8, fp32 image [N,3,H,W])")
    u = check_u(u, N, img.device, "diffaug_concat")
    img = img.contiguous()
    if flags & _lib.DIFFAUG_COLOR and mean is None:
        mean = T.diffaug_mean(img.detach())
    if not flags & _lib.DIFFAUG_COLOR:
        mean = None
    return Act(_DiffAugConcatFn.apply(parse7.t, parse7.C, img, u, flags, mean), parse7.C + 3)


# ------------------------------------------------------------------ the training script's side
def add_diffaug_args(parser):
    """--diffaug of train_generator.py.  Like the guard's flags it appears in the parsed namespace only when given."""
    import argparse
    parser.add_argument("--diffaug", type=str, default=argparse.SUPPRESS,
                        help="augment both discriminator calls of an iteration on the device: any subset of "
                             "color,translation,cutout (default: off)")


def diffaug_from_opt(opt) -> Optional[DiffAugment]:
    """The run's DiffAugment, or None (the plain iteration: no new launch) without --diffaug or with an empty policy."""
    aug = DiffAugment(getattr(opt, "diffaug", "") or "")
    return aug if aug.flags else None
