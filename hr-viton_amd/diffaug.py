"""DiffAugment (Zhao et al., NeurIPS 2020: ``color,translation,cutout``) for the PatchGAN of train_generator.py, applied INSIDE the
kernels that assemble the discriminator's input (csrc/diffaug.hip; the transform is defined in include/hrviton_hip.h).

One row of uniforms ``u[n]`` (fp32 [N, 8], in [0, 1)) is shared by the parse map, the fake image and the real image of sample n: the
discriminator is conditional on the parse map, and the feature-matching loss compares fake and real features position by position,
so both halves must see the same transform.  The decision is taken on the device from ``u``; nothing is read back to the host, and
``torch.rand`` on the device is graph-safe, so the draw may live inside a captured iteration.

``AdaptiveAugment`` (Karras et al., "Training Generative Adversarial Networks with Limited Data", NeurIPS 2020) applies each transform
of the policy to a sample with probability ``p``: a second row of uniforms ``ug[n]`` (fp32 [N, 4]) gates color, translation and cutout
of sample n inside the same kernels, and ``p`` is ONE fp64 word on the device that a controller launch moves after every
discriminator step so that the windowed overfitting heuristic r_t = E[sign D(real)] of the loss head (lecam.py) stays at a target."""
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


_ADA_HYPER = ("policy", "target", "fixed_p", "kimg", "interval", "p_max")
_ADA_NAMES = {"p": _lib.ADA_P, "acc": _lib.ADA_ACC, "seen": _lib.ADA_SEEN, "updates": _lib.ADA_UPDATES, "r_t_window": _lib.ADA_RT_WINDOW,
              "steps": _lib.ADA_STEPS, "r_t": _lib.ADA_RT_LAST}


class AdaptiveAugment(DiffAugment):
    """The policy under per-sample gates.  Exactly one of ``target`` -- adaptive: ``update`` moves p by +-``step`` once per ``interval``
    discriminator steps toward r_t == target, step = images_per_step * interval / (kimg * 1000) (StyleGAN2-ADA's rule), clamped to
    [0, ``p_max``], from ``p_init`` -- and ``fixed_p`` -- a constant probability: no controller, no loss head needed.  The state
    (fp64 [HRV_ADA_WORDS], include/hrviton_hip.h) is this object's own device buffer; the gates read its first word in place."""

    def __init__(self, policy: Union[str, int], *, target: Optional[float] = None, fixed_p: Optional[float] = None, kimg: float = 500,
                 interval: int = 4, p_init: float = 0.0, p_max: float = 1.0):
        super().__init__(policy)
        if (target is None) == (fixed_p is None):
            raise HrvError("AdaptiveAugment: give exactly one of target (adaptive) and fixed_p (constant probability)")
        if not 0.0 <= float(p_max) <= 1.0:
            raise HrvError(f"AdaptiveAugment: p_max in [0, 1], got {p_max}")
        if target is not None:
            if not (-1.0 <= float(target) <= 1.0 and float(kimg) > 0.0 and int(interval) == interval and interval >= 1
                    and 0.0 <= float(p_init) <= float(p_max)):
                raise HrvError(f"AdaptiveAugment: target in [-1, 1], kimg > 0, an integer interval >= 1 and 0 <= p_init <= p_max are "
                               f"required, got {target}, {kimg}, {interval}, {p_init}")
        elif not 0.0 <= float(fixed_p) <= 1.0:
            raise HrvError(f"AdaptiveAugment: fixed_p in [0, 1], got {fixed_p}")
        self.target = None if target is None else float(target)
        self.fixed_p = None if fixed_p is None else float(fixed_p)
        self.kimg, self.interval, self.p_max = float(kimg), int(interval), float(p_max)
        self._p0 = self.fixed_p if target is None else float(p_init)
        self._state: Optional[torch.Tensor] = None
        self._pending: Optional[torch.Tensor] = None

    @property
    def adaptive(self) -> bool:
        return self.target is not None

    def _buffers(self, device):
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if self._state is None or self._state.device != device:
            host = torch.zeros(_lib.ADA_WORDS, dtype=torch.float64)
            host[_lib.ADA_P] = self._p0
            if self._state is not None:
                host = self._state.cpu()
            if self._pending is not None:
                host, self._pending = self._pending, None
            self._state = host.to(device)
        return self._state

    def draw(self, N: int, device):
        """(u [N,8], ug [N,4]): the transform's uniforms and the gates' (two draws, in this order)."""
        self._buffers(device)
        return torch.rand((N, 8), dtype=torch.float32, device=device), torch.rand((N, 4), dtype=torch.float32, device=device)

    def p_tensor(self, device=None) -> torch.Tensor:
        """The fp64 word the gates read: a view of the state on the device (no copy, no synchronisation)."""
        if device is None and self._state is None:
            raise HrvError("AdaptiveAugment.p_tensor: no device yet (draw first, or name one)")
        state = self._state if device is None else self._buffers(device)
        return state[_lib.ADA_P:_lib.ADA_P + 1]

    def step_size(self, images_per_step: int) -> float:
        return float(images_per_step) * self.interval / (self.kimg * 1000.0)

    def update(self, lecam, images_per_step: int):
        """One controller launch, right after the loss head's forward of the D step: the p it leaves is the one the two discriminator
        calls of the NEXT iteration see.  ``images_per_step``: the global batch."""
        if not self.adaptive:
            raise HrvError("AdaptiveAugment.update: this object has a fixed p (no controller)")
        if lecam is None or getattr(lecam, "_record", None) is None or lecam.num_D < 1:
            raise HrvError("AdaptiveAugment.update: needs the loss head (lecam.LeCam) after its d_losses of this step")
        step = self.step_size(images_per_step)
        if not 0.0 < step <= 1.0:
            raise HrvError(f"AdaptiveAugment.update: step = images_per_step * interval / (kimg * 1000) = {step} is outside (0, 1]")
        T.ada_update(lecam._record, lecam.num_D, self.target, step, self.interval, self.p_max, self._buffers(lecam._record.device))

    def state(self) -> torch.Tensor:
        """The state, fp64 [HRV_ADA_WORDS], on the device (no synchronisation)."""
        if self._state is None:
            raise HrvError("AdaptiveAugment.state: no device yet")
        return self._state

    def _host_state(self) -> torch.Tensor:
        if self._state is not None:
            return self._state.detach().cpu()
        if self._pending is not None:
            return self._pending.clone()
        host = torch.zeros(_lib.ADA_WORDS, dtype=torch.float64)
        host[_lib.ADA_P] = self._p0
        return host

    def scalars(self) -> dict:
        """The state as Python numbers (ONE device-to-host copy: call it only where the script synchronises anyway)."""
        h = self._host_state().tolist()
        return {name: h[word] for name, word in _ADA_NAMES.items()}

    # ------------------------------------------------------------------ checkpoints
    def state_dict(self) -> dict:
        return {"policy": self.flags, "target": self.target, "fixed_p": self.fixed_p, "kimg": self.kimg, "interval": self.interval,
                "p_max": self.p_max, "state": self._host_state()}

    def load_state_dict(self, sd: dict):
        """Strict: exactly the keys of ``state_dict()`` and the same hyper-parameters (``p_init`` is what the file replaces)."""
        want = set(_ADA_HYPER) | {"state"}
        if set(sd.keys()) != want:
            raise HrvError(f"AdaptiveAugment.load_state_dict: keys {sorted(sd.keys())}, expected {sorted(want)}")
        mine = self.state_dict()
        for key in _ADA_HYPER:
            if sd[key] != mine[key]:
                raise HrvError(f"AdaptiveAugment.load_state_dict: the file was written with {key}={sd[key]!r}, this run has {mine[key]!r}")
        state = torch.as_tensor(sd["state"], dtype=torch.float64).reshape(-1).clone()
        if state.numel() != _lib.ADA_WORDS or not bool(torch.isfinite(state).all()) or not 0.0 <= float(state[_lib.ADA_P]) <= 1.0:
            raise HrvError(f"AdaptiveAugment.load_state_dict: the state is {_lib.ADA_WORDS} finite float64 words with p in [0, 1]")
        if self._state is None:
            self._pending = state      # (no device yet: written when the first draw allocates the state)
        else:
            self._state.copy_(state)

    def __repr__(self):
        how = "target=%g, kimg=%g, interval=%d, p_max=%g" % (self.target, self.kimg, self.interval, self.p_max) if self.adaptive \
            else "fixed_p=%g" % self.fixed_p
        return "AdaptiveAugment(%r, %s)" % (",".join(self.names), how)


def check_u(u: torch.Tensor, N: int, device, what: str) -> torch.Tensor:
    if not (isinstance(u, torch.Tensor) and tuple(u.shape) == (N, 8) and u.dtype == torch.float32 and u.device == device):
        raise HrvError(f"{what}: the uniforms must be an fp32 [{N}, 8] tensor on {device}")
    return u.contiguous()


def check_ug(ug: torch.Tensor, N: int, device, what: str) -> torch.Tensor:
    if not (isinstance(ug, torch.Tensor) and tuple(ug.shape) == (N, 4) and ug.dtype == torch.float32 and ug.device == device):
        raise HrvError(f"{what}: the gate uniforms must be an fp32 [{N}, 4] tensor on {device}")
    return ug.contiguous()


def resolve_aug(aug: DiffAugment, aug_u, N: int, device, what: str) -> tuple:
    """What the assembly launches take: (policy bits, u) of a DiffAugment, (policy bits, u, ug, p) of an AdaptiveAugment, whose
    ``aug_u`` is a (u, ug) pair.  ``aug_u`` None: drawn here."""
    if not isinstance(aug, AdaptiveAugment):
        return aug.flags, aug.draw(N, device) if aug_u is None else check_u(aug_u, N, device, what)
    if aug_u is None:
        aug_u = aug.draw(N, device)
    if not (isinstance(aug_u, (tuple, list)) and len(aug_u) == 2):
        raise HrvError(f"{what}: the uniforms of an AdaptiveAugment are a (u [N,8], ug [N,4]) pair")
    return aug.flags, check_u(aug_u[0], N, device, what), check_ug(aug_u[1], N, device, what), aug.p_tensor(device)


class _DiffAugConcatFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, parse_t, Ca, img, u, flags, mean, gate=None):
        N, _, H, W = img.shape
        out = torch.empty((N, H, W, 12), dtype=torch.float32, device=img.device)
        if gate is None:
            T.diffaug_concat(Act(parse_t, Ca), img, u, mean, flags, Act(out, Ca + 3))
        else:
            T.diffaug_concat_gated(Act(parse_t, Ca), img, u, mean, flags, Act(out, Ca + 3), *gate)
        ctx.aug = (Ca, u, flags)
        ctx.gate = gate
        return out

    @staticmethod
    def backward(ctx, g):
        Ca, u, flags = ctx.aug
        d_img = None
        if ctx.needs_input_grad[2] and ctx.gate is None:
            ga = Act(g.contiguous(), Ca + 3)
            gsum = T.diffaug_gsum(ga, Ca, u, flags) if flags & _lib.DIFFAUG_COLOR else None
            d_img = T.diffaug_bwd(ga, Ca, u, gsum, flags)
        elif ctx.needs_input_grad[2]:      # (the gates read p as it stands NOW: no controller launch between forward and backward)
            ga = Act(g.contiguous(), Ca + 3)
            gsum = T.diffaug_gsum_gated(ga, Ca, u, flags, *ctx.gate) if flags & _lib.DIFFAUG_COLOR else None
            d_img = T.diffaug_bwd_gated(ga, Ca, u, gsum, flags, *ctx.gate)
        return None, None, d_img, None, None, None, None


def diffaug_concat(parse7: Act, img: torch.Tensor, u: torch.Tensor, policy: Union[str, int, DiffAugment],
                   mean: Optional[torch.Tensor] = None, gate=None) -> Act:
    """augment(cat((parse7, img), channels)) as an NHWC activation [N,H,W,12] -- the stand-alone form of what
    ``MultiscaleDiscriminator.forward_pair(..., aug=...)`` does per half.  ``parse7``: the label-map activation (channel stride 8,
    no gradient), ``img``: fp32 NCHW [N,3,H,W] (differentiable), ``u``: [N,8] uniforms, ``mean``: the per-sample image means the
    color transform uses (default: computed here from ``img``).  ``gate``: None, or (ug [N,4], p) -- the gate uniforms and the fp64
    device word of the probability: sample n keeps a transform of the policy only where ug[n, column] < p (the gated kernels)."""
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
    if gate is None:
        return Act(_DiffAugConcatFn.apply(parse7.t, parse7.C, img, u, flags, mean), parse7.C + 3)
    gate = (check_ug(gate[0], N, img.device, "diffaug_concat"), gate[1])
    return Act(_DiffAugConcatFn.apply(parse7.t, parse7.C, img, u, flags, mean, gate), parse7.C + 3)


# ------------------------------------------------------------------ the training script's side
def add_diffaug_args(parser):
    """--diffaug of train_generator.py.  Like the guard's flags it appears in the parsed namespace only when given."""
    import argparse
    parser.add_argument("--diffaug", type=str, default=argparse.SUPPRESS,
                        help="augment both discriminator calls of an iteration on the device: any subset of "
                             "color,translation,cutout (default: off)")


ADA_FLAGS = ("ada_target", "ada_fixed_p", "ada_kimg", "ada_interval", "ada_p_init", "ada_p_max", "ada_checkpoint")


def add_ada_args(parser):
    """--ada_target / --ada_kimg / --ada_interval / --ada_p_init / --ada_p_max / --ada_fixed_p / --ada_checkpoint of
    train_generator.py; each appears in the parsed namespace only when given."""
    import argparse
    parser.add_argument("--ada_target", type=float, default=argparse.SUPPRESS,
                        help="adaptive discriminator augmentation: every transform of --diffaug is applied to a sample with probability "
                             "p, moved on the device so that the windowed r_t = E[sign D(real)] stays at this value (ADA's 0.6)")
    parser.add_argument("--ada_kimg", type=float, default=argparse.SUPPRESS,
                        help="thousands of images over which p may travel from 0 to 1 (500)")
    parser.add_argument("--ada_interval", type=int, default=argparse.SUPPRESS, help="discriminator steps per adjustment of p (4)")
    parser.add_argument("--ada_p_init", type=float, default=argparse.SUPPRESS, help="p at the first step (0)")
    parser.add_argument("--ada_p_max", type=float, default=argparse.SUPPRESS, help="upper clamp of p (1)")
    parser.add_argument("--ada_fixed_p", type=float, default=argparse.SUPPRESS,
                        help="a constant probability for every transform of --diffaug instead of a controller")
    parser.add_argument("--ada_checkpoint", type=str, default=argparse.SUPPRESS,
                        help="an ada_*.pth file that seeds p and the open window of a resumed run")


def diffaug_from_opt(opt) -> Optional[DiffAugment]:
    """The run's DiffAugment, or None (the plain iteration: no new launch) without --diffaug or with an empty policy.  With
    --ada_target / --ada_fixed_p: an AdaptiveAugment over the same policy; an --ada_* flag without a policy, or both of them, ends
    the run with a message."""
    aug = DiffAugment(getattr(opt, "diffaug", "") or "")
    given = [f for f in ADA_FLAGS if hasattr(opt, f)]
    if not given:
        return aug if aug.flags else None
    if not aug.flags:
        raise SystemExit("--%s needs --diffaug with a policy (the gates select among its transforms)" % given[0])
    if hasattr(opt, "ada_target") and hasattr(opt, "ada_fixed_p"):
        raise SystemExit("--ada_target (a controller) and --ada_fixed_p (a constant) exclude each other")
    if not hasattr(opt, "ada_target") and not hasattr(opt, "ada_fixed_p"):
        raise SystemExit("--%s needs --ada_target or --ada_fixed_p" % given[0])
    if hasattr(opt, "ada_fixed_p"):
        ada = AdaptiveAugment(aug.flags, fixed_p=opt.ada_fixed_p)
    else:
        ada = AdaptiveAugment(aug.flags, target=opt.ada_target, kimg=getattr(opt, "ada_kimg", 500), interval=getattr(opt, "ada_interval", 4),
                              p_init=getattr(opt, "ada_p_init", 0.0), p_max=getattr(opt, "ada_p_max", 1.0))
    ck = getattr(opt, "ada_checkpoint", "")
    if ck:
        ada.load_state_dict(torch.load(ck, map_location="cpu"))
    return ada


def ada_scalars(aug):
    """[(tag, value)] for --board: Aug/p and Aug/r_t (the last closed window's mean); one host copy.  [] without an AdaptiveAugment."""
    if not isinstance(aug, AdaptiveAugment) or aug._state is None:
        return []
    s = aug.scalars()
    return [("Aug/p", s["p"]), ("Aug/r_t", s["r_t_window"])]


def ada_line(aug) -> str:
    """The tail of the script's printed line: '' without an AdaptiveAugment."""
    if not isinstance(aug, AdaptiveAugment):
        return ""
    return ", ada_p: %.6f" % aug.scalars()["p"]
