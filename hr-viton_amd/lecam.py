"""LeCam regulariser (Tseng et al., "Regularizing GANs under Limited Data", CVPR 2021) and logit statistics of the PatchGAN, as ONE
loss head of the discriminator step (csrc/dhead.hip; the record is laid out in include/hrviton_hip.h).

``LeCam.d_losses(pred_fake, pred_real)`` replaces the D step's four ``GANLoss`` calls: one reduce launch over the logit maps of all
scales and both halves, one finalize block (means, anchor update, r_t, count, lambda_eff, the three loss scalars) and, in the
backward, one launch that writes all four gradients.  The anchors are moving averages of the mean real / fake logits; they are
updated BEFORE they are used, as the published code does, and are constants of the gradient.  Nothing is read back to the host:
the published implementation's ``.item()`` per step is what this removes, and the head lives inside a captured iteration.

``weight=0`` keeps the statistics (the mean logits and ADA's overfitting heuristic r_t = E[sign D(real)], Karras et al. 2020) and
gives the hinge gradients of the four-call path bit for bit."""
from __future__ import annotations

from typing import Dict, List, Optional

import torch

from . import _lib
from . import train_ops as T
from .ops import HrvError

FORMS = {"paper": _lib.DHEAD_FORM_PAPER, "relu": _lib.DHEAD_FORM_RELU}
_HYPER = ("weight", "decay", "start", "form")


def _dense(t: torch.Tensor) -> torch.Tensor:
    """The logits as the kernels read them: in place when dense (any dense layout: the head is elementwise + full reductions and
    hands the gradient back in the same layout), else a contiguous copy -- as losses._LossFn does."""
    if t.is_contiguous() or (t.dim() == 4 and t.is_contiguous(memory_format=torch.channels_last)):
        return t
    return t.contiguous()


class _DHeadFn(torch.autograd.Function):
    """(head, num_D, fake_0, real_0, fake_1, real_1, ...) -> losses [3]"""

    @staticmethod
    def forward(ctx, head, k, *logits):
        xs = [_dense(t.detach()) for t in logits]
        x_fake, x_real = xs[0::2], xs[1::2]
        losses = torch.empty(3, dtype=torch.float32, device=xs[0].device)
        world = head._world()
        T.dhead_forward(x_fake, x_real, FORMS[head.form], head.weight, head.decay, head.start, head._part, head._record, losses,
                        world=world, reduce_sums=head._all_reduce if world > 1 else None)
        ctx.head, ctx.x_fake, ctx.x_real = head, x_fake, x_real
        return losses

    @staticmethod
    def backward(ctx, g):
        head, x_fake, x_real = ctx.head, ctx.x_fake, ctx.x_real
        ctx.x_fake = ctx.x_real = None
        g = g.contiguous()
        d_fake = [torch.empty_like(x) for x in x_fake]
        d_real = [torch.empty_like(x) for x in x_real]
        # (the record still holds this step's anchors and lambda_eff: one forward, one backward, as a training step has them)
        T.dhead_backward(x_fake, x_real, FORMS[head.form], head._record, g[0:1], g[1:2], g[2:3], d_fake, d_real)
        out = [None, None]
        for f, r in zip(d_fake, d_real):
            out += [f, r]
        return tuple(out)


class LeCam:
    """``weight``: lambda (0: statistics only); ``decay``: of the anchors and of the r_t average; ``start``: lambda_eff is 0 until
    ``start`` anchor updates have been applied (the anchors move from the first step on); ``form``: 'paper' --
    R = mean((x_r - a_F)^2) + mean((x_f - a_R)^2) -- or 'relu', the published code's mean(relu(x_r - a_F)^2) + mean(relu(a_R - x_f)^2).
    The record and the partials are this object's own buffers (not the shared workspace of ops._workspace)."""

    def __init__(self, weight: float, decay: float = 0.99, start: int = 0, form: str = "paper", process_group=None):
        if form not in FORMS:
            raise HrvError(f"LeCam: form is 'paper' or 'relu', got {form!r}")
        if not (weight >= 0.0 and 0.0 <= decay < 1.0 and int(start) == start and start >= 0):
            raise HrvError(f"LeCam: weight >= 0, 0 <= decay < 1 and an integer start >= 0 are required, got {weight}, {decay}, {start}")
        self.weight, self.decay, self.start, self.form = float(weight), float(decay), int(start), form
        self.pg = process_group
        self.num_D = 0
        self._record: Optional[torch.Tensor] = None
        self._part: Optional[torch.Tensor] = None
        self._pending: Optional[dict] = None

    # ------------------------------------------------------------------ buffers
    def _buffers(self, device):
        if self._record is None or self._record.device != device:
            old = self._record
            self._record = torch.zeros(_lib.DHEAD_WORDS, dtype=torch.float64, device=device)
            self._part = torch.zeros(_lib.DHEAD_PART_WORDS, dtype=torch.float64, device=device)
            if old is not None:
                self._record.copy_(old)
            if self._pending is not None:
                self._apply(self._pending)
                self._pending = None

    def _world(self) -> int:
        import torch.distributed as dist
        return dist.get_world_size(self.pg) if (dist.is_available() and dist.is_initialized()) else 1

    def _all_reduce(self, sums: torch.Tensor):
        import torch.distributed as dist
        if torch.cuda.is_current_stream_capturing():
            raise HrvError("LeCam: the all-reduce of the logit sums cannot be captured; under data-parallel training run the "
                           "iteration eagerly")
        dist.all_reduce(sums, op=dist.ReduceOp.SUM, group=self.pg, async_op=True).wait()      # (parallel.GradSync's call)

    # ------------------------------------------------------------------ the D step's loss tail
    def d_losses(self, pred_fake: List, pred_real: List) -> Dict[str, torch.Tensor]:
        """``pred_fake`` / ``pred_real``: what ``forward_pair`` / ``forward(split=True)`` return (per scale a list whose last element
        is the logit map, or the map itself).  Returns D_Fake, D_Real (GANLoss's hinge terms, averaged over the scales) and
        D_LeCam = lambda_eff * R, each of shape [1]."""
        if not isinstance(pred_fake, (list, tuple)) or not isinstance(pred_real, (list, tuple)) or len(pred_fake) != len(pred_real) \
                or not 1 <= len(pred_fake) <= _lib.DHEAD_MAX_SCALES:
            raise HrvError(f"LeCam.d_losses: one entry per scale (1..{_lib.DHEAD_MAX_SCALES}) in both lists")
        logits = []
        for f, r in zip(pred_fake, pred_real):
            f = f[-1] if isinstance(f, (list, tuple)) else f
            r = r[-1] if isinstance(r, (list, tuple)) else r
            for t in (f, r):
                if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
                    raise HrvError("LeCam.d_losses: the logit maps are fp32 tensors, got %s" % (getattr(t, "dtype", type(t).__name__),))
                if not t.is_cuda:
                    raise HrvError("LeCam.d_losses: the logits live on the GPU (the head has no CPU path)")
            if f.numel() != r.numel() or f.numel() < 1:
                raise HrvError(f"LeCam.d_losses: the halves of a scale have {f.numel()} and {r.numel()} elements")
            logits += [f, r]
        k = len(pred_fake)
        if self.num_D not in (0, k):
            raise HrvError(f"LeCam.d_losses: this head has anchors for {self.num_D} scales, got {k}")
        self._buffers(logits[0].device)
        self.num_D = k
        out = _DHeadFn.apply(self, k, *logits)
        return {"D_Fake": out[0:1], "D_Real": out[1:2], "D_LeCam": out[2:3]}

    # ------------------------------------------------------------------ reading it
    def stats(self) -> torch.Tensor:
        """The record, fp64 [HRV_DHEAD_WORDS], on the device (no synchronisation; zeros before the first step)."""
        if self._record is None:
            raise HrvError("LeCam.stats: no step has run yet")
        return self._record

    def scalars(self) -> dict:
        """The record as Python numbers (ONE device-to-host copy: call it only where the script synchronises anyway).  Before the
        first step: zeros, or what ``load_state_dict`` left for it."""
        K = self.num_D
        if self._record is None:
            p = self._pending or {"count": 0, "anchor_real": [0.0] * K, "anchor_fake": [0.0] * K, "r_t_avg": [0.0] * K}
            zeros = [0.0] * len(p["anchor_real"])
            return dict(p, nonfinite=0, lambda_eff=0.0, reg=0.0, steps=0, r_t=zeros, mean_real=zeros, mean_fake=zeros)
        h = self._record.detach().cpu().tolist()
        S, W = _lib.DHEAD_STATE, _lib.DHEAD_SCALE_WORDS
        col = lambda j: [h[S + W * k + j] for k in range(K)]      # noqa: E731
        return {"count": int(h[_lib.DHEAD_COUNT]), "nonfinite": int(h[_lib.DHEAD_NONFINITE]), "lambda_eff": h[_lib.DHEAD_LAMBDA],
                "reg": h[_lib.DHEAD_REG], "steps": int(h[_lib.DHEAD_STEPS]),
                "anchor_real": col(_lib.DHEAD_ANCHOR_REAL), "anchor_fake": col(_lib.DHEAD_ANCHOR_FAKE),
                "r_t_avg": col(_lib.DHEAD_RT_AVG), "r_t": col(_lib.DHEAD_RT),
                "mean_real": col(_lib.DHEAD_MEAN_REAL), "mean_fake": col(_lib.DHEAD_MEAN_FAKE)}

    # ------------------------------------------------------------------ checkpoints
    def state_dict(self) -> dict:
        s = self.scalars()
        return {"weight": self.weight, "decay": self.decay, "start": self.start, "form": self.form, "count": s["count"],
                "anchor_real": torch.tensor(s["anchor_real"], dtype=torch.float64),
                "anchor_fake": torch.tensor(s["anchor_fake"], dtype=torch.float64),
                "r_t_avg": torch.tensor(s["r_t_avg"], dtype=torch.float64)}

    def load_state_dict(self, sd: dict):
        """Strict: exactly the keys of ``state_dict()``, the same hyper-parameters, one anchor pair per scale."""
        want = set(_HYPER) | {"count", "anchor_real", "anchor_fake", "r_t_avg"}
        if set(sd.keys()) != want:
            raise HrvError(f"LeCam.load_state_dict: keys {sorted(sd.keys())}, expected {sorted(want)}")
        for key in _HYPER:
            if sd[key] != getattr(self, key):
                raise HrvError(f"LeCam.load_state_dict: the file was written with {key}={sd[key]!r}, this run has {getattr(self, key)!r}")
        cols = {key: [float(v) for v in torch.as_tensor(sd[key], dtype=torch.float64).reshape(-1).tolist()]
                for key in ("anchor_real", "anchor_fake", "r_t_avg")}
        k = len(cols["anchor_real"])
        if not (len(cols["anchor_fake"]) == len(cols["r_t_avg"]) == k and 0 <= k <= _lib.DHEAD_MAX_SCALES) or int(sd["count"]) < 0:
            raise HrvError("LeCam.load_state_dict: anchor_real, anchor_fake and r_t_avg hold one value per scale, count >= 0")
        if self.num_D not in (0, k) and k:
            raise HrvError(f"LeCam.load_state_dict: the file has {k} scales, this head {self.num_D}")
        state = dict(count=int(sd["count"]), **cols)
        self.num_D = k or self.num_D
        if self._record is None:
            self._pending = state      # (no device yet: written when the first step allocates the record)
        else:
            self._apply(state)

    def _apply(self, state: dict):
        h = self._record.detach().cpu()
        h[_lib.DHEAD_COUNT] = float(state["count"])
        for k in range(len(state["anchor_real"])):
            base = _lib.DHEAD_STATE + _lib.DHEAD_SCALE_WORDS * k
            h[base + _lib.DHEAD_ANCHOR_REAL] = state["anchor_real"][k]
            h[base + _lib.DHEAD_ANCHOR_FAKE] = state["anchor_fake"][k]
            h[base + _lib.DHEAD_RT_AVG] = state["r_t_avg"][k]
        self._record.copy_(h)

    def __repr__(self):
        return "LeCam(weight=%g, decay=%g, start=%d, form=%r)" % (self.weight, self.decay, self.start, self.form)


# ------------------------------------------------------------------ the training script's side
def add_lecam_args(parser):
    """--lecam / --lecam_decay / --lecam_start / --lecam_form / --d_stats / --lecam_checkpoint of train_generator.py.  Like the
    guard's flags they appear in the parsed namespace only when given."""
    import argparse
    parser.add_argument("--lecam", type=float, default=argparse.SUPPRESS,
                        help="weight of the LeCam regulariser of the discriminator step, computed with the hinge terms in one fused "
                             "loss head on the device (0: off)")
    parser.add_argument("--lecam_decay", type=float, default=argparse.SUPPRESS, help="decay of the anchors and the r_t average (0.99)")
    parser.add_argument("--lecam_start", type=int, default=argparse.SUPPRESS,
                        help="anchor updates before the regulariser acts, counted on the device (0)")
    parser.add_argument("--lecam_form", type=str, choices=sorted(FORMS), default=argparse.SUPPRESS,
                        help="paper: squared distances; relu: the published code's one-sided form (paper)")
    parser.add_argument("--d_stats", action="store_true", default=argparse.SUPPRESS,
                        help="the loss head with weight 0: mean logits and r_t = E[sign D(real)] on the device, hinge gradients unchanged")
    parser.add_argument("--lecam_checkpoint", type=str, default=argparse.SUPPRESS,
                        help="a lecam_*.pth file that seeds anchors, r_t average and count of a resumed run")


def lecam_from_opt(opt, process_group=None) -> Optional[LeCam]:
    """The run's head, or None (the plain iteration: nothing allocated, no new launch) without --lecam W > 0 and without --d_stats."""
    weight = float(getattr(opt, "lecam", 0.0) or 0.0)
    if weight == 0.0 and not getattr(opt, "d_stats", False):
        if getattr(opt, "lecam_checkpoint", ""):
            raise HrvError("--lecam_checkpoint needs --lecam or --d_stats")
        return None
    head = LeCam(weight, decay=float(getattr(opt, "lecam_decay", 0.99)), start=int(getattr(opt, "lecam_start", 0)),
                 form=getattr(opt, "lecam_form", "paper"), process_group=process_group)
    ck = getattr(opt, "lecam_checkpoint", "")
    if ck:
        head.load_state_dict(torch.load(ck, map_location="cpu"))
    return head


def lecam_scalars(head: Optional[LeCam]):
    """[(tag, value)] for --board: Reg/r_t, Reg/D_real, Reg/D_fake, Reg/anchor_real, Reg/anchor_fake per scale (one host copy; call
    only where the script synchronises anyway).  [] without a head."""
    if head is None or head._record is None:
        return []
    s = head.scalars()
    out = []
    for k in range(head.num_D):
        for tag, key in (("Reg/r_t", "r_t_avg"), ("Reg/D_real", "mean_real"), ("Reg/D_fake", "mean_fake"),
                         ("Reg/anchor_real", "anchor_real"), ("Reg/anchor_fake", "anchor_fake")):
            out.append(("%s/%d" % (tag, k), float(s[key][k])))
    return out


def lecam_line(head: Optional[LeCam], losses: Optional[dict] = None) -> str:
    """The tail of the script's printed line: '' without a head."""
    if head is None or head._record is None:
        return ""
    s = head.scalars()
    val = float(losses["D_LeCam"].item()) if losses is not None and "D_LeCam" in losses else s["lambda_eff"] * s["reg"]
    return ", D_lecam: %.4g, r_t: %s" % (val, "/".join("%.3f" % v for v in s["r_t_avg"]))
