"""R1 gradient penalty (Mescheder et al., "Which Training Methods for GANs do actually Converge?", ICML 2018) of the PatchGAN,
gamma / 2 * E_real ||d D(x) / d x||^2, applied lazily every ``interval``-th iteration as StyleGAN2 does -- exact, without a
second-order engine (csrc/r1.hip).

With S_n the per-sample mean logit (mean over the scales of the mean over a scale's logits), g_n = dS_n / dx_n over the image
channels and P = gamma / (2 N) sum_n ||g_n||^2:

    grad_theta P = gamma * grad_theta [ sum_n <g_n(theta), v_n> ],   v_n = stop_grad(g_n) / N

and <g_n, v_n> is the directional derivative of S_n along v_n: a forward-mode TANGENT pass through D with tangent v, then one
ordinary reverse pass over the (primal, tangent) pair.  Convolutions and the average pool between the scales are linear (their
tangent is the same kernel on the tangent tensor, without bias), LeakyReLU's tangent is a mask multiply, and InstanceNorm -- the
one layer that couples tangent and primal -- has the closed form of include/hrviton_hip.h, served by the two launches of
``instnorm_jvp``.  Everything else is the training path's own kernels (train_ops).

``R1.phase`` is one such pass over the REAL half, un-augmented, on fp32 operands whatever the step's precision, with sigma taken
from the current weights and the stored (u, v), which it leaves alone.  It writes the parameter gradients of
``interval * gamma / 2 * penalty`` where a backward plan writes them (the flat buffer of the fused Adam) and returns the loss and
the penalty as device scalars; nothing is read back."""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Tuple

import torch

from . import _lib, ops
from . import train_ops as T
from .gen_train import Grads, MultiscaleDTrainPlan, _acc, _EngineMode, grad_buffer
from .ops import ACT_LRELU, ACT_NONE, Act, HrvError, _ceil4, _stream, _Timed

SLOPE = 0.2      # the PatchGAN's LeakyReLU (network_generator.py:263-272)


# ---------------------------------------------------------------------------------------------------------------
# the three new launches
# ---------------------------------------------------------------------------------------------------------------
def _jvp_desc(c: Act, mean, rstd, f: Act, t: Act, df: Act, cin: Optional[Act], tbar: Optional[Act], cbar: Optional[Act],
              record: torch.Tensor, ws: Optional[torch.Tensor], slope: float):
    d = _lib.hrv_instnorm_jvp_t()
    d.N, d.H, d.W, d.C = c.N, c.H, c.W, c.Cp
    for name, a in (("x", c), ("f", f), ("t", t), ("df", df), ("cin", cin), ("tbar", tbar), ("cbar", cbar)):
        if a is None:
            continue
        if a.bf16 or (a.N, a.H, a.W) != (c.N, c.H, c.W) or a.Cp != c.Cp:
            raise HrvError(f"instnorm_jvp: {name} must be an fp32 view of the extents and channels of the InstanceNorm input")
        setattr(d, name, a.t.data_ptr())
        setattr(d, name + "_cstride", a.cstride)
        setattr(d, name + "_coff", a.coff)
    d.mean, d.rstd, d.record, d.slope = mean.data_ptr(), rstd.data_ptr(), record.data_ptr(), slope
    d.workspace = None if ws is None else ws.data_ptr()
    return d


def instnorm_jvp_stats(c: Act, mean: torch.Tensor, rstd: torch.Tensor, f: Act, t: Act, df: Act, slope: float = SLOPE) -> torch.Tensor:
    """record [N, Cp, 5] float64 = sum q, sum t, sum y q, sum y t, sum q t per (sample, channel), q = lrelu'(f) * df
    (hrv_instnorm_jvp_stats_nhwc_f32)."""
    lib = _lib.load()
    ops.require_cuda(c.t, "instnorm_jvp_stats")
    dev = c.t.device
    record = torch.empty((c.N, c.Cp, 5), dtype=torch.float64, device=dev)
    ws = torch.empty(max(1, lib.hrv_instnorm_jvp_workspace_elems(c.N, c.H, c.W, c.Cp)), dtype=torch.float64, device=dev)
    d = _jvp_desc(c, mean, rstd, f, t, df, None, None, None, record, ws, slope)
    with _Timed("r1", "instnorm_jvp_stats", 0.0, 16.0 * c.N * c.H * c.W * c.Cp, "instnorm_jvp_partial_kernel"):
        _lib.check(lib.hrv_instnorm_jvp_stats_nhwc_f32(C.byref(d), _stream()), "hrv_instnorm_jvp_stats_nhwc_f32")
    return record


def instnorm_jvp_bwd(c: Act, mean: torch.Tensor, rstd: torch.Tensor, f: Act, t: Act, df: Act, record: torch.Tensor,
                     cin: Optional[Act] = None, slope: float = SLOPE, tbar: Optional[Act] = None,
                     cbar: Optional[Act] = None) -> Tuple[Act, Act]:
    """(tbar, cbar): the adjoint of the tangent ``t`` and the tangent path's adjoint of ``c`` (+ ``cin``), one element-wise launch
    over the record of instnorm_jvp_stats (hrv_instnorm_jvp_bwd_nhwc_f32)."""
    lib = _lib.load()
    dev = c.t.device
    if tbar is None:
        tbar = ops.alloc(c.N, c.H, c.W, c.C, dev)
    if cbar is None:
        cbar = ops.alloc(c.N, c.H, c.W, c.C, dev)
    d = _jvp_desc(c, mean, rstd, f, t, df, cin, tbar, cbar, record, None, slope)
    with _Timed("r1", "instnorm_jvp_bwd", 0.0, (24.0 + (4.0 if cin is not None else 0.0)) * c.N * c.H * c.W * c.Cp, "instnorm_jvp_bwd_kernel"):
        _lib.check(lib.hrv_instnorm_jvp_bwd_nhwc_f32(C.byref(d), _stream()), "hrv_instnorm_jvp_bwd_nhwc_f32")
    return tbar, cbar


def r1_seed(d_in: Act, Ca: int, Cb: int, gamma: float):
    """``d_in``: dense NHWC gradient of sum_n S_n w.r.t. [parse (Ca) ; image (Cb) ; pad].  Returns (v Act: d_in / N on the image
    channels, exactly 0 elsewhere; sums float64 [N]: ||g_n||^2; out float32 [2]: penalty, gamma / 2 * penalty) --
    hrv_r1_seed_nhwc_f32."""
    lib = _lib.load()
    ops.require_cuda(d_in.t, "r1_seed")
    if d_in.bf16 or d_in.coff != 0 or d_in.cstride != d_in.Cp or not d_in.t.is_contiguous() or Ca + Cb != d_in.C:
        raise HrvError("r1_seed: d_in is a dense fp32 NHWC activation of Ca + Cb channels")
    dev = d_in.t.device
    v = torch.empty_like(d_in.t)
    part = torch.empty((d_in.N, lib.hrv_r1_seed_slots()), dtype=torch.float64, device=dev)
    sums = torch.empty(d_in.N, dtype=torch.float64, device=dev)
    out = torch.empty(2, dtype=torch.float32, device=dev)
    with _Timed("r1", "r1_seed", 0.0, 8.0 * d_in.t.numel(), "r1_seed_kernel"):
        _lib.check(lib.hrv_r1_seed_nhwc_f32(d_in.t.data_ptr(), d_in.N, d_in.H, d_in.W, d_in.cstride, Ca, Cb, float(gamma), v.data_ptr(),
                                            part.data_ptr(), sums.data_ptr(), out.data_ptr(), _stream()), "hrv_r1_seed_nhwc_f32")
    return Act(v, d_in.C), sums, out


# ---------------------------------------------------------------------------------------------------------------
# the phase
# ---------------------------------------------------------------------------------------------------------------
def _const_map(N: int, H: int, W: int, value: float, device) -> Act:
    """a one-channel map holding ``value`` (pad channels 0): the gradient of a mean over the logits"""
    t = torch.zeros((N, H, W, _ceil4(1)), dtype=torch.float32, device=device)
    t[..., 0] = value
    return Act(t, 1)


class R1:
    """``gamma``: the penalty weight; ``interval``: the phase runs every interval-th iteration (``due``) with its gradient
    multiplied by ``interval`` (lazy regularisation, Karras et al. 2020).  Adam's lr / betas are NOT rescaled by
    interval / (interval + 1) as StyleGAN2 does."""

    def __init__(self, gamma: float, interval: int = 16):
        if not (gamma > 0.0 and int(interval) == interval and interval >= 1):
            raise HrvError(f"R1: gamma > 0 and an integer interval >= 1 are required, got {gamma}, {interval}")
        self.gamma, self.interval = float(gamma), int(interval)
        self.phases = 0
        self.last: Optional[Dict[str, torch.Tensor]] = None      # what the last phase returned (device tensors)

    def due(self, step: int) -> bool:
        return step % self.interval == 0

    def state_dict(self) -> dict:
        return {"gamma": self.gamma, "interval": self.interval, "phases": self.phases}

    def load_state_dict(self, sd: dict):
        self.phases = int(sd.get("phases", 0))

    # ---- sigma of the spectral-normalised convolutions from the CURRENT weights and the stored (u, v), which stay as they are; the
    # batch is cached on this object, the plan's own (TConv.sigma, its SpectralBatch) is not touched
    def _sigmas(self, convs) -> Dict[int, tuple]:
        return {id(c): (s_, u_, v_) for c, s_, u_, v_ in T.spectral_sigmas(self, convs, power_iteration=False)}

    def phase(self, discriminator, parse7: Act, real: torch.Tensor) -> Dict[str, torch.Tensor]:
        """One R1 phase on ``real`` [N,3,H,W] under the label map ``parse7``: the gradients of
        interval * gamma / 2 * mean_n ||dS_n / d real_n||^2 land where the D step's land (call ``opt_d.zero_grad()`` before and
        ``opt_d.step()`` after).  Returns {'D_R1': gamma / 2 * penalty, 'r1_penalty': penalty}, device tensors of shape [1]."""
        ops.require_cuda(real, "R1.phase")
        if torch.cuda.is_current_stream_capturing():
            raise HrvError("R1.phase is eager: it cannot be captured in a hipGraph")
        plan = getattr(discriminator, "_train_plan", None)
        if plan is None:
            plan = discriminator._train_plan = MultiscaleDTrainPlan(discriminator)
        N, Cb, H, W = real.shape
        if (parse7.N, parse7.H, parse7.W) != (N, H, W) or parse7.bf16 or real.dtype != torch.float32:
            raise HrvError("R1.phase: parse7 and real are fp32 and share batch and extent")
        Ca = parse7.C
        with torch.no_grad(), _EngineMode(True):
            out = self._phase(plan, parse7, real.detach().contiguous(), N, Ca, Cb, H, W)
        self.phases += 1
        self.last = out
        return out

    def _phase(self, plan, parse7, real, N, Ca, Cb, H, W):
        dev = real.device
        nD = len(plan.plans)
        sig = self._sigmas([conv for p in plan.plans for _, conv in p.layers])

        def sigma(conv):
            return sig[id(conv)][0] if conv.spectral else None

        def fwd(conv, a: Act, act: int, bias: bool) -> Act:
            b = conv.bparam if bias else None
            return T.conv_forward_dev(conv.wparam.data, [(a, 0)], conv.stride, conv.pad, sigma=sigma(conv),
                                      shift=None if b is None else b.data, act=act, slope=SLOPE, name=conv.name + ".r1")

        def dgrad(conv, dy: Act, src: Act) -> Act:
            return T.conv_dgrad(dy, conv.wparam.data, src.H, src.W, conv.stride, conv.pad, sigma=sigma(conv), name=conv.name + ".r1.dgrad")

        # ---- 1. primal forward: c, mean, rstd, f per layer
        a = Act(torch.empty((N, H, W, _ceil4(Ca + Cb)), dtype=torch.float32, device=dev), Ca + Cb)
        T.concat_nhwc_nchw(parse7, real, a)
        inputs, ctxs = [], []
        for k, p in enumerate(plan.plans):
            inputs.append(a)
            ctx, x = [], a
            for kind, conv in p.layers:
                if kind == "in":
                    c = fwd(conv, x, ACT_NONE, True)
                    mean, rstd = ops.instnorm_stats(c)
                    f = ops.instnorm_apply(c, mean, rstd, ACT_LRELU, SLOPE)
                    ctx.append(dict(src=x, c=c, mean=mean, rstd=rstd, f=f))
                elif kind in ("lrelu", "plain"):
                    f = fwd(conv, x, ACT_LRELU if kind == "lrelu" else ACT_NONE, True)
                    ctx.append(dict(src=x, f=f))
                else:
                    raise HrvError(f"R1.phase: layer kind {kind!r} (dropout) is not served")
                x = f
            ctxs.append(ctx)
            if k + 1 < nD:
                a = ops.avgpool3x3s2(a)

        # ---- 2. reverse for the input gradient of sum_n S_n only, then the seed
        d_in: Optional[Act] = None
        for k in range(nD - 1, -1, -1):
            layers, ctx = plan.plans[k].layers, ctxs[k]
            lg = ctx[-1]["f"]
            d = _const_map(N, lg.H, lg.W, 1.0 / (nD * lg.H * lg.W), dev)
            for i in range(len(layers) - 1, -1, -1):
                kind, conv = layers[i]
                e = ctx[i]
                if kind == "in":
                    d, _ = T.norm_bwd(e["c"], e["mean"], e["rstd"], d, act=ACT_LRELU, slope=SLOPE, out=e["f"])
                elif kind == "lrelu":
                    T.act_bwd_(d, e["f"], ACT_LRELU, SLOPE)
                d = dgrad(conv, d, e["src"])
            if d_in is not None:
                T.avgpool3x3s2_bwd(d_in, inputs[k].H, inputs[k].W, dx=d, accumulate=True)
            d_in = d
        v, _, scalars = r1_seed(d_in, Ca, Cb, self.gamma)

        # ---- 3. tangent forward with v, 4. reverse over the (primal, tangent) pair -- the scales are independent here: v is a constant
        grads: Grads = {}
        t_in = v
        for k, p in enumerate(plan.plans):
            layers, ctx = p.layers, ctxs[k]
            x = t_in
            for (kind, conv), e in zip(layers, ctx):
                e["tsrc"] = x
                tc = fwd(conv, x, ACT_NONE, False)
                if kind == "in":
                    e["t"] = tc
                    x, _ = T.norm_bwd(e["c"], e["mean"], e["rstd"], tc, act=ACT_NONE)      # J(c) t: the Jacobian is symmetric
                    T.act_bwd_(x, e["f"], ACT_LRELU, SLOPE)
                elif kind == "lrelu":
                    T.act_bwd_(tc, e["f"], ACT_LRELU, SLOPE)
                    x = tc
                else:
                    x = tc
            lg = x
            a_df: Act = _const_map(N, lg.H, lg.W, self.gamma * self.interval / (nD * lg.H * lg.W), dev)
            a_f: Optional[Act] = None
            for i in range(len(layers) - 1, -1, -1):
                kind, conv = layers[i]
                e = ctx[i]
                if kind == "in":
                    cin = None
                    if a_f is not None:
                        cin, _ = T.norm_bwd(e["c"], e["mean"], e["rstd"], a_f, act=ACT_LRELU, slope=SLOPE, out=e["f"])
                    rec = instnorm_jvp_stats(e["c"], e["mean"], e["rstd"], e["f"], e["t"], a_df, SLOPE)
                    tbar, cbar = instnorm_jvp_bwd(e["c"], e["mean"], e["rstd"], e["f"], e["t"], a_df, rec, cin, SLOPE)
                else:
                    if kind == "lrelu":
                        T.act_bwd_(a_df, e["f"], ACT_LRELU, SLOPE)
                        if a_f is not None:
                            T.act_bwd_(a_f, e["f"], ACT_LRELU, SLOPE)
                    tbar, cbar = a_df, a_f
                self._param_grads(conv, sig, grads, cbar, e["src"], tbar, e["tsrc"])
                if i > 0:
                    a_f = dgrad(conv, cbar, e["src"]) if cbar is not None else None
                    a_df = dgrad(conv, tbar, e["tsrc"])
            if k + 1 < nD:
                t_in = ops.avgpool3x3s2(t_in)
        T.wgrad_join()
        for p_, g in grads.items():      # (a parameter outside a fused optimizer: the gradient is handed over here)
            p_.grad = g if p_.grad is None else p_.grad.add_(g)
        return {"D_R1": scalars[1:2], "r1_penalty": scalars[0:1]}

    @staticmethod
    def _param_grads(conv, sig, grads: Grads, cbar: Optional[Act], src: Act, tbar: Act, tsrc: Act):
        """dW = cbar (*) src + tbar (*) tsrc (the second through the same kernel, accumulating); the bias gradient comes from cbar alone
        -- the tangent convolution has no bias -- and is an exact zero where the primal carries no adjoint."""
        w = conv.wparam.data
        Cout, cin, KH, KW = w.shape
        G = torch.empty_like(w) if conv.spectral else grad_buffer(conv.wparam)
        b = conv.bparam
        db = grad_buffer(b) if b is not None else None
        if cbar is not None:
            T.conv_wgrad(cbar, src, 0, 0, cin, KH, KW, conv.stride, conv.pad, G, name=conv.name + ".r1.wgrad", dbias=db)
        elif db is not None:
            db.zero_()
        T.conv_wgrad(tbar, tsrc, 0, 0, cin, KH, KW, conv.stride, conv.pad, G, accumulate=cbar is not None, name=conv.name + ".r1.wgrad_t")
        if conv.spectral:
            s_, u_, v_ = sig[id(conv)]
            dwo = grad_buffer(conv.wparam)
            T.spectral_grad(G, w, u_, v_, s_, dwo)
            _acc(grads, conv.wparam, dwo)
        else:
            _acc(grads, conv.wparam, G)
        if db is not None:
            _acc(grads, b, db)


# ---------------------------------------------------------------------------------------------------------------
# the training script's side
# ---------------------------------------------------------------------------------------------------------------
def add_r1_args(parser):
    """--r1_gamma / --r1_interval of train_generator.py.  Like the guard's flags they appear in the parsed namespace only when given."""
    import argparse
    parser.add_argument("--r1_gamma", type=float, default=argparse.SUPPRESS,
                        help="R1 gradient penalty gamma / 2 * E_real ||dD/dx||^2 on the PatchGAN, as a separate lazy phase behind the "
                             "D step (0: off)")
    parser.add_argument("--r1_interval", type=int, default=argparse.SUPPRESS,
                        help="the R1 phase runs every this many iterations, its gradient multiplied by it (default 16)")


def r1_from_opt(opt) -> Optional[R1]:
    """The script's R1, or None without --r1_gamma (nothing allocated or launched)."""
    gamma = float(getattr(opt, "r1_gamma", 0.0) or 0.0)
    if gamma == 0.0:
        return None
    return R1(gamma, int(getattr(opt, "r1_interval", 16)))


def r1_line(r1: Optional[R1], losses) -> str:
    """The tail of the script's printed line: '' without --r1_gamma and in the iterations between two phases."""
    if r1 is None or "D_R1" not in losses:
        return ""
    return ", D_r1: %.4g, r1_pen: %.4g" % (float(losses["D_R1"]), float(r1.last["r1_penalty"]))
