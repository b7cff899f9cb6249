"""torch.optim.Adam drop-in whose step is ONE fused HIP launch over a flat parameter buffer
(train_generator.py:154-157,322,360).  Parameters are re-pointed to views of the flat buffer on the
first step; gradients are gathered into a flat buffer (or taken from a ``GradSync``'s all-reduced
buckets).  LambdaLR and friends work unchanged (it is a torch.optim.Optimizer)."""
from __future__ import annotations

import contextlib
import os

import torch

from . import ops
from . import train_ops as T


def _flat_order(ps):
    """Order of the parameters inside the flat buffers: registration order, except that a parameter carrying
    ``_hrv_flat_after = mate`` sits right behind its mate (SPADE's conv_beta behind conv_gamma: their gradients are
    produced as one [gamma ; beta] matrix, gen_train.SpadeT.backward).  The optimizer's arithmetic is element-wise:
    the order changes no value."""
    ids = {id(p) for p in ps}
    follow = {}
    for p in ps:
        mate = getattr(p, "_hrv_flat_after", None)
        if mate is not None and id(mate) in ids and mate is not p:
            follow.setdefault(id(mate), []).append(p)
    placed, out = set(), []

    def put(p):
        if id(p) in placed:
            return
        placed.add(id(p))
        out.append(p)
        for q in follow.get(id(p), ()):
            put(q)
    for p in ps:
        mate = getattr(p, "_hrv_flat_after", None)
        if mate is not None and id(mate) in ids and mate is not p and id(p) not in placed:
            put(mate)
        put(p)
    return out


class Adam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, grad_sync=None, device_step=False,
                 max_grad_norm=None, skip_nonfinite=False, ema_decay=None, ema_warmup=False):
        """``device_step``: the step count and the learning rate live on the device (hrv_adam_hyper_f32 / _dev_f32), so a
        hipGraph-captured iteration (graph.GraphedTrainStep) keeps counting and follows the scheduler; every parameter must
        then receive a gradient in every iteration (or in none at all, without weight decay: it is then left as it is).

        ``max_grad_norm`` / ``skip_nonfinite``: the guarded step (csrc/grad_guard.hip).  With either set, step() first reduces the
        whole flat gradient buffer of a group to its 2-norm (fp64 accumulation, deterministic) and a count of non-finite elements,
        and the Adam launch consumes the decision ON THE DEVICE: no host synchronisation, capturable in a hipGraph.
        ``max_grad_norm``: the gradients of a group are scaled by min(1, max_grad_norm / (norm + 1e-6)), the expression of
        torch.nn.utils.clip_grad_norm_ (with ``skip_nonfinite`` off a non-finite norm propagates into the weights, as with
        ``error_if_nonfinite=False`` there).  ``skip_nonfinite``: a step whose gradients hold an Inf / NaN, or whose norm overflows
        fp32, touches neither weights nor moments nor the step count; it needs ``device_step=True`` (a host-side step count
        cannot learn of a skip without a synchronisation).  With both at their defaults nothing is allocated or launched for it.
        The norm is taken per parameter group (one flat buffer each), over the all-reduced and averaged gradients under data
        parallelism, so every rank decides alike.

        The guard covers the optimizer's state: weights, moments, step count.  State a forward pass wrote BEFORE the gradient
        existed is not rolled back by a skip: BatchNorm running statistics (the condition generator), spectral norm's ``u``.

        ``ema_decay`` (None or 0: off; otherwise 0 < ema_decay < 1): an exponential moving average of the weights, kept in one more
        flat buffer by the SAME launch that updates them (csrc/adam_ema.hip): e <- e + (1 - d) (w' - e), with d = ema_decay, or
        with ``ema_warmup`` d = min(ema_decay, (1 + t) / (10 + t)) at the step count t of the launch.  The average starts at the
        initial (or loaded) weights.  The weights, moments and step counts are bit for bit those of the optimizer without it.  A
        step the guard skips leaves the average alone, and under ``device_step`` the schedule follows the device-side count, so a
        captured iteration keeps averaging.  On the host-count path a parameter WITHOUT a gradient in some iteration keeps its
        average as well as its weight: the weight did not move, and the average is not pulled further towards it.  Under
        ``device_step`` a parameter that never has a gradient rides along: w' == w keeps its average at w up to rounding.  The
        average is element-wise over the flat buffer: data-parallel ranks hold the same one without communication.
        ``ema_buffer()``, ``ema_state_dict(module)`` and ``swap_ema()`` read and use it."""
        defaults = dict(lr=lr, betas=(float(betas[0]), float(betas[1])), eps=eps, weight_decay=weight_decay)
        super().__init__(params, defaults)
        self.grad_sync = grad_sync
        self._flat = {}
        self.device_step = bool(device_step)
        self.max_grad_norm = float(max_grad_norm) if max_grad_norm else None
        if self.max_grad_norm is not None and not self.max_grad_norm > 0.0:
            raise ops.HrvError(f"Adam: max_grad_norm must be positive (None or 0 switches clipping off), got {max_grad_norm}")
        self.skip_nonfinite = bool(skip_nonfinite)
        if self.skip_nonfinite and not self.device_step:
            raise ops.HrvError("Adam: skip_nonfinite=True needs the step count on the device; build the optimizer with "
                               "device_step=True")
        self.guarded = self.max_grad_norm is not None or self.skip_nonfinite
        self.ema_decay = float(ema_decay) if ema_decay else None
        if self.ema_decay is not None and not 0.0 < self.ema_decay < 1.0:
            raise ops.HrvError(f"Adam: ema_decay must lie strictly between 0 and 1 (None or 0 switches the average off), got {ema_decay}")
        self.ema_warmup = bool(ema_warmup)
        self._swapped = False

    @property
    def guard_record(self):
        """The device-side guard record of parameter group 0 (int32 [16]; layout: include/hrviton_hip.h), for callers that must
        not synchronise; ``guard_records()`` lists every group's.  None before the first step, or with the guard off."""
        st = self._flat.get(0)
        return st.get("guard") if st else None

    def guard_records(self):
        return [(self._flat.get(gi) or {}).get("guard") for gi in range(len(self.param_groups))]

    def guard_stats(self, group: int = 0):
        """The guard record of one parameter group as Python numbers (ONE host copy, which synchronises): ``norm`` and ``scale`` of
        the last step, ``apply`` (0: it was skipped), its ``nonfinite`` element count, its un-scaled ``sumsq``, and the running
        totals ``steps`` / ``skipped`` / ``clipped``.  None with the guard off or before the first step."""
        st = self._flat.get(group)
        if not st or "guard" not in st:
            return None
        return T.guard_read(st["guard"])

    # ------------------------------------------------------------------ per-parameter statistics
    def prepare_layer_stats(self):
        """Build what layer_stats() needs for every parameter group -- the flat buffers if no step has run yet, the piece table,
        the partials and the records (train_ops.span_stats_alloc) -- so that a later call allocates nothing: call it before
        capturing ``layer_stats(read=False)`` in a hipGraph.  Nothing is launched."""
        for gi, group in enumerate(self.param_groups):
            st = self._flat.get(gi) or self._setup(gi, group)
            if "span_ws" not in st:
                st["span_ws"] = T.span_stats_alloc(st["spans"], st["w"].device)

    def layer_stats(self, group: int = 0, read: bool = True):
        """Per-parameter statistics of one group's flat buffers in two launches on the current stream (csrc/span_stats.hip; read-only:
        weights, moments and gradients keep their bits, and an optimizer that is never asked allocates and launches nothing for it).
        Meant for any time after a step(): the flat gradient buffer still holds that step's gradient until the next backward.  One
        dict per parameter, in the order of the flat buffer:
          param, numel
          grad_norm, grad_maxabs      with the data-parallel 1 / world factor step() applies;  grad_nonfinite, grad_zeros (elements == +-0)
          weight_norm, weight_maxabs, weight_nonfinite
          update_norm      (lr / bc1) * ||u||, u = m / (sqrt(v) / bc2_sqrt + eps) formed like the Adam kernel forms it from the CURRENT
                           moments: after an applied step this is ||w_before - w_after||, with or without weight decay or clipping
          update_ratio     update_norm / weight_norm (None where weight_norm is 0);  update_nonfinite
        Non-finite elements are counted and left out of norms and maxima.  After a step the guard SKIPPED, ``grad_*`` describe the
        poisoned gradient and ``update_*`` the stale moments' direction.  On the host-count path a parameter whose own step count
        differs from the group's (it had no gradient in some iteration) gets None for update_norm and update_ratio.  Inside
        ``swap_ema()`` the flat weight buffer holds the averaged weights: ``weight_*`` and ``update_ratio`` then describe those.
        Reading costs at most two device-to-host copies (the records; on the device-step path lr and the bias corrections).
        ``read=False``: only the two launches; returns the device record tensor (int32 [n][16]; layout: include/hrviton_hip.h)
        for a captured iteration -- after prepare_layer_stats() it allocates nothing.  Capture it with ``device_step=True``: the
        kernel then reads the bias correction from the device; on the host-count path the scalar of the capture would be replayed."""
        import numpy as np
        grp = self.param_groups[group]
        st = self._flat.get(group)
        if st is None or "span_ws" not in st:
            self.prepare_layer_stats()
            st = self._flat[group]
        b1, b2 = grp["betas"]
        hyper = st.get("hyper")
        t = max(int(st["step"]), 1)
        bc2_sqrt = float(np.sqrt(np.float32(1.0) - np.power(np.float32(b2), np.float32(t))))
        rec = T.span_stats(st["span_ws"], st["g"], st["w"], st["m"], st["v"], hyper, bc2_sqrt, grp["eps"])
        if not read:
            return rec
        rows = T.span_stats_read(rec)
        if hyper is not None:
            lr, bc1 = (float(x) for x in hyper[:2].tolist())
        else:
            lr, bc1 = float(grp["lr"]), 1.0 - b1 ** t
        step_size = lr / bc1 if bc1 != 0.0 else 0.0      # (a device count that never advanced: every step so far was skipped)
        gscale = 1.0 / self.grad_sync.world if self.grad_sync is not None else 1.0
        out = []
        for i, ((p, _, k), r) in enumerate(zip(st["spans"], rows)):
            wn = r["w_sumsq"] ** 0.5
            un = step_size * r["u_sumsq"] ** 0.5
            if hyper is None and st["steps"][i] != st["step"]:
                un = None
            out.append({"param": p, "numel": k, "grad_norm": gscale * r["g_sumsq"] ** 0.5, "grad_maxabs": gscale * r["g_maxabs"],
                        "grad_nonfinite": r["g_nonfinite"], "grad_zeros": r["g_zeros"], "weight_norm": wn,
                        "weight_maxabs": r["w_maxabs"], "weight_nonfinite": r["w_nonfinite"], "update_norm": un,
                        "update_ratio": un / wn if un is not None and wn > 0.0 else None, "update_nonfinite": r["u_nonfinite"]})
        return out

    def push_lr(self):
        """device_step: copy each group's current learning rate to its device scalar (call BEFORE replaying a captured
        iteration; an eager step() does it itself)."""
        for gi, group in enumerate(self.param_groups):
            st = self._flat.get(gi)
            if st is not None and "lr_dev" in st:
                st["lr_dev"].fill_(float(group["lr"]))

    def _setup(self, gi, group):
        ps = _flat_order([p for p in group["params"] if p.requires_grad])
        for p in ps:
            ops.require_cuda(p.data, "hr_viton_amd.optim.Adam parameter")
        # every parameter starts on a 16-byte boundary of the flat buffer: the conv epilogues take
        # float4 loads of bias / scale vectors (unaligned ones fall back to the scalar epilogue)
        n = sum((p.numel() + 3) // 4 * 4 for p in ps)
        dev = ps[0].device
        w = torch.zeros(n, dtype=torch.float32, device=dev)
        off = 0
        spans = []
        for p in ps:
            k = p.numel()
            w[off:off + k].copy_(p.data.reshape(-1))
            p.data = w[off:off + k].view_as(p.data)      # the parameter now lives in the flat buffer
            spans.append((p, off, k))
            off += (k + 3) // 4 * 4
        # ``steps``: one counter per parameter, like torch.optim.Adam's state[p]["step"] -- a parameter without a gradient
        # in some iteration (skipped below) falls behind the others, and its bias correction must use ITS count
        st = dict(w=w, m=torch.zeros_like(w), v=torch.zeros_like(w), g=torch.zeros_like(w), spans=spans, step=0,
                  steps=[0] * len(spans))
        if self.ema_decay is not None:
            st["ema"] = w.clone()
        if self.guarded:      # record + workspace exist before any step (a captured step() allocates nothing)
            st["guard"], st["guard_part"], st["guard_cnt"] = T.guard_alloc(dev)
        self._flat[gi] = st
        # the backward plans write gradients straight into these slots (gen_train.grad_buffer / _acc)
        for p, off, k in spans:
            p._hrv_flat_grad = st["g"][off:off + k].view_as(p.data)
        return st

    def make_grad_sync(self, bucket_mb: float = 64.0, process_group=None, graph: bool = False):
        """Data-parallel gradient synchronisation that all-reduces contiguous slices of THIS optimizer's flat
        gradient buffer in place (parallel.GradSync): the backward plans write each gradient into its slot, the
        bucket collectives run on the buffer itself, the fused step reads it -- zero gradient copies.
        ``graph=True``: the variant for a hipGraph-captured iteration (parallel.GraphGradSync: one collective over the whole
        buffer between two graph segments)."""
        from .parallel import GradSync, GraphGradSync
        if len(self.param_groups) != 1:
            raise ops.HrvError("make_grad_sync: one parameter group per fused optimizer")
        st = self._flat.get(0) or self._setup(0, self.param_groups[0])
        if graph:
            self.grad_sync = GraphGradSync(st["g"], st["spans"], process_group, bucket_mb)
        else:
            self.grad_sync = GradSync(None, bucket_mb, process_group, flat=st["g"], spans=st["spans"])
        return self.grad_sync

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():            # like torch.optim: the closure may call backward()
                loss = closure()
        if self._swapped:
            raise ops.HrvError("Adam.step() inside swap_ema(): the flat weight buffer holds the averaged weights; leave the context first")
        from . import train_ops as _T
        _T.wgrad_join()            # weight gradients of the last backward may sit on the side stream (train_ops.wgrad_side)
        world_scale = 1.0
        if self.grad_sync is not None:
            self.grad_sync.wait()
            world_scale = 1.0 / self.grad_sync.world
        for gi, group in enumerate(self.param_groups):
            st = self._flat.get(gi) or self._setup(gi, group)
            g = st["g"]
            base = g.data_ptr()
            skipped, missing = [], 0
            steps = st["steps"]
            for i, (p, off, k) in enumerate(st["spans"]):
                src = self.grad_sync.grad_of(p) if self.grad_sync is not None else p.grad
                if src is None:
                    # torch's Adam SKIPS a parameter without a gradient (weight, moments, weight decay and its step count
                    # untouched): the fused launch covers whole runs of the flat buffer, so the span is snapshotted here
                    # and restored below
                    g[off:off + k].zero_()
                    if self.device_step:
                        # a parameter that has NEVER had a gradient (a block the configured generator does not use) rides along:
                        # zero gradient on zero moments without weight decay is an exact no-op of the update.  One that had
                        # gradients before would need its own step count: refused below.
                        missing += steps[i] != 0 or group["weight_decay"] != 0
                        st.setdefault("never", set()).add(i)
                        continue
                    skipped.append((off, k, st["w"][off:off + k].clone(), st["m"][off:off + k].clone(),
                                    st["v"][off:off + k].clone(), st["ema"][off:off + k].clone() if "ema" in st else None))
                else:
                    if self.device_step and i in st.get("never", ()):      # ... and one that rode along cannot join later
                        missing += 1
                    steps[i] += 1
                    if src.data_ptr() != base + 4 * off:   # already produced in place by the backward plan otherwise
                        g[off:off + k].copy_(src.reshape(-1))
            st["step"] += 1
            b1, b2 = group["betas"]
            ema, decay, warm = st.get("ema"), self.ema_decay, self.ema_warmup
            if self.guarded:
                # the padding between spans is zero (zeros_like; every writer takes a k-element view): the sum over the buffer
                # is the sum over the parameters' elements
                T.grad_sumsq(g, st["guard_part"], st["guard_cnt"])
            if self.device_step:
                if missing:
                    raise ops.HrvError("device_step Adam: every parameter needs a gradient in every iteration (one device-side "
                                       f"step count serves the whole buffer); {missing} parameter(s) had none")
                if "step_dev" not in st:
                    dev = g.device
                    st["step_dev"] = torch.full((1,), st["step"] - 1, dtype=torch.int32, device=dev)
                    st["lr_dev"] = torch.full((1,), float(group["lr"]), dtype=torch.float32, device=dev)
                    st["hyper"] = torch.zeros(3, dtype=torch.float32, device=dev)
                if not torch.cuda.is_current_stream_capturing():
                    st["lr_dev"].fill_(float(group["lr"]))       # (a captured iteration reads what push_lr() wrote)
                if self.guarded:
                    T.grad_guard_finalize(st["guard_part"], st["guard_cnt"], st["guard"], world_scale, self.max_grad_norm,
                                          self.skip_nonfinite, st["step_dev"], st["lr_dev"], st["hyper"], b1, b2)
                    if ema is not None:
                        T.adam_step_dev_guarded_ema(st["w"], g, st["m"], st["v"], ema, st["hyper"], b1, b2, group["eps"],
                                                    group["weight_decay"], world_scale, st["guard"], st["step_dev"], decay, warm)
                    else:
                        T.adam_step_dev_guarded(st["w"], g, st["m"], st["v"], st["hyper"], b1, b2, group["eps"], group["weight_decay"],
                                                world_scale, st["guard"])
                elif ema is not None:
                    T.adam_step_dev_ema(st["w"], g, st["m"], st["v"], ema, st["step_dev"], st["lr_dev"], st["hyper"], b1, b2, group["eps"],
                                        group["weight_decay"], world_scale, decay, warm)
                else:
                    T.adam_step_dev(st["w"], g, st["m"], st["v"], st["step_dev"], st["lr_dev"], st["hyper"], b1, b2, group["eps"],
                                    group["weight_decay"], world_scale)
                continue
            if self.guarded:      # (clipping alone: every launch below reads the same scale)
                T.grad_guard_finalize(st["guard_part"], st["guard_cnt"], st["guard"], world_scale, self.max_grad_norm, False)
            # one launch per run of consecutive spans that share a step count (a skipped span rides along with either
            # neighbour: it is restored afterwards) -- ONE launch over the whole buffer unless some parameter fell behind
            runs, n_sp = [], len(st["spans"])
            skipped_offs = {s[0] for s in skipped}
            i = 0
            while i < n_sp:
                if st["spans"][i][1] in skipped_offs:
                    i += 1
                    continue
                j, cnt = i, steps[i]
                while j + 1 < n_sp and (st["spans"][j + 1][1] in skipped_offs or steps[j + 1] == cnt):
                    j += 1
                a = st["spans"][i][1]
                b = st["spans"][j][1] + (st["spans"][j][2] + 3) // 4 * 4
                runs.append((a, min(b, g.numel()), cnt))
                i = j + 1
            if len(runs) == 1 and len(skipped) == 0:
                runs = [(0, g.numel(), runs[0][2])]
            for a, b, cnt in runs:
                if ema is not None and self.guarded:
                    T.adam_step_guarded_ema(st["w"][a:b], g[a:b], st["m"][a:b], st["v"][a:b], ema[a:b], float(group["lr"]), b1, b2,
                                            group["eps"], group["weight_decay"], cnt, world_scale, st["guard"], decay, warm)
                elif ema is not None:
                    T.adam_step_ema(st["w"][a:b], g[a:b], st["m"][a:b], st["v"][a:b], ema[a:b], float(group["lr"]), b1, b2, group["eps"],
                                    group["weight_decay"], cnt, world_scale, decay, warm)
                elif self.guarded:
                    T.adam_step_guarded(st["w"][a:b], g[a:b], st["m"][a:b], st["v"][a:b], float(group["lr"]), b1, b2, group["eps"],
                                        group["weight_decay"], cnt, world_scale, st["guard"])
                else:
                    T.adam_step(st["w"][a:b], g[a:b], st["m"][a:b], st["v"][a:b], float(group["lr"]), b1, b2, group["eps"],
                                group["weight_decay"], cnt, world_scale)
            for off, k, w0, m0, v0, e0 in skipped:
                st["w"][off:off + k].copy_(w0)
                st["m"][off:off + k].copy_(m0)
                st["v"][off:off + k].copy_(v0)
                if e0 is not None:
                    st["ema"][off:off + k].copy_(e0)
        self._bump_epochs()
        return loss

    def _bump_epochs(self):
        for group in self.param_groups:          # cached inference plans of THESE parameters are stale now
            for p in group["params"]:
                p._hrv_epoch = getattr(p, "_hrv_epoch", 0) + 1
        ops.WEIGHTS_EPOCH[0] += 1

    # ------------------------------------------------------------------ the averaged weights
    def _ema_state(self, gi, what):
        if self.ema_decay is None:
            raise ops.HrvError(f"Adam.{what}: the optimizer was built without ema_decay")
        return self._flat.get(gi) or self._setup(gi, self.param_groups[gi])

    def ema_buffer(self, group: int = 0):
        """The flat fp32 buffer of averaged weights of one parameter group, laid out like the flat weight buffer."""
        return self._ema_state(group, "ema_buffer")["ema"]

    def ema_state_dict(self, module):
        """``module.state_dict()`` with every parameter this optimizer owns replaced by (a copy of) its averaged value; the keys
        are the module's, so the file loads wherever the raw checkpoint does.  Buffers stay the live ones -- spectral norm's
        ``weight_u`` / ``weight_v``, BatchNorm statistics: they are no parameters and are not averaged, the usual practice."""
        where = {}
        for gi in range(len(self.param_groups)):
            st = self._ema_state(gi, "ema_state_dict")
            for p, off, k in st["spans"]:
                where[id(p)] = (st["ema"], off, k)
        sd = module.state_dict()
        for name, p in module.named_parameters():
            if id(p) in where and name in sd:
                e, off, k = where[id(p)]
                sd[name] = e[off:off + k].view_as(p).clone()
        return sd

    def load_ema_state_dict(self, module, sd):
        """Seed the average from a file ema_state_dict() produced: every parameter of ``module`` this optimizer owns whose key is
        in ``sd`` takes that value; the others keep theirs."""
        where = {}
        for gi in range(len(self.param_groups)):
            st = self._ema_state(gi, "load_ema_state_dict")
            for p, off, k in st["spans"]:
                where[id(p)] = (st["ema"], off, k)
        for name, p in module.named_parameters():
            if id(p) in where and name in sd:
                e, off, k = where[id(p)]
                if sd[name].numel() != k:
                    raise ops.HrvError(f"load_ema_state_dict: {name} has {sd[name].numel()} elements, the parameter {k}")
                e[off:off + k].copy_(sd[name].reshape(-1).to(e.device, torch.float32))

    @contextlib.contextmanager
    def swap_ema(self):
        """Inside the context the parameters HOLD the averaged weights (the flat weight and average buffers are exchanged in place
        by hrv_swap_f32, per group, on entry and again on exit: no clone of the buffer), for evaluation.  Cached inference plans
        rebuild (ops.WEIGHTS_EPOCH and every parameter's ``_hrv_epoch`` move both times).  Not exchanged: buffers (spectral
        norm's ``u`` / ``v``); a hipGraph captured before still works on the same addresses and would read the averaged weights
        while inside.  step() raises inside the context."""
        if self._swapped:
            raise ops.HrvError("Adam.swap_ema(): already inside swap_ema()")
        states = [self._ema_state(gi, "swap_ema") for gi in range(len(self.param_groups))]

        def exchange():
            for st in states:
                T.swap_(st["w"], st["ema"])
            self._bump_epochs()
        exchange()
        self._swapped = True
        try:
            yield self
        finally:
            exchange()
            self._swapped = False

    # ------------------------------------------------------------------ (de)serialisation
    def state_dict(self):
        """torch.optim.Adam-compatible state_dict: per-parameter ``step`` / ``exp_avg`` / ``exp_avg_sq`` cut out
        of the flat moment buffers (an extension: the reference saves weights only)."""
        state, groups, idx = {}, [], 0
        for gi, group in enumerate(self.param_groups):
            st = self._flat.get(gi)
            spans = {id(p): (off, k) for p, off, k in st["spans"]} if st else {}
            pos = {id(p): i for i, (p, _, _) in enumerate(st["spans"])} if st else {}
            ids = []
            dev_step = int(st["step_dev"].item()) if st and "step_dev" in st else None      # ONE host sync per group
            never = st.get("never", ()) if st else ()      # (device_step: parameters that ride along without a gradient)
            for p in group["params"]:
                if st and id(p) in spans and pos[id(p)] not in never:      # like torch: no state for a parameter never stepped
                    off, k = spans[id(p)]
                    stp = dev_step if dev_step is not None else st["steps"][pos[id(p)]]
                    state[idx] = {"step": torch.tensor(float(stp)),
                                  "exp_avg": st["m"][off:off + k].view_as(p).clone(),
                                  "exp_avg_sq": st["v"][off:off + k].view_as(p).clone()}
                    if "ema" in st:
                        state[idx]["ema"] = st["ema"][off:off + k].view_as(p).clone()
                ids.append(idx)
                idx += 1
            g = {k: v for k, v in group.items() if k != "params"}
            g["params"] = ids
            groups.append(g)
        return {"state": state, "param_groups": groups}

    def load_state_dict(self, sd):
        idx = 0
        for gi, (group, saved) in enumerate(zip(self.param_groups, sd["param_groups"])):
            for k, v in saved.items():
                if k != "params":
                    group[k] = tuple(v) if k == "betas" else v
            st = self._flat.get(gi) or self._setup(gi, group)
            spans = {id(p): (off, k) for p, off, k in st["spans"]}
            pos = {id(p): i for i, (p, _, _) in enumerate(st["spans"])}
            loaded = None
            if "ema" in st:      # a state without "ema" (saved with the average off): the average starts at the weights
                st["ema"].copy_(st["w"])
            for p in group["params"]:
                ent = sd["state"].get(idx)
                if ent is not None and id(p) in spans:
                    off, k = spans[id(p)]
                    if "ema" in st and "ema" in ent:
                        st["ema"][off:off + k].copy_(ent["ema"].reshape(-1).to(st["ema"].device))
                    st["m"][off:off + k].copy_(ent["exp_avg"].reshape(-1).to(st["m"].device))
                    st["v"][off:off + k].copy_(ent["exp_avg_sq"].reshape(-1).to(st["v"].device))
                    st["steps"][pos[id(p)]] = int(ent["step"])
                    loaded = int(ent["step"]) if loaded is None else max(loaded, int(ent["step"]))
                idx += 1
            if loaded is not None:
                st["step"] = loaded
            if "step_dev" in st:
                # device-side step count / learning rate (device_step=True after the first step): a resume must continue the
                # bias correction from the LOADED count, not from the one this optimizer had reached before the load
                st["step_dev"].fill_(int(st["step"]))
                st["lr_dev"].fill_(float(group["lr"]))


# ------------------------------------------------------------------ the training scripts' side of the guard
def add_guard_args(parser):
    """--max_grad_norm_G / --max_grad_norm_D / --skip_nonfinite of train_generator.py and train_condition.py.  The options appear
    in the parsed namespace only when given (argparse.SUPPRESS): a run without them prints the option line it always printed;
    guard_kwargs() reads them with their defaults (0 / 0 / off)."""
    import argparse
    parser.add_argument("--max_grad_norm_G", type=float, default=argparse.SUPPRESS,
                        help="clip the generator's gradient 2-norm to this value on the device (0: off)")
    parser.add_argument("--max_grad_norm_D", type=float, default=argparse.SUPPRESS,
                        help="clip the discriminator's gradient 2-norm to this value on the device (0: off)")
    parser.add_argument("--skip_nonfinite", action="store_true", default=argparse.SUPPRESS,
                        help="skip, on the device, an optimizer step whose gradients hold an Inf / NaN (the optimizers then keep "
                             "their step count and learning rate on the device)")


def guard_kwargs(opt, which):
    """Adam's keyword arguments for the ``which`` ("G" / "D") optimizer of a script; empty (the plain construction) without the
    flags."""
    kw = {}
    max_norm = float(getattr(opt, "max_grad_norm_" + which, 0.0) or 0.0)
    if max_norm > 0:
        kw["max_grad_norm"] = max_norm
    if getattr(opt, "skip_nonfinite", False):
        kw.update(skip_nonfinite=True, device_step=True)
    return kw


def add_ema_args(parser):
    """--ema_decay / --ema_warmup / --ema_eval / --ema_checkpoint of train_generator.py (the generator's optimizer only).  Like the
    guard's flags they appear in the parsed namespace only when given."""
    import argparse
    parser.add_argument("--ema_decay", type=float, default=argparse.SUPPRESS,
                        help="keep an exponential moving average of the generator's weights with this decay, inside the fused Adam "
                             "launch (0: off); gen_ema_step_*.pth / gen_ema_model_final.pth are written beside the raw checkpoints")
    parser.add_argument("--ema_warmup", action="store_true", default=argparse.SUPPRESS,
                        help="decay min(ema_decay, (1 + t) / (10 + t)) at optimizer step t")
    parser.add_argument("--ema_eval", action="store_true", default=argparse.SUPPRESS,
                        help="run the test/LPIPS pass and the test_images grids with the averaged weights")
    parser.add_argument("--ema_checkpoint", type=str, default=argparse.SUPPRESS,
                        help="a gen_ema_*.pth file that seeds the average of a resumed run")


def ema_kwargs(opt):
    """Adam's keyword arguments for the generator's optimizer; empty (the plain construction) without --ema_decay."""
    decay = float(getattr(opt, "ema_decay", 0.0) or 0.0)
    if decay == 0.0:
        return {}
    return dict(ema_decay=decay, ema_warmup=bool(getattr(opt, "ema_warmup", False)))


def guard_scalars(opt_g, opt_d):
    """[(tag, value)] of the guarded optimizers: Grad/norm_*, Grad/skipped_*, Grad/clipped_* (one host copy each; call only where
    the script synchronises anyway).  Both optimizers are listed as soon as one of them is guarded; an unguarded one reports zeros."""
    stats = [(sfx, o.guard_stats() if o is not None and o.guarded else None) for sfx, o in (("G", opt_g), ("D", opt_d))]
    if all(st is None for _, st in stats):
        return []
    out = []
    for key in ("norm", "skipped", "clipped"):
        for sfx, st in stats:
            out.append(("Grad/%s_%s" % (key, sfx), float(st[key]) if st else 0.0))
    return out


def guard_line(opt_g, opt_d):
    """The tail of the scripts' printed line: '' without a guard."""
    sc = dict(guard_scalars(opt_g, opt_d))
    if not sc:
        return ""
    return ", gnorm_G: %.4g, gnorm_D: %.4g, skipped_G: %d, skipped_D: %d" % (sc["Grad/norm_G"], sc["Grad/norm_D"],
                                                                             sc["Grad/skipped_G"], sc["Grad/skipped_D"])


# ------------------------------------------------------------------ per-parameter reports (Adam.layer_stats) and the scripts' side of them
LAYER_FIELDS = ("numel", "grad_norm", "grad_maxabs", "grad_nonfinite", "grad_zeros", "weight_norm", "weight_maxabs", "weight_nonfinite",
                "update_norm", "update_ratio", "update_nonfinite")


def layer_report(opt, module):
    """{name: Adam.layer_stats() entry without "param"} over every parameter group of ``opt``, keyed by ``module.named_parameters()``
    names in the order of the flat buffers (a spectral-norm weight reports under ``weight_orig``, as in the state dict).  A
    parameter of the optimizer that ``module`` does not own is left out."""
    names = {id(p): n for n, p in module.named_parameters()}
    out = {}
    for gi in range(len(opt.param_groups)):
        for e in opt.layer_stats(gi):
            name = names.get(id(e["param"]))
            if name is not None:
                out[name] = {k: e[k] for k in LAYER_FIELDS}
    return out


def add_layer_stats_args(parser):
    """--layer_stats_count / --layer_stats_top / --layer_stats_on_skip of train_generator.py and train_condition.py.  Like the
    guard's flags they appear in the parsed namespace only when given."""
    import argparse
    parser.add_argument("--layer_stats_count", type=int, default=argparse.SUPPRESS,
                        help="every N steps, after both optimizers have stepped, append one per-parameter report per optimizer "
                             "(gradient, weight and update norms, maxima, non-finite and zero counts; two launches and one small "
                             "copy each) to <tensorboard_dir>/<name>/layer_stats.jsonl (0: off)")
    parser.add_argument("--layer_stats_top", type=int, default=argparse.SUPPRESS,
                        help="how many parameters, by gradient norm, the printed line names per optimizer (default 5)")
    parser.add_argument("--layer_stats_on_skip", action="store_true", default=argparse.SUPPRESS,
                        help="needs --skip_nonfinite: write and print the report of an optimizer right after a step its guard "
                             "skipped, while the flat gradient buffer still holds the poisoned gradient.  Reads the guard record "
                             "after EVERY step: one host synchronisation per step and optimizer")


class LayerStatsLog:
    """The scripts' per-parameter reports: ``after_step`` writes the due ones and returns the text the printed line gains."""

    def __init__(self, path, count, top, on_skip, pairs):
        self.path, self.count, self.top, self.on_skip = path, int(count), int(top), bool(on_skip)
        self.pairs = pairs          # [(tag "G" / "D", optimizer, module)]

    def _text(self, tag, params):
        by_norm = sorted(params, key=lambda n: -params[n]["grad_norm"])[:self.top]
        bad = [n for n in params if params[n]["grad_nonfinite"] or params[n]["weight_nonfinite"] or params[n]["update_nonfinite"]]
        txt = ", layers_%s: " % tag + " ".join("%s=%.4g" % (n, params[n]["grad_norm"]) for n in by_norm)
        if bad:
            txt += ", nonfinite_%s: " % tag + " ".join(
                "%s(g%d/w%d/u%d)" % (n, params[n]["grad_nonfinite"], params[n]["weight_nonfinite"], params[n]["update_nonfinite"])
                for n in bad)
        return txt

    def _write(self, step, tag, o, module, board):
        import json
        params = layer_report(o, module)
        os.makedirs(os.path.dirname(self.path), exist_ok=True)
        with open(self.path, "a") as f:
            f.write(json.dumps({"step": step, "opt": tag, "params": params}) + "\n")
        if board is not None:
            ratios = [e["update_ratio"] for e in params.values() if e["update_ratio"] is not None]
            board.add_scalar("Layers/%s/update_ratio_max" % tag, max(ratios) if ratios else 0.0, step)
            board.add_scalar("Layers/%s/update_ratio_min" % tag, min(ratios) if ratios else 0.0, step)
            board.add_scalar("Layers/%s/nonfinite_params" % tag, float(sum(
                1 for e in params.values() if e["grad_nonfinite"] or e["weight_nonfinite"] or e["update_nonfinite"])), step)
            board.add_scalar("Layers/%s/zero_grad_params" % tag, float(sum(1 for e in params.values() if e["grad_zeros"] == e["numel"])), step)
        return self._text(tag, params)

    def after_step(self, step, board=None):
        """``step``: the 1-based count of the iteration that just ran.  Returns '' when no report was due."""
        due = self.count > 0 and step % self.count == 0
        text = ""
        for tag, o, module in self.pairs:
            skipped = False
            if self.on_skip:
                gs = o.guard_stats()      # (the host synchronisation --layer_stats_on_skip costs)
                skipped = gs is not None and gs["apply"] == 0
            if due or skipped:
                t = self._write(step, tag, o, module, board)
                if skipped:
                    print("step: %8d, optimizer %s skipped its step%s" % (step, tag, t), flush=True)
                text += t
        return text


def check_layer_stats_args(opt):
    """(count, on_skip) of the parsed flags; exits with a message on a combination that cannot work (the scripts call it before
    they build anything)."""
    count = int(getattr(opt, "layer_stats_count", 0) or 0)
    on_skip = bool(getattr(opt, "layer_stats_on_skip", False))
    if on_skip and not getattr(opt, "skip_nonfinite", False):
        raise SystemExit("--layer_stats_on_skip needs --skip_nonfinite (without it no step is ever skipped)")
    if count < 0 or int(getattr(opt, "layer_stats_top", 5)) < 0:
        raise SystemExit("--layer_stats_count and --layer_stats_top must be >= 0")
    return count, on_skip


def layer_stats_from_opt(opt, pairs):
    """The scripts' LayerStatsLog, or None without --layer_stats_count / --layer_stats_on_skip (nothing is allocated or launched)."""
    count, on_skip = check_layer_stats_args(opt)
    if count == 0 and not on_skip:
        return None
    return LayerStatsLog(os.path.join(opt.tensorboard_dir, opt.name, "layer_stats.jsonl"), count,
                         int(getattr(opt, "layer_stats_top", 5)), on_skip, pairs)
