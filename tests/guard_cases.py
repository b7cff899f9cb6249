"""Cases and float64 restatement of the guarded Adam step (csrc/grad_guard.hip, optim.Adam(max_grad_norm=, skip_nonfinite=)).
Pure CPU torch: tests/test_guard_cases_cpu.py holds the restatement against torch.nn.utils.clip_grad_norm_ + torch.optim.Adam,
tests/test_gpu_grad_guard.py holds the kernels against the restatement.

The restatement follows the kernels' contract, in float64 except where the contract says fp32:
  sumsq  = sum of (double)g^2                   nonfinite = elements whose exponent field is all ones
  norm   = fp32(gscale * sqrt(sumsq))           scale = fp32 min(1, max_norm / (norm + 1e-6)), a NaN kept; 1 with clipping off
  apply  = 0 iff skip_nonfinite and (nonfinite != 0 or norm is not finite in fp32)
  Adam (torch.optim.Adam, no amsgrad) on gi = (g * gscale) * scale for applied steps; a skipped step moves nothing, the step
  count included."""
import math

import numpy as np
import torch

P = 1024                    # partial slots of the reduction (hrv_grad_guard_slots(); GUARD_SLOTS in csrc/grad_guard.hip)
BLOCK = 256                 # threads per slot; one float4 group each and trip: P * 1024 elements per pass of the grid
PASS = P * BLOCK * 4
# one wave, one block, the block edge, exactly one pass of the grid, one past it, a second trip of the grid-stride loop
SIZES = [1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, PASS - 1, PASS, PASS + 1, 2 * PASS + 7]
BAND = 64                   # NaNs on either side of every buffer: a read outside [0, n) shows up in the count
POISONS = {"nan": float("nan"), "pinf": float("inf"), "ninf": float("-inf")}


def banded(vals: torch.Tensor, shift: int):
    """(storage, view): ``vals`` between two bands of NaNs; ``shift`` = 0 starts the view on a 16-byte boundary of the storage
    (torch allocations are at least 64-byte aligned), 1 makes it 4-byte aligned only (the ``buf[1:]`` of the issue)."""
    n = vals.numel()
    buf = torch.full((BAND + shift + n + BAND,), float("nan"), dtype=torch.float32)
    buf[BAND + shift:BAND + shift + n] = vals
    return buf, (BAND + shift, n)


def int_grads(n: int, seed: int) -> torch.Tensor:
    """values in {0, +-1, +-2}: every partial sum of squares is an integer below 2^24 (4 n <= 8.4e6), so any order of summation,
    in fp32 or fp64, gives the same value"""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-2, 3, (n,), generator=g).float()


def gauss_grads(n: int, seed: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, generator=g)


def sumsq_ref(vals: torch.Tensor):
    """(float64 sum of squares, count of non-finite elements)"""
    bits = vals.contiguous().view(torch.int32)
    return float((vals.double() ** 2).sum()), int(((bits & 0x7f800000) == 0x7f800000).sum())


def finalize_ref(sumsq: float, nonfinite: int, gscale: float = 1.0, max_norm=None, skip_nonfinite: bool = False):
    """{norm, scale, apply} as Python floats holding fp32 values"""
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        norm = np.float32(np.float64(np.float32(gscale)) * np.sqrt(np.float64(sumsq)))
        scale = np.float32(1.0)
        if max_norm:
            coef = np.float32(max_norm) / (norm + np.float32(1e-6))
            scale = coef if (coef < 1.0 or np.isnan(coef)) else np.float32(1.0)
    apply = 0 if (skip_nonfinite and (nonfinite != 0 or not np.isfinite(norm))) else 1
    return {"norm": float(norm), "scale": float(scale), "apply": apply}


def ulp32(x: float) -> float:
    return float(np.spacing(np.float32(abs(x))))


def block_edge_positions(n: int, shift: int):
    """Where the non-finite cases plant their element: first, last, the last element of block 0's first trip (element
    head + 1023: the float4 body starts ``head`` elements in), the scalar tail behind the float4 body (the last element when
    (n - head) % 4 != 0)"""
    head = min(n, (4 - shift) % 4)      # the storage is 16-byte aligned, the view starts ``shift`` elements in
    pos = {0, n - 1}
    if n > head + 1024:
        pos.add(head + 1023)
    if (n - head) % 4 and n > head:
        pos.add(n - 1 - ((n - head) % 4 - 1))      # first element of the tail
    return sorted(pos)


# ---------------------------------------------------------------------------------------------------------------
# optimizer cases
# ---------------------------------------------------------------------------------------------------------------
SHAPES = [(300,), (13, 7), (801,)]       # 1192 elements; 91 and 801 are no multiples of 4: the flat buffer pads their spans
LR, BETAS, EPS = 1e-2, (0.5, 0.999), 1e-8


def start_weights(seed: int = 11):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=g) for s in SHAPES]


def square_grads(step: int):
    """Integer gradients over SHAPES whose sum of squares is 4096 = 64^2: 1000 elements of +-2 and 96 of +-1 at positions and
    signs drawn per step.  norm = 64 (32 with gscale 0.5): norm + 1e-6 == norm in fp32, and max_norm = norm / 2^k gives
    scale = 2^-k exactly."""
    n = sum(math.prod(s) for s in SHAPES)
    g = torch.Generator().manual_seed(500 + step)
    perm = torch.randperm(n, generator=g)
    sign = torch.randint(0, 2, (n,), generator=g).float() * 2 - 1
    flat = torch.zeros(n)
    flat[perm[:1000]] = 2.0
    flat[perm[1000:1096]] = 1.0
    return split(flat * sign)


SQUARE_NORM = 64.0


def gauss_grad_list(step: int, scale: float = 1.0):
    g = torch.Generator().manual_seed(700 + step)
    return [torch.randn(s, generator=g) * scale for s in SHAPES]


def split(flat: torch.Tensor):
    out, o = [], 0
    for s in SHAPES:
        k = math.prod(s)
        out.append(flat[o:o + k].reshape(s).clone())
        o += k
    return out


def poison(grads, kind: str = "nan"):
    out = [g.clone() for g in grads]
    out[1].view(-1)[5] = POISONS[kind]
    return out


def adam_ref64(weights, grad_steps, gscale=1.0, max_norm=None, skip_nonfinite=False, lr=LR, betas=BETAS, eps=EPS, wd=0.0):
    """The guarded optimizer in float64 over a list of per-step gradient lists.  Returns per step
    {w, m, v (lists of float64 tensors), step (applied steps so far), rec (finalize_ref + running totals)}."""
    b1, b2 = betas
    w = [x.double().clone() for x in weights]
    m = [torch.zeros_like(x) for x in w]
    v = [torch.zeros_like(x) for x in w]
    t, seen, skipped, clipped, out = 0, 0, 0, 0, []
    for grads in grad_steps:
        flat = torch.cat([g.reshape(-1) for g in grads])
        ss, nf = sumsq_ref(flat)
        rec = finalize_ref(ss, nf, gscale, max_norm, skip_nonfinite)
        seen += 1
        if rec["apply"]:
            t += 1
            clipped += rec["scale"] < 1.0
            bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
            for i, g in enumerate(grads):
                gi = (g.double() * float(np.float32(gscale))) * rec["scale"]
                if wd:
                    gi = gi + wd * w[i]
                m[i] = b1 * m[i] + (1 - b1) * gi
                v[i] = b2 * v[i] + (1 - b2) * gi * gi
                w[i] = w[i] - (lr / bc1) * (m[i] / (v[i].sqrt() / math.sqrt(bc2) + eps))
        else:
            skipped += 1
        rec.update(steps=seen, skipped=skipped, clipped=int(clipped), nonfinite=nf, sumsq=ss)
        out.append({"w": [x.clone() for x in w], "m": [x.clone() for x in m], "v": [x.clone() for x in v], "step": t, "rec": rec})
    return out


def torch_clip_adam(weights, grad_steps, max_norm, lr=LR, betas=BETAS, eps=EPS, dtype=torch.float32):
    """torch.nn.utils.clip_grad_norm_ followed by torch.optim.Adam on the CPU, in ``dtype``; per step the list of weights"""
    ps = [torch.nn.Parameter(x.to(dtype).clone()) for x in weights]
    opt = torch.optim.Adam(ps, lr=lr, betas=betas, eps=eps)
    out = []
    for grads in grad_steps:
        for p, g in zip(ps, grads):
            p.grad = g.to(dtype).clone()
        if max_norm:
            torch.nn.utils.clip_grad_norm_(ps, max_norm)
        opt.step()
        out.append([p.detach().clone() for p in ps])
    return out


def rel_err(got, want64):
    """max over tensors of max|got - want| / max|want|, in float64"""
    return max(float((g.double().cpu() - w).abs().max() / w.abs().max()) for g, w in zip(got, want64))
