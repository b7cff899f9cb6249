"""Cases and restatements of the Adam step that keeps an exponential moving average of the weights (csrc/adam_ema.hip,
optim.Adam(ema_decay=, ema_warmup=)).  Pure CPU torch / numpy: tests/test_ema_cases_cpu.py holds the restatements against a plain
float64 loop, tests/test_gpu_ema.py holds the kernels against the restatements.

The contract per element, in fp32 (include/hrviton_hip.h):
  w'  = what the plain / guarded kernel of the same arguments writes, bit for bit (m, v likewise)
  d   = warmup ? min(decay, (1 + t) / (10 + t)) : decay        t = the launch's step count, as float
  omd = 1 - d
  e'  = w' if omd == 1 else fma(omd, w' - e, e)                 (w' - e rounded to fp32 first)

Geometry of the kernels (EMA_BLOCK / EMA_CAP in csrc/adam_ema.hip): 256-thread blocks, at most 2048 of them, grid-stride; with all
pointers on 16-byte boundaries one 16-byte group of each array per thread and trip, so one pass of the full grid covers
2048 * 256 * 4 elements; otherwise 4 bytes per thread and trip for the whole launch."""
import math
from fractions import Fraction

import numpy as np
import torch

from guard_cases import BAND, banded  # noqa: F401  (the NaN bands of the guard's cases)

BLOCK = 256                 # threads per block
CAP = 2048                  # blocks at most
PASS = CAP * BLOCK * 4      # elements per pass of the grid on the 16-byte path
# one element, the tail alone, one group, group + tail, around one block of the scalar path, around one block of the 16-byte path,
# exactly one pass of the grid, one to either side, a second trip of the grid-stride loop plus a tail
SIZES = [1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, PASS - 1, PASS, PASS + 1, 2 * PASS + 7]
SHIFTS = [0, 1]             # 0: the view starts on a 16-byte boundary; 1: buf[1:], 4-byte aligned only
LR, BETAS, EPS = 1e-2, (0.5, 0.999), 1e-8


def gauss(n: int, seed: int, scale: float = 1.0) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, generator=g) * scale


def gauss_state(n: int, seed: int):
    """(w, g, m, v, e): Gaussian weights, gradients and first moments, non-negative second moments, an average near the weights"""
    w = gauss(n, seed)
    return w, gauss(n, seed + 1, 0.1), gauss(n, seed + 2, 0.05), gauss(n, seed + 3, 0.05) ** 2, w + gauss(n, seed + 4, 0.01)


def int_values(n: int, seed: int) -> torch.Tensor:
    """integers in [-64, 64]: with omd in {1/2, 1/4, 1/8} every intermediate of the average is exact in fp32"""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-64, 65, (n,), generator=g).float()


def schedule(decay: float, warmup: bool, t: int):
    """(d, omd) as numpy fp32, formed as the kernel forms them"""
    d = np.float32(decay)
    if warmup:
        tf = np.float32(t)
        d = np.minimum(d, (np.float32(1.0) + tf) / (np.float32(10.0) + tf))
    return np.float32(d), np.float32(np.float32(1.0) - d)


def warmup_reaches_decay_at(decay: float) -> int:
    """the first step t with (1 + t) / (10 + t) >= decay: t >= (10 decay - 1) / (1 - decay)"""
    d = Fraction(str(decay))          # the decimal the caller wrote, not its binary neighbour
    return max(math.ceil((10 * d - 1) / (1 - d)), 0)


def ema_ref32(w_new: torch.Tensor, e: torch.Tensor, omd) -> torch.Tensor:
    """The contract in numpy fp32: t = fp32(w' - e); fma as the float64 product omd * t (exact: 24 x 24 bits) plus e in float64,
    rounded once to fp32.  Equal to the fused operation wherever the float64 sum is itself exact, which the tests that use it
    arrange."""
    omd = np.float32(omd)
    wn, e0 = w_new.numpy().astype(np.float32), e.numpy().astype(np.float32)
    if omd == np.float32(1.0):
        return torch.from_numpy(wn.copy())
    t = (wn - e0).astype(np.float32)
    return torch.from_numpy((np.float64(omd) * t.astype(np.float64) + e0.astype(np.float64)).astype(np.float32))


def ema_ref64(w_new: torch.Tensor, e: torch.Tensor, omd) -> torch.Tensor:
    """The average in float64 from the kernel's own fp32 w' and previous e, with the fp32 omd"""
    omd = float(np.float32(omd))
    if omd == 1.0:
        return w_new.double().clone()
    return e.double() + omd * (w_new.double() - e.double())


def ulp32(x: torch.Tensor) -> torch.Tensor:
    """the spacing of fp32 numbers in the binade of |x| (float64 in, float64 out; 2^-149 at and below the subnormals)"""
    _, ex = np.frexp(np.abs(x.numpy().astype(np.float64)))
    return torch.from_numpy(np.ldexp(1.0, np.maximum(ex - 24, -149)))


def ema_bound(w_new: torch.Tensor, e: torch.Tensor, omd, e64: torch.Tensor) -> torch.Tensor:
    """|e' - e64| <= 0.5 ulp32(e64) + 2^-22 |omd (w' - e)|: half an ulp from the final rounding, 2^-24 |omd t| from rounding
    t = w' - e, up to 2^-23 |omd t| from the rounding of d and omd (the division of the warm-up schedule included)"""
    omd = float(np.float32(omd))
    return 0.5 * ulp32(e64) + 2.0 ** -22 * (omd * (w_new.double() - e.double())).abs()


def ema_loop64(weights, decay: float, warmup: bool, e0: torch.Tensor):
    """a plain float64 EMA over a list of weights, step t = 1, 2, ...: e <- d e + (1 - d) w, d and 1 - d the fp32 values"""
    e, out = e0.double().clone(), []
    for t, w in enumerate(weights, 1):
        d, omd = schedule(decay, warmup, t)
        e = e * (1.0 - float(omd)) + float(omd) * w.double()
        out.append(e.clone())
    return out
