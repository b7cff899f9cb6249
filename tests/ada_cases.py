"""Cases and restatements of adaptive discriminator augmentation (the gated kernels and the controller of csrc/diffaug.hip,
hr_viton_amd/diffaug.py AdaptiveAugment; both are defined in include/hrviton_hip.h).  Pure CPU torch / numpy / Python floats:
tests/test_ada_cases_cpu.py checks the restatements on hand-worked cases, tests/test_gpu_ada.py holds the kernels against them.

The gated reference is the restatement of tests/diffaug_cases.py called sample by sample under ``flags & mask(ug[n], p)``; the
comparison of the mask is (double)ug < p in fp64, as the kernel makes it.  The controller is restated in Python floats (IEEE fp64)
in the order the header spells out, so the device state is compared to the bit."""
import numpy as np
import torch

import diffaug_cases as D

# the state of hrv_ada_update_f64 and the words of the loss head's record it reads (include/hrviton_hip.h)
WORDS = 8
P, ACC, SEEN, UPDATES, RT_WINDOW, STEPS, RT_LAST = range(7)
DHEAD_WORDS, DHEAD_NONFINITE, DHEAD_STATE, DHEAD_SCALE_WORDS, DHEAD_RT = 72, 1, 8, 8, 3
GATE_P = 0.5                     # the probability of the forced gate table
ON, OFF = 0.25, 0.75             # a gate below / above GATE_P
EDGE_P = 0.25 + 2.0 ** -40       # above (float)0.25 in fp64, equal to it once rounded to fp32


# ------------------------------------------------------------------ the gates
def gate_mask(ugrow, p: float) -> int:
    """the transforms sample n keeps: bit b where (double)ug[b] < p, strict, in fp64"""
    ugrow = np.asarray(ugrow, dtype=np.float32)
    p = float(p)
    return ((D.COLOR if float(ugrow[0]) < p else 0) | (D.TRANSLATION if float(ugrow[1]) < p else 0)
            | (D.CUTOUT if float(ugrow[2]) < p else 0))


def forced_gate_rows():
    """[(mask, row of 4)]: all eight masks at GATE_P; the spare column holds a value that would switch everything on if it were read"""
    return [(m, np.asarray([ON if m & D.COLOR else OFF, ON if m & D.TRANSLATION else OFF, ON if m & D.CUTOUT else OFF, 0.0],
                           dtype=np.float32)) for m in range(8)]


def gate_batches(N: int):
    """the table as ([masks], [N, 4] tensor) batches (the last one wraps around)"""
    rows, out = forced_gate_rows(), []
    for i in range(0, len(rows), N):
        pick = [rows[(i + j) % len(rows)] for j in range(N)]
        out.append(([m for m, _ in pick], torch.from_numpy(np.stack([r for _, r in pick]))))
    return out


def paired_batches(H: int, W: int, N: int):
    """[(names, u [N,8], masks, ug [N,4])]: every batch of the forced table of uniforms under the gate batches in rotation"""
    gates = gate_batches(N)
    return [(names, u) + gates[i % len(gates)] for i, (names, u) in enumerate(D.batches(D.forced_rows(H, W), N))]


def random_gates(N: int, seed: int) -> torch.Tensor:
    return torch.rand(N, 4, generator=torch.Generator().manual_seed(4000 + seed))


def _per_sample(fn, N, ug, p, flags):
    return torch.cat([fn(n, flags & gate_mask(ug[n].numpy(), p)) for n in range(N)])


def forward_ref(parse, Ca, img, u, ug, p, flags, mean=None):
    """float64 [N,H,W,12]: D.forward_ref of sample n under flags & mask(ug[n], p)"""
    return _per_sample(lambda n, f: D.forward_ref(parse[n:n + 1], Ca, img[n:n + 1], u[n:n + 1], f,
                                                  mean=None if mean is None else mean[n:n + 1]), img.shape[0], ug, p, flags)


def forward_bound(Ca, img, u, ug, p, flags, mean):
    return _per_sample(lambda n, f: D.forward_bound(Ca, img[n:n + 1], u[n:n + 1], f, mean[n:n + 1]), img.shape[0], ug, p, flags)


def backward_ref(g, Ca, u, ug, p, flags):
    return _per_sample(lambda n, f: D.backward_ref(g[n:n + 1], Ca, u[n:n + 1], f), g.shape[0], ug, p, flags)


def backward_bound(g, Ca, u, ug, p, flags):
    return _per_sample(lambda n, f: D.backward_bound(g[n:n + 1], Ca, u[n:n + 1], f), g.shape[0], ug, p, flags)


def gsum_ref(g, Ca, u, ug, p, flags):
    return _per_sample(lambda n, f: D.gsum_ref(g[n:n + 1], Ca, u[n:n + 1], f), g.shape[0], ug, p, flags)


# ------------------------------------------------------------------ the controller
def make_record(rts, nonfinite: float = 0.0) -> torch.Tensor:
    """a loss-head record holding only what the controller reads (everything else a value that would show if it were read)"""
    rec = torch.full((DHEAD_WORDS,), 7.0, dtype=torch.float64)
    rec[DHEAD_NONFINITE] = nonfinite
    for k, r in enumerate(rts):
        rec[DHEAD_STATE + DHEAD_SCALE_WORDS * k + DHEAD_RT] = r
    return rec


def controller_step(state, record, num_d: int, target: float, step: float, interval: int, p_max: float):
    """one hrv_ada_update_f64 call on ``state`` (a list of WORDS Python floats), in the header's order; returns the new list"""
    st = [float(v) for v in state]
    rec = [float(v) for v in record]
    st[STEPS] += 1.0
    if rec[DHEAD_NONFINITE] != 0.0:
        return st
    total = 0.0
    for k in range(num_d):
        total += rec[DHEAD_STATE + DHEAD_SCALE_WORDS * k + DHEAD_RT]
    r = total / float(num_d)
    st[RT_LAST] = r
    st[ACC] += r
    st[SEEN] += 1.0
    if st[SEEN] == float(interval):
        m = st[ACC] / float(interval)
        st[RT_WINDOW] = m
        s = float((m > target) - (m < target))
        st[P] = min(max(st[P] + s * step, 0.0), p_max)
        st[ACC] = 0.0
        st[SEEN] = 0.0
        st[UPDATES] += 1.0
    return st


def initial_state(p: float = 0.0):
    st = [0.0] * WORDS
    st[P] = float(p)
    return st


# Two scales, interval 2, step 1/4, p_max 1/2, target 1/4, from p = 0; every value a dyadic fraction, so the expected P, SEEN and
# UPDATES after each launch (the last three columns) are worked out by hand:
#   ((r_t of scale 0, r_t of scale 1), NONFINITE)                      P     SEEN UPDATES
HAND = dict(num_d=2, target=0.25, step=0.25, interval=2, p_max=0.5, p_init=0.0)
HAND_SEQ = [
    ((0.5, 0.5), 0.0, 0.0, 1, 0),          # r = 1/2: the window opens
    ((0.75, 0.25), 0.0, 0.25, 0, 1),       # r = 1/2, m = 1/2 > target: p up
    ((1.0, 1.0), 0.0, 0.25, 1, 1),         # r = 1
    ((9.0, 9.0), 3.0, 0.25, 1, 1),         # poisoned in the middle of the window: neither accumulated nor counted
    ((0.5, 0.5), 0.0, 0.5, 0, 2),          # m = (1 + 1/2) / 2 = 3/4 > target: p up, reaching p_max exactly
    ((1.0, 1.0), 0.0, 0.5, 1, 2),
    ((1.0, 1.0), 0.0, 0.5, 0, 3),          # m = 1 > target: 3/4 clamped to p_max
    ((0.25, 0.25), 0.0, 0.5, 1, 3),
    ((0.5, 0.0), 0.0, 0.5, 0, 4),          # m = 1/4 == target: nothing moves, the adjustment is counted
    ((-0.5, 0.0), 0.0, 0.5, 1, 4),
    ((-1.0, 0.5), 0.0, 0.25, 0, 5),        # m = -1/4 < target: p down
    ((0.0, 0.0), 0.0, 0.25, 1, 5),
    ((0.0, 0.0), 0.0, 0.0, 0, 6),          # p down to 0 exactly
    ((-1.0, -1.0), 0.0, 0.0, 1, 6),
    ((-1.0, -1.0), 0.0, 0.0, 0, 7),        # -1/4 clamped to 0
    ((0.1, 0.3), 0.0, 0.0, 1, 7),          # a window left open
]

# One scale, interval 3; step, target and r_t are no dyadic fractions (the order of the operations shows); one poisoned step in the
# middle of the third window; windows above the target into p_max, one whose mean is 0.6 up to rounding, windows below it into 0
ROUNDED = dict(num_d=1, target=0.6, step=0.1, interval=3, p_max=0.2, p_init=0.05)
ROUNDED_RT = [0.9, 0.7, 0.95, 0.61, 0.59, 0.6, 0.8, None, 0.9, 0.7, 0.99, 0.65, 0.77, -0.3, 0.2, 0.1, -0.9, -0.8, -0.7, -1.0, -1.0, -1.0]


def rounded_seq():
    return [((0.123,), 2.0) if r is None else ((r,), 0.0) for r in ROUNDED_RT]


def run_sequence(cfg, seq):
    """[state after launch i] of the restatement"""
    st, out = initial_state(cfg["p_init"]), []
    for item in seq:
        st = controller_step(st, make_record(item[0], item[1]).tolist(), cfg["num_d"], cfg["target"], cfg["step"], cfg["interval"],
                             cfg["p_max"])
        out.append(list(st))
    return out
