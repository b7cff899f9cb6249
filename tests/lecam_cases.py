"""Cases, float64 restatement and error bounds of the discriminator step's fused loss head (hr_viton_amd.lecam, csrc/dhead.hip).
No GPU and no library is needed to import this file: the CPU test checks the restatement against torch autograd, the GPU tests
check the kernels against the restatement.

Definitions restated (per scale k, n logits per half, x_r / x_f the real / fake logits):
  sums      sum x_r, sum x_f, sum sign(x_r) (sign(0) = 0), sum max(1 - x_r, 0), sum max(1 + x_f, 0), count of non-finite logits
  means     m_r = sum x_r / n, m_f = sum x_f / n, r = sum sign(x_r) / n
  anchors   a_R <- d a_R + (1 - d) m_r, a_F <- d a_F + (1 - d) m_f, rt_avg <- d rt_avg + (1 - d) r; d = decay, 0 while count == 0;
            updated BEFORE they are used; constants of the gradient
  R         paper: mean((x_r - a_F)^2) + mean((x_f - a_R)^2); relu: mean(relu(x_r - a_F)^2) + mean(relu(a_R - x_f)^2)
  lambda    weight when the count of applied updates, as it stood BEFORE this step, is >= start, else 0
  outputs   D_Fake = sum_k mean max(1 + x_f, 0) / num_D, D_Real likewise, D_LeCam = lambda * sum_k R_k / num_D
  poisoned  any non-finite logit in any scale: anchors, rt_avg and count stay; D_LeCam is NaN; the hinge terms are what the sums give
"""
import torch

BLOCK = 256          # threads of a reduce block
SLOTS = 64           # HRV_DHEAD_SLOTS: blocks per half = slots of the partial pass
SWEEP = 4 * BLOCK * SLOTS      # logits one sweep of a half's row of the grid covers (16-byte loads)

# element counts per half the table must cover: tiny, around one block, odd (the real half then starts 4-byte aligned only), and
# one short of / exactly / 5 past one full sweep
REQUIRED_N = (1, 3, 4, 5, 255, 256, 257, 1023, SWEEP - 1, SWEEP, SWEEP + 5)

# name -> the logit shape N x 1 x h x w of every scale (num_D = 1, 2, 3; a different n per scale)
CASES = {
    "one":        [(1, 1, 1, 1)],
    "n3_n4":      [(1, 1, 1, 3), (1, 1, 2, 2)],
    "n5_255_256": [(1, 1, 1, 5), (3, 1, 5, 17), (2, 1, 8, 16)],
    "n257_1023":  [(1, 1, 1, 257), (3, 1, 11, 31)],
    "sweep_m1":   [(3, 1, 85, 257)],
    "sweep_p5":   [(2, 1, 128, 256), (3, 1, 7, 3121)],
    "three":      [(3, 1, 7, 3121), (1, 1, 255, 257), (3, 1, 11, 31)],
}


def numel(shape):
    n = 1
    for s in shape:
        n *= s
    return n


def covered_n():
    return sorted({numel(s) for shapes in CASES.values() for s in shapes})


# the integer-exact family: power-of-two n, weight, decay and num_D; integer logits in [-8, 8].  Every anchor, loss term and
# gradient of the float64 restatement is then exactly representable in fp32 over 6 chained steps (checked by the CPU test).
EXACT = dict(n=(1, 64, 256, 4096), decay=0.5, weight=0.25, num_D=2, start=2, steps=6, lo=-8, hi=8)


def exact_logits(n_per_scale, steps, seed):
    """[step][scale] -> (x_fake, x_real) float64 integer-valued tensors"""
    g = torch.Generator().manual_seed(seed)
    return [[(torch.randint(EXACT["lo"], EXACT["hi"] + 1, (n,), generator=g).double(),
              torch.randint(EXACT["lo"], EXACT["hi"] + 1, (n,), generator=g).double()) for n in n_per_scale]
            for _ in range(steps)]


def gaussian_logits(shapes, seed, mean_fake=-0.4, mean_real=0.6, std=1.5):
    """[scale] -> (x_fake, x_real) fp32 tensors of the case's shapes: logits on both sides of the hinge's kinks"""
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(s, generator=g) * std + mean_fake, torch.randn(s, generator=g) * std + mean_real) for s in shapes]


class Restated:
    """The loss head in float64 torch on the CPU, written from the definitions."""

    def __init__(self, weight, decay=0.99, start=0, form="paper"):
        assert form in ("paper", "relu")
        self.weight, self.decay, self.start, self.form = float(weight), float(decay), int(start), form
        self.count = 0
        self.anchor_real, self.anchor_fake, self.rt_avg = [], [], []

    def sums(self, x_fake, x_real):
        xf, xr = x_fake.double().reshape(-1), x_real.double().reshape(-1)
        return {"sum_real": xr.sum().item(), "sum_fake": xf.sum().item(), "sign_real": torch.sign(xr).sum().item(),
                "hinge_real": (1 - xr).clamp_min(0).sum().item(), "hinge_fake": (1 + xf).clamp_min(0).sum().item(),
                "sumsq_real": (xr * xr).sum().item(), "sumsq_fake": (xf * xf).sum().item(),
                "nonfinite": int((~torch.isfinite(xr)).sum() + (~torch.isfinite(xf)).sum())}

    def step(self, pairs, g=(1.0, 1.0, 1.0), n_mult=1):
        """``pairs``: [(x_fake, x_real)] per scale.  Returns a dictionary: 'losses' (D_Fake, D_Real, D_LeCam as Python floats),
        'mag' (the same expressions with every term's absolute value: what the error bounds scale with), 'grads' [(d_fake, d_real)]
        float64 for the upstream gradients ``g``, 'hinge' / 'reg' their two parts, 'lambda', 'sums', 'r_t', 'means'."""
        K = len(pairs)
        if not self.anchor_real:
            self.anchor_real, self.anchor_fake, self.rt_avg = [0.0] * K, [0.0] * K, [0.0] * K
        sums = [self.sums(f, r) for f, r in pairs]
        poisoned = any(s["nonfinite"] for s in sums)
        lam = self.weight if self.count >= self.start else 0.0
        d = 0.0 if self.count == 0 else self.decay
        d_fake_l = d_real_l = reg_l = 0.0
        mag_f = mag_r = mag_reg = 0.0
        grads, hinge, regp, rts, means = [], [], [], [], []
        for k, (f, r) in enumerate(pairs):
            xf, xr = f.double(), r.double()
            n = xf.numel()
            nt = n * n_mult
            m_r, m_f, rt = sums[k]["sum_real"] / nt, sums[k]["sum_fake"] / nt, sums[k]["sign_real"] / nt
            if not poisoned:
                self.anchor_real[k] = d * self.anchor_real[k] + (1 - d) * m_r
                self.anchor_fake[k] = d * self.anchor_fake[k] + (1 - d) * m_f
                self.rt_avg[k] = d * self.rt_avg[k] + (1 - d) * rt
            a_r, a_f = self.anchor_real[k], self.anchor_fake[k]
            rts.append(rt)
            means.append((m_r, m_f))
            d_fake_l += sums[k]["hinge_fake"] / nt
            d_real_l += sums[k]["hinge_real"] / nt
            mag_f += sums[k]["hinge_fake"] / nt
            mag_r += sums[k]["hinge_real"] / nt
            if self.form == "paper":
                reg_l += ((xr - a_f) ** 2).mean().item() + ((xf - a_r) ** 2).mean().item()
                tr, tf = xr - a_f, xf - a_r
                # the kernel's closed form: (sum x^2 - 2 a sum x + n a^2) / n, every term taken positive
                mag_reg += ((xr * xr).mean() + 2 * abs(a_f) * xr.abs().mean() + a_f * a_f).item() + \
                           ((xf * xf).mean() + 2 * abs(a_r) * xf.abs().mean() + a_r * a_r).item()
            else:
                reg_l += ((xr - a_f).clamp_min(0) ** 2).mean().item() + ((a_r - xf).clamp_min(0) ** 2).mean().item()
                tr, tf = (xr - a_f).clamp_min(0), -(a_r - xf).clamp_min(0)
                mag_reg += ((xr - a_f).clamp_min(0) ** 2).mean().item() + ((a_r - xf).clamp_min(0) ** 2).mean().item()
            h_f = torch.where(xf > -1, 1.0, 0.0).double() * (1.0 / n) * (g[0] / K)
            h_r = torch.where(xr < 1, -1.0, 0.0).double() * (1.0 / n) * (g[1] / K)
            c = (g[2] / K) * lam * 2.0 / n
            r_f = c * tf if lam != 0.0 else torch.zeros_like(xf)
            r_r = c * tr if lam != 0.0 else torch.zeros_like(xr)
            hinge.append((h_f, h_r))
            regp.append((r_f, r_r))
            grads.append((h_f + r_f, h_r + r_r))
        if not poisoned:
            self.count += 1
        lecam = float("nan") if poisoned else (lam * reg_l / K if lam != 0.0 else 0.0)
        return {"losses": (d_fake_l / K, d_real_l / K, lecam), "mag": (mag_f / K, mag_r / K, lam * mag_reg / K), "grads": grads,
                "hinge": hinge, "reg": regp, "lambda": lam, "sums": sums, "r_t": rts, "means": means, "poisoned": poisoned}


def torch_loss(pairs, anchors, lam, form):
    """The same three losses written with differentiable torch ops on float64 leaves; ``anchors``: [(a_R, a_F)] as constants."""
    K = len(pairs)
    d_fake = d_real = reg = 0.0
    for (xf, xr), (a_r, a_f) in zip(pairs, anchors):
        d_fake = d_fake + torch.relu(1 + xf).mean()
        d_real = d_real + torch.relu(1 - xr).mean()
        if form == "paper":
            reg = reg + ((xr - a_f) ** 2).mean() + ((xf - a_r) ** 2).mean()
        else:
            reg = reg + (torch.relu(xr - a_f) ** 2).mean() + (torch.relu(a_r - xf) ** 2).mean()
    return d_fake / K, d_real / K, lam * reg / K


# ---------------------------------------------------------------------------------------------------------------- error bounds
EPS32 = 2.0 ** -24      # unit round-off of fp32 (round to nearest)
EPS64 = 2.0 ** -53


def loss_bound(value, mag, n_max):
    """|kernel - restatement| for one of the three losses.  The kernel forms every sum in fp64 (at most n + 16 additions deep per
    output counting the trips, the shuffle trees and the slot tree: relative (n + 16) eps64 of the sum of magnitudes ``mag``, and the
    same again for the restatement's own sum and for the anchors that enter R), then rounds the fp64 value ONCE to fp32."""
    return EPS32 * abs(value) + 4.0 * (n_max + 16) * EPS64 * mag + 1e-300


def grad_bound(hinge, reg, x, anchor, c, n):
    """Elementwise |kernel - restatement| of one half's gradient.  Hinge part h in fp32: (float)(1 / n) is rounded once, g / num_D once,
    their product once -> 3 eps32 |h|.  Regulariser part r in fp64 from an fp32-rounded g / num_D -> eps32 |r|, plus the fp64 noise of
    the anchor (n + 16 additions) and of the four fp64 operations: 4 (n + 16) eps64 |c| (|x| + |anchor|).  The sum is rounded once:
    eps32 |h + r|."""
    return EPS32 * (3.0 * hinge.abs() + reg.abs() + (hinge + reg).abs()) * (1.0 + 2.0 ** -20) + \
        4.0 * (n + 16) * EPS64 * abs(c) * (x.abs() + abs(anchor))


def ulp_distance(a: torch.Tensor, b: torch.Tensor) -> int:
    """max distance in units in the last place between two finite fp32 tensors of one sign pattern"""
    a, b = a.detach().cpu().contiguous().reshape(-1), b.detach().cpu().contiguous().reshape(-1)
    ia, ib = a.view(torch.int32).long(), b.view(torch.int32).long()
    ia = torch.where(ia < 0, -(ia & 0x7FFFFFFF), ia)
    ib = torch.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return int((ia - ib).abs().max()) if a.numel() else 0
