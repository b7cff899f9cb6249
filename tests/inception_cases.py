"""Shared by tests/test_inception_cpu.py and tests/test_gpu_inception.py: torchvision's Inception-v3 (eval mode, no AuxLogits branch,
transform_input=False) stated a second time, independently of hr_viton_amd/inception.py.

  * ``UNITS``: the conv units as data, (name, in, out, (kh, kw), stride, (pad_h, pad_w)), AuxLogits' two included (parameter count);
  * ``forward(sd, x, dtype)``: the network in ``torch.nn.functional`` on the CPU, float64 for the reference and float32 for the
    yardstick of the GPU parity tests; it can record every unit's output and every block's input;
  * ``make_weights(seed)``: seeded, CALIBRATED random weights.  With plain He-scaled convolutions and random BatchNorm statistics
    every image lands on nearly the same class, probabilities underflow in fp32 and the score is nan: such a network tests nothing.
    So the maker runs ``forward`` once in float64 over a fixed calibration batch and sets each unit's ``running_mean`` / ``running_var``
    to the per-channel statistics of that unit's convolution output (what the BatchNorm normalises), in forward order; ``fc.weight`` is
    ``randn * FC_GAIN / sqrt(2048)``.  The GPU test asserts on the float64 result alone that the test images then give IS >= 1.5 and
    probabilities > 0 everywhere;
  * ``images(n, seed)``: smooth random fields of differing coarseness plus noise, uint8 [n, 299, 299, 3];
  * ``score64``: the Inception Score of evaluate.py:97-106 in float64 numpy.
"""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

BN_EPS = 0.001
FC_GAIN = 8.0
N_CALIB, N_TEST = 8, 12


def _u(name, cin, cout, k, s=1, p=0):
    k = (k, k) if isinstance(k, int) else k
    p = (p, p) if isinstance(p, int) else p
    return (name, cin, cout, k, s, p)


def _inception_a(n, cin, pf):
    return [_u(f"{n}.branch1x1", cin, 64, 1), _u(f"{n}.branch5x5_1", cin, 48, 1), _u(f"{n}.branch5x5_2", 48, 64, 5, 1, 2),
            _u(f"{n}.branch3x3dbl_1", cin, 64, 1), _u(f"{n}.branch3x3dbl_2", 64, 96, 3, 1, 1), _u(f"{n}.branch3x3dbl_3", 96, 96, 3, 1, 1),
            _u(f"{n}.branch_pool", cin, pf, 1)]


def _inception_b(n, cin):
    return [_u(f"{n}.branch3x3", cin, 384, 3, 2), _u(f"{n}.branch3x3dbl_1", cin, 64, 1), _u(f"{n}.branch3x3dbl_2", 64, 96, 3, 1, 1),
            _u(f"{n}.branch3x3dbl_3", 96, 96, 3, 2)]


def _inception_c(n, cin, c7):
    return [_u(f"{n}.branch1x1", cin, 192, 1),
            _u(f"{n}.branch7x7_1", cin, c7, 1), _u(f"{n}.branch7x7_2", c7, c7, (1, 7), 1, (0, 3)),
            _u(f"{n}.branch7x7_3", c7, 192, (7, 1), 1, (3, 0)),
            _u(f"{n}.branch7x7dbl_1", cin, c7, 1), _u(f"{n}.branch7x7dbl_2", c7, c7, (7, 1), 1, (3, 0)),
            _u(f"{n}.branch7x7dbl_3", c7, c7, (1, 7), 1, (0, 3)), _u(f"{n}.branch7x7dbl_4", c7, c7, (7, 1), 1, (3, 0)),
            _u(f"{n}.branch7x7dbl_5", c7, 192, (1, 7), 1, (0, 3)), _u(f"{n}.branch_pool", cin, 192, 1)]


def _inception_d(n, cin):
    return [_u(f"{n}.branch3x3_1", cin, 192, 1), _u(f"{n}.branch3x3_2", 192, 320, 3, 2),
            _u(f"{n}.branch7x7x3_1", cin, 192, 1), _u(f"{n}.branch7x7x3_2", 192, 192, (1, 7), 1, (0, 3)),
            _u(f"{n}.branch7x7x3_3", 192, 192, (7, 1), 1, (3, 0)), _u(f"{n}.branch7x7x3_4", 192, 192, 3, 2)]


def _inception_e(n, cin):
    return [_u(f"{n}.branch1x1", cin, 320, 1), _u(f"{n}.branch3x3_1", cin, 384, 1),
            _u(f"{n}.branch3x3_2a", 384, 384, (1, 3), 1, (0, 1)), _u(f"{n}.branch3x3_2b", 384, 384, (3, 1), 1, (1, 0)),
            _u(f"{n}.branch3x3dbl_1", cin, 448, 1), _u(f"{n}.branch3x3dbl_2", 448, 384, 3, 1, 1),
            _u(f"{n}.branch3x3dbl_3a", 384, 384, (1, 3), 1, (0, 1)), _u(f"{n}.branch3x3dbl_3b", 384, 384, (3, 1), 1, (1, 0)),
            _u(f"{n}.branch_pool", cin, 192, 1)]


UNITS = ([_u("Conv2d_1a_3x3", 3, 32, 3, 2), _u("Conv2d_2a_3x3", 32, 32, 3), _u("Conv2d_2b_3x3", 32, 64, 3, 1, 1),
          _u("Conv2d_3b_1x1", 64, 80, 1), _u("Conv2d_4a_3x3", 80, 192, 3)] +
         _inception_a("Mixed_5b", 192, 32) + _inception_a("Mixed_5c", 256, 64) + _inception_a("Mixed_5d", 288, 64) +
         _inception_b("Mixed_6a", 288) +
         _inception_c("Mixed_6b", 768, 128) + _inception_c("Mixed_6c", 768, 160) + _inception_c("Mixed_6d", 768, 160) +
         _inception_c("Mixed_6e", 768, 192) +
         _inception_d("Mixed_7a", 768) + _inception_e("Mixed_7b", 1280) + _inception_e("Mixed_7c", 2048))
AUX_UNITS = [_u("AuxLogits.conv0", 768, 128, 1), _u("AuxLogits.conv1", 128, 768, 5)]
UNIT = {u[0]: u for u in UNITS}
BN_KEYS = ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")
BLOCKS = ["Mixed_5b", "Mixed_5c", "Mixed_5d", "Mixed_6a", "Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e", "Mixed_7a", "Mixed_7b",
          "Mixed_7c"]
# (block, expected channels, expected extent at 299x299) of the restatement's taps the CPU test pins
TAPS_299 = {"stem": (192, 35), "Mixed_5d": (288, 35), "Mixed_6e": (768, 17), "Mixed_7c": (2048, 8)}


def state_keys(aux=False):
    keys = set()
    for name, *_ in UNITS + (AUX_UNITS if aux else []):
        keys.add(f"{name}.conv.weight")
        keys |= {f"{name}.bn.{k}" for k in BN_KEYS}
    keys |= {"fc.weight", "fc.bias"}
    if aux:
        keys |= {"AuxLogits.fc.weight", "AuxLogits.fc.bias"}
    return keys


def param_count(aux=False):
    """learnable parameters: conv weights, BatchNorm weight and bias, the classifier(s)"""
    n = 2048 * 1000 + 1000
    for _, cin, cout, (kh, kw), _, _ in UNITS + (AUX_UNITS if aux else []):
        n += cout * cin * kh * kw + 2 * cout
    if aux:
        n += 768 * 1000 + 1000
    return n


# ----------------------------------------------------------------------------------------------------------------- the forward
class _Run:
    """One pass: applies units by name; optionally records unit outputs / block inputs, optionally calibrates BatchNorm statistics."""

    def __init__(self, sd, dtype, calibrate=False, record=None):
        self.sd, self.dtype, self.calibrate, self.record = sd, dtype, calibrate, record

    def unit(self, name, x):
        _, _, _, _, s, p = UNIT[name]
        sd, d = self.sd, self.dtype
        y = F.conv2d(x, sd[f"{name}.conv.weight"].to(d), None, stride=s, padding=p)
        if self.calibrate:
            sd[f"{name}.bn.running_mean"] = y.mean(dim=(0, 2, 3)).to(torch.float32)
            sd[f"{name}.bn.running_var"] = y.var(dim=(0, 2, 3), unbiased=False).to(torch.float32)
        y = F.batch_norm(y, sd[f"{name}.bn.running_mean"].to(d), sd[f"{name}.bn.running_var"].to(d), sd[f"{name}.bn.weight"].to(d),
                         sd[f"{name}.bn.bias"].to(d), False, 0.0, BN_EPS)
        y = F.relu(y)
        if self.record is not None:
            self.record[name] = y
        return y


def block_a(r, n, x):
    b1 = r.unit(f"{n}.branch1x1", x)
    b5 = r.unit(f"{n}.branch5x5_2", r.unit(f"{n}.branch5x5_1", x))
    b3 = r.unit(f"{n}.branch3x3dbl_3", r.unit(f"{n}.branch3x3dbl_2", r.unit(f"{n}.branch3x3dbl_1", x)))
    bp = r.unit(f"{n}.branch_pool", F.avg_pool2d(x, kernel_size=3, stride=1, padding=1))
    return [b1, b5, b3, bp]


def block_b(r, n, x):
    b3 = r.unit(f"{n}.branch3x3", x)
    bd = r.unit(f"{n}.branch3x3dbl_3", r.unit(f"{n}.branch3x3dbl_2", r.unit(f"{n}.branch3x3dbl_1", x)))
    return [b3, bd, F.max_pool2d(x, kernel_size=3, stride=2)]


def block_c(r, n, x):
    b1 = r.unit(f"{n}.branch1x1", x)
    b7 = r.unit(f"{n}.branch7x7_3", r.unit(f"{n}.branch7x7_2", r.unit(f"{n}.branch7x7_1", x)))
    bd = x
    for k in range(1, 6):
        bd = r.unit(f"{n}.branch7x7dbl_{k}", bd)
    bp = r.unit(f"{n}.branch_pool", F.avg_pool2d(x, kernel_size=3, stride=1, padding=1))
    return [b1, b7, bd, bp]


def block_d(r, n, x):
    b3 = r.unit(f"{n}.branch3x3_2", r.unit(f"{n}.branch3x3_1", x))
    b7 = x
    for k in range(1, 5):
        b7 = r.unit(f"{n}.branch7x7x3_{k}", b7)
    return [b3, b7, F.max_pool2d(x, kernel_size=3, stride=2)]


def block_e(r, n, x):
    b1 = r.unit(f"{n}.branch1x1", x)
    b3 = r.unit(f"{n}.branch3x3_1", x)
    b3 = torch.cat([r.unit(f"{n}.branch3x3_2a", b3), r.unit(f"{n}.branch3x3_2b", b3)], 1)
    bd = r.unit(f"{n}.branch3x3dbl_2", r.unit(f"{n}.branch3x3dbl_1", x))
    bd = torch.cat([r.unit(f"{n}.branch3x3dbl_3a", bd), r.unit(f"{n}.branch3x3dbl_3b", bd)], 1)
    bp = r.unit(f"{n}.branch_pool", F.avg_pool2d(x, kernel_size=3, stride=1, padding=1))
    return [b1, b3, bd, bp]


BLOCK_FN = {"Mixed_5b": block_a, "Mixed_5c": block_a, "Mixed_5d": block_a, "Mixed_6a": block_b, "Mixed_6b": block_c,
            "Mixed_6c": block_c, "Mixed_6d": block_c, "Mixed_6e": block_c, "Mixed_7a": block_d, "Mixed_7b": block_e,
            "Mixed_7c": block_e}


def forward(sd, x, dtype=torch.float64, calibrate=False, taps=None, block_io=None):
    """x: [N,3,H,W] already normalised -> logits [N,1000] in ``dtype``.  ``taps``: dict receiving "stem" and every block's output;
    ``block_io``: dict receiving per block (input, [branch outputs in cat order])."""
    r = _Run(sd, dtype, calibrate)
    x = x.to(dtype)
    x = r.unit("Conv2d_2b_3x3", r.unit("Conv2d_2a_3x3", r.unit("Conv2d_1a_3x3", x)))
    x = F.max_pool2d(x, kernel_size=3, stride=2)
    x = r.unit("Conv2d_4a_3x3", r.unit("Conv2d_3b_1x1", x))
    x = F.max_pool2d(x, kernel_size=3, stride=2)
    if taps is not None:
        taps["stem"] = x
    for n in BLOCKS:
        branches = BLOCK_FN[n](r, n, x)
        if block_io is not None:
            block_io[n] = (x, branches)
        x = torch.cat(branches, 1)
        if taps is not None:
            taps[n] = x
    x = x.mean(dim=(2, 3))          # adaptive_avg_pool2d((1, 1)) + flatten; dropout is the identity in eval mode
    return F.linear(x, sd["fc.weight"].to(dtype), sd["fc.bias"].to(dtype))


def normalize_u8(img_u8):
    """evaluate.py's T3 minus the resize: ToTensor + Normalize(0.5, 0.5) in fp32, as torchvision computes them -> [N,3,H,W] fp32"""
    return torch.from_numpy(np.ascontiguousarray(img_u8)).permute(0, 3, 1, 2).float().div(255).sub(0.5).div(0.5)


def log_probs(logits):
    return F.log_softmax(logits, dim=1)


# ----------------------------------------------------------------------------------------------------------------- inputs, weights
def images(n, seed):
    """n images uint8 [n, 299, 299, 3]: a bilinear blow-up of a coarse random grid (2 .. 48 cells across, differing per image) plus
    pixel noise of differing strength"""
    from PIL import Image
    rng = np.random.default_rng(seed)
    out = np.empty((n, 299, 299, 3), np.uint8)
    cells = [2, 3, 5, 8, 12, 20, 32, 48]
    for i in range(n):
        c = cells[(i * 3 + seed) % len(cells)]
        coarse = (rng.random((c, c + i % 3, 3)) * 255).astype(np.uint8)
        base = np.asarray(Image.fromarray(coarse).resize((299, 299), Image.BILINEAR), np.float64)
        out[i] = np.clip(base + rng.normal(0, 2.0 + 6.0 * (i % 4), base.shape), 0, 255).astype(np.uint8)
    return out


def raw_weights(seed):
    """He-scaled convolutions, BatchNorm weight in [0.75, 1.25], bias in [-0.25, 0.25], identity statistics, the scaled classifier"""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, cin, cout, (kh, kw), _, _ in UNITS:
        sd[f"{name}.conv.weight"] = torch.randn(cout, cin, kh, kw, generator=g) * math.sqrt(2.0 / (cin * kh * kw))
        sd[f"{name}.bn.weight"] = 0.75 + 0.5 * torch.rand(cout, generator=g)
        sd[f"{name}.bn.bias"] = 0.5 * torch.rand(cout, generator=g) - 0.25
        sd[f"{name}.bn.running_mean"] = torch.zeros(cout)
        sd[f"{name}.bn.running_var"] = torch.ones(cout)
        sd[f"{name}.bn.num_batches_tracked"] = torch.tensor(0, dtype=torch.long)
    sd["fc.weight"] = torch.randn(1000, 2048, generator=g) * (FC_GAIN / math.sqrt(2048))
    sd["fc.bias"] = 0.1 * torch.randn(1000, generator=g)
    return sd


@functools.lru_cache(maxsize=2)
def make_weights(seed=0):
    sd = raw_weights(seed)
    with torch.no_grad():
        forward(sd, normalize_u8(images(N_CALIB, 1000 + seed)), torch.float64, calibrate=True)
    return sd


@functools.lru_cache(maxsize=1)
def reference_run(seed=0):
    """The calibrated weights, the test images and both CPU passes over them: float64 (the reference, with taps and block
    inputs / branch outputs) and float32 (the yardstick).  Computed once per process."""
    sd = make_weights(seed)
    img = images(N_TEST, 2000 + seed)
    x = normalize_u8(img)
    taps, io = {}, {}
    with torch.no_grad():
        l64 = forward(sd, x, torch.float64, taps=taps, block_io=io)
        l32 = forward(sd, x, torch.float32)
    return {"sd": sd, "img": img, "x": x, "logits64": l64, "logits32": l32, "taps": taps, "io": io}


# ----------------------------------------------------------------------------------------------------------------- the score
def score64(preds, splits=1):
    """evaluate.py:97-106: per split exp(mean_i KL(p_i || mean_j p_j)), both arguments normalised as scipy.stats.entropy does;
    returns (mean, std) over the splits"""
    preds = np.asarray(preds, np.float64)
    n = preds.shape[0] // splits
    out = []
    for k in range(splits):
        part = preds[k * n:(k + 1) * n]
        q = part.mean(axis=0)
        q = q / q.sum()
        kls = []
        for row in part:
            p = row / row.sum()
            with np.errstate(divide="ignore", invalid="ignore"):
                t = np.where(p > 0, p * np.log(p / q), 0.0)
            kls.append(t.sum())
        out.append(np.exp(np.mean(kls)))
    return float(np.mean(out)), float(np.std(out))
