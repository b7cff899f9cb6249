"""Cases and the host restatement for the image-grid tests (test_viz_cpu.py, test_gpu_viz.py).

The restatement is the reference's chain, literally, in fp32 torch on the CPU: ``t / 2 + 0.5`` and ``(t + 1) / 2``,
``utils.visualize_segmap`` (np.argmax -> PIL 'P' image -> putpalette -> convert('RGB') -> ToTensor's / 255), ``.expand(3, -1, -1)``
for masks, torchvision's ``make_grid`` restated (it is not installed here), ``mul(255).add_(0.5).clamp_(0, 255).to(uint8)`` of
torchvision ``save_image`` (ROUND), tensorboard's ``(g * 255).clip(0, 255).astype(uint8)`` (TRUNC) and ``utils.save_images``'
expression.  Nothing here touches the package under test.
"""
import math

import numpy as np
import torch
from PIL import Image

ROUND, TRUNC = 0, 1

# utils.py:50-55
PALETTE = [
    0, 0, 0, 128, 0, 0, 254, 0, 0, 0, 85, 0, 169, 0, 51,
    254, 85, 0, 0, 0, 85, 0, 119, 220, 85, 85, 0, 0, 85, 85,
    85, 51, 0, 52, 86, 128, 0, 128, 0, 0, 0, 254, 51, 169, 220,
    0, 254, 254, 85, 254, 169, 169, 254, 85, 254, 254, 0, 254, 169, 0
]

SIZES = [(5, 7), (16, 12), (33, 25), (64, 48)]                 # H x W: odd widths put every row start at another byte alignment
BATCHES = [1, 3]
COUNTS = [(1, 4), (2, 4), (4, 4), (5, 4), (10, 4), (12, 4), (5, 3)]      # (panels, nrow)
PADDINGS = [2, 0]


# ------------------------------------------------------------------------------------------ the reference's expressions
def signed_a(t):
    return t / 2 + 0.5


def signed_b(t):
    return (t + 1) / 2


def signed_c(t):
    """the float part of utils.save_images: (t + 1) * 0.5"""
    return (t + 1) * 0.5


def ref_visualize_segmap(input, batch=0):
    """utils.py:44-68 with multi_channel=True, tensor_out=True; ``input`` [N,C,H,W] on the CPU -> float [3,H,W]."""
    image_numpy = input.detach()[batch].cpu().float().numpy()
    idx = np.argmax(image_numpy, axis=0).astype(np.uint8)
    im = Image.fromarray(idx, "P")
    im.putpalette(PALETTE)
    rgb = np.asarray(im.convert("RGB"))
    # torchvision ToTensor on a uint8 HWC image: permute to CHW, float, div(255)
    return torch.from_numpy(np.array(rgb)).permute(2, 0, 1).contiguous().to(torch.float32).div(255)


def ref_make_grid(tensors, nrow=8, padding=2, pad_value=0.0):
    """torchvision.utils.make_grid over a list of [3,H,W] tensors (normalize=False), restated."""
    tensor = torch.stack(list(tensors), dim=0)
    if tensor.size(0) == 1:
        return tensor.squeeze(0)
    nmaps = tensor.size(0)
    xmaps = min(nrow, nmaps)
    ymaps = int(math.ceil(float(nmaps) / xmaps))
    height, width = int(tensor.size(2) + padding), int(tensor.size(3) + padding)
    grid = tensor.new_full((3, height * ymaps + padding, width * xmaps + padding), pad_value)
    k = 0
    for y in range(ymaps):
        for x in range(xmaps):
            if k >= nmaps:
                break
            grid.narrow(1, y * height + padding, height - padding).narrow(2, x * width + padding, width - padding).copy_(tensor[k])
            k = k + 1
    return grid


def quant_round(grid):
    """torchvision save_image: float [3,H,W] -> uint8 [H,W,3]."""
    return grid.clone().mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to("cpu", torch.uint8).contiguous()


def quant_trunc(grid):
    """tensorboard's image conversion of a float CHW array -> uint8 [H,W,3]."""
    g = grid.numpy()
    return torch.from_numpy(np.ascontiguousarray((g * 255).clip(0, 255).astype(np.uint8).transpose(1, 2, 0)))


def save_images_array(t):
    """utils.py:95-106 for one [C,H,W] tensor: the uint8 array handed to PIL."""
    tensor = (t.clone() + 1) * 0.5 * 255
    tensor = tensor.cpu().clamp(0, 255)
    array = tensor.numpy().astype("uint8")
    if array.shape[0] == 1:
        array = array.squeeze(0)
    elif array.shape[0] == 3:
        array = array.swapaxes(0, 1).swapaxes(1, 2)
    return array


# A panel on the host: (how, tensor [N,C,H,W] on the CPU).  how: 'signed_a' / 'signed_b' (3 channels), 'unit' (3 channels),
# 'mask' (1 channel, expanded), 'seg' (C channels).  A tensor with N == 1 is the reference's ``x[0]`` panel: sample 0 in every grid.
def ref_panel(how, t, i):
    s = t[0] if t.shape[0] == 1 else t[i]
    if how == "signed_a":
        return signed_a(s)
    if how == "signed_b":
        return signed_b(s)
    if how == "unit":
        return s
    if how == "mask":
        return s.expand(3, -1, -1)
    if how == "seg":
        return ref_visualize_segmap(t, batch=0 if t.shape[0] == 1 else i)
    raise ValueError(how)


def ref_grid(specs, i, nrow=4, padding=2, quant=ROUND):
    """uint8 [Hg,Wg,3]: grid of sample ``i``."""
    g = ref_make_grid([ref_panel(how, t, i) for how, t in specs], nrow=nrow, padding=padding)
    return quant_round(g) if quant == ROUND else quant_trunc(g)


def ref_grids(specs, N, nrow=4, padding=2, quant=ROUND):
    return torch.stack([ref_grid(specs, i, nrow, padding, quant) for i in range(N)])


def ref_shape(n, H, W, nrow=4, padding=2):
    if n == 1:
        return H, W
    xmaps = min(nrow, n)
    ymaps = -(-n // xmaps)
    return ymaps * (H + padding) + padding, xmaps * (W + padding) + padding


# ------------------------------------------------------------------------------------------ the boundary table
def boundary_table():
    """For every k = 1..255 the fp32 nearest to (k - 0.5) / 255 and its 6 neighbours on each side: 3315 values around the points
    where ``v * 255`` crosses a half-integer -- where a fused multiply-add, round-half-even or a truncation would give another byte."""
    vals = []
    for k in range(1, 256):
        c = np.float32((k - 0.5) / 255.0)
        lo = c
        hi = c
        side = [c]
        for _ in range(6):
            lo = np.nextafter(lo, np.float32(-np.inf), dtype=np.float32)
            hi = np.nextafter(hi, np.float32(np.inf), dtype=np.float32)
            side += [lo, hi]
        vals += sorted(side)
    return torch.from_numpy(np.asarray(vals, dtype=np.float32))


def table_signed(table):
    """2v - 1: the SIGNED input whose ``t / 2 + 0.5`` lands on (or next to) the table value."""
    return table * 2 - 1


def fill(shape, seed, signed):
    """A tensor of ``shape`` whose leading elements walk the boundary table (as far as it fits, from an offset that depends on the
    seed) and whose rest is uniform in [-1.2, 1.2], so that both clamps act."""
    g = torch.Generator().manual_seed(seed)
    n = int(np.prod(shape))
    tab = boundary_table()
    tab = table_signed(tab) if signed else tab
    out = torch.rand(n, generator=g) * 2.4 - 1.2
    take = min(n * 3 // 4, tab.numel())
    off = (seed * 977) % tab.numel()
    idx = (torch.arange(take) + off) % tab.numel()
    out[:take] = tab[idx]
    return out.reshape(shape)


def seg_scores(N, C, H, W, seed):
    """Blocky random scores with plenty of exact ties."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-3, 4, (N, C, H, W), generator=g).to(torch.float32) * 0.25
    return x


def kind_cycle(n, N, H, W, seed):
    """n host panels cycling through the kinds: [('signed_a', t), ('unit', t), ('seg', t13), ('mask', t1), ('signed_b', t), ('seg', t7)]"""
    specs = []
    for k in range(n):
        j = k % 6
        s = seed * 31 + k
        if j == 0:
            specs.append(("signed_a", fill((N, 3, H, W), s, True)))
        elif j == 1:
            specs.append(("unit", fill((N, 3, H, W), s, False)))
        elif j == 2:
            specs.append(("seg", seg_scores(N, 13, H, W, s)))
        elif j == 3:
            specs.append(("mask", fill((N, 1, H, W), s, False)))
        elif j == 4:
            specs.append(("signed_b", fill((N, 3, H, W), s, True)))
        else:
            specs.append(("seg", seg_scores(N, 7, H, W, s)))
    return specs
