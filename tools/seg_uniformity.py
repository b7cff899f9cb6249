#!/usr/bin/env python3
"""CPU estimate of how many 16x16-pixel tiles of a label map the fused SPADE forward can serve without matrix work
(csrc/spade_tiles.hip; the rule is in tests/spade_uniform_cases.py): per generator level, the fraction of tiles whose 20x20 patch
of sampled labels lies inside the level image and carries one label.  No GPU, no library build.

    tools/seg_uniformity.py labels.pt            # int tensor [N, H, W] (argmax labels) or [N, C, H, W] / [N, H, W, C] one-hot scores
    tools/seg_uniformity.py parse_dir/           # a directory of single-channel label PNGs (needs PIL)
    tools/seg_uniformity.py --blobs 4            # a synthetic stand-in: 4 maps of argmax(blurred random scores) at 1024 x 768

The count excludes border and partial tiles (they are heavy by rule) and does not subtract the <= 8 representatives per level."""
import argparse
import os
import sys

import torch
import torch.nn.functional as F


def load_labels(path):
    if os.path.isdir(path):
        from PIL import Image
        import numpy as np
        maps = [torch.from_numpy(np.array(Image.open(os.path.join(path, f)))).long() for f in sorted(os.listdir(path))
                if f.lower().endswith(".png")]
        assert maps, "no .png under " + path
        return torch.stack([m if m.dim() == 2 else m[..., 0] for m in maps])
    t = torch.load(path, map_location="cpu")
    if t.dim() == 4:
        t = t.argmax(1 if t.shape[1] <= t.shape[3] else 3)
    return t.long()


def blobs(n, H, W, classes=7, seed=0):
    g = torch.Generator().manual_seed(seed)
    s = torch.rand(n, classes, H // 4, W // 4, generator=g)
    s = F.avg_pool2d(F.pad(s, (7, 7, 7, 7), mode="replicate"), 15, 1)
    return F.interpolate(s, size=(H, W), mode="bilinear", align_corners=False).argmax(1)


def level_fraction(lab, shift):
    """(light-classified tiles, tiles) of the level that samples ``lab`` [N, H, W] at (y << shift, x << shift)"""
    L = lab[:, ::(1 << shift), ::(1 << shift)].float().unsqueeze(1)
    N, _, H, W = L.shape
    tiles = N * ((H + 15) // 16) * ((W + 15) // 16)
    if H < 14 + 20 or W < 14 + 20:
        return 0, tiles
    p = L[:, :, 14:, 14:]                        # the patch of tile (16 i, 16 j), i, j >= 1, starts at (16 i - 2, 16 j - 2)
    hi, lo = F.max_pool2d(p, 20, 16), -F.max_pool2d(-p, 20, 16)
    return int((hi == lo).sum()), tiles


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("labels", nargs="?", help="labels .pt file or a directory of label PNGs")
    ap.add_argument("--blobs", type=int, default=0, metavar="N", help="N synthetic maps instead of a file")
    ap.add_argument("--levels", type=int, default=4, help="levels to report, finest first")
    a = ap.parse_args()
    if a.blobs:
        lab = blobs(a.blobs, 1024, 768)
    elif a.labels:
        lab = load_labels(a.labels)
    else:
        ap.error("give a labels file / directory or --blobs N")
    print("label histogram:", torch.bincount(lab.flatten()).tolist())
    print("level        tiles   light-classified  fraction")
    for s in range(a.levels):
        n, m = level_fraction(lab, s)
        print("%4d x %-4d %7d %10d        %.3f" % (lab.shape[1] >> s, lab.shape[2] >> s, m, n, n / max(1, m)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
