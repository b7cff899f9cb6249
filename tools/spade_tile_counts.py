#!/usr/bin/env python3
"""Heavy / light tile counts per generator level (csrc/spade_tiles.hip) of the label maps the benchmark's train_generator batch
produces: the bench's own set-up (same seeds, random-init condition generator), one make_generator_inputs, one tile plan per level.
Needs the GPU.  ``--batch`` as bench.py's."""
import argparse
import os
import sys

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--levels", type=int, default=5)
    a = ap.parse_args()
    import hr_viton_amd  # noqa: F401
    import train_generator as tg
    from hr_viton_amd import ops, train_ops as T
    from hr_viton_amd.networks import ConditionGenerator
    from hr_viton_amd.pipeline import make_generator_inputs
    dev = torch.device("cuda")
    opt = tg.get_opt(["--name", "bench", "--synthetic", "-b", str(a.batch), "--fp16"])
    torch.manual_seed(0)
    tocg = ConditionGenerator(opt, 4, 16, 13, ngf=96, norm_layer=nn.BatchNorm2d).to(dev).eval()
    batch = tg.synthetic_batch(opt, a.batch, 1234, dev)
    T.MMA_BF16[0] = True
    with torch.no_grad():
        _, parse7 = make_generator_inputs(opt, tocg, batch)
    seg = ops.Act(parse7.t.to(torch.bfloat16), parse7.C)
    print("class histogram:", parse7.t[..., :7].sum((0, 1, 2)).long().tolist())
    print("level        tiles    heavy    light  light fraction  representatives")
    for s in range(a.levels):
        H, W = seg.H >> s, seg.W >> s
        p = T.spade_tile_plan(seg, s, seg.N, H, W)
        h, l = p.counts()
        print("%4d x %-4d %7d %8d %8d      %.3f       %s" % (H, W, p.tiles, h, l, l / p.tiles, [r for r in p.lists()[2] if r >= 0]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
