#!/usr/bin/env python3
"""The per-sample image grids of the reference's two test scripts, composed on the device.

  python write_grids.py generator --grid_dir DIR [--image_workers K] [--with_outputs] <test_generator.py flags>
  python write_grids.py condition --grid_dir DIR [--image_workers K] <test_condition.py flags>

``generator`` is the visualisation of test_generator.py:221-229: the same flags, models, checkpoints and loop as
``test_generator.py`` (its ``get_opt`` parses the remaining flags), and for every sample the reference's 12-panel grid as
``DIR/<paired>_<unpaired>.png``; ``--grid_dir ./output/<test_name>/<datamode>/<datasetting>/generator/grid`` is the reference's
location.  ``--with_outputs`` writes the try-on JPEGs of ``test_generator.py`` (under a .png name, utils.py:93-109) to
``--output_dir`` as well, quantised on the device (hr_viton_amd.viz.save_images: the same file bytes).  ``condition`` is
test_condition.py:135-143: the flags of ``test_condition.py``, the 12-panel condition grid of every sample under the reference's
file name (``synthetic_<n>.png`` under ``--synthetic``); the rejection scores stay with ``test_condition.py``.

``visualize_segmap``, ``make_grid`` and the float -> uint8 conversion of a batch's grids are ONE HIP launch (hr_viton_amd.viz,
csrc/viz.hip); a quarter of the reference's bytes travel back, as uint8.  ``--image_workers K`` (0 .. 4) encodes the files on K
threads.  ``test_generator.py`` and ``test_condition.py`` themselves write what they always wrote.
"""
import argparse
import os
import sys
import time

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import hr_viton_amd  # noqa: E402,F401
from hr_viton_amd import viz  # noqa: E402


def get_opt(argv=None):
    """(own options, the remaining flags for the test script's get_opt)."""
    p = argparse.ArgumentParser(add_help=False)
    p.add_argument("which", choices=["generator", "condition"])
    p.add_argument("--grid_dir", type=str, required=True, help="the grids are written here, one PNG per sample")
    p.add_argument("--image_workers", type=int, default=0, help="threads that encode the files (0 .. 4; 0: in the loop)")
    p.add_argument("--with_outputs", action="store_true", help="generator: write test_generator.py's try-on JPEGs too")
    return p.parse_known_args(argv)


def generator_grids(own, rest):
    """test_generator.py's main() and test() with the visualisation block (:221-229) put back."""
    import test_generator as tg
    from hr_viton_amd.checkpoint import load_checkpoint, load_checkpoint_G
    from hr_viton_amd.network_generator import SPADEGenerator
    from hr_viton_amd.networks import ConditionGenerator
    from hr_viton_amd.pipeline import tryon_step
    opt = tg.get_opt(rest)
    print(opt)
    if opt.gpu_ids:
        os.environ["CUDA_VISIBLE_DEVICES"] = opt.gpu_ids
    if opt.synthetic > 0:
        batches = tg.synthetic_batches(opt, opt.synthetic)
    else:
        from hr_viton_amd.cp_dataset import CPDataLoader, CPDatasetTest
        batches = CPDataLoader(opt, CPDatasetTest(opt)).data_loader
    tocg = ConditionGenerator(opt, input1_nc=4, input2_nc=opt.semantic_nc + 3, output_nc=opt.output_nc, ngf=opt.tocg_ngf,
                              norm_layer=nn.BatchNorm2d)
    opt.semantic_nc = 7
    generator = SPADEGenerator(opt, 3 + 3 + 3)
    if not opt.random_init_tocg:
        load_checkpoint(tocg, opt.tocg_checkpoint, opt)
    load_checkpoint_G(generator, opt.gen_checkpoint, opt)
    tocg.cuda().eval()
    generator.cuda().eval()
    os.makedirs(own.grid_dir, exist_ok=True)
    if own.with_outputs:
        os.makedirs(opt.output_dir, exist_ok=True)
    num, t0 = 0, time.time()
    with viz.ImageWriter(own.image_workers) as writer:
        for inputs in batches:
            dev = {"cloth": inputs["cloth"][opt.datasetting].cuda(), "cloth_mask": inputs["cloth_mask"][opt.datasetting].cuda(),
                   "parse_agnostic": inputs["parse_agnostic"].cuda(), "densepose": inputs["densepose"].cuda(),
                   "agnostic": inputs["agnostic"].cuda()}
            res = tryon_step(opt, tocg, generator, dev)
            n = dev["cloth"].shape[0]
            names = [inputs["c_name"]["paired"][i].split(".")[0] + "_" + inputs["c_name"][opt.datasetting][i].split(".")[0] + ".png"
                     for i in range(n)]
            dev["pose"], dev["image"] = inputs["pose"].cuda(), inputs["image"].cuda()
            for g, name in zip(viz.to_host(viz.tryon_grid(dev, res)), names):       # :223-229
                viz.save_image(g, os.path.join(own.grid_dir, name), writer)
            if own.with_outputs:
                viz.save_images(res["output"], names, opt.output_dir, writer)        # :233
            num += n
            print(num)
    torch.cuda.synchronize()
    print(f"Grid time {time.time() - t0}")
    return num


def condition_grids(own, rest):
    """test_condition.py's loop (:79-145) without the discriminator: the grid of every sample."""
    import test_condition as tcd
    from hr_viton_amd.networks import ConditionGenerator, load_checkpoint
    from hr_viton_amd.rejection import rejection_scores
    from train_condition import synthetic_batch, synthetic_image
    opt = tcd.get_opt(rest)
    print(opt)
    dev = torch.device("cuda", 0)
    tocg = ConditionGenerator(opt, input1_nc=4, input2_nc=opt.semantic_nc + 3, output_nc=opt.output_nc, ngf=opt.ngf,
                              norm_layer=nn.BatchNorm2d)
    if opt.tocg_checkpoint:
        load_checkpoint(tocg, opt.tocg_checkpoint, opt)
    tocg.to(dev).eval()
    disk = None
    if not opt.synthetic:
        from hr_viton_amd.cp_dataset import CPDataLoader, CPDatasetTest
        disk = iter(CPDataLoader(opt, CPDatasetTest(opt)).data_loader)
    os.makedirs(own.grid_dir, exist_ok=True)
    num, t0 = 0, time.time()
    with viz.ImageWriter(own.image_workers) as writer:
        for i in range(opt.num_batches if disk is None else 1 << 30):
            if disk is None:
                batch = synthetic_batch(opt, opt.batch_size, 555 + i, dev)
                batch["image"] = synthetic_image(opt, opt.batch_size, 555 + i, dev)
                names = ["synthetic_%05d.png" % (num + j) for j in range(opt.batch_size)]
            else:
                raw = next(disk, None)
                if raw is None:
                    break
                key = opt.datasetting
                batch = {"cloth": raw["cloth"][key].to(dev), "cloth_mask": raw["cloth_mask"][key].to(dev),
                         "parse_agnostic": raw["parse_agnostic"].to(dev), "densepose": raw["densepose"].to(dev),
                         "parse": raw["parse"].to(dev), "image": raw["image"].to(dev), "pcm": raw["pcm"].to(dev),
                         "parse_cloth": raw["parse_cloth"].to(dev)}
                names = [raw["c_name"]["paired"][j].split(".")[0] + "_" + raw["c_name"]["unpaired"][j].split(".")[0] + ".png"
                         for j in range(batch["cloth"].shape[0])]
            _, misalign, fake_segmap, warped_c, warped_cm1 = rejection_scores(opt, tocg, None, batch, 1.0)
            fields = {"fake_segmap": fake_segmap, "warped_cloth": warped_c, "warped_cm_onehot": warped_cm1, "misalign": misalign}
            for g, name in zip(viz.to_host(viz.condition_grid(batch, fields)), names):      # :136-143
                viz.save_image(g, os.path.join(own.grid_dir, name), writer)
            num += len(names)
            print(num)
    print(f"Grid time {time.time() - t0}")
    return num


def main(argv=None):
    own, rest = get_opt(argv)
    return generator_grids(own, rest) if own.which == "generator" else condition_grids(own, rest)


if __name__ == "__main__":
    main()
