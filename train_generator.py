#!/usr/bin/env python3
"""Drop-in for the reference's ``train_generator.py`` (same flags / loop / checkpoint files)
on the MI355X-native hot path.

  * one process per GPU: ``python -m torch.distributed.run --nproc-per-node N train_generator.py ...``
    (``--gpu_ids 0,1,..`` is accepted for CLI compatibility; the rank's device is LOCAL_RANK).  Replicas
    hold identical weights; gradients are bucket-all-reduced on RCCL during the backward
    (hr_viton_amd.parallel.GradSync) instead of the reference's nn.DataParallel wrapper.
  * ``-b`` is the GLOBAL batch like the reference (split over ranks, train_generator.py:124-126).
  * ``--fp16``: mixed precision like the reference's apex O1 -- every training convolution (forward, data and
    weight gradient) runs on the bf16 matrix cores over fp32 tensors (hr_viton_amd.train_ops.MMA_BF16);
    normalisations, losses, the optimizer and everything in HBM stay fp32.
  * ``--synthetic`` feeds VITON-HD-shaped random batches (no dataset / torchvision in this image).
  * LPIPS evaluation (train_generator.py:480-584): every ``--lpips_count`` steps rank 0 runs the frozen pipeline and the generator in
    eval mode over the first ``--val_items`` items of the test list (``--test_dataroot`` / ``--test_data_list``; fixed-seed synthetic
    batches under ``--synthetic``), batch ``--val_batch_size``, and logs ``test/LPIPS`` of the 128x128 resizes to
    ``<tensorboard_dir>/<name>/scalars.jsonl`` (and to tensorboard where a SummaryWriter is importable): hr_viton_amd.validate,
    which states the deviations.  The LPIPS weights are read from ``--lpips_weights`` / ``--alexnet_weights`` and never downloaded;
    where they are missing the pass is skipped with one note.
  * recording (train_generator.py:364-478) is opt-in: with ``--board`` rank 0 records, every ``--tensorboard_count`` steps, the loss
    scalars under the reference's tags (``Loss/gen``, ``Loss/gen/adv``, ``Loss/gen/feat``, ``Loss/gen/vgg``, ``Loss/dis``,
    ``Loss/dis/adv_fake``, ``Loss/dis/adv_real``; a term that is switched off is skipped) into ``scalars.jsonl``, and the 10-panel
    grids (the reference's ``make_image_grid``) ``train_images`` and ``test_images/{i}``, i < ``--num_test_visualize`` (frozen
    pipeline + generator in eval mode on test items) as PNGs under ``<tensorboard_dir>/<name>/images/``, composed and quantised in one
    HIP launch (hr_viton_amd.viz, which states the deviations).  Without ``--board`` nothing of this is computed or written and
    ``--tensorboard_count`` is ignored.
  * ``--diffaug color,translation,cutout`` (any subset; default off): DiffAugment of both discriminator calls of an iteration, applied
    inside the kernels that assemble the PatchGAN input (hr_viton_amd.diffaug).  The VGG term, ``test/LPIPS`` and the grids see the
    un-augmented output.
  * ``--lecam W`` (default 0 = off; ``--lecam_decay 0.99 --lecam_start 0 --lecam_form paper|relu``): the LeCam regulariser of the
    discriminator step, and ``--d_stats``: the same loss head with weight 0 (mean logits and r_t = E[sign D(real)] only, hinge
    gradients unchanged) -- hr_viton_amd.lecam.  Anchors, r_t and the count stay on the device; the printed line gains ``D_lecam`` and
    ``r_t``, ``--board`` records ``Loss/dis/lecam`` and ``Reg/*`` per scale, and ``lecam_step_*.pth`` / ``lecam_final.pth`` are
    written beside the discriminator's files (``--lecam_checkpoint FILE`` resumes from one).
  * ``--ada_target T`` (``--ada_kimg 500 --ada_interval 4 --ada_p_init 0 --ada_p_max 1``) or ``--ada_fixed_p P``, both with ``--diffaug``:
    adaptive discriminator augmentation (Karras et al. 2020) -- every transform of the policy is applied to a sample with
    probability p, gated inside the same kernels; with a target, one controller launch per discriminator step moves p on the
    device so that the windowed r_t of the loss head stays at T (without ``--lecam`` / ``--d_stats`` the head is switched on with
    weight 0).  The printed line gains ``ada_p``, ``--board`` records ``Aug/p`` and ``Aug/r_t``, and ``ada_step_*.pth`` /
    ``ada_final.pth`` are written beside the LeCam files (``--ada_checkpoint FILE`` resumes from one).
  * ``--layer_stats_count N`` (default 0 = off; ``--layer_stats_top 5``): every N steps, after both optimizers have stepped, one
    per-parameter report per optimizer (hr_viton_amd.optim.layer_report: gradient, weight and update norms, maxima, non-finite and
    zero counts; two launches and one small copy) is appended to ``<tensorboard_dir>/<name>/layer_stats.jsonl``; the printed line
    names the top parameters by gradient norm, ``--board`` records ``Layers/{G,D}/*``.  ``--layer_stats_on_skip`` (with
    ``--skip_nonfinite``) reports right after a skipped step; it reads the guard record after every step, a host synchronisation.
  * ``--r1_gamma G`` (default 0 = off; ``--r1_interval 16``): the R1 gradient penalty G / 2 * E_real ||dD/dx||^2 as a separate lazy
    phase behind the discriminator step of every ``--r1_interval``-th iteration, exact, by a tangent pass through the PatchGAN
    (hr_viton_amd.r1) on fp32 operands, on the un-augmented real images; the phase is eager.  In those iterations the printed line
    gains ``D_r1`` and ``r1_pen`` and ``--board`` records ``Loss/dis/r1`` and ``Reg/r1_penalty``.
Bug-fixes of the reference call sites: tocg(input1, input2) arity, load_checkpoint arity,
Adam betas as floats.
"""
import argparse
import contextlib
import os
import sys
import time

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import hr_viton_amd  # noqa: E402,F401
from hr_viton_amd import dist as hdist  # noqa: E402
from hr_viton_amd import viz  # noqa: E402
from hr_viton_amd.checkpoint import load_checkpoint, save_checkpoint  # noqa: E402
from hr_viton_amd.diffaug import AdaptiveAugment, ada_line, ada_scalars, add_ada_args, add_diffaug_args, diffaug_from_opt  # noqa: E402
from hr_viton_amd.gen_train import attach_grad_sync  # noqa: E402
from hr_viton_amd.lecam import add_lecam_args, lecam_from_opt, lecam_line, lecam_scalars  # noqa: E402
from hr_viton_amd.losses import GANLoss, L1Loss  # noqa: E402
from hr_viton_amd.network_generator import MultiscaleDiscriminator, SPADEGenerator  # noqa: E402
from hr_viton_amd.networks import ConditionGenerator  # noqa: E402
from hr_viton_amd.optim import (Adam, add_ema_args, add_guard_args, add_layer_stats_args, ema_kwargs, guard_kwargs, guard_line,  # noqa: E402
                                check_layer_stats_args, guard_scalars, layer_stats_from_opt)
from hr_viton_amd.parallel import broadcast_module  # noqa: E402
from hr_viton_amd.pipeline import generator_train_step, make_generator_inputs  # noqa: E402
from hr_viton_amd.r1 import add_r1_args, r1_from_opt, r1_line  # noqa: E402
from hr_viton_amd.validate import (generator_validation_lpips, load_validation_lpips, val_items_loader,  # noqa: E402
                                   validation_due)
from hr_viton_amd.vgg import VGGLoss  # noqa: E402


def get_opt(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--name", type=str, required=True)
    p.add_argument("--gpu_ids", type=str, default="0")
    p.add_argument("-j", "--workers", type=int, default=4)
    p.add_argument("-b", "--batch_size", type=int, default=8)
    p.add_argument("--fp16", action="store_true", help="use amp")
    p.add_argument("--cuda", default=True)
    p.add_argument("--dataroot", default="./data/")
    p.add_argument("--datamode", default="train")
    p.add_argument("--data_list", default="train_pairs.txt")
    p.add_argument("--fine_width", type=int, default=768)
    p.add_argument("--fine_height", type=int, default=1024)
    p.add_argument("--radius", type=int, default=20)
    p.add_argument("--grid_size", type=int, default=5)
    p.add_argument("--tensorboard_dir", type=str, default="tensorboard")
    p.add_argument("--checkpoint_dir", type=str, default="checkpoints")
    p.add_argument("--tocg_checkpoint", type=str)
    p.add_argument("--gen_checkpoint", type=str, default="")
    p.add_argument("--dis_checkpoint", type=str, default="")
    p.add_argument("--tensorboard_count", type=int, default=100)
    p.add_argument("--display_count", type=int, default=100)
    p.add_argument("--save_count", type=int, default=10000)
    p.add_argument("--load_step", type=int, default=0)
    p.add_argument("--keep_step", type=int, default=100000)
    p.add_argument("--decay_step", type=int, default=100000)
    p.add_argument("--shuffle", action="store_true")
    p.add_argument("--lpips_count", type=int, default=1000)
    p.add_argument("--test_datasetting", default="paired")
    p.add_argument("--test_dataroot", default="./data/")
    p.add_argument("--test_data_list", default="test_pairs.txt")
    p.add_argument("--G_lr", type=float, default=0.0001)
    p.add_argument("--D_lr", type=float, default=0.0004)
    p.add_argument("--GMM_const", type=float, default=None)
    p.add_argument("--semantic_nc", type=int, default=13)
    p.add_argument("--gen_semantic_nc", type=int, default=7)
    p.add_argument("--norm_G", type=str, default="spectralaliasinstance")
    p.add_argument("--norm_D", type=str, default="spectralinstance")
    p.add_argument("--ngf", type=int, default=64)
    p.add_argument("--ndf", type=int, default=64)
    p.add_argument("--num_upsampling_layers", choices=["normal", "more", "most"], default="most")
    p.add_argument("--init_type", type=str, default="xavier")
    p.add_argument("--init_variance", type=float, default=0.02)
    p.add_argument("--no_ganFeat_loss", action="store_true")
    p.add_argument("--no_vgg_loss", action="store_true")
    p.add_argument("--lambda_l1", type=float, default=1.0)
    p.add_argument("--lambda_feat", type=float, default=10.0)
    p.add_argument("--lambda_vgg", type=float, default=10.0)
    p.add_argument("--n_layers_D", type=int, default=3)
    p.add_argument("--netD_subarch", type=str, default="n_layer")
    p.add_argument("--num_D", type=int, default=2)
    p.add_argument("--GT", action="store_true")
    p.add_argument("--occlusion", action="store_true")
    p.add_argument("--warp_feature", choices=["encoder", "T1"], default="T1")
    p.add_argument("--out_layer", choices=["relu", "conv"], default="relu")
    p.add_argument("--clothmask_composition", type=str, choices=["no_composition", "detach", "warp_grad"], default="warp_grad")
    p.add_argument("--num_test_visualize", type=int, default=3)
    # additions
    p.add_argument("--synthetic", action="store_true", help="synthetic VITON-HD-shaped batches")
    p.add_argument("--max_steps", type=int, default=0, help="stop after this many steps (0: keep_step+decay_step)")
    p.add_argument("--tocg_ngf", type=int, default=96)
    p.add_argument("--vgg_weights", type=str, default="", help="torchvision vgg19 state_dict (.pth): the reference's models.vgg19(pretrained=True) weights")
    p.add_argument("--vgg_random_init", action="store_true",
                   help="plumbing / bench runs only: a RANDOMLY initialised VGG19 in the perceptual loss (no network here to "
                        "download the pretrained weights); implied by --synthetic")
    p.add_argument("--lpips_weights", default="./eval_models/weights/v0.1/alex.pth", help="LPIPS v0.1 lin layers (alex.pth)")
    p.add_argument("--alexnet_weights", default=None,
                   help="torchvision alexnet state dict (default: torch's hub cache; read only if present)")
    p.add_argument("--lpips_random_init", action="store_true",
                   help="plumbing only: test/LPIPS on randomly initialised AlexNet / lin weights (labelled); implied by --synthetic")
    p.add_argument("--val_items", type=int, default=500, help="test items scored per test/LPIPS pass (the reference's 500)")
    p.add_argument("--val_batch_size", type=int, default=1, help="batch of the test/LPIPS pass (the reference's 1)")
    p.add_argument("--board", action="store_true",
                   help="every --tensorboard_count steps record the loss scalars and the image grids (train_generator.py:364-478)")
    add_guard_args(p)
    add_ema_args(p)
    add_layer_stats_args(p)
    add_diffaug_args(p)
    add_ada_args(p)
    add_lecam_args(p)
    add_r1_args(p)
    opt = p.parse_args(argv)
    opt.gpu_ids = [int(s) for s in str(opt.gpu_ids).split(",") if s.strip() and int(s) >= 0]
    return opt


def synthetic_batch(opt, n, seed, device):
    g = torch.Generator().manual_seed(seed)
    H, W = opt.fine_height, opt.fine_width
    lab = torch.randint(0, 13, (n, 1, H // 32, W // 32), generator=g).repeat_interleave(32, 2).repeat_interleave(32, 3)
    u = lambda c: (torch.rand(n, c, H, W, generator=g) * 2 - 1).to(device)  # noqa: E731
    onehot = torch.zeros(n, 13, H, W).scatter_(1, lab, 1.0).to(device)
    return {"cloth": u(3), "cloth_mask": (torch.rand(n, 1, H, W, generator=g) > 0.4).float().to(device),
            "parse_agnostic": onehot, "densepose": u(3), "agnostic": u(3), "image": u(3),
            "parse": onehot, "parse_cloth": u(3)}


VAL_SEED = 9_000_011      # synthetic validation batches: the same draws at every pass, so the series is comparable over a run
VIS_SEED = 9_100_003      # the synthetic test-visualisation batch


def disk_batch(raw, dev, datasetting="paired"):
    """cp_dataset.py batch -> the flat dictionary make_generator_inputs takes (train_generator.py:194-212)."""
    return {"cloth": raw["cloth"][datasetting].to(dev), "cloth_mask": raw["cloth_mask"][datasetting].to(dev),
            "parse_agnostic": raw["parse_agnostic"].to(dev), "densepose": raw["densepose"].to(dev),
            "agnostic": raw["agnostic"].to(dev), "image": raw["image"].to(dev),
            "parse": raw["parse"].to(dev), "parse_cloth": raw["parse_cloth"].to(dev)}


class _Validation(object):
    """The test/LPIPS pass of one run: LPIPS model and test loader are built at first use, the log at the first record."""

    def __init__(self, opt, device):
        self.opt, self.device = opt, device
        self.loader, self.model, self.tried = None, None, False
        self.board = viz.BoardLog(os.path.join(opt.tensorboard_dir, opt.name))
        self.vis = None
        self.opt_g = self.opt_d = None      # the optimizers whose guard records ride along with the loss scalars (main sets them)
        self.ema_eval = False               # --ema_eval: the test passes run on opt_g's averaged weights (main sets it)
        self.lecam = None                   # --lecam / --d_stats: the D step's loss head (main sets it)
        self.aug = None                     # --ada_target / --ada_fixed_p: the adaptive augmentation (main sets it)
        self.r1 = None                      # --r1_gamma: the lazy R1 phase (main sets it)

    def weights(self):
        """The context the test passes run in: the generator's averaged weights with --ema_eval, the raw ones otherwise."""
        return self.opt_g.swap_ema() if self.ema_eval else contextlib.nullcontext()

    def vis_batch(self):
        """The test-visualisation batch (:383-395): the first --num_test_visualize test items with the unpaired cloth, loaded once."""
        if self.vis is None:
            opt, n = self.opt, self.opt.num_test_visualize
            if opt.synthetic:
                self.vis = synthetic_batch(opt, n, VIS_SEED, self.device)
            else:
                loader, _ = val_items_loader(opt, n, n)
                self.vis = disk_batch(next(iter(loader)), self.device, "unpaired")
        return self.vis

    def record(self, tocg, generator, step, losses, batch, aux, output):
        """train_generator.py:364-478: ``train_images`` (sample 0 of the training batch), the loss scalars and ``test_images/{i}``."""
        opt, s = self.opt, step + 1
        self.board.add_image("train_images", viz.generator_train_grid(batch, aux, output, quant=viz.TRUNC, count=1)[0], s)
        losses = {k: v.detach() for k, v in losses.items()}
        gen = [v for k, v in losses.items() if not k.startswith("D_")]
        dis = [v for k, v in losses.items() if k.startswith("D_")]
        self.board.add_scalar("Loss/gen", float(sum(gen).mean()), s)
        for tag, key in (("Loss/gen/adv", "GAN"), ("Loss/gen/feat", "GAN_Feat"), ("Loss/gen/vgg", "VGG")):
            if key in losses:
                self.board.add_scalar(tag, float(losses[key].mean()), s)
        self.board.add_scalar("Loss/dis", float(sum(dis).mean()), s)
        self.board.add_scalar("Loss/dis/adv_fake", float(losses["D_Fake"].mean()), s)
        self.board.add_scalar("Loss/dis/adv_real", float(losses["D_Real"].mean()), s)
        for tag, val in guard_scalars(self.opt_g, self.opt_d):      # (nothing without --max_grad_norm_* / --skip_nonfinite)
            self.board.add_scalar(tag, val, s)
        if "D_LeCam" in losses:                                     # (nothing without --lecam / --d_stats)
            self.board.add_scalar("Loss/dis/lecam", float(losses["D_LeCam"].mean()), s)
            for tag, val in lecam_scalars(self.lecam):
                self.board.add_scalar(tag, val, s)
        for tag, val in ada_scalars(self.aug):                       # (nothing without --ada_target / --ada_fixed_p)
            self.board.add_scalar(tag, val, s)
        if "D_R1" in losses:                                        # (nothing without --r1_gamma, or between two phases)
            self.board.add_scalar("Loss/dis/r1", float(losses["D_R1"].mean()), s)
            self.board.add_scalar("Reg/r1_penalty", float(self.r1.last["r1_penalty"]), s)
        if opt.num_test_visualize > 0:
            vb = self.vis_batch()
            with self.weights():
                fields, out = viz.generator_fields(opt, tocg, generator, vb)
                grids = viz.to_host(viz.generator_train_grid(vb, fields, out, quant=viz.TRUNC))
            for i in range(grids.shape[0]):
                self.board.add_image("test_images/%d" % i, grids[i], s)

    def batches(self):
        opt, bs = self.opt, max(1, self.opt.val_batch_size)
        if opt.synthetic:
            for k in range(-(-opt.val_items // bs)):
                yield synthetic_batch(opt, bs, VAL_SEED + k, self.device)
            return
        if self.loader is None:
            self.loader, _ = val_items_loader(opt, opt.val_items, bs)
        for raw in self.loader:
            yield disk_batch(raw, self.device)

    def run(self, tocg, generator, step):
        if not self.tried:
            self.tried = True
            self.model = load_validation_lpips(self.opt)       # None, with one note, when the weights are missing
        if self.model is None:
            return None
        print("LPIPS")
        with self.weights():
            res = generator_validation_lpips(self.opt, tocg, generator, self.model, self.batches(), max_items=self.opt.val_items)
        if res["items"]:
            avg_distance = res["lpips"]
            print(f"LPIPS{avg_distance}")
            self.board.add_scalar("test/LPIPS", avg_distance, step + 1)
        return res


def main(argv=None):
    opt = get_opt(argv)
    check_layer_stats_args(opt)
    rank, local_rank, world = hdist.init_from_env()
    if opt.fp16:
        from hr_viton_amd import train_ops as _T
        _T.MMA_BF16[0] = True      # bf16 matrix cores for the training convolutions (fp32 storage / accumulate)
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    assert opt.batch_size % world == 0, "Batch size %d must be a multiple of # GPUs %d." % (opt.batch_size, world)
    per_rank = opt.batch_size // world
    if rank == 0:
        print(opt)
        print("Start to train %s!" % opt.name)

    tocg = ConditionGenerator(opt, input1_nc=4, input2_nc=opt.semantic_nc + 3, output_nc=opt.semantic_nc,
                              ngf=opt.tocg_ngf, norm_layer=nn.BatchNorm2d)
    if opt.tocg_checkpoint:
        load_checkpoint(tocg, opt.tocg_checkpoint, opt)
    tocg.to(dev).eval()
    generator = SPADEGenerator(opt, 3 + 3 + 3)
    generator.print_network() if rank == 0 else None
    generator.init_weights(opt.init_type, opt.init_variance)
    discriminator = MultiscaleDiscriminator(opt)
    discriminator.init_weights(opt.init_type, opt.init_variance)
    if opt.gen_checkpoint and os.path.exists(opt.gen_checkpoint):
        load_checkpoint(generator, opt.gen_checkpoint, opt)
    if opt.dis_checkpoint and os.path.exists(opt.dis_checkpoint):
        load_checkpoint(discriminator, opt.dis_checkpoint, opt)
    generator.to(dev).train()
    discriminator.to(dev).train()
    broadcast_module(generator)
    broadcast_module(discriminator)

    crit_gan, crit_feat = GANLoss("hinge"), L1Loss()
    crit_vgg = None
    if not opt.no_vgg_loss:
        crit_vgg = VGGLoss(opt)
        if opt.vgg_weights:
            crit_vgg.vgg.load_torchvision_state_dict(torch.load(opt.vgg_weights, map_location="cpu"))
        elif opt.vgg_random_init or opt.synthetic:
            if rank == 0:
                print("WARNING: VGGLoss runs on a RANDOMLY initialised VGG19 (--vgg_random_init / --synthetic): the "
                      "perceptual term is not the reference's objective; pass --vgg_weights for real training.", flush=True)
        else:
            # the reference builds models.vgg19(pretrained=True) (networks.py:204); silently optimising random features
            # would be a different objective
            raise SystemExit("VGGLoss needs the pretrained torchvision vgg19 weights: pass --vgg_weights <state_dict.pth>, "
                             "or --no_vgg_loss, or --vgg_random_init for plumbing runs")
        crit_vgg.to(dev)
        broadcast_module(crit_vgg)

    ema = ema_kwargs(opt)      # (empty without --ema_decay: the plain construction, nothing allocated)
    if not ema and (getattr(opt, "ema_eval", False) or getattr(opt, "ema_checkpoint", "")):
        raise SystemExit("--ema_eval / --ema_checkpoint need --ema_decay")
    opt_g = Adam(generator.parameters(), lr=opt.G_lr, betas=(0.0, 0.9), **guard_kwargs(opt, "G"), **ema)
    if ema and getattr(opt, "ema_checkpoint", ""):
        opt_g.load_ema_state_dict(generator, torch.load(opt.ema_checkpoint, map_location="cpu"))
    opt_d = Adam(discriminator.parameters(), lr=opt.D_lr, betas=(0.0, 0.9), **guard_kwargs(opt, "D"))
    # in-place bucketed all-reduce on the optimizers' flat gradient buffers, fired from inside the backward
    sync_g = opt_g.make_grad_sync() if world > 1 else None
    sync_d = opt_d.make_grad_sync() if world > 1 else None
    for s in (sync_g, sync_d):
        if s is not None:
            attach_grad_sync(s)
    aug = diffaug_from_opt(opt)      # (None without --diffaug: the plain iteration, no new launch)
    ada = aug if isinstance(aug, AdaptiveAugment) else None      # (None without --ada_target / --ada_fixed_p: nothing allocated)
    if ada is not None and ada.adaptive and not float(getattr(opt, "lecam", 0.0) or 0.0):
        opt.d_stats = True           # the controller follows the head's r_t: the head with weight 0
    lecam = lecam_from_opt(opt)      # (None without --lecam / --d_stats: the four GANLoss calls, nothing allocated)
    r1 = r1_from_opt(opt)            # (None without --r1_gamma: nothing allocated or launched)
    lam = lambda step: 1.0 - max(0, step * 1000 + opt.load_step - opt.keep_step) / float(opt.decay_step + 1)  # noqa: E731
    sched_g = torch.optim.lr_scheduler.LambdaLR(opt_g, lr_lambda=lam)
    sched_d = torch.optim.lr_scheduler.LambdaLR(opt_d, lr_lambda=lam)

    loader = None
    if not opt.synthetic:
        import copy
        from hr_viton_amd.cp_dataset import CPDataLoader, CPDataset
        o = copy.copy(opt)
        o.batch_size = per_rank
        torch.manual_seed(hdist.shard_seed(97, rank))
        loader = CPDataLoader(o, CPDataset(o), rank, world)
    last = opt.keep_step + opt.decay_step
    if opt.max_steps:
        last = min(last, opt.load_step + opt.max_steps)
    validation = _Validation(opt, dev) if rank == 0 else None
    if validation is not None:
        validation.opt_g, validation.opt_d = opt_g, opt_d
        validation.ema_eval = bool(ema) and bool(getattr(opt, "ema_eval", False))
        validation.lecam = lecam
        validation.aug = ada
        validation.r1 = r1
    # (None without --layer_stats_count / --layer_stats_on_skip: nothing allocated or launched; rank 0 reports -- the gradient
    # buffers are the all-reduced ones, every rank would report the same)
    layers = layer_stats_from_opt(opt, [("G", opt_g, generator), ("D", opt_d, discriminator)])
    if rank != 0:
        layers = None
    for step in range(opt.load_step, last):
        t0 = time.time()
        if loader is None:
            batch = synthetic_batch(opt, per_rank, hdist.shard_seed(1234 + step * 97, rank), dev)
        else:
            batch = disk_batch(loader.next_batch(), dev)               # train_generator.py:194-212
        record = opt.board and validation is not None and validation_due(step, opt.tensorboard_count)       # :364
        aux = {} if record else None
        x, parse7 = make_generator_inputs(opt, tocg, batch, aux=aux)
        kw = {} if lecam is None else {"lecam": lecam}
        if r1 is not None and r1.due(step):      # the lazy R1 phase behind the D step, every --r1_interval iterations
            kw["r1"] = r1
        losses, _ = generator_train_step(opt, generator, discriminator, crit_gan, crit_feat, crit_vgg, opt_g, opt_d, x,
                                         parse7, batch["image"], sync_g, sync_d, aux=aux, aug=aug, **kw)
        layer_text = layers.after_step(step + 1, validation.board if opt.board else None) if layers is not None else ""
        if record:
            validation.record(tocg, generator, step, losses, batch, aux, aux["output"])
        if validation_due(step, opt.lpips_count) and validation is not None:        # :480-584
            validation.run(tocg, generator, step)
        if (step + 1) % opt.display_count == 0 and rank == 0:
            torch.cuda.synchronize()
            t = time.time() - t0
            ld = sum(v.item() for k, v in losses.items() if k.startswith("D_"))
            lg = sum(v.item() for k, v in losses.items() if not k.startswith("D_"))
            print("step: %8d, time: %.3f, G_loss: %.4f, G_adv_loss: %.4f, D_loss: %.4f, D_fake_loss: %.4f, D_real_loss: %.4f"
                  % (step + 1, t, lg, losses["GAN"].item(), ld, losses["D_Fake"].item(), losses["D_Real"].item())
                  + guard_line(opt_g, opt_d) + lecam_line(lecam, losses) + ada_line(ada) + r1_line(r1, losses) + layer_text, flush=True)
        if (step + 1) % opt.save_count == 0 and rank == 0:
            save_checkpoint(generator, os.path.join(opt.checkpoint_dir, opt.name, "gen_step_%06d.pth" % (step + 1)), opt)
            save_checkpoint(discriminator, os.path.join(opt.checkpoint_dir, opt.name, "dis_step_%06d.pth" % (step + 1)), opt)
            if ema:
                save_checkpoint(generator, os.path.join(opt.checkpoint_dir, opt.name, "gen_ema_step_%06d.pth" % (step + 1)), opt,
                                state_dict=opt_g.ema_state_dict(generator))
            if lecam is not None:
                torch.save(lecam.state_dict(), os.path.join(opt.checkpoint_dir, opt.name, "lecam_step_%06d.pth" % (step + 1)))
            if ada is not None:
                torch.save(ada.state_dict(), os.path.join(opt.checkpoint_dir, opt.name, "ada_step_%06d.pth" % (step + 1)))
        if (step + 1) % 1000 == 0:
            sched_g.step()
            sched_d.step()
    if rank == 0:
        save_checkpoint(generator, os.path.join(opt.checkpoint_dir, opt.name, "gen_model_final.pth"), opt)
        save_checkpoint(discriminator, os.path.join(opt.checkpoint_dir, opt.name, "dis_model_final.pth"), opt)
        if ema:
            save_checkpoint(generator, os.path.join(opt.checkpoint_dir, opt.name, "gen_ema_model_final.pth"), opt,
                            state_dict=opt_g.ema_state_dict(generator))
        if lecam is not None:
            torch.save(lecam.state_dict(), os.path.join(opt.checkpoint_dir, opt.name, "lecam_final.pth"))
        if ada is not None:
            torch.save(ada.state_dict(), os.path.join(opt.checkpoint_dir, opt.name, "ada_final.pth"))
        validation.board.close()
        print("Finished training %s!" % opt.name)


if __name__ == "__main__":
    main()
