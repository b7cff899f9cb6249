"""The validation passes of the reference's training scripts on the HIP path.

``condition_validation_iou`` is train_condition.py:314-360 (``val/iou`` every ``--val_count`` steps): the condition generator in
eval mode over test items, ``iou_metric`` of ``softmax(fake_segmap * cloth_mask)`` against the one-hot parse map (:18-36; counts
by csrc/validate.hip through ``metrics.seg_iou_counts``).  ``generator_validation_lpips`` is train_generator.py:480-584
(``test/LPIPS`` every ``--lpips_count`` steps): the frozen pipeline (``pipeline.make_generator_inputs``), the generator in eval
mode, LPIPS of the 128x128 resizes (``PerceptualLoss.forward_resized``).  Both run under ``no_grad``, touch no optimizer and
leave every parameter and buffer as it was (BatchNorm running statistics, ``num_batches_tracked``, the spectral-norm ``u`` / ``v``);
the modules' train / eval mode is restored in a ``finally``.  ``ScalarLog`` records the scalars, ``validation_due`` says when.

Stated deviations from the reference:

* Under ``--clothmask_composition detach`` the reference's validation block multiplies by ``warped_cm_onehot`` left over from the
  last TRAINING batch (train_condition.py:347); here the validation batch's own thresholded mask is used.
* The reference's validation only exists when ``--no_test_visualize`` is absent (its ``val_loader`` is undefined otherwise); here it
  depends on ``--val_count`` alone.
* The reference takes ``Subset(test, arange(500 | 2000))`` and fails on a shorter list; here the first ``min(limit, len)`` items are
  scored and the mean divides by that count.  The mean is over samples, which equals the reference's mean over equal-sized batches.
* The SPADE noise is drawn in eval mode too (network_generator.py:104-107): ``test/LPIPS`` is a random variable, as in the
  reference.
* Under data-parallel training rank 0 evaluates and the other ranks wait in their next gradient all-reduce; sharding the pass is
  out of scope.
* The tensorboard image grids (``visualize_segmap``, ``make_image_grid``) and loss scalars are not part of these passes: the
  scripts record them under ``--board`` through hr_viton_amd.viz (``BoardLog`` extends ``ScalarLog``).
"""
from __future__ import annotations

import json
import os
import sys
from typing import Dict, Iterable, Optional

import torch

from . import metrics
from .pipeline import make_generator_inputs


def validation_due(step: int, count: int) -> bool:
    """The reference's ``(step + 1) % count == 0`` (train_condition.py:314, train_generator.py:480); a count of 0 or less: never."""
    return count > 0 and (step + 1) % count == 0


def _take(n_batch: int, done: int, max_items: Optional[int]) -> int:
    return n_batch if max_items is None else max(0, min(n_batch, max_items - done))


def condition_validation_iou(opt, tocg, batches: Iterable[Dict[str, torch.Tensor]], max_items: Optional[int] = None) -> dict:
    """Mean ``iou_metric`` of ``tocg`` in eval mode over ``batches`` (dictionaries as ``condition_train_step`` takes them: cloth,
    cloth_mask, parse_agnostic, densepose, parse; CUDA, NCHW fp32).  Returns {'iou': mean over samples (float), 'items': samples
    scored, 'counts': int64 CPU tensor [items,3] of (intersection, sum_pred, sum_true)}.  ``max_items`` stops after that many
    samples."""
    comp = getattr(opt, "clothmask_composition", "warp_grad")
    was_training = tocg.training
    rows, done = [], 0
    tocg.eval()
    try:
        with torch.no_grad():
            for batch in batches:
                take = _take(batch["cloth"].shape[0], done, max_items)
                if take == 0:
                    break
                cm = (batch["cloth_mask"] > 0.5).to(torch.float32)                 # train_condition.py:324, on the device
                input1 = torch.cat([batch["cloth"], cm], 1)
                input2 = torch.cat([batch["parse_agnostic"], batch["densepose"]], 1)
                _, fake_segmap, _, warped_cm = tocg(input1, input2)                # :341
                rows.append(metrics.seg_iou_counts(fake_segmap, warped_cm, batch["parse"], comp)[:take])   # :344-356
                done += take
    finally:
        tocg.train(was_training)
    if not rows:
        return {"iou": float("nan"), "items": 0, "counts": torch.zeros((0, 3), dtype=torch.int64)}
    counts = torch.cat(rows, 0).cpu()
    return {"iou": float(metrics.seg_iou(counts).mean()), "items": done, "counts": counts}


def generator_validation_lpips(opt, tocg, generator, lpips, batches: Iterable[Dict[str, torch.Tensor]], noise=None,
                               max_items: Optional[int] = None) -> dict:
    """Mean LPIPS of the try-on output against ``batch['image']`` at 128x128 over ``batches`` (dictionaries as
    ``make_generator_inputs`` takes them plus 'image').  ``noise``: the generator forward's injection hook -- one dictionary for
    every batch or a sequence with one per batch; default: drawn as the reference draws it.  Returns {'lpips': mean over samples
    (float), 'items': samples scored, 'distances': fp32 CPU tensor [items]}."""
    modes = [(m, m.training) for m in (generator, tocg) if m is not None]
    per_batch = isinstance(noise, (list, tuple))
    dists, done = [], 0
    for m, _ in modes:
        m.eval()
    try:
        with torch.no_grad():
            for k, batch in enumerate(batches):
                take = _take(batch["image"].shape[0], done, max_items)
                if take == 0:
                    break
                x, parse7 = make_generator_inputs(opt, tocg, batch)                # train_generator.py:503-574
                z = noise[k] if per_batch else noise
                output = generator(x, parse7, noise=z) if z is not None else generator(x, parse7)      # :576
                dists.append(lpips.forward_resized(batch["image"], output).reshape(-1)[:take])           # :578
                done += take
    finally:
        for m, was in modes:
            m.train(was)
    if not dists:
        return {"lpips": float("nan"), "items": 0, "distances": torch.zeros(0)}
    d = torch.cat(dists).cpu()
    return {"lpips": float(d.double().mean()), "items": done, "distances": d}


def _summary_writer_class():
    try:
        from tensorboardX import SummaryWriter          # the reference's (train_condition.py:11)
        return SummaryWriter
    except ImportError:
        pass
    try:
        from torch.utils.tensorboard import SummaryWriter
        return SummaryWriter
    except ImportError:
        return None


class ScalarLog(object):
    """Scalars of a run: one JSON line {"tag", "value", "step"} per record appended to ``<dir>/scalars.jsonl`` (``dir`` is the
    reference's ``<tensorboard_dir>/<name>``), and forwarded to a ``SummaryWriter(log_dir=dir)`` under the same tag where
    tensorboardX or torch.utils.tensorboard is importable.  Nothing is created before the first record."""

    FILE = "scalars.jsonl"

    def __init__(self, dir: str):
        self.dir = dir
        self.path = os.path.join(dir, self.FILE)
        self._board = None
        self._board_tried = False

    def add_scalar(self, tag: str, value, step: int):
        os.makedirs(self.dir, exist_ok=True)
        with open(self.path, "a") as f:
            f.write(json.dumps({"tag": tag, "value": float(value), "step": int(step)}) + "\n")
        board = self._writer()
        if board is not None:
            board.add_scalar(tag, float(value), int(step))

    def _writer(self):
        """The run's SummaryWriter, made at the first record; None where neither package imports."""
        if not self._board_tried:
            self._board_tried = True
            cls = _summary_writer_class()
            self._board = cls(log_dir=self.dir) if cls is not None else None
        return self._board

    def close(self):
        if self._board is not None:
            self._board.close()
            self._board = None
            self._board_tried = False


def read_scalars(dir: str):
    """The records of ``<dir>/scalars.jsonl`` (an empty list when there is none)."""
    path = os.path.join(dir, ScalarLog.FILE)
    if not os.path.exists(path):
        return []
    with open(path) as f:
        return [json.loads(line) for line in f if line.strip()]


def val_items_loader(opt, limit: int, batch_size: int):
    """The first ``min(limit, len)`` items of ``CPDatasetTest`` over ``--test_dataroot`` / ``--test_data_list`` (datamode 'test',
    train_condition.py:463-472, train_generator.py:613-619) in order, no shuffle.  Returns (DataLoader, item count)."""
    import copy
    from .cp_dataset import CPDatasetTest
    o = copy.copy(opt)
    o.dataroot, o.datamode, o.data_list = opt.test_dataroot, "test", opt.test_data_list
    ds = CPDatasetTest(o)
    n = min(int(limit), len(ds))
    sub = torch.utils.data.Subset(ds, range(n))
    return torch.utils.data.DataLoader(sub, batch_size=batch_size, shuffle=False, num_workers=opt.workers, drop_last=False), n


ALEXNET_FILE = "alexnet-owt-7be5be79.pth"


def default_alexnet_weights() -> str:
    """torch's hub-cache file of torchvision's AlexNet (evaluate.py's default); read only if present."""
    return os.path.join(torch.hub.get_dir(), "checkpoints", ALEXNET_FILE)


def load_validation_lpips(opt):
    """``PerceptualLoss(model='net-lin', net='alex')`` for the ``test/LPIPS`` pass from ``--lpips_weights`` / ``--alexnet_weights``
    (files only; nothing is downloaded), randomly initialised with a labelled warning under ``--lpips_random_init`` /
    ``--synthetic``, or None -- with one note -- when the weights are missing: a training run does not stop for its validation."""
    alex = opt.alexnet_weights or default_alexnet_weights()
    have = os.path.isfile(opt.lpips_weights) and os.path.isfile(alex)
    if not have and not (opt.lpips_random_init or getattr(opt, "synthetic", False)):
        print("NOTE: test/LPIPS is skipped: the LPIPS v0.1 lin layers (--lpips_weights, now %r) or torchvision's AlexNet "
              "(--alexnet_weights, now %r) are missing and nothing is downloaded; pass --lpips_random_init for plumbing runs"
              % (opt.lpips_weights, alex), flush=True)
        return None
    from .eval_models import PerceptualLoss
    with torch.random.fork_rng(devices=[]):         # the random initialisation must not move the training run's CPU stream
        torch.manual_seed(1234)
        model = PerceptualLoss(model="net-lin", net="alex", use_gpu=True)
    if have:
        model.load_torchvision_alexnet(torch.load(alex, map_location="cpu"))
        model.load_lpips_weights(torch.load(opt.lpips_weights, map_location="cpu"))
    else:
        print("WARNING: test/LPIPS runs on RANDOMLY initialised AlexNet / lin weights (--lpips_random_init / --synthetic): the "
              "score is not the paper's metric; pass --lpips_weights and --alexnet_weights for real training.", file=sys.stderr,
              flush=True)
    model.eval()
    return model
