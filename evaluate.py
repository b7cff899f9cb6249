#!/usr/bin/env python3
"""Drop-in for the reference's ``evaluate.py`` (same flags, same pairing, same output files): SSIM, MSE and LPIPS of a folder
of try-on outputs against the ground-truth photos and the Inception Score of the outputs, computed on the MI355X-native kernels
(csrc/metrics.hip, csrc/inception.hip + the fp32 conv engine for LPIPS's AlexNet and the score's Inception-v3).

Decoding and resizing stay on the CPU in DataLoader workers (data loading, like cp_dataset); the metrics run on the GPU in
batches.  Differences from the reference script:
  * LPIPS weights are read from files, never downloaded: ``--lpips_weights`` (the v0.1 ``alex.pth``, default the reference's
    location) and ``--alexnet_weights`` (torchvision's AlexNet state dict, default torch's hub-cache file).  Missing weights
    stop the run unless ``--lpips_random_init`` is given (plumbing only; the output says so).
  * the Inception Score needs torchvision's pretrained Inception-v3 state dict, read from a file and never downloaded:
    ``--inception_weights`` (default: torch's hub-cache file).  Without the file the score is not computed and is written as nan;
    ``--inception_random_init`` computes it on seeded random weights instead (plumbing only; the output says so).
    ``--is_splits`` is the reference's constant ``splits = 1``.
  * the reference sizes its array of Inception predictions by the number of ground-truth files, so a ground-truth folder with
    more files than predictions leaves zero rows and its score is nan.  Here the predictions there are get scored, and a note is
    printed when the two counts differ.
  * MSE is written as a plain float (the reference's f-string prints the CUDA tensor).
  * non-image files in --predict_dir (e.g. the lpips.txt / eval.txt of an earlier run) are skipped.
  * ``--fid`` adds what the paper reports for the unpaired setting and the reference script does not compute: FID and KID between
    ALL images of --predict_dir and ALL images of --ground_truth_dir (no pairing), on pytorch-fid's Inception-v3
    (``--fid_inception_weights``, default torch's hub-cache ``pt_inception-2015-12-05-6726825d.pth``, never downloaded; without the
    file the values are written as nan, ``--fid_random_init`` runs on seeded random weights and says so) with torch-fidelity's KID
    subsets (``--kid_subsets`` x ``--kid_subset_size``).  One more line goes to eval.txt.  ``--fid_only`` computes nothing else: no
    pairing, no LPIPS weights, lpips.txt untouched.  The workers only decode for this metric; the 299x299 resize is the input kernel's.
  * ``--prdc`` adds improved precision / recall (Kynkaanniemi et al. 2019) and density / coverage (Naeem et al. 2020) between the same
    two image sets on the same features and weights flags as ``--fid`` (``--prdc_k`` neighbours, default 5; hr_viton_amd/manifold.py):
    they separate the loss of fidelity from the loss of diversity that FID and KID merge.  One more line goes to eval.txt.  With
    ``--fid`` or ``--fid_only`` the feature banks are computed once and scored by both; ``--fid_only --prdc`` writes the two unpaired
    lines and nothing paired.
The reference's quirk of dividing the three averages by the number of ground-truth files is kept, so the numbers stay
comparable; a note is printed when that count differs from the number of predictions.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

IMAGE_EXT = (".jpg", ".jpeg", ".png", ".bmp", ".webp", ".tif", ".tiff")
ALEXNET_FILE = "alexnet-owt-7be5be79.pth"
INCEPTION_FILES = ("inception_v3_google-0cc3c7bd.pth", "inception_v3_google-1a9a5a14.pth")    # torchvision's, newer release first
FID_INCEPTION_FILE = "pt_inception-2015-12-05-6726825d.pth"                                   # pytorch-fid's / torch-fidelity's
PRDC_K_MAX = 16                                                                               # the library's hrv_row_kth_max()


def _default_alexnet_weights():
    return os.path.join(torch.hub.get_dir(), "checkpoints", ALEXNET_FILE)


def _default_inception_weights():
    """The first of torchvision's two file names that exists in torch's hub cache (else the first name, which then does not exist)."""
    paths = [os.path.join(torch.hub.get_dir(), "checkpoints", f) for f in INCEPTION_FILES]
    return next((p for p in paths if os.path.isfile(p)), paths[0])


def _parser():
    p = argparse.ArgumentParser()
    p.add_argument("--evaluation", default="LPIPS", help="parsed and unused, as in the reference")
    p.add_argument("--predict_dir", default="./result/bg_ver1/output/")
    p.add_argument("--ground_truth_dir", default="./data/zalando-hd-resize/test/image")
    p.add_argument("--resolution", type=int, default=1024, choices=[1024, 512, 256])
    p.add_argument("--lpips_weights", default="./eval_models/weights/v0.1/alex.pth", help="LPIPS v0.1 lin layers (alex.pth)")
    p.add_argument("--alexnet_weights", default=None,
                   help="torchvision alexnet state dict (default: torch's hub cache, %s; read only if present)" % ALEXNET_FILE)
    p.add_argument("--lpips_random_init", action="store_true",
                   help="plumbing only: LPIPS on randomly initialised AlexNet / lin weights (the output is labelled)")
    p.add_argument("--inception_weights", default=None,
                   help="torchvision inception_v3 state dict for the Inception Score (default: torch's hub cache, %s; without the "
                        "file the score is written as nan)" % " or ".join(INCEPTION_FILES))
    p.add_argument("--inception_random_init", action="store_true",
                   help="plumbing only: the Inception Score on a randomly initialised Inception-v3 (the output is labelled)")
    p.add_argument("--is_splits", type=int, default=1, help="splits of the Inception Score (the reference's constant 1)")
    p.add_argument("--seed", type=int, default=0,
                   help="torch seed of the random initialisations (--lpips_random_init, --inception_random_init)")
    p.add_argument("-j", "--workers", type=int, default=4)
    p.add_argument("-b", "--batch-size", type=int, default=16)
    p.add_argument("--fid", action="store_true",
                   help="also score FID and KID between all images of --predict_dir and all of --ground_truth_dir (no pairing)")
    p.add_argument("--fid_only", action="store_true", help="FID and KID alone: no pairing, no SSIM / MSE / LPIPS / IS")
    p.add_argument("--fid_inception_weights", default=None,
                   help="the FID Inception-v3 state dict (default: torch's hub cache, %s; without the file the values are written "
                        "as nan)" % FID_INCEPTION_FILE)
    p.add_argument("--fid_random_init", action="store_true",
                   help="plumbing only: FID / KID on a randomly initialised network (the output is labelled)")
    p.add_argument("--kid_subsets", type=int, default=100, help="KID subsets (torch-fidelity's default)")
    p.add_argument("--kid_subset_size", type=int, default=1000, help="images per KID subset (torch-fidelity's default)")
    p.add_argument("--prdc", action="store_true",
                   help="also score precision / recall / density / coverage between all images of --predict_dir and all of "
                        "--ground_truth_dir, on the FID network's features (its weights flags apply)")
    p.add_argument("--prdc_k", type=int, default=5, help="nearest neighbours of --prdc (prdc's default; 1 .. %d)" % PRDC_K_MAX)
    return p


def get_opt(argv=None):
    p = _parser()
    opt = p.parse_args(argv)
    if opt.alexnet_weights is None:
        opt.alexnet_weights = _default_alexnet_weights()
    if opt.inception_weights is None:
        opt.inception_weights = _default_inception_weights()
    if opt.is_splits < 1:
        p.error("--is_splits must be at least 1")
    if opt.fid_inception_weights is None:
        opt.fid_inception_weights = os.path.join(torch.hub.get_dir(), "checkpoints", FID_INCEPTION_FILE)
    if opt.kid_subsets < 1 or opt.kid_subset_size < 2:
        p.error("--kid_subsets must be at least 1 and --kid_subset_size at least 2")
    if not 1 <= opt.prdc_k <= PRDC_K_MAX:
        p.error("--prdc_k must lie in 1 .. %d" % PRDC_K_MAX)
    return opt


def gt_name(pred_name: str) -> str:
    """evaluate.py:54 -- the ground truth of prediction ``P`` is ``P.split('_')[0] + '_00.jpg'``."""
    return pred_name.split("_")[0] + "_00.jpg"


def list_predictions(predict_dir: str):
    return sorted(f for f in os.listdir(predict_dir) if f.lower().endswith(IMAGE_EXT))


def _rgb(img: Image.Image) -> np.ndarray:
    return np.asarray(img if img.mode == "RGB" else img.convert("RGB"), dtype=np.uint8)


class PairDataset(torch.utils.data.Dataset):
    """One prediction and its ground truth as decoded: full-size RGB uint8 (SSIM / MSE), the 128x128 resizes (LPIPS) and, with
    ``with_is``, the prediction's 299x299 resize (Inception Score)."""

    def __init__(self, opt, pred_list, with_is=False):
        self.opt, self.pred_list, self.with_is = opt, pred_list, with_is

    def __len__(self):
        return len(self.pred_list)

    def __getitem__(self, i):
        opt, name = self.opt, self.pred_list[i]
        gt_img = Image.open(os.path.join(opt.ground_truth_dir, gt_name(name)))
        if opt.resolution != 1024:
            if opt.resolution == 512:
                gt_img = gt_img.resize((384, 512), Image.BILINEAR)
            elif opt.resolution == 256:
                gt_img = gt_img.resize((192, 256), Image.BILINEAR)
            else:
                raise NotImplementedError(opt.resolution)
        pred_img = Image.open(os.path.join(opt.predict_dir, name))
        assert gt_img.size == pred_img.size, f"{gt_img.size} vs {pred_img.size}"
        item = {"name": name, "gt": _rgb(gt_img), "pred": _rgb(pred_img),
                "gt128": _rgb(gt_img.resize((128, 128), Image.BILINEAR)),        # Transforms.Resize((128, 128)) on a PIL image
                "pred128": _rgb(pred_img.resize((128, 128), Image.BILINEAR))}
        if self.with_is:
            item["pred299"] = _rgb(pred_img.resize((299, 299), Image.BILINEAR))  # Transforms.Resize((299, 299)), evaluate.py:34
        return item


def load_lpips(opt):
    """PerceptualLoss(model='net-lin', net='alex') with its weights, or SystemExit when they are missing."""
    have = os.path.isfile(opt.lpips_weights) and os.path.isfile(opt.alexnet_weights)
    if not have and not opt.lpips_random_init:
        raise SystemExit("LPIPS needs the pretrained weights: the LPIPS v0.1 lin layers (--lpips_weights, now %r) and torchvision's "
                         "AlexNet (--alexnet_weights, now %r); nothing is downloaded. Pass --lpips_random_init for plumbing runs"
                         % (opt.lpips_weights, opt.alexnet_weights))
    import hr_viton_amd  # noqa: F401
    from hr_viton_amd.eval_models import PerceptualLoss
    torch.manual_seed(opt.seed)
    model = PerceptualLoss(model="net-lin", net="alex", use_gpu=True)
    if have:
        model.load_torchvision_alexnet(torch.load(opt.alexnet_weights, map_location="cpu"))
        model.load_lpips_weights(torch.load(opt.lpips_weights, map_location="cpu"))
    else:
        print("WARNING: LPIPS runs on RANDOMLY initialised AlexNet / lin weights (--lpips_random_init): the score is not "
              "the paper's metric", file=sys.stderr, flush=True)
    model.eval()
    return model, not have


def load_inception(opt):
    """(Inception3 or None, random_init): torchvision's inception_v3 from ``--inception_weights``; seeded random weights with
    ``--inception_random_init`` when the file is missing; None when there is neither (the score is then written as nan)."""
    have = os.path.isfile(opt.inception_weights)
    if not have and not opt.inception_random_init:
        return None, False
    import hr_viton_amd  # noqa: F401
    from hr_viton_amd.inception import Inception3
    torch.manual_seed(opt.seed)
    model = Inception3(transform_input=False)
    if have:
        model.load_state_dict(torch.load(opt.inception_weights, map_location="cpu"))
    else:
        print("WARNING: the Inception Score runs on a RANDOMLY initialised Inception-v3 (--inception_random_init): it is not "
              "the paper's metric", file=sys.stderr, flush=True)
    model.eval()
    return model, not have


class InceptionScorer:
    """softmax(inception_v3(pred299)) of a loader batch as float64 rows [n, 1000] on the host (evaluate.py:76)."""

    def __init__(self, model):
        self.model = model
        self.dev = torch.device("cuda")

    def __call__(self, batch):
        x = torch.from_numpy(np.stack([it["pred299"] for it in batch])).pin_memory().to(self.dev, non_blocking=True)
        return self.model.forward_u8(x).cpu().numpy().astype(np.float64)


def inception_score(preds, splits=1):
    """evaluate.py:97-106 in float64: per split ``exp(mean_i KL(p_i || p_mean))`` with ``scipy.stats.entropy(pk, qk)``'s
    normalisation of both arguments (terms with p == 0 contribute 0); returns (mean, std) over the splits."""
    preds = np.asarray(preds, dtype=np.float64)
    n = (preds.shape[0] if preds.ndim == 2 else 0) // splits
    if n < 1:
        return float("nan"), float("nan")
    split_scores = []
    for k in range(splits):
        part = preds[k * n:(k + 1) * n, :]
        py = np.mean(part, axis=0)
        q = py / py.sum()
        scores = []
        for i in range(part.shape[0]):
            p = part[i, :] / part[i, :].sum()
            nz = p > 0
            scores.append(float(np.sum(p[nz] * np.log(p[nz] / q[nz]))))
        split_scores.append(np.exp(np.mean(scores)))
    return float(np.mean(split_scores)), float(np.std(split_scores))


class GpuScorer:
    """(ssim, mse, lpips) per pair of a loader batch: pair statistics per image size, LPIPS over the batch."""

    def __init__(self, model):
        from hr_viton_amd import metrics
        self.model, self.metrics = model, metrics
        self.dev = torch.device("cuda")

    def _up(self, arrs):
        return torch.from_numpy(np.stack(arrs)).pin_memory().to(self.dev, non_blocking=True)

    def __call__(self, batch):
        n = len(batch)
        ssim, mse = [0.0] * n, [0.0] * n
        groups = {}
        for i, it in enumerate(batch):
            groups.setdefault(it["gt"].shape, []).append(i)
        outs = []
        for idx in groups.values():
            s, m = self.metrics.pair_stats(self._up([batch[i]["gt"] for i in idx]), self._up([batch[i]["pred"] for i in idx]))
            outs.append((idx, s, m))
        # evaluate.py:72: model.forward(gt, pred)
        lp = self.model.forward_u8(self._up([it["gt128"] for it in batch]), self._up([it["pred128"] for it in batch]))
        for idx, s, m in outs:
            s, m = s.cpu().tolist(), m.cpu().tolist()
            for j, i in enumerate(idx):
                ssim[i], mse[i] = s[j], m[j]
        return list(zip(ssim, mse, [float(v) for v in lp.cpu().tolist()]))


# ------------------------------------------------------------------------------------------------------------------ FID / KID
class ImageDataset(torch.utils.data.Dataset):
    """Images of one folder as decoded, RGB uint8; ``resolution``: the ground truths' resize of the paired path (512, 256) or None."""

    def __init__(self, folder, names, resolution=None):
        self.folder, self.names, self.resolution = folder, names, resolution

    def __len__(self):
        return len(self.names)

    def __getitem__(self, i):
        img = Image.open(os.path.join(self.folder, self.names[i]))
        if self.resolution == 512:
            img = img.resize((384, 512), Image.BILINEAR)
        elif self.resolution == 256:
            img = img.resize((192, 256), Image.BILINEAR)
        return {"name": self.names[i], "img": _rgb(img)}


def load_fid_inception(opt):
    """(FIDInceptionV3 or None, random_init), as load_inception: the file, else seeded random weights when asked, else None."""
    have = os.path.isfile(opt.fid_inception_weights)
    if not have and not opt.fid_random_init:
        return None, False
    import hr_viton_amd  # noqa: F401
    from hr_viton_amd.inception import FIDInceptionV3
    torch.manual_seed(opt.seed)
    model = FIDInceptionV3()
    if have:
        model.load_state_dict(torch.load(opt.fid_inception_weights, map_location="cpu"))
    else:
        print("WARNING: FID / KID run on a RANDOMLY initialised Inception-v3 (--fid_random_init): they are not the paper's metrics",
              file=sys.stderr, flush=True)
    model.eval()
    return model, not have


class FidScorer:
    """The GPU side of --fid: two feature banks that stay on the device, rows filled batch by batch, and their statistics."""

    WIDTH = 2048

    def __init__(self, model):
        from hr_viton_amd import feat_stats
        self.model, self.stats = model, feat_stats
        self.dev = torch.device("cuda")

    def bank(self, n):
        return torch.empty((n, self.WIDTH), dtype=torch.float32, device=self.dev)

    def fill(self, bank, row0, batch):
        """features of a loader batch into bank[row0 : row0 + len(batch)]; images of one size go through the network together"""
        groups = {}
        for i, it in enumerate(batch):
            groups.setdefault(it["img"].shape, []).append(i)
        for idx in groups.values():
            x = torch.from_numpy(np.stack([batch[i]["img"] for i in idx])).pin_memory().to(self.dev, non_blocking=True)
            if len(groups) == 1:
                self.model.features_u8(x, out=bank[row0:row0 + len(batch)])
            else:
                bank[torch.as_tensor(idx, device=self.dev) + row0] = self.model.features_u8(x)

    def score(self, bank_pred, bank_gt, subsets, subset_size):
        return self.stats.fid_kid(bank_pred, bank_gt, subsets, subset_size)

    def prdc(self, bank_pred, bank_gt, k):
        """dict(precision, recall, density, coverage, ...): the ground truths are the real bank, the predictions the fake one"""
        from hr_viton_amd import manifold
        return manifold.prdc(bank_gt, bank_pred, k)


def feature_banks(opt, pred_list, gt_images, fid_scorer):
    """The two feature banks (predictions, ground truths) of the unpaired metrics, filled batch by batch."""
    banks = []
    for folder, names, res in ((opt.predict_dir, pred_list, None),
                               (opt.ground_truth_dir, gt_images, opt.resolution if opt.resolution != 1024 else None)):
        loader = torch.utils.data.DataLoader(ImageDataset(folder, names, res), batch_size=max(1, opt.batch_size), shuffle=False,
                                             num_workers=opt.workers, collate_fn=list)
        bank, row = fid_scorer.bank(len(names)), 0
        for batch in loader:
            fid_scorer.fill(bank, row, batch)
            row += len(batch)
        banks.append(bank)
    return banks


def write_fid(predict_dir, fid, kid_mean, kid_std, random_init=False):
    with open(os.path.join(predict_dir, "eval.txt"), "a") as f:
        f.write(f"FID : {fid} / KID_mean : {kid_mean} / KID_std : {kid_std}\n")
        if random_init:
            f.write("FID Inception weights : random init (plumbing only)\n")


def write_prdc(predict_dir, precision, recall, density, coverage, k, random_init=False):
    with open(os.path.join(predict_dir, "eval.txt"), "a") as f:
        f.write(f"Precision : {precision} / Recall : {recall} / Density : {density} / Coverage : {coverage} / k : {k}\n")
        if random_init:
            f.write("FID Inception weights : random init (plumbing only)\n")


def run_fid(opt, pred_list, fid_scorer=None):
    """The unpaired part of main() -- FID / KID under --fid or --fid_only, precision / recall / density / coverage under --prdc, both
    on one pair of feature banks: returns the dict entries and the timings and writes eval.txt's extra line(s)."""
    with_fid, with_prdc = opt.fid or opt.fid_only, opt.prdc
    gt_images = list_predictions(opt.ground_truth_dir)
    if with_fid and opt.kid_subset_size > min(len(pred_list), len(gt_images)):
        _parser().error(f"--kid_subset_size {opt.kid_subset_size} is larger than an image set: {len(pred_list)} predictions in "
                        f"{opt.predict_dir}, {len(gt_images)} ground truths in {opt.ground_truth_dir}")
    if with_prdc and opt.prdc_k > min(len(pred_list), len(gt_images)) - 1:
        _parser().error(f"--prdc_k {opt.prdc_k} is larger than an image set minus one: {len(pred_list)} predictions in "
                        f"{opt.predict_dir}, {len(gt_images)} ground truths in {opt.ground_truth_dir}")
    random_init = fid_scorer is not None and opt.fid_random_init
    if fid_scorer is None:
        model, random_init = load_fid_inception(opt)
        if model is not None:
            fid_scorer = FidScorer(model)
    what = " / ".join(n for n, on in (("FID / KID", with_fid), ("precision / recall / density / coverage", with_prdc)) if on)
    res, timings, banks = {}, {}, None
    if fid_scorer is None:
        print("%s: not computed (they need the FID Inception-v3: --fid_inception_weights, now %r, does not exist and nothing "
              "is downloaded; --fid_random_init for plumbing runs): written as nan" % (what, opt.fid_inception_weights), file=sys.stderr)
    else:
        print("Calculate %s..." % ("FID, KID" if with_fid else "precision, recall, density, coverage"))
        t0 = time.perf_counter()
        with torch.no_grad():
            banks = feature_banks(opt, pred_list, gt_images, fid_scorer)
        timings["fid_features_s"] = time.perf_counter() - t0
    if with_fid:
        fid = kid_mean = kid_std = float("nan")
        if banks is not None:
            t1 = time.perf_counter()
            with torch.no_grad():
                fid, kid_mean, kid_std = (float(v) for v in fid_scorer.score(banks[0], banks[1], opt.kid_subsets, opt.kid_subset_size))
            timings["fid_stats_s"] = time.perf_counter() - t1
        write_fid(opt.predict_dir, fid, kid_mean, kid_std, random_init)
        print("FID : %f / KID_mean : %f / KID_std : %f" % (fid, kid_mean, kid_std))
        if random_init:
            print("(FID / KID from randomly initialised weights: plumbing only)")
        res.update({"fid": fid, "kid_mean": kid_mean, "kid_std": kid_std, "fid_images": [len(pred_list), len(gt_images)]})
    if with_prdc:
        vals = dict.fromkeys(("precision", "recall", "density", "coverage"), float("nan"))
        if banks is not None:
            t1 = time.perf_counter()
            with torch.no_grad():
                got = fid_scorer.prdc(banks[0], banks[1], opt.prdc_k)
            vals = {key: float(got[key]) for key in vals}
            timings["prdc_s"] = time.perf_counter() - t1
        write_prdc(opt.predict_dir, vals["precision"], vals["recall"], vals["density"], vals["coverage"], opt.prdc_k, random_init)
        print("Precision : %f / Recall : %f / Density : %f / Coverage : %f / k : %d"
              % (vals["precision"], vals["recall"], vals["density"], vals["coverage"], opt.prdc_k))
        if random_init:
            print("(precision / recall / density / coverage from randomly initialised weights: plumbing only)")
        res.update(vals, prdc_k=opt.prdc_k)
    return res, timings


def write_results(predict_dir, lpips_list, avg_ssim, avg_mse, avg_distance, is_mean, is_std, random_init=False,
                  inception_random_init=False):
    lpips_list = sorted(lpips_list, key=lambda x: x[1], reverse=True)
    with open(os.path.join(predict_dir, "lpips.txt"), "a") as f:
        for name, score in lpips_list:
            f.write(f"{name} {score}\n")
    with open(os.path.join(predict_dir, "eval.txt"), "a") as f:
        f.write(f"SSIM : {avg_ssim} / MSE : {avg_mse} / LPIPS : {avg_distance}\n")
        f.write(f"IS_mean : {is_mean} / IS_std : {is_std}\n")
        if random_init:
            f.write("LPIPS weights : random init (plumbing only)\n")
        if inception_random_init:
            f.write("Inception weights : random init (plumbing only)\n")


def evaluation(opt, pred_list, gt_list, scorer, is_scorer=None):
    """evaluate.py:28-114 up to the score itself.  Returns (avg_ssim, avg_mse, avg_distance, lpips_list, timings); with an
    ``is_scorer`` the Inception predictions of all pairs, float64 [pairs, 1000] in loader order, are ``timings["inception_preds"]``
    (main() takes them out again) and the time spent on them ``timings["inception_s"]``."""
    loader = torch.utils.data.DataLoader(PairDataset(opt, pred_list, with_is=is_scorer is not None),
                                         batch_size=max(1, opt.batch_size), shuffle=False, num_workers=opt.workers, collate_fn=list)
    preds, t_is = [], 0.0
    sum_ssim = sum_mse = sum_dist = 0.0
    lpips_list = []
    t_wait = t_gpu = 0.0
    print("Calculate SSIM, MSE, LPIPS...")
    step = 0
    it = iter(loader)
    while True:
        t0 = time.perf_counter()
        batch = next(it, None)
        t1 = time.perf_counter()
        t_wait += t1 - t0
        if batch is None:
            break
        res = scorer(batch)
        t_gpu += time.perf_counter() - t1
        if is_scorer is not None:
            t2 = time.perf_counter()
            preds.append(np.asarray(is_scorer(batch), dtype=np.float64))
            t_is += time.perf_counter() - t2
        for item, (s, m, d) in zip(batch, res):
            step += 1
            sum_ssim += s
            sum_mse += m
            sum_dist += d
            lpips_list.append((item["name"], d))
            print(f"step: {step} evaluation... lpips:{d}")
    n = len(gt_list)
    if n != len(pred_list):
        print(f"note: averages are divided by the number of ground-truth files ({n}), as in the reference, not by the number "
              f"of predictions ({len(pred_list)})", file=sys.stderr)
    timings = {"loader_wait_s": t_wait, "gpu_s": t_gpu}
    if is_scorer is not None:
        timings["inception_s"] = t_is
        timings["inception_preds"] = np.concatenate(preds, axis=0) if preds else np.zeros((0, 1000))
    return sum_ssim / n, sum_mse / n, sum_dist / n, lpips_list, timings


def main(argv=None, scorer=None, is_scorer=None, fid_scorer=None):
    """``scorer`` / ``is_scorer`` / ``fid_scorer``: stand-ins for GpuScorer / InceptionScorer / FidScorer (tests).  With a ``scorer``
    and no ``is_scorer`` nothing is loaded and the Inception Score is nan."""
    opt = get_opt(argv)
    pred_list = list_predictions(opt.predict_dir)
    if opt.fid_only:
        res, timings = run_fid(opt, pred_list, fid_scorer)
        res["timings"] = timings
        return res
    gt_list = sorted(os.listdir(opt.ground_truth_dir))
    random_init = False
    is_random_init = is_scorer is not None and opt.inception_random_init
    if scorer is None:
        model, random_init = load_lpips(opt)
        scorer = GpuScorer(model)
        if is_scorer is None:
            inception, is_random_init = load_inception(opt)
            if inception is not None:
                is_scorer = InceptionScorer(inception)
    t0 = time.perf_counter()
    with torch.no_grad():
        avg_ssim, avg_mse, avg_distance, lpips_list, timings = evaluation(opt, pred_list, gt_list, scorer, is_scorer)
    timings["total_s"] = time.perf_counter() - t0
    preds = timings.pop("inception_preds", None)
    print("Calculate Inception Score...")
    if preds is None:
        print("Inception Score: not computed (it needs a pretrained Inception-v3: --inception_weights, now %r, does not exist and "
              "nothing is downloaded; --inception_random_init for plumbing runs): written as nan" % opt.inception_weights,
              file=sys.stderr)
        is_mean = is_std = float("nan")
    else:
        if len(gt_list) != len(pred_list):
            print(f"note: the Inception Score is computed over the {len(pred_list)} predictions; the reference sizes its array by "
                  f"the number of ground-truth files ({len(gt_list)}) and would score the zero rows that leaves as nan",
                  file=sys.stderr)
        is_mean, is_std = inception_score(preds, opt.is_splits)
    write_results(opt.predict_dir, lpips_list, avg_ssim, avg_mse, avg_distance, is_mean, is_std, random_init, is_random_init)
    print("SSIM : %f / MSE : %f / LPIPS : %f" % (avg_ssim, avg_mse, avg_distance))
    print("IS_mean : %f / IS_std : %f" % (is_mean, is_std))
    if random_init:
        print("(LPIPS from randomly initialised weights: plumbing only)")
    if is_random_init:
        print("(Inception Score from randomly initialised weights: plumbing only)")
    res = {"ssim": avg_ssim, "mse": avg_mse, "lpips": avg_distance, "is_mean": is_mean, "is_std": is_std, "pairs": len(pred_list),
           "timings": timings}
    if opt.fid or opt.prdc:
        fid_res, fid_timings = run_fid(opt, pred_list, fid_scorer)
        res.update(fid_res)
        timings.update(fid_timings)
    return res


if __name__ == "__main__":
    main()
