"""What the reference's scripts let their user look at, composed on the device: the image grids of test_generator.py:221-229,
test_condition.py:135-143, train_condition.py:377-381 / :430-435 and train_generator.py:365-370 / :471-476, ``utils.visualize_segmap``
and the quantisation of ``utils.save_images``.

The reference copies about twelve fp32 [3,H,W] tensors per sample to the host and runs ``visualize_segmap`` (numpy argmax + PIL
palette), torchvision ``make_grid`` and ``mul(255).add_(0.5).clamp_`` there.  Here one launch of csrc/viz.hip (``hrv_viz_grid_u8``)
gathers N grids from tensors that already sit on the device -- NCHW tensors, channel slices of wider ones, NHWC ``Act``s, masks --
through per-panel strides, with no layout conversion, no fp32 grid and no per-panel launch, and writes uint8 [N,Hg,Wg,3]: a quarter
of the bytes travel back.  ``grid_u8`` is the kernel's face, ``Panel`` one panel; ``tryon_grid``, ``condition_grid`` and
``generator_train_grid`` list the panels of the reference's call sites in its order; ``visualize_segmap``, ``save_images`` and
``save_image`` keep the reference's names; ``ImageWriter`` takes the PNG / JPEG encodes off the serving thread; ``BoardLog`` is
``validate.ScalarLog`` plus ``add_image``.

Bytes.  ``SIGNED`` is the reference's ``t / 2 + 0.5`` = ``(t + 1) / 2`` = the ``(t + 1) * 0.5`` of ``save_images`` (one fp32 number:
scaling by 2 commutes with rounding).  ``ROUND`` is torchvision ``save_image``'s ``mul(255).add_(0.5).clamp_(0, 255).to(uint8)``
(two roundings, then truncation: not round-half-even), ``TRUNC`` is ``(v * 255).clip(0, 255).astype(uint8)``: ``save_images`` and
tensorboard's float -> uint8 conversion.  A segmentation map's palette byte p survives ``ToTensor``'s p / 255 and either
quantisation unchanged, so ``SEGMAP`` panels emit the palette directly.

Stated deviations from the reference:

* The reference draws the test-visualisation batch of the training scripts from a shuffled loader; here it is the first
  ``--num_test_visualize`` items of the test list (``validate.val_items_loader``), or a fixed-seed synthetic batch under ``--synthetic``,
  so the series of ``test_images/{i}`` shows the same items over a run.  The pass draws its random numbers (the SPADE noise) from a
  forked generator: the training run's streams do not move.
* Under data parallelism rank 0 logs the losses of its own shard; no collective is added.
* ``misalign`` is float, not ``long``; the bytes are the same.
* ``train_generator.py --GT`` has no ``fake_parse_gauss`` (the reference's recording block would fail on the undefined name): the
  panel shows the ground-truth parse map.
* Board images are quantised with ``TRUNC``, which is what tensorboard does to the reference's float grid; the PNG under ``images/``
  and the event carry the same bytes.
"""
from __future__ import annotations

import os
import threading
from concurrent.futures import ThreadPoolExecutor
from typing import Dict, Optional, Sequence, Union

import numpy as np
import torch

from . import _lib
from ._lib import HrvError
from .ops import Act, _stream
from .validate import ScalarLog

SIGNED, UNIT, SEGMAP = _lib.VIZ_SIGNED, _lib.VIZ_UNIT, _lib.VIZ_SEGMAP
ROUND, TRUNC = _lib.VIZ_ROUND, _lib.VIZ_TRUNC
MAX_PANELS, MAX_CLASSES = _lib.HRV_VIZ_MAX_PANELS, _lib.HRV_VIZ_MAX_CLASSES

# utils.visualize_segmap's palette (utils.py:50-55): 20 colours
PALETTE = [0, 0, 0, 128, 0, 0, 254, 0, 0, 0, 85, 0, 169, 0, 51,
           254, 85, 0, 0, 0, 85, 0, 119, 220, 85, 85, 0, 0, 85, 85,
           85, 51, 0, 52, 86, 128, 0, 128, 0, 0, 0, 254, 51, 169, 220,
           0, 254, 254, 85, 254, 169, 169, 254, 85, 254, 254, 0, 254, 169, 0]


class Panel(object):
    """One panel of a grid: ``src`` is an fp32 CUDA tensor [N,C,H,W] in any strides (a channel slice ``x[:, 6:9]``, an expanded
    mask, ...) or an NHWC ``Act``; ``kind`` SIGNED / UNIT (C == 3, or C == 1: a mask shown as grey) or SEGMAP (1 <= C <= 20).  N == 1
    next to panels of a larger batch shows that sample in every grid (the reference's ``c_paired[0]`` panels).  Nothing is copied:
    the kernel reads ``src`` through its strides, so ``src`` must stay alive until ``grid_u8`` returns."""

    def __init__(self, src: Union[torch.Tensor, Act], kind: int):
        if kind not in (SIGNED, UNIT, SEGMAP):
            raise ValueError(f"Panel: kind {kind!r}")
        self.kind, self.src = kind, src
        if isinstance(src, Act):
            t = src.t
            if t.dim() != 4 or not t.is_contiguous():
                raise ValueError("Panel: an Act holds a contiguous [N,H,W,Cs] tensor")
            if src.coff + src.C > t.shape[3]:
                raise ValueError("Panel: Act slice outside its tensor")
            self.N, self.H, self.W, self.C = t.shape[0], t.shape[1], t.shape[2], src.C
            self.sn, self.sy, self.sx, self.sc = t.stride(0), t.stride(1), t.stride(2), 1
            off = src.coff
        elif torch.is_tensor(src):
            t = src
            if t.dim() != 4:
                raise ValueError(f"Panel: expected [N,C,H,W], got {tuple(t.shape)}")
            self.N, self.C, self.H, self.W = t.shape
            self.sn, self.sc, self.sy, self.sx = t.stride()
            off = 0
        else:
            raise TypeError(f"Panel: a tensor or an Act, not {type(src).__name__}")
        if not t.is_cuda:
            raise HrvError(f"viz.Panel: tensor is on {t.device}; the MI355X path has no CPU fallback")
        if t.dtype != torch.float32:
            raise HrvError(f"viz.Panel: expected float32, got {t.dtype}")
        if min(self.N, self.H, self.W) < 1:
            raise ValueError(f"Panel: empty tensor {tuple(t.shape)}")
        if kind == SEGMAP:
            if not 1 <= self.C <= MAX_CLASSES:
                raise ValueError(f"Panel: SEGMAP over {self.C} channels (1 .. {MAX_CLASSES})")
        elif self.C not in (1, 3):
            raise ValueError(f"Panel: SIGNED / UNIT take 1 or 3 channels, got {self.C}")
        if min(self.sn, self.sy, self.sx, self.sc) < 0:
            raise ValueError("Panel: negative strides")
        if self.N == 1:
            self.sn = 0
        self.device = t.device
        self.ptr = t.data_ptr() + 4 * off
        # The kernel reads a pixel as float4 groups where the channel stride is 1, the pointer is 16-byte aligned and the other
        # strides are multiples of 4: the channels rounded up to 4 must then lie inside the storage.  Acts do (their channel
        # stride is a multiple of 4); a dense channels-last view whose last pixel ends the allocation does not, and is shown
        # from an NCHW copy, which the kernel reads plane by plane.
        if self.sc == 1 and self.ptr % 16 == 0 and (self.sn | self.sy | self.sx) % 4 == 0:
            last = t.storage_offset() + off + (self.N - 1) * self.sn + (self.H - 1) * self.sy + (self.W - 1) * self.sx
            if last + (self.C + 3) // 4 * 4 > t.untyped_storage().nbytes() // 4:
                if isinstance(src, Act):
                    raise ValueError("Panel: the Act's channels, rounded up to 4, leave its tensor")
                self.src = t = t.contiguous(memory_format=torch.contiguous_format)
                self.sn, self.sc, self.sy, self.sx = t.stride()
                self.sn = 0 if self.N == 1 else self.sn
                self.ptr = t.data_ptr()


def grid_shape(n: int, H: int, W: int, nrow: int = 4, padding: int = 2):
    """(Hg, Wg) of torchvision's make_grid over n images of H x W; a single image comes back bare."""
    if n == 1:
        return H, W
    xmaps = min(nrow, n)
    ymaps = -(-n // xmaps)
    return ymaps * (H + padding) + padding, xmaps * (W + padding) + padding


def grid_u8(panels: Sequence[Panel], nrow: int = 4, padding: int = 2, quant: int = ROUND, count: Optional[int] = None) -> torch.Tensor:
    """torchvision ``make_grid(panels, nrow, padding, pad_value=0)`` of every sample, quantised: uint8 [N,Hg,Wg,3] on the device, in
    one launch.  ``count``: only the first ``count`` samples (``train_images`` shows sample 0; ``--num_test_visualize``)."""
    panels = list(panels)
    if not 1 <= len(panels) <= MAX_PANELS:
        raise ValueError(f"grid_u8: {len(panels)} panels (1 .. {MAX_PANELS})")
    if not all(isinstance(p, Panel) for p in panels):
        raise TypeError("grid_u8: a sequence of viz.Panel")
    p0 = panels[0]
    N = max(p.N for p in panels)
    for p in panels:
        if (p.H, p.W) != (p0.H, p0.W) or p.N not in (1, N) or p.device != p0.device:
            raise ValueError(f"grid_u8: panels of one size, batch and device, got {[(q.N, q.H, q.W) for q in panels]}")
    if count is not None:
        N = max(1, min(N, int(count)))
    Hg, Wg = grid_shape(len(panels), p0.H, p0.W, nrow, padding)
    out = torch.empty((N, Hg, Wg, 3), dtype=torch.uint8, device=p0.device)
    arr = (_lib.hrv_viz_panel_t * len(panels))()
    for d, p in zip(arr, panels):
        d.ptr, d.sn, d.sy, d.sx, d.sc, d.C, d.kind = p.ptr, p.sn, p.sy, p.sx, p.sc, p.C, p.kind
    lib = _lib.load()
    with torch.cuda.device(p0.device):
        _lib.check(lib.hrv_viz_grid_u8(arr, len(panels), nrow, padding, N, p0.H, p0.W, quant, out.data_ptr(), _stream()),
                   "hrv_viz_grid_u8")
    return out


def visualize_segmap(input, multi_channel: bool = True, tensor_out: bool = True, batch: int = 0) -> torch.Tensor:
    """utils.py:49-70 on the device: the [3,H,W] float tensor (palette byte / 255) of sample ``batch`` of an NCHW score tensor or an
    NHWC ``Act``."""
    if not multi_channel or not tensor_out:
        raise NotImplementedError("visualize_segmap: multi_channel=False / tensor_out=False are used by no script")
    if isinstance(input, Act):
        src = Act(input.t[batch:batch + 1], input.C, input.coff)
    else:
        src = input.detach()[batch:batch + 1]
    u8 = grid_u8([Panel(src, SEGMAP)])
    # ToTensor's byte / 255, looked up in a table divided on the host: a device division by a scalar is a multiplication by its
    # reciprocal, which rounds 126 of the 256 quotients differently
    lut = torch.arange(256, dtype=torch.float32).div(255).to(u8.device)
    return lut[u8[0].permute(2, 0, 1).long()]


def to_host(u8: torch.Tensor) -> np.ndarray:
    """A device uint8 tensor as a numpy array, through a pinned buffer."""
    if not u8.is_cuda:
        return u8.contiguous().numpy()
    host = torch.empty(u8.shape, dtype=u8.dtype, pin_memory=True)
    host.copy_(u8, non_blocking=True)
    torch.cuda.current_stream(u8.device).synchronize()
    return host.numpy()


# ------------------------------------------------------------------------------------------------ files
def _encode(arr: np.ndarray, path: str, fmt: str):
    from PIL import Image
    Image.fromarray(arr).save(path, format=fmt)


class ImageWriter(object):
    """A bounded pool of ``workers`` threads (at most 4; 0: encode in the caller) for the PIL encodes: a 1024x768 grid is about 28 MB
    raw and its PNG encode would otherwise serialise the loop that produced it.  Every job owns its host array.  ``close()`` waits
    for the jobs and re-raises the first exception one of them met; a ``write`` after ``close`` encodes in the caller."""

    MAX_WORKERS = 4

    def __init__(self, workers: int = 0, pending: Optional[int] = None):
        if not 0 <= workers <= self.MAX_WORKERS:
            raise ValueError(f"ImageWriter: workers {workers} (0 .. {self.MAX_WORKERS})")
        self.workers = workers
        self._pool = ThreadPoolExecutor(max_workers=workers) if workers else None
        self._slots = threading.BoundedSemaphore(pending or 2 * workers) if workers else None
        self._lock = threading.Lock()
        self._error = None

    def _run(self, arr, path, fmt):
        try:
            _encode(arr, path, fmt)
        except BaseException as e:                # kept for close()
            with self._lock:
                if self._error is None:
                    self._error = e
        finally:
            self._slots.release()

    def write(self, arr: np.ndarray, path: str, fmt: str = "PNG"):
        if self._pool is None:
            _encode(arr, path, fmt)
            return
        self._slots.acquire()                     # bounded: at most `pending` arrays wait in memory
        try:
            self._pool.submit(self._run, arr, path, fmt)
        except BaseException:
            self._slots.release()
            raise

    def close(self):
        if self._pool is not None:
            self._pool.shutdown(wait=True)
            self._pool = None
        err, self._error = self._error, None
        if err is not None:
            raise err

    def __enter__(self):
        return self

    def __exit__(self, et, ev, tb):
        if et is None:
            self.close()
        elif self._pool is not None:
            self._pool.shutdown(wait=True)
            self._pool = None
        return False


def save_image(grid, path: str, writer: Optional[ImageWriter] = None):
    """One uint8 [H,W,3] (or [H,W]) image -- a row of ``grid_u8``'s result, on the device or not -- as a PNG through PIL."""
    arr = to_host(grid) if torch.is_tensor(grid) else np.asarray(grid)
    if arr.dtype != np.uint8:
        raise ValueError(f"save_image: uint8 expected, got {arr.dtype}")
    if writer is None:
        _encode(arr, path, "PNG")
    else:
        writer.write(np.array(arr), path, "PNG")        # the job owns its array


def quantize_images(img_tensors: torch.Tensor) -> torch.Tensor:
    """``save_images``' ``((t + 1) * 0.5 * 255).clamp(0, 255)`` truncated to uint8, by the kernel: [N,C,H,W] -> uint8 [N,H,W,3]."""
    return grid_u8([Panel(img_tensors, SIGNED)], quant=TRUNC)


def save_images(img_tensors, img_names, save_dir, writer: Optional[ImageWriter] = None):
    """utils.py:93-109: JPEG bytes under the given names (whatever their extension).  ``img_tensors``: [N,C,H,W] on the device, C 3 or
    1 (a one-channel image is saved as greyscale, like the reference's ``squeeze(0)``)."""
    if not torch.is_tensor(img_tensors):
        img_tensors = torch.stack(list(img_tensors))
    n = min(img_tensors.shape[0], len(img_names))
    if n == 0:
        return
    host = to_host(quantize_images(img_tensors[:n]))
    grey = img_tensors.shape[1] == 1
    for i in range(n):
        arr = host[i, :, :, 0] if grey else host[i]
        path = os.path.join(save_dir, img_names[i])
        if writer is None:
            _encode(arr, path, "JPEG")
        else:
            writer.write(np.array(arr), path, "JPEG")


class BoardLog(ScalarLog):
    """``ScalarLog`` plus images: ``add_image(tag, u8_hwc, step)`` writes ``<dir>/images/<tag with '/' -> '_'>/<step:08d>.png`` and,
    where a SummaryWriter is importable, forwards the same uint8 array as ``add_image(tag, u8, step, dataformats='HWC')`` (tensorboard
    passes a uint8 image through unchanged)."""

    IMAGES = "images"

    def image_path(self, tag: str, step: int) -> str:
        return os.path.join(self.dir, self.IMAGES, tag.replace("/", "_"), "%08d.png" % int(step))

    def add_image(self, tag: str, u8_hwc, step: int, writer: Optional[ImageWriter] = None):
        arr = to_host(u8_hwc) if torch.is_tensor(u8_hwc) else np.asarray(u8_hwc)
        if arr.dtype != np.uint8 or arr.ndim != 3 or arr.shape[2] != 3:
            raise ValueError(f"add_image: uint8 [H,W,3] expected, got {arr.dtype} {arr.shape}")
        arr = np.array(arr)                              # owned: an encode in flight and the board both read it
        path = self.image_path(tag, step)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        if writer is None:
            _encode(arr, path, "PNG")
        else:
            writer.write(arr, path, "PNG")
        board = self._writer()
        if board is not None:
            board.add_image(tag, arr, int(step), dataformats="HWC")


# ------------------------------------------------------------------------------------------------ the reference's grids
def _mask(t: torch.Tensor) -> Panel:
    return Panel(t, UNIT)


def tryon_grid(inputs: Dict[str, torch.Tensor], res: Dict[str, torch.Tensor], quant: int = ROUND, count: Optional[int] = None) -> torch.Tensor:
    """test_generator.py:223-227, 12 panels in rows of 4: cloth, its binarised mask, parse_agnostic, densepose | warped cloth, warped
    mask, fake_parse_gauss, pose | warped cloth, agnostic, image, output.  ``inputs``: the device batch ``tryon_step`` took plus
    'pose' and 'image'; ``res``: what ``tryon_step`` returned."""
    return grid_u8([Panel(inputs["cloth"], SIGNED), _mask(res["pre_clothes_mask"]), Panel(inputs["parse_agnostic"], SEGMAP),
                    Panel(inputs["densepose"], SIGNED),
                    Panel(res["warped_cloth"], SIGNED), _mask(res["warped_clothmask"]), Panel(res["fake_parse_gauss"], SEGMAP),
                    Panel(inputs["pose"], SIGNED),
                    Panel(res["warped_cloth"], SIGNED), Panel(inputs["agnostic"], SIGNED), Panel(inputs["image"], SIGNED),
                    Panel(res["output"], SIGNED)], nrow=4, quant=quant, count=count)


def condition_grid(batch: Dict[str, torch.Tensor], fields: Dict[str, torch.Tensor], quant: int = ROUND,
                   count: Optional[int] = None) -> torch.Tensor:
    """train_condition.py:377-380 / :431-434 and test_condition.py:136-139, 12 panels in rows of 4: cloth, its binarised mask,
    parse_agnostic, densepose | parse_cloth, pcm, warped cloth, binarised warped mask | parse, fake_segmap, image, misalign.
    ``batch``: the device batch (cloth, cloth_mask, parse_agnostic, densepose, parse_cloth, pcm, parse, image); ``fields``:
    fake_segmap (composed), warped_cloth, warped_cm_onehot, misalign -- ``condition_train_step``'s ``aux`` or ``condition_fields``."""
    cm = fields.get("cm_paired")
    if cm is None:
        cm = (batch["cloth_mask"] > 0.5).to(torch.float32)
    mis = fields["misalign"]
    return grid_u8([Panel(batch["cloth"], SIGNED), _mask(cm), Panel(batch["parse_agnostic"], SEGMAP), Panel(batch["densepose"], SIGNED),
                    Panel(batch["parse_cloth"], SIGNED), _mask(batch["pcm"]), Panel(fields["warped_cloth"], SIGNED),
                    _mask(fields["warped_cm_onehot"]),
                    Panel(batch["parse"], SEGMAP), Panel(fields["fake_segmap"], SEGMAP), Panel(batch["image"], SIGNED),
                    _mask(mis if mis.dtype == torch.float32 else mis.to(torch.float32))], nrow=4, quant=quant, count=count)


def generator_train_grid(batch: Dict[str, torch.Tensor], fields: Dict[str, torch.Tensor], output: torch.Tensor, quant: int = ROUND,
                         count: Optional[int] = None) -> torch.Tensor:
    """train_generator.py:366-369 / :472-475, 10 panels in rows of 4 (the last row has two empty cells): cloth, its binarised mask,
    densepose, parse_agnostic | warped cloth, agnostic, densepose, fake_parse_gauss | output, image.  ``fields``:
    ``make_generator_inputs``' ``aux`` (warped_cloth, fake_parse_gauss)."""
    cm = fields.get("cm")
    if cm is None:
        cm = (batch["cloth_mask"] > 0.5).to(torch.float32)
    return grid_u8([Panel(batch["cloth"], SIGNED), _mask(cm), Panel(batch["densepose"], SIGNED), Panel(batch["parse_agnostic"], SEGMAP),
                    Panel(fields["warped_cloth"], SIGNED), Panel(batch["agnostic"], SIGNED), Panel(batch["densepose"], SIGNED),
                    Panel(fields["fake_parse_gauss"], SEGMAP),
                    Panel(output.detach(), SIGNED), Panel(batch["image"], SIGNED)], nrow=4, quant=quant, count=count)


# ------------------------------------------------------------------------------------------------ the recording blocks' eval passes
def misalign_mask(fake_segmap: torch.Tensor, warped_cm_onehot: torch.Tensor) -> torch.Tensor:
    """train_condition.py:179-181: (argmax == 3) - warped_cm_onehot, negatives to 0 (float)."""
    fake_clothmask = (torch.argmax(fake_segmap.detach(), dim=1, keepdim=True) == 3).to(torch.float32)
    return (fake_clothmask - warped_cm_onehot).clamp_min_(0)


def condition_fields(opt, tocg, batch: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """train_condition.py:401-428: ``tocg`` in eval mode under no_grad over ``batch``; the mode is restored and no parameter or
    buffer moves (eval BatchNorm reads its running statistics).  Returns the fields ``condition_grid`` takes."""
    from .pipeline import remove_overlap
    from . import functional as HF
    was = tocg.training
    tocg.eval()
    try:
        with torch.no_grad():
            cm = (batch["cloth_mask"] > 0.5).to(torch.float32)
            input1 = torch.cat([batch["cloth"], cm], 1)
            input2 = torch.cat([batch["parse_agnostic"], batch["densepose"]], 1)
            _, fake_segmap, warped_cloth, warped_cm = tocg(input1, input2)
            onehot = (warped_cm > 0.5).to(torch.float32)
            comp = getattr(opt, "clothmask_composition", "warp_grad")
            if comp != "no_composition":
                mask = torch.ones_like(fake_segmap)
                mask[:, 3:4, :, :] = onehot if comp == "detach" else warped_cm
                fake_segmap = fake_segmap * mask
            if getattr(opt, "occlusion", False):
                warped_cm = remove_overlap(HF.softmax(fake_segmap, dim=1), warped_cm)
                warped_cloth = warped_cloth * warped_cm + torch.ones_like(warped_cloth) * (1 - warped_cm)
            return {"cm_paired": cm, "fake_segmap": fake_segmap, "warped_cloth": warped_cloth, "warped_cm_onehot": onehot,
                    "misalign": misalign_mask(fake_segmap, onehot)}
    finally:
        tocg.train(was)


VIS_SEED = 20_221_107     # the forked generator of the test-visualisation passes


def generator_fields(opt, tocg, generator, batch: Dict[str, torch.Tensor], noise=None):
    """train_generator.py:381-478: the frozen pipeline and the generator in eval mode under no_grad over ``batch``.  The pass runs
    on forked random-number generators seeded with VIS_SEED (the SPADE noise is drawn in eval mode too), so the training run's CPU
    and device streams are where they were; modes are restored; eval mode runs no spectral-norm power iteration.  Returns
    (fields for ``generator_train_grid``, output)."""
    from .pipeline import make_generator_inputs
    modes = [(m, m.training) for m in (generator, tocg) if m is not None]
    for m, _ in modes:
        m.eval()
    try:
        dev = batch["image"].device
        with torch.no_grad(), torch.random.fork_rng(devices=[dev]), torch.cuda.device(dev):
            # seed exactly what was forked -- the CPU generator and this device's: torch.manual_seed would reseed every visible
            # device, and only the forked ones are restored
            torch.default_generator.manual_seed(VIS_SEED)
            torch.cuda.manual_seed(VIS_SEED)
            aux: Dict[str, torch.Tensor] = {}
            x, parse7 = make_generator_inputs(opt, tocg, batch, aux=aux)
            output = generator(x, parse7, noise=noise) if noise is not None else generator(x, parse7)
            return aux, output
    finally:
        for m, was in modes:
            m.train(was)
