"""LPIPS v0.1 (net-lin, AlexNet) of the reference's eval_models package on the HIP path.

``PerceptualLoss(model='net-lin', net='alex')`` has the reference's signature and ``forward(pred, target, normalize=False)
-> [N,1,1,1]`` (eval_models/__init__.py:12-40).  The module tree mirrors PNetLin's state-dict keys (``scaling_layer.shift|scale``,
``net.slice{1..5}.{0,3,6,8,10}.weight|bias``, ``lin{0..4}.model.1.weight``) under ``model.net``, so a v0.1 ``alex.pth`` loads with
``load_state_dict(sd, strict=False)`` exactly as dist_model.py:67-73 does, and ``load_torchvision_alexnet`` takes torchvision's
``alexnet().state_dict()`` (``features.N.*``).  The reference fetches both over the network; there is none here, so without them
the module stays random-initialised and says so (the VGG19 precedent, vgg.py).

Forward: ScalingLayer (csrc/metrics.hip) -> the five AlexNet convolutions + ReLU on the fp32 conv engine (frozen, host-packed
weights) with two 3x3 stride-2 max-pools, both images as ONE batch -> the fused head (normalize_tensor, squared difference,
1x1 lin, spatial mean, sum over the taps).  No autograd: evaluation only.
"""
from __future__ import annotations

import ctypes as C
import sys
from typing import Dict, List

import torch
import torch.nn as nn

from . import _lib, ops
from ._lib import HrvError
from .ops import ACT_RELU, Act, ConvLayer, _stream

# torchvision alexnet().features up to [11]: (index, in, out, kernel, stride, pad) of the convs; MaxPool2d(3, 2) at 2 and 5
_CONVS = [(0, 3, 64, 11, 4, 2), (3, 64, 192, 5, 1, 2), (6, 192, 384, 3, 1, 1), (8, 384, 256, 3, 1, 1), (10, 256, 256, 3, 1, 1)]
_POOLS = [2, 5]
_SLICES = [(0, 2), (2, 5), (5, 8), (8, 10), (10, 12)]    # pretrained_networks.alexnet: relu1 .. relu5
CHNS = [64, 192, 384, 256, 256]
SHIFT = (-.030, -.088, -.188)                              # networks_basic.ScalingLayer (v0.1)
SCALE = (.458, .448, .450)


class ScalingLayer(nn.Module):
    def __init__(self):
        super().__init__()
        self.register_buffer("shift", torch.tensor(SHIFT, dtype=torch.float32)[None, :, None, None])
        self.register_buffer("scale", torch.tensor(SCALE, dtype=torch.float32)[None, :, None, None])

    def host_arrays(self):
        sh = self.shift.detach().to("cpu", torch.float32).reshape(3)
        sc = self.scale.detach().to("cpu", torch.float32).reshape(3)
        return (C.c_float * 3)(*sh.tolist()), (C.c_float * 3)(*sc.tolist())


class NetLinLayer(nn.Module):
    """A 1x1 convolution to one channel, no bias; ``model.0`` is the reference's (eval-mode) Dropout, ``model.1`` the conv."""

    def __init__(self, chn_in: int, chn_out: int = 1):
        super().__init__()
        self.model = nn.Sequential(nn.Dropout(), nn.Conv2d(chn_in, chn_out, 1, stride=1, padding=0, bias=False))


class AlexNet(nn.Module):
    def __init__(self):
        super().__init__()
        layers: Dict[int, nn.Module] = {}
        for idx, cin, cout, k, s, p in _CONVS:
            layers[idx] = nn.Conv2d(cin, cout, kernel_size=k, stride=s, padding=p)
            layers[idx + 1] = nn.ReLU(inplace=True)
        for idx in _POOLS:
            layers[idx] = nn.MaxPool2d(kernel_size=3, stride=2)
        for k, (a, b) in enumerate(_SLICES):
            seq = nn.Sequential()
            for i in range(a, b):
                seq.add_module(str(i), layers[i])
            setattr(self, f"slice{k + 1}", seq)
        for p in self.parameters():
            p.requires_grad = False

    def conv(self, idx: int) -> nn.Conv2d:
        for k, (a, b) in enumerate(_SLICES):
            if a <= idx < b:
                return getattr(self, f"slice{k + 1}")._modules[str(idx)]
        raise KeyError(idx)


class PNetLin(nn.Module):
    """networks_basic.PNetLin(pnet_type='alex', version='0.1', lpips=True, spatial=False) on the HIP path."""

    def __init__(self):
        super().__init__()
        self.scaling_layer = ScalingLayer()
        self.net = AlexNet()
        self.chns = list(CHNS)
        self.L = len(CHNS)
        for k, c in enumerate(CHNS):
            setattr(self, f"lin{k}", NetLinLayer(c))
        for p in self.parameters():
            p.requires_grad = False
        self._plan = None

    def load_torchvision_alexnet(self, sd):
        """Accepts torchvision.models.alexnet().state_dict() (keys 'features.N.weight|bias'; the classifier is ignored)."""
        own = {}
        for idx, *_ in _CONVS:
            for suf in ("weight", "bias"):
                key = f"features.{idx}.{suf}"
                if key not in sd:
                    raise KeyError(f"load_torchvision_alexnet: {key} missing (expected torchvision alexnet().state_dict())")
                own[f"{suf}"] = sd[key]
            self.net.conv(idx).load_state_dict(own, strict=True)
        self._plan = None

    def plan(self, device):
        # frozen weights, host-packed once; re-packed when a parameter is written in place (load_state_dict bumps _version)
        ps = list(self.parameters())
        key = (str(device), tuple(p._version for p in ps), ops.weights_epoch(ps), ops.LOAD_EPOCH[0])
        if self._plan is None or self._plan[0] != key:
            convs = {idx: ConvLayer(self.net.conv(idx).weight, [cin], device, shift=self.net.conv(idx).bias, stride=s, pad=p,
                                    act=ACT_RELU, name=f"alexnet.features.{idx}") for idx, cin, cout, k, s, p in _CONVS}
            lins = [getattr(self, f"lin{k}").model[1].weight.detach().to(device, torch.float32).reshape(-1).contiguous()
                    for k in range(self.L)]
            self._plan = (key, convs, lins, self.scaling_layer.host_arrays())
        return self._plan[1:]

    def features(self, x: Act) -> List[Act]:
        """relu1 .. relu5 of a dense NHWC batch (3 real channels of 4)."""
        convs, _, _ = self.plan(x.t.device)
        taps, cur = [], x
        for idx, cin, cout, k, s, p in _CONVS:
            if idx - 1 in _POOLS:
                cur = maxpool3x3s2(cur)
            Ho, Wo = convs[idx].out_hw(cur.H, cur.W)
            if Ho < 1 or Wo < 1:
                raise ValueError(f"LPIPS/AlexNet: input too small (features.{idx} gets {cur.H}x{cur.W})")
            cur = convs[idx]([cur])
            taps.append(cur)        # every conv's ReLU closes a slice (_SLICES)
        return taps

    def distance_prepped(self, both: Act) -> torch.Tensor:
        """LPIPS of images [0, N) against [N, 2N) of a ScalingLayer output ``both`` [2N,H,W,4] -> fp32 [N]."""
        _, lins, _ = self.plan(both.t.device)
        taps = self.features(both)
        N = both.N // 2
        arr = (_lib.hrv_lpips_tap_t * self.L)()
        for k, t in enumerate(taps):
            assert not t.bf16 and t.coff == 0 and t.C == self.chns[k]
            a = arr[k]
            a.f0, a.f1, a.lin = t.t.data_ptr(), t.t[N:].data_ptr(), lins[k].data_ptr()
            a.HW, a.C, a.cstride = t.H * t.W, t.C, t.cstride
        out = torch.empty(N, dtype=torch.float32, device=both.t.device)
        lib = _lib.load()
        with ops._Timed("lpips", "lpips_head", 0.0, sum(ops.act_bytes(t) for t in taps)):
            _lib.check(lib.hrv_lpips_head_f32(arr, self.L, N, out.data_ptr(), _stream()), "hrv_lpips_head_f32")
        return out

    def forward_u8(self, in0: torch.Tensor, in1: torch.Tensor) -> torch.Tensor:
        """in0, in1: uint8 [N,H,W,3] CUDA images as decoded (evaluate.py's T2 minus the resize) -> fp32 [N]."""
        for t in (in0, in1):
            if not t.is_cuda or t.dtype != torch.uint8 or t.dim() != 4 or t.shape[3] != 3:
                raise HrvError("LPIPS: expected uint8 CUDA images [N,H,W,3]")
        assert in0.shape == in1.shape
        N, H, W, _ = in0.shape
        both = torch.empty((2 * N, H, W, 4), dtype=torch.float32, device=in0.device)
        _, _, (sh, sc) = self.plan(in0.device)
        lib = _lib.load()
        for i, t in enumerate((in0, in1)):
            _lib.check(lib.hrv_lpips_prep_u8(t.contiguous().data_ptr(), N, H, W, sh, sc, both[i * N:].data_ptr(), _stream()),
                       "hrv_lpips_prep_u8")
        return self.distance_prepped(Act(both, 3))

    def forward(self, in0: torch.Tensor, in1: torch.Tensor, normalize: bool = False) -> torch.Tensor:
        """in0, in1: fp32 NCHW [N,3,H,W] CUDA images in [-1, 1] (or [0, 1] with ``normalize``) -> [N,1,1,1]."""
        for t in (in0, in1):
            ops.require_cuda(t, "LPIPS")
            if t.dtype != torch.float32 or t.dim() != 4 or t.shape[1] != 3:
                raise HrvError("LPIPS: expected fp32 images [N,3,H,W]")
        assert in0.shape == in1.shape, (in0.shape, in1.shape)
        N, _, H, W = in0.shape
        both = torch.empty((2 * N, H, W, 4), dtype=torch.float32, device=in0.device)
        _, _, (sh, sc) = self.plan(in0.device)
        lib = _lib.load()
        for i, t in enumerate((in0, in1)):
            _lib.check(lib.hrv_lpips_prep_nchw_f32(t.detach().contiguous().data_ptr(), N, H, W, int(bool(normalize)), sh, sc,
                                                   both[i * N:].data_ptr(), _stream()), "hrv_lpips_prep_nchw_f32")
        return self.distance_prepped(Act(both, 3)).view(N, 1, 1, 1)

    def forward_resized(self, in0: torch.Tensor, in1: torch.Tensor, size=(128, 128), normalize: bool = False) -> torch.Tensor:
        """``forward(T2(in0), T2(in1))`` with ``T2 = transforms.Resize(size)`` applied to fp32 NCHW tensors, the LPIPS call of
        train_generator.py:482,578 -> [N,1,1,1].  The resize is bilinear, align_corners=False, WITHOUT antialiasing: that is what
        the reference's pinned environment (pytorch-lts 1.8, torchvision 0.9) does to tensor inputs; current torchvision
        antialiases them by default, and we follow the former.  Resize and ScalingLayer of both images are one launch
        (csrc/validate.hip), bit-identical to ``forward(glue.resize_nchw(in0, size), glue.resize_nchw(in1, size))``."""
        for t in (in0, in1):
            ops.require_cuda(t, "LPIPS")
            if t.dtype != torch.float32 or t.dim() != 4 or t.shape[1] != 3:
                raise HrvError("LPIPS: expected fp32 images [N,3,H,W]")
        assert in0.shape == in1.shape, (in0.shape, in1.shape)
        N, _, H, W = in0.shape
        Ho, Wo = int(size[0]), int(size[1])
        both = torch.empty((2 * N, Ho, Wo, 4), dtype=torch.float32, device=in0.device)
        _, _, (sh, sc) = self.plan(in0.device)
        lib = _lib.load()
        _lib.check(lib.hrv_lpips_prep_resize_nchw_f32(in0.detach().contiguous().data_ptr(), in1.detach().contiguous().data_ptr(),
                                                      N, H, W, Ho, Wo, int(bool(normalize)), sh, sc, both.data_ptr(), _stream()),
                   "hrv_lpips_prep_resize_nchw_f32")
        return self.distance_prepped(Act(both, 3)).view(N, 1, 1, 1)


def maxpool3x3s2(a: Act) -> Act:
    """AlexNet's MaxPool2d(3, 2) over a dense fp32 NHWC activation."""
    assert not a.bf16 and a.coff == 0 and a.cstride == a.Cp
    Ho, Wo = (a.H - 3) // 2 + 1, (a.W - 3) // 2 + 1
    if Ho < 1 or Wo < 1:
        raise ValueError(f"LPIPS/AlexNet: max-pool input {a.H}x{a.W} is smaller than its 3x3 window")
    out = Act(torch.empty((a.N, Ho, Wo, a.cstride), dtype=torch.float32, device=a.t.device), a.C, 0)
    lib = _lib.load()
    with ops._Timed("pool", "maxpool3x3s2", 0.0, ops.act_bytes(a) + ops.act_bytes(out)):
        _lib.check(lib.hrv_maxpool3x3s2_nhwc_f32(a.t.data_ptr(), a.N, a.H, a.W, a.cstride, out.t.data_ptr(), _stream()),
                   "hrv_maxpool3x3s2_nhwc_f32")
    return out


class DistModel(nn.Module):
    """The part of dist_model.DistModel evaluate.py uses: ``net`` (PNetLin) and ``forward(in0, in1)``."""

    def __init__(self):
        super().__init__()
        self.net = PNetLin()
        self.model_name = "net-lin [alex]"

    def name(self):
        return self.model_name

    def forward(self, in0, in1, retPerLayer=False):
        if retPerLayer:
            raise NotImplementedError("retPerLayer: the fused head returns the tap sum only")
        return self.net.forward(in0, in1)


class PerceptualLoss(nn.Module):
    def __init__(self, model='net-lin', net='alex', colorspace='rgb', spatial=False, use_gpu=True, gpu_ids=[0]):  # noqa: B006
        super().__init__()
        if model != "net-lin" or net != "alex" or spatial or colorspace != "rgb":
            raise NotImplementedError(f"PerceptualLoss(model={model!r}, net={net!r}, colorspace={colorspace!r}, spatial={spatial}): "
                                      "only model='net-lin', net='alex', colorspace='rgb', spatial=False runs on the HIP path")
        if not use_gpu:
            raise NotImplementedError("PerceptualLoss(use_gpu=False): the HIP path has no CPU implementation")
        self.use_gpu, self.spatial, self.gpu_ids = use_gpu, spatial, gpu_ids
        self.model = DistModel()
        self.pretrained = {"alexnet": False, "lin": False}
        print("PerceptualLoss: AlexNet features and lin layers are random-initialised -- load a torchvision AlexNet state dict "
              "(load_torchvision_alexnet) and the LPIPS v0.1 alex.pth (load_lpips_weights) for real scores", file=sys.stderr)
        if torch.cuda.is_available():
            self.model.cuda(gpu_ids[0] if gpu_ids else None)

    @property
    def net(self) -> PNetLin:
        return self.model.net

    def load_torchvision_alexnet(self, sd):
        self.net.load_torchvision_alexnet(sd)
        self.pretrained["alexnet"] = True

    def load_lpips_weights(self, sd):
        """A v0.1 ``alex.pth`` (lin{0..4}.model.1.weight), loaded like dist_model.py:73: strict=False."""
        res = self.net.load_state_dict(sd, strict=False)
        missing = [k for k in (f"lin{i}.model.1.weight" for i in range(5)) if k in res.missing_keys]
        if missing:
            raise KeyError(f"load_lpips_weights: {missing} missing (expected the LPIPS v0.1 alex.pth)")
        self.pretrained["lin"] = True
        return res

    def forward(self, pred, target, normalize=False):
        """eval_models/__init__.py:26-40: pred, target fp32 [N,3,H,W] in [-1, 1] ([0, 1] with normalize) -> [N,1,1,1]."""
        with torch.no_grad():
            return self.net.forward(target, pred, normalize=normalize)

    def forward_resized(self, pred, target, size=(128, 128)):
        """train_generator.py:578 ``model.forward(T2(im), T2(output))`` with ``T2 = transforms.Resize((128, 128))``: both images
        resized without antialiasing (PNetLin.forward_resized states the choice), then ``forward`` -> [N,1,1,1]."""
        with torch.no_grad():
            return self.net.forward_resized(target, pred, size=size)

    def forward_u8(self, pred_u8, target_u8) -> torch.Tensor:
        """evaluate.py's LPIPS of uint8 [N,H,W,3] images (T2 = ToTensor + Normalize(0.5, 0.5) fused into the input kernel) -> [N]."""
        with torch.no_grad():
            return self.net.forward_u8(target_u8, pred_u8)
