"""torchvision's Inception-v3 (eval mode, ``aux_logits`` unused, ``transform_input=False``) on the HIP path: the network of the
reference's Inception Score (evaluate.py:43-44,76).

The module tree carries torchvision's names, so the state dict torchvision downloads (``inception_v3_google-0cc3c7bd.pth``, older
releases ``inception_v3_google-1a9a5a14.pth``) loads as it is: every conv unit is a ``BasicConv2d`` (``NAME.conv.weight``, no bias;
``NAME.bn.*`` with eps 0.001; ReLU), the classifier is ``fc``.  ``AuxLogits.*`` keys are accepted and ignored -- eval mode never runs
that branch.  Nothing is fetched: without a state dict the module stays random-initialised (the VGG19 / AlexNet precedent), which is
good for plumbing only.

Forward: the input kernel (uint8 NHWC -> fp32, ToTensor + Normalize(0.5, 0.5)) -> 94 convolutions on the fp32 conv engine, BatchNorm
folded into the engine's per-channel scale / shift on the host in float64, ReLU in its epilogue, every branch written at its channel
offset of the block's output (no concatenation pass) -> the 3x3 pools and the head of csrc/inception.hip (mean over the last map, fc,
softmax).  No autograd, no training mode, no CPU path.

``FIDInceptionV3`` is the network behind pytorch-fid and torch-fidelity (``pt_inception-2015-12-05-6726825d.pth``): the same units
under the same names, no ``AuxLogits``, ``fc`` [1008, 2048], and other 3x3 pools in the pooled branch of four block types
(``FID_POOLS``).  It is the same plan, stem and block runner over that table; ``features_u8`` gives the 2048-wide pooled vector.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Tuple

import torch
import torch.nn as nn

from . import _lib, ops
from ._lib import HrvError
from .ops import ACT_RELU, Act, ConvLayer, _stream

BN_EPS = 0.001
NUM_CLASSES = 1000
FC_INIT_GAIN = 8.0


def _pair(v) -> Tuple[int, int]:
    return (v, v) if isinstance(v, int) else (int(v[0]), int(v[1]))


class BasicConv2d(nn.Module):
    """torchvision.models.inception.BasicConv2d: Conv2d(bias=False) -> BatchNorm2d(eps=0.001) -> ReLU."""

    def __init__(self, cin: int, cout: int, kernel_size, stride: int = 1, padding=0):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, kernel_size=_pair(kernel_size), stride=stride, padding=_pair(padding), bias=False)
        self.bn = nn.BatchNorm2d(cout, eps=BN_EPS)
        # random initialisation (plumbing runs only): He-scaled, so that activations keep their scale through the ReLU chain
        nn.init.kaiming_normal_(self.conv.weight, nonlinearity="relu")

    def folded(self):
        """(weight OIHW fp32, scale, shift): eval-mode BatchNorm as y = conv * scale + shift, folded in float64."""
        bn = self.bn
        scale = bn.weight.detach().double().cpu() / torch.sqrt(bn.running_var.detach().double().cpu() + bn.eps)
        shift = bn.bias.detach().double().cpu() - bn.running_mean.detach().double().cpu() * scale
        return self.conv.weight.detach(), scale.float(), shift.float()


# The blocks as data: per block type the branches in torch.cat order; a branch is a chain of steps:
#   "name"                   one BasicConv2d, input = the previous step's output (the block input for the first step)
#   ("name_a", "name_b")     two units over the SAME input whose outputs are concatenated (Mixed_7b/7c's 1x3 | 3x1 pairs)
#   "avg" / "max"            the 3x3 pool of the block input (average: stride 1, padding 1; max: stride 2); a network variant may
#                            name another pool step of POOL_MODES for a block's "avg" (FID_POOLS)
# and per unit (out channels or a key into the block's constructor arguments, kernel, stride, padding (h, w)).
_A = {"branches": [["branch1x1"], ["branch5x5_1", "branch5x5_2"], ["branch3x3dbl_1", "branch3x3dbl_2", "branch3x3dbl_3"],
                   ["avg", "branch_pool"]],
      "units": {"branch1x1": (64, 1, 1, 0), "branch5x5_1": (48, 1, 1, 0), "branch5x5_2": (64, 5, 1, 2),
                "branch3x3dbl_1": (64, 1, 1, 0), "branch3x3dbl_2": (96, 3, 1, 1), "branch3x3dbl_3": (96, 3, 1, 1),
                "branch_pool": ("pf", 1, 1, 0)}}
_B = {"branches": [["branch3x3"], ["branch3x3dbl_1", "branch3x3dbl_2", "branch3x3dbl_3"], ["max"]],
      "units": {"branch3x3": (384, 3, 2, 0), "branch3x3dbl_1": (64, 1, 1, 0), "branch3x3dbl_2": (96, 3, 1, 1),
                "branch3x3dbl_3": (96, 3, 2, 0)}}
_C = {"branches": [["branch1x1"], ["branch7x7_1", "branch7x7_2", "branch7x7_3"],
                   ["branch7x7dbl_1", "branch7x7dbl_2", "branch7x7dbl_3", "branch7x7dbl_4", "branch7x7dbl_5"], ["avg", "branch_pool"]],
      "units": {"branch1x1": (192, 1, 1, 0), "branch7x7_1": ("c7", 1, 1, 0), "branch7x7_2": ("c7", (1, 7), 1, (0, 3)),
                "branch7x7_3": (192, (7, 1), 1, (3, 0)), "branch7x7dbl_1": ("c7", 1, 1, 0),
                "branch7x7dbl_2": ("c7", (7, 1), 1, (3, 0)), "branch7x7dbl_3": ("c7", (1, 7), 1, (0, 3)),
                "branch7x7dbl_4": ("c7", (7, 1), 1, (3, 0)), "branch7x7dbl_5": (192, (1, 7), 1, (0, 3)),
                "branch_pool": (192, 1, 1, 0)}}
_D = {"branches": [["branch3x3_1", "branch3x3_2"], ["branch7x7x3_1", "branch7x7x3_2", "branch7x7x3_3", "branch7x7x3_4"], ["max"]],
      "units": {"branch3x3_1": (192, 1, 1, 0), "branch3x3_2": (320, 3, 2, 0), "branch7x7x3_1": (192, 1, 1, 0),
                "branch7x7x3_2": (192, (1, 7), 1, (0, 3)), "branch7x7x3_3": (192, (7, 1), 1, (3, 0)), "branch7x7x3_4": (192, 3, 2, 0)}}
_E = {"branches": [["branch1x1"], ["branch3x3_1", ("branch3x3_2a", "branch3x3_2b")],
                   ["branch3x3dbl_1", "branch3x3dbl_2", ("branch3x3dbl_3a", "branch3x3dbl_3b")], ["avg", "branch_pool"]],
      "units": {"branch1x1": (320, 1, 1, 0), "branch3x3_1": (384, 1, 1, 0), "branch3x3_2a": (384, (1, 3), 1, (0, 1)),
                "branch3x3_2b": (384, (3, 1), 1, (1, 0)), "branch3x3dbl_1": (448, 1, 1, 0), "branch3x3dbl_2": (384, 3, 1, 1),
                "branch3x3dbl_3a": (384, (1, 3), 1, (0, 1)), "branch3x3dbl_3b": (384, (3, 1), 1, (1, 0)),
                "branch_pool": (192, 1, 1, 0)}}
_TYPES = {"A": _A, "B": _B, "C": _C, "D": _D, "E": _E}
# pool step -> mode of hrv_pool3x3_nhwc_f32.  "avg_inside": the stride-1 average divided by the taps inside the image
# (count_include_pad=False); "max_same": max, stride 1, padding 1.
POOL_MODES = {"max": 0, "avg": 1, "avg_inside": 2, "max_same": 3}
POOL_LABELS = {0: "maxpool3x3s2", 1: "avgpool3x3s1", 2: "avgpool3x3s1_inside", 3: "maxpool3x3s1"}

# the stem: (name, in, out, kernel, stride, padding) or "max"
STEM = [("Conv2d_1a_3x3", 3, 32, 3, 2, 0), ("Conv2d_2a_3x3", 32, 32, 3, 1, 0), ("Conv2d_2b_3x3", 32, 64, 3, 1, 1), "max",
        ("Conv2d_3b_1x1", 64, 80, 1, 1, 0), ("Conv2d_4a_3x3", 80, 192, 3, 1, 0), "max"]
# (name, type, input channels, constructor arguments)
MIXED = [("Mixed_5b", "A", 192, {"pf": 32}), ("Mixed_5c", "A", 256, {"pf": 64}), ("Mixed_5d", "A", 288, {"pf": 64}),
         ("Mixed_6a", "B", 288, {}),
         ("Mixed_6b", "C", 768, {"c7": 128}), ("Mixed_6c", "C", 768, {"c7": 160}), ("Mixed_6d", "C", 768, {"c7": 160}),
         ("Mixed_6e", "C", 768, {"c7": 192}),
         ("Mixed_7a", "D", 768, {}), ("Mixed_7b", "E", 1280, {}), ("Mixed_7c", "E", 2048, {})]
# The FID network (pytorch-fid's FIDInceptionA / C / E_1 / E_2): the pool step that stands for "avg" in the pooled branch, per block.
# Mixed_6a, Mixed_7a and the stem keep torchvision's pools.
FID_POOLS = {"Mixed_5b": "avg_inside", "Mixed_5c": "avg_inside", "Mixed_5d": "avg_inside",
             "Mixed_6b": "avg_inside", "Mixed_6c": "avg_inside", "Mixed_6d": "avg_inside", "Mixed_6e": "avg_inside",
             "Mixed_7b": "avg_inside", "Mixed_7c": "max_same"}
FID_NUM_CLASSES = 1008
FID_SIZE = 299


def _step_names(step) -> Tuple[str, ...]:
    return step if isinstance(step, tuple) else (step,)


class InceptionBlock(nn.Module):
    """One Mixed_* block: the BasicConv2d children of torchvision's InceptionA..E under their names."""

    def __init__(self, kind: str, cin: int, args: Dict[str, int], pool: Optional[str] = None):
        super().__init__()
        spec = _TYPES[kind]
        self.kind, self.cin = kind, cin
        assert pool is None or pool in POOL_MODES, pool
        self.branches = spec["branches"] if pool is None else [[pool if st == "avg" else st for st in br] for br in spec["branches"]]
        self.widths: List[int] = []        # output channels per branch, in cat order
        for br in self.branches:
            c = cin
            for step in br:
                if isinstance(step, str) and step in POOL_MODES:
                    continue
                outs = 0
                for nm in _step_names(step):
                    co, k, s, p = spec["units"][nm]
                    co = args[co] if isinstance(co, str) else co
                    setattr(self, nm, BasicConv2d(c, co, k, s, p))
                    outs += co
                c = outs
            self.widths.append(c)
        self.cout = sum(self.widths)

    def offsets(self) -> List[int]:
        o, out = 0, []
        for w in self.widths:
            out.append(o)
            o += w
        return out


def pool3x3(a: Act, mode: int, out: Optional[Act] = None) -> Act:
    """hrv_pool3x3_nhwc_f32 over a channel slice: mode 0 max stride 2 (no padding), mode 1 average stride 1 padding 1 (/ 9), mode 2
    that average divided by the taps inside the image, mode 3 max stride 1 padding 1."""
    assert not a.bf16 and a.C % 4 == 0 and mode in POOL_LABELS, (a.C, a.t.dtype, mode)
    Ho, Wo = ((a.H - 3) // 2 + 1, (a.W - 3) // 2 + 1) if mode == 0 else (a.H, a.W)
    if Ho < 1 or Wo < 1:
        raise ValueError(f"Inception3: max-pool input {a.H}x{a.W} is smaller than its 3x3 window")
    if out is None:
        out = Act(torch.empty((a.N, Ho, Wo, a.C), dtype=torch.float32, device=a.t.device), a.C, 0)
    assert (out.N, out.H, out.W, out.C) == (a.N, Ho, Wo, a.C) and not out.bf16, (out.t.shape, out.C)
    lib = _lib.load()
    with ops._Timed("pool", POOL_LABELS[mode], 0.0, ops.act_bytes(a) + ops.act_bytes(out),
                    "pool3x3_kernel"):
        _lib.check(lib.hrv_pool3x3_nhwc_f32(a.t.data_ptr(), a.N, a.H, a.W, a.C, a.cstride, a.coff, mode, out.t.data_ptr(), out.cstride,
                                            out.coff, _stream()), "hrv_pool3x3_nhwc_f32")
    return out


class Inception3(nn.Module):
    """torchvision.models.inception.Inception3 in eval mode on the HIP path.  ``forward(x)``: fp32 NCHW [N,3,H,W] CUDA -> logits
    [N,1000]; ``forward_u8(img)``: uint8 [N,H,W,3] CUDA as decoded -> softmax probabilities [N,1000]."""

    STATE_DICT_OF = "torchvision inception_v3().state_dict()"
    POOLS: Dict[str, str] = {}      # block name -> the pool step that replaces "avg" (a variant's table; torchvision: none)

    def __init__(self, num_classes: int = NUM_CLASSES, aux_logits: bool = True, transform_input: bool = False):
        super().__init__()
        if transform_input:
            raise NotImplementedError("Inception3(transform_input=True): the reference passes False; only that runs on the HIP path")
        self.aux_logits, self.transform_input = aux_logits, False      # (AuxLogits is never built: eval mode does not run it)
        for st in STEM:
            if st != "max":
                nm, cin, cout, k, s, p = st
                setattr(self, nm, BasicConv2d(cin, cout, k, s, p))
        for nm, kind, cin, args in MIXED:
            setattr(self, nm, InceptionBlock(kind, cin, args, self.POOLS.get(nm)))
        self.fc = nn.Linear(2048, num_classes)
        nn.init.normal_(self.fc.weight, std=FC_INIT_GAIN / 2048 ** 0.5)      # (random initialisation: logits that tell images apart)
        nn.init.zeros_(self.fc.bias)
        for p in self.parameters():
            p.requires_grad = False
        self._plan = None
        super().train(False)

    # ---------------------------------------------------------------------------------------------------------- state
    def train(self, mode: bool = True):
        if mode:
            raise NotImplementedError("Inception3: evaluation only (no BatchNorm statistics update, no AuxLogits) on the HIP path")
        return super().train(False)

    def load_state_dict(self, state_dict, strict: bool = True, **kw):
        """torchvision's ``inception_v3`` state dict.  ``AuxLogits.*`` entries are ignored; every other key of this module is required
        (KeyError names a missing one), except BatchNorm's ``num_batches_tracked``, which the older released file predates and eval
        mode does not read."""
        sd = {k: v for k, v in state_dict.items() if not k.startswith("AuxLogits.")}
        for k in self.state_dict().keys():
            if k not in sd and not k.endswith("num_batches_tracked"):
                raise KeyError(f"{type(self).__name__}.load_state_dict: {k} missing (expected {self.STATE_DICT_OF})")
        res = super().load_state_dict(sd, strict=strict, **kw)
        self._plan = None
        return res

    def units(self) -> List[Tuple[str, BasicConv2d]]:
        """(state-dict prefix, unit) of all 94 conv units in module order."""
        return [(n, m) for n, m in self.named_modules() if isinstance(m, BasicConv2d)]

    def plan(self, device):
        # frozen weights, folded and host-packed once per device; re-packed when a tensor is written (load_state_dict bumps _version)
        ps = list(self.parameters()) + list(self.buffers())
        key = (str(device), tuple(p._version for p in ps), ops.weights_epoch(ps), ops.LOAD_EPOCH[0])
        if self._plan is None or self._plan[0] != key:
            convs = {}
            for name, u in self.units():
                w, scale, shift = u.folded()
                ph, pw = u.conv.padding
                convs[name] = ConvLayer(w, [w.shape[1]], device, scale=scale, shift=shift, stride=u.conv.stride[0], pad=ph,
                                        pad_w=None if pw == ph else pw, act=ACT_RELU, name=f"inception.{name}")
            fc_w = self.fc.weight.detach().to(device, torch.float32).contiguous()
            fc_b = self.fc.bias.detach().to(device, torch.float32).contiguous()
            self._plan = (key, convs, fc_w, fc_b)
        return self._plan[1:]

    # ---------------------------------------------------------------------------------------------------------- forward
    def run_block(self, name: str, x: Act, convs=None) -> Act:
        """One Mixed_* block over an NHWC activation: every branch lands in its slice of the returned tensor."""
        blk: InceptionBlock = getattr(self, name)
        if convs is None:
            convs = self.plan(x.t.device)[0]
        assert x.C == blk.cin, (name, x.C, blk.cin)
        out = None
        for br, off, width in zip(blk.branches, blk.offsets(), blk.widths):
            cur = x
            for i, step in enumerate(br):
                last = i == len(br) - 1
                if isinstance(step, str) and step in POOL_MODES:
                    if last:        # Mixed_6a / Mixed_7a: the pooled input is the branch
                        if out is None:
                            out = self._block_out(blk, x, convs, name)
                        cur = pool3x3(x, POOL_MODES[step], out.slice(off, width))
                    else:
                        cur = pool3x3(x, POOL_MODES[step])
                    continue
                names = _step_names(step)
                if last and out is None:
                    out = self._block_out(blk, x, convs, name)
                o = 0
                src, nxt = cur, None
                for nm in names:
                    conv = convs[f"{name}.{nm}"]
                    if last:
                        conv([src], out=out.slice(off + o, conv.Cout))
                    elif len(names) == 1:
                        nxt = conv([src])
                    else:
                        raise AssertionError("a unit pair closes its branch")
                    o += conv.Cout
                cur = nxt
        return out

    def _block_out(self, blk: InceptionBlock, x: Act, convs, name: str) -> Act:
        # output extent of the block: that of its first branch's last unit (all branches agree)
        H, W = x.H, x.W
        for step in blk.branches[0]:
            nm = _step_names(step)[0]
            H, W = convs[f"{name}.{nm}"].out_hw(H, W)
        if H < 1 or W < 1:
            raise ValueError(f"Inception3: input too small ({name} gets {x.H}x{x.W})")
        return Act(torch.empty((x.N, H, W, blk.cout), dtype=torch.float32, device=x.t.device), blk.cout, 0)

    def stem(self, x: Act, convs=None) -> Act:
        if convs is None:
            convs = self.plan(x.t.device)[0]
        cur = x
        for st in STEM:
            if st == "max":
                cur = pool3x3(cur, 0)
                continue
            conv = convs[st[0]]
            Ho, Wo = conv.out_hw(cur.H, cur.W)
            if Ho < 1 or Wo < 1:
                raise ValueError(f"Inception3: input too small ({st[0]} gets {cur.H}x{cur.W})")
            cur = conv([cur])
        return cur

    def features(self, x: Act, taps: Optional[dict] = None) -> Act:
        """The last feature map (Mixed_7c's output) of a dense NHWC batch (3 real channels of 4).  ``taps``: a dict that receives every
        block's output by name (and ``"stem"``)."""
        convs = self.plan(x.t.device)[0]
        cur = self.stem(x, convs)
        if taps is not None:
            taps["stem"] = cur
        for name, *_ in MIXED:
            cur = self.run_block(name, cur, convs)
            if taps is not None:
                taps[name] = cur
        return cur

    def head(self, f: Act, want_probs: bool) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        """(logits, probabilities or None) of the last feature map: mean over H x W, dropout (identity in eval mode), fc, softmax."""
        _, fc_w, fc_b = self.plan(f.t.device)
        K, Cf = fc_w.shape
        assert f.coff == 0 and f.C == Cf and not f.bf16, (f.C, Cf)
        dev = f.t.device
        pooled = torch.empty((f.N, Cf), dtype=torch.float32, device=dev)
        logits = torch.empty((f.N, K), dtype=torch.float32, device=dev)
        probs = torch.empty((f.N, K), dtype=torch.float32, device=dev) if want_probs else None
        lib = _lib.load()
        with ops._Timed("head", "inception_head", 2.0 * f.N * K * Cf, ops.act_bytes(f) + 4.0 * K * Cf, "incep_fc_kernel"):
            _lib.check(lib.hrv_inception_head_f32(f.t.data_ptr(), f.N, f.H * f.W, Cf, f.cstride, fc_w.data_ptr(), fc_b.data_ptr(), K,
                                                  pooled.data_ptr(), logits.data_ptr(), None if probs is None else probs.data_ptr(),
                                                  _stream()), "hrv_inception_head_f32")
        return logits, probs

    def pooled(self, f: Act, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The mean over H x W of the last feature map, fp32 [N, C], in the head's fixed pixel order (the head's first stage on its
        own).  ``out``: a contiguous fp32 [N, C] CUDA tensor to write into, e.g. rows of a feature bank."""
        assert f.coff == 0 and not f.bf16, (f.coff, f.t.dtype)
        if out is None:
            out = torch.empty((f.N, f.C), dtype=torch.float32, device=f.t.device)
        if out.shape != (f.N, f.C) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != f.t.device:
            raise HrvError(f"{type(self).__name__}.pooled: out must be a contiguous fp32 [{f.N}, {f.C}] tensor on {f.t.device}")
        lib = _lib.load()
        with ops._Timed("head", "inception_pool", 0.0, ops.act_bytes(f), "incep_mean_kernel"):
            _lib.check(lib.hrv_inception_pool_f32(f.t.data_ptr(), f.N, f.H * f.W, f.C, f.cstride, out.data_ptr(), _stream()),
                       "hrv_inception_pool_f32")
        return out

    def _check_mode(self):
        if self.training:
            raise NotImplementedError("Inception3: evaluation only on the HIP path (call .eval())")

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """x: fp32 NCHW [N,3,H,W] CUDA, already normalised (transform_input=False) -> logits [N,1000]."""
        self._check_mode()
        ops.require_cuda(x, "Inception3")
        if x.dtype != torch.float32 or x.dim() != 4 or x.shape[1] != 3:
            raise HrvError("Inception3: expected fp32 images [N,3,H,W]")
        with torch.no_grad():
            return self.head(self.features(ops.to_nhwc(x.detach())), False)[0]

    def forward_u8(self, img: torch.Tensor) -> torch.Tensor:
        """img: uint8 [N,H,W,3] CUDA images as decoded (evaluate.py's T3 minus the resize: ToTensor, Normalize(0.5, 0.5), in fp32
        ``x / 255``, ``- 0.5``, ``/ 0.5``) -> softmax probabilities fp32 [N,1000] (evaluate.py:76)."""
        self._check_mode()
        if not isinstance(img, torch.Tensor) or not img.is_cuda or img.dtype != torch.uint8 or img.dim() != 4 or img.shape[3] != 3:
            raise HrvError("Inception3: expected uint8 CUDA images [N,H,W,3]")
        N, H, W, _ = img.shape
        with torch.no_grad():
            x = torch.empty((N, H, W, 4), dtype=torch.float32, device=img.device)
            # the LPIPS input kernel with an identity ScalingLayer: (t - 0) / 1 is exact, so this is x / 255, - 0.5, / 0.5 and no more
            lib = _lib.load()
            _lib.check(lib.hrv_lpips_prep_u8(img.contiguous().data_ptr(), N, H, W, _ZERO3, _ONE3, x.data_ptr(), _stream()),
                       "hrv_lpips_prep_u8")
            return self.head(self.features(Act(x, 3)), True)[1]


class FIDInceptionV3(Inception3):
    """pytorch-fid's / torch-fidelity's FID Inception-v3 (``pt_inception-2015-12-05-6726825d.pth``) on the HIP path: ``Inception3``'s
    plan, stem and block runner over ``FID_POOLS``.  ``fc`` ([1008, 2048]) belongs to the state dict and is never run: the metric
    reads the pooled 2048-wide vector.  ``features_u8(img)``: uint8 [N,H,W,3] CUDA of any size -> fp32 [N, 2048]."""

    STATE_DICT_OF = "the FID Inception-v3 state dict, pt_inception-2015-12-05-6726825d.pth"
    POOLS = FID_POOLS

    def __init__(self):
        super().__init__(num_classes=FID_NUM_CLASSES, aux_logits=False, transform_input=False)

    def features_u8(self, img: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """img: uint8 [N,H,W,3] CUDA images as decoded, any size.  The input kernel resizes to 299x299 as pytorch-fid does
        (x / 255, bilinear with align_corners=False on the full-size image, 2v - 1); returns the mean over the last 8x8 map, fp32
        [N, 2048] (into ``out`` when given)."""
        self._check_mode()
        if not isinstance(img, torch.Tensor) or not img.is_cuda or img.dtype != torch.uint8 or img.dim() != 4 or img.shape[3] != 3:
            raise HrvError("FIDInceptionV3: expected uint8 CUDA images [N,H,W,3]")
        N, H, W, _ = img.shape
        with torch.no_grad():
            x = torch.empty((N, FID_SIZE, FID_SIZE, 4), dtype=torch.float32, device=img.device)
            lib = _lib.load()
            _lib.check(lib.hrv_fid_prep_u8(img.contiguous().data_ptr(), N, H, W, FID_SIZE, FID_SIZE, x.data_ptr(), _stream()),
                       "hrv_fid_prep_u8")
            return self.pooled(self.features(Act(x, 3)), out)


_ZERO3 = (C.c_float * 3)(0.0, 0.0, 0.0)
_ONE3 = (C.c_float * 3)(1.0, 1.0, 1.0)


def inception_v3(pretrained: bool = False, transform_input: bool = False, **kw) -> Inception3:
    """torchvision's constructor name.  ``pretrained=True`` would download: load a state dict from a file instead."""
    if pretrained:
        raise NotImplementedError("inception_v3(pretrained=True) downloads; load a torchvision state dict with load_state_dict()")
    return Inception3(transform_input=transform_input, **kw)
