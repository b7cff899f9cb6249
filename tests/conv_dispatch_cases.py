"""Case table, float64 reference and error limit of the convolution-dispatcher sweep (tests/test_gpu_conv_dispatch.py runs the
cases on the GPU, tests/test_conv_dispatch_cases_cpu.py pins the limit to the reference and checks the table,
tests/test_conv_dispatch_plan_cpu.py asks hr_viton_amd/conv_dispatch.py for every case's kernel without a GPU).  Plain module: no GPU.

The three entry points of hr_viton_amd/train_ops.py -- conv_forward_dev, conv_dgrad, conv_wgrad -- choose among about ten kernel
families by predicates that live half in Python and half in the C host code.  The table walks a shape across each predicate: one case
just inside, one just outside, only the quantity the gate reads changed.  Every case names the kernel family that has to serve it
(``ops.profile_end(kernels=True, variants=True)``), so a dispatch change has to be made on purpose, by editing this table.

Reference: torch.nn.functional.conv2d / torch.nn.grad.conv2d_input / conv2d_weight in float64 on the CPU over the operands as the
mode rounds them (mode "f32": unrounded; "mb" -- MMA_BF16 over fp32 tensors -- and "st" -- bf16-stored source / dY / output:
round-to-nearest-even bf16 of x, w, dY), epilogue terms in float64.

Statistic:  E = max |got - ref64| / A,  A = the same convolution over |x|, |w| (|dY|) plus |bias|, |residual|, |addends|.
Limit:      E <= min(LIMIT_U, 2 K) * 2^-24  (+ 2^-8 |ref64| per element of a bf16-stored output), K = products per output element.
LIMIT_U is NOT tuned on the kernels: it is 8 x the worst E a strictly sequential fp32 chain (numpy.cumsum, float32) and torch's own
fp32 CPU convolution reach against the float64 reference over THIS table (the CPU test asserts 4 x worst <= LIMIT_U <= 16 x worst).
Measured worst over this table: 3.97 * 2^-24 (torch's fp32 CPU weight gradient, wgrad-f32-xup-slice, K = 960; the sequential chain's
own worst is 2.7 * 2^-24); LIMIT_U = 32.  The factor 8 covers split-K / slab / two-stage
reductions that re-round partial sums, matrix-core accumulation whose internal rounding is not documented as round-to-nearest, and
trial-to-trial spread.  Inputs keep the products zero-mean (randn weights and dY; activations may be post-ReLU), for which the chain's
error does not grow with K.
"""
import math
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
LIMIT_U = 32.0
BF16_OUT = 2.0 ** -8

ACT_NONE, ACT_RELU, ACT_LRELU, ACT_TANH = 0, 1, 2, 3        # (hr_viton_amd._lib.ACT_*; asserted equal by the GPU test)
SLOPE = 0.2
POISON = -7168.0            # exact in bf16; what surrounds an output slice and must survive
SRC_POISON = 3.0e3          # finite junk around a SOURCE slice (a kernel may multiply a neighbour by a zero weight, never by a real one)

Case = namedtuple("Case", "id entry gate side mode family p env")

# ---------------------------------------------------------------------------------------------------------------------------------
# Gates walked (each has >= 1 inside and >= 1 outside case below; a gate's predicate: the function of hr_viton_amd/conv_dispatch.py
# whose docstring names the id)
# ---------------------------------------------------------------------------------------------------------------------------------
GATES = (
    # conv_forward_dev / _cout1_ok
    "fwd.cout1.Cout", "fwd.cout1.cin%4", "fwd.cout1.pad", "fwd.cout1.K<=4", "fwd.cout1.epilogue", "fwd.cout1.env",
    # _p2_fwd_ok / hrv_conv_p2_supported
    "fwd.p2.tiles", "fwd.p2.min_tiles_env", "fwd.p2.odd.Cout>=64", "fwd.p2.Cout%oal", "fwd.p2.act", "fwd.p2.nsrc", "fwd.p2.up0",
    "fwd.p2.out_up", "fwd.p2.kernel3x3", "fwd.p2.src_bf16", "fwd.p2.env",
    # _thin_ok / hrv_thin_conv_supported
    "fwd.thin.pixels", "fwd.thin.supported", "fwd.thin.env", "fwd.thin.1x1.kb",
    # generic engine tiles: ops.patch_tile, the 1x1 tile 6
    "fwd.patch.tiles512", "fwd.patch.c64pad", "fwd.patch.C%128", "fwd.patch.env", "fwd.tile6.Cout%64", "fwd.tile6.Cp<=128",
    # conv_dgrad
    "dgrad.cout1.res_mode", "dgrad.cout1.Cout", "dgrad.p2.tiles", "dgrad.p2.Cout%16", "dgrad.p2.odd.Cout>=64", "dgrad.p2.mask_bf16",
    "dgrad.p2.add", "dgrad.p2.stride", "dgrad.ride.env", "dgrad.ride.p2", "dgrad.thin.pixels", "dgrad.patch.tiles512",
    "dgrad.s2.phase",
    # conv_wgrad / hrv_conv2d_wgrad_route (wgrad_route, wgrad_tr_class, wgrad_s2_class)
    "wgrad.cout1.Cout", "wgrad.tr.pixels", "wgrad.tr.W>=32", "wgrad.tr.W>=32.odd", "wgrad.tr.x_granule", "wgrad.tr.dy_granule", "wgrad.s2.x_granule",
    "wgrad.tr.Cout%64", "wgrad.tr.Cp", "wgrad.tr.min_pix_env", "wgrad.tr.env",
    "wgrad.tr.x_up", "wgrad.tr.storage", "wgrad.s2.pixels", "wgrad.s2.Wo>=32", "wgrad.s2.Cout%128", "wgrad.s2.env",
    "wgrad.pad.bf16.Wo%4", "wgrad.pad.f32.Wo%4", "wgrad.pad.f32.Wo>=32",
)

# Gates NOT walked on both sides, with the reason (the far side is no legal input of any kernel, or cannot be built)
NOT_WALKED = {
    "a0.cstride % 8, a0.coff % 8 (bf16 source; forward and data gradient only)":
        "the forward / data-gradient engine and conv_p2 / thin_conv require the 16-byte granule of a bf16 source: the far side is HRV_ERR_ARG "
        "by contract (inside case: fwd-p2-srcslice).  The WEIGHT gradient is different -- its generic kernel takes 4-channel (8-byte) "
        "granules, so an off-granule slice is a legal input that the LDS-DMA kernels decline: gates wgrad.tr.x_granule, "
        "wgrad.tr.dy_granule and wgrad.s2.x_granule walk it",
    "out.cstride % oal, out.coff % oal": "an output slice off its 16-byte granule is rejected by every kernel (inside: fwd-p2-outslice)",
    "residual/add_after.data_ptr() % 16": "torch allocations are 256-byte aligned: the far side cannot be built without pointer surgery",
    "wgrad_s2 slab extent (31-bit offsets)": "needs one slab of >= 2 GiB: with Cout = 8192 (one slab) and X as a 64-channel slice of a "
                                             "16384-channel tensor, X alone is 2.1 GB and the float64 reference 279 GFLOP; not reachable at "
                                             "test size.  The check sits in wgrad_s2_class, which hrv_conv2d_wgrad_route and the launch both answer "
                                             "from (one predicate), so there is no accept-then-decline window left to test.",
    "wgrad_tr slab extent (31-bit offsets)": "as above; part of wgrad_tr_class",
    "cin <= 2048 (_cout1_ok)": "a 2052-channel fp32 source: no layer shape, and the far side is the generic engine already covered",
    "HRV_CONV_P2_WIDE=0, HRV_CONV_PATCHW, HRV_CONV_PATCH=16, HRV_CONV_TILE_TRAIN": "A/B and test knobs, off by default",
}


def _f(**kw):
    d = dict(N=1, H=16, W=16, srcs=((8, 0),), Cout=8, K=3, stride=1, pad=1, act=ACT_NONE, res=None, shift=True, out=None, out_up=0,
             out_bf16=False, src=None)
    d.update(kw)
    return d


def _d(**kw):
    d = dict(N=1, H=16, W=16, Cout=8, cin=8, K=3, stride=1, pad=1, mask=None, add=None, add_after=None, pair=False, out=None,
             out_bf16=False, dy=None)
    d.update(kw)
    return d


def _w(**kw):
    d = dict(N=1, H=16, W=16, Cout=8, C=8, K=3, stride=1, pad=1, x_up=0, ci_base=0, cin_tot=None, accumulate=False, dbias=True,
             dbias_accumulate=False, x=None, dy=None, dyl=None, Ho=None, Wo=None, x_bf16=None, ref_round=None)
    d.update(kw)
    return d


G8, G9 = "conv_mfma_kernel[tile 8]", "conv_mfma_kernel[tile 9]"
P2M0, P2M1, P2M2 = "conv_p2_kernel[mode 0]", "conv_p2_kernel[mode 1]", "conv_p2_kernel[mode 2]"
THIN, COUT1 = "thin_conv_kernel", "cout1_kernel"
NOP2 = {"HRV_CONV_P2": "0"}

# id, entry, gate (or ""), side ("in" / "out" / "-"), mode, expected family, parameters, environment switches
_FWD = (
    # ---- one-output-channel kernel (fp32 engine; PatchGAN's last convolution)
    ("fwd-cout1", "fwd.cout1.Cout", "in", "f32", COUT1, _f(H=20, W=17, srcs=((8, 0),), Cout=1, K=4, pad=2), {}),
    ("fwd-cout1-Cout2", "fwd.cout1.Cout", "out", "f32", "conv_mfma_kernel[tile 5]", _f(H=20, W=17, srcs=((8, 0),), Cout=2, K=4, pad=2), {}),
    ("fwd-cout1-mb", "fwd.cout1.cin%4", "in", "mb", COUT1, _f(H=20, W=17, srcs=((8, 0),), Cout=1, K=4, pad=2), {}),
    ("fwd-cout1-cin6", "fwd.cout1.cin%4", "out", "mb", G9, _f(H=20, W=17, srcs=((6, 0),), Cout=1, K=4, pad=2), {}),
    ("fwd-cout1-pad1", "fwd.cout1.pad", "in", "f32", COUT1, _f(H=20, W=17, Cout=1, K=3, pad=1), {}),
    ("fwd-cout1-pad0", "fwd.cout1.pad", "out", "f32", "conv_mfma_kernel[tile 5]", _f(H=20, W=17, Cout=1, K=3, pad=0), {}),
    ("fwd-cout1-K4", "fwd.cout1.K<=4", "in", "f32", COUT1, _f(H=20, W=17, Cout=1, K=4, pad=3), {}),
    ("fwd-cout1-K5", "fwd.cout1.K<=4", "out", "f32", "conv_mfma_kernel[tile 5]", _f(H=20, W=17, Cout=1, K=5, pad=3), {}),
    ("fwd-cout1-noepi", "fwd.cout1.epilogue", "in", "f32", COUT1, _f(H=9, W=33, Cout=1, K=4, pad=2, shift=False), {}),
    ("fwd-cout1-relu", "fwd.cout1.epilogue", "out", "f32", "conv_mfma_kernel[tile 5]", _f(H=9, W=33, Cout=1, K=4, pad=2, shift=False, act=ACT_RELU), {}),
    ("fwd-cout1-envon", "fwd.cout1.env", "in", "f32", COUT1, _f(H=12, W=12, Cout=1, K=4, pad=2), {"HRV_CONV_COUT1": "fwd"}),
    ("fwd-cout1-envoff", "fwd.cout1.env", "out", "f32", "conv_mfma_kernel[tile 5]", _f(H=12, W=12, Cout=1, K=4, pad=2), {"HRV_CONV_COUT1": "0"}),
    # ---- conv_p2, forward (bf16-stored source).  256 columns = 2 passes: 96 tiles of 16 x 16 pixels are the 192 units of the default
    #      HRV_CONV_P2_MIN_TILES_X4 = 3 on 256 CUs
    ("fwd-p2-tiles96", "fwd.p2.tiles", "in", "st", P2M0, _f(H=96, W=256, srcs=((32, 0),), Cout=256, act=ACT_RELU), {}),
    ("fwd-p2-tiles80", "fwd.p2.tiles", "out", "st", G8, _f(H=80, W=256, srcs=((32, 0),), Cout=256, act=ACT_RELU), {}),
    ("fwd-p2-x4-3", "fwd.p2.min_tiles_env", "in", "st", P2M0, _f(H=96, W=256, srcs=((32, 0),), Cout=256, out_bf16=True), {"HRV_CONV_P2_MIN_TILES_X4": "3"}),
    ("fwd-p2-x4-4", "fwd.p2.min_tiles_env", "out", "st", G8, _f(H=96, W=256, srcs=((32, 0),), Cout=256, out_bf16=True), {"HRV_CONV_P2_MIN_TILES_X4": "4"}),
    ("fwd-p2-odd-Cout64", "fwd.p2.odd.Cout>=64", "in", "st", P2M0, _f(H=192, W=256, srcs=((3, 0),), Cout=64, act=ACT_RELU), {}),
    ("fwd-p2-odd-Cout60", "fwd.p2.odd.Cout>=64", "out", "st", G9, _f(H=192, W=256, srcs=((3, 0),), Cout=60, act=ACT_RELU), {}),
    ("fwd-p2-Cout64-bf16out", "fwd.p2.Cout%oal", "in", "st", P2M0, _f(H=192, W=256, srcs=((32, 0),), Cout=64, out_bf16=True, act=ACT_LRELU), {}),
    ("fwd-p2-Cout60-f32out", "fwd.p2.Cout%oal", "in", "st", P2M0, _f(H=192, W=256, srcs=((32, 0),), Cout=60, act=ACT_LRELU), {}),
    ("fwd-p2-Cout62-f32out", "fwd.p2.Cout%oal", "out", "st", G9, _f(H=192, W=256, srcs=((32, 0),), Cout=62, act=ACT_LRELU), {}),
    ("fwd-p2-lrelu-res", "fwd.p2.act", "in", "st", P2M0, _f(H=96, W=256, srcs=((48, 0),), Cout=256, act=ACT_LRELU, res="f32"), {}),
    ("fwd-p2-tanh", "fwd.p2.act", "out", "st", G8, _f(H=96, W=256, srcs=((48, 0),), Cout=256, act=ACT_TANH), {}),
    ("fwd-p2-1src", "fwd.p2.nsrc", "in", "st", P2M0, _f(H=96, W=256, srcs=((32, 0),), Cout=256, res="bf16"), {}),
    ("fwd-p2-2src", "fwd.p2.nsrc", "out", "st", G8, _f(H=96, W=256, srcs=((16, 0), (16, 0)), Cout=256, res="bf16"), {}),
    ("fwd-p2-up0", "fwd.p2.up0", "in", "st", P2M0, _f(H=96, W=256, srcs=((32, 0),), Cout=256, shift=False), {}),
    ("fwd-p2-up1", "fwd.p2.up0", "out", "st", G8, _f(H=48, W=128, srcs=((32, 1),), Cout=256, shift=False), {}),
    ("fwd-p2-srcslice", "fwd.p2.out_up", "in", "st", P2M0, _f(H=96, W=256, srcs=((32, 0),), Cout=256, src=(48, 8)), {}),
    ("fwd-p2-outup1", "fwd.p2.out_up", "out", "st", G8, _f(H=96, W=256, srcs=((32, 0),), Cout=256, src=(48, 8), out_up=1), {}),
    ("fwd-p2-outslice", "fwd.p2.kernel3x3", "in", "st", P2M0, _f(H=96, W=256, srcs=((32, 0),), Cout=256, out=(272, 8, False)), {}),
    ("fwd-p2-s2", "fwd.p2.kernel3x3", "out", "st", G8, _f(H=96, W=256, srcs=((32, 0),), Cout=256, stride=2, out=(272, 8, False)), {}),
    ("fwd-p2-srcbf16", "fwd.p2.src_bf16", "in", "st", P2M0, _f(H=96, W=256, srcs=((64, 0),), Cout=256), {}),
    ("fwd-p2-srcf32", "fwd.p2.src_bf16", "out", "mb", G8, _f(H=96, W=256, srcs=((64, 0),), Cout=256), {}),
    ("fwd-p2-envon", "fwd.p2.env", "in", "st", P2M0, _f(H=96, W=256, srcs=((32, 0),), Cout=256, out=(256, 0, True)), {"HRV_CONV_P2": "1"}),
    ("fwd-p2-envoff", "fwd.p2.env", "out", "st", G8, _f(H=96, W=256, srcs=((32, 0),), Cout=256, out=(256, 0, True)), NOP2),
    # ---- thin_conv (bf16-stored source, >= 65536 pixels)
    ("fwd-thin-65536", "fwd.thin.pixels", "in", "st", THIN, _f(H=256, W=256, srcs=((16, 0),), Cout=32, act=ACT_LRELU), {}),
    ("fwd-thin-65280", "fwd.thin.pixels", "out", "st", G9, _f(H=255, W=256, srcs=((16, 0),), Cout=32, act=ACT_LRELU), {}),
    ("fwd-thin-kb2", "fwd.thin.supported", "in", "st", THIN, _f(H=256, W=256, srcs=((24, 0),), Cout=32, res="f32", out=(40, 4, False)), {}),
    ("fwd-thin-kb3", "fwd.thin.supported", "out", "st", P2M0, _f(H=256, W=256, srcs=((48, 0),), Cout=32, res="f32", out=(40, 4, False)), {}),
    ("fwd-thin-envon", "fwd.thin.env", "in", "st", THIN, _f(N=2, H=128, W=256, srcs=((9, 0),), Cout=16, out_bf16=True), {"HRV_THIN_CONV": "1"}),
    ("fwd-thin-envoff", "fwd.thin.env", "out", "st", G9, _f(N=2, H=128, W=256, srcs=((9, 0),), Cout=16, out_bf16=True), {"HRV_THIN_CONV": "0"}),
    ("fwd-thin-1x1-kb5", "fwd.thin.1x1.kb", "in", "st", THIN, _f(H=256, W=256, srcs=((72, 0),), Cout=24, K=1, pad=0, act=ACT_RELU), {}),
    ("fwd-thin-1x1-kb6", "fwd.thin.1x1.kb", "out", "st", G9, _f(H=256, W=256, srcs=((88, 0),), Cout=24, K=1, pad=0, act=ACT_RELU), {}),
    # ---- generic engine, LDS-resident patch tiles 17 / 18 (conv_p2 switched off: it takes every such layer first)
    ("fwd-patch-512", "fwd.patch.tiles512", "in", "st", "conv_mfma_kernel[tile 17]", _f(H=128, W=128, srcs=((128, 0),), Cout=512), NOP2),
    ("fwd-patch-480", "fwd.patch.tiles512", "out", "st", G8, _f(H=120, W=128, srcs=((128, 0),), Cout=512), NOP2),
    ("fwd-patch-pad32", "fwd.patch.c64pad", "in", "st", "conv_mfma_kernel[tile 18]", _f(H=96, W=240, srcs=((128, 0),), Cout=160, act=ACT_RELU), NOP2),
    ("fwd-patch-pad33", "fwd.patch.c64pad", "out", "st", G9, _f(H=96, W=240, srcs=((128, 0),), Cout=159, act=ACT_RELU), NOP2),
    ("fwd-patch-C128", "fwd.patch.C%128", "in", "st", "conv_mfma_kernel[tile 18]", _f(H=96, W=240, srcs=((128, 0),), Cout=192, res="f32"), NOP2),
    ("fwd-patch-C120", "fwd.patch.C%128", "out", "st", G9, _f(H=96, W=240, srcs=((120, 0),), Cout=192, res="f32"), NOP2),
    ("fwd-patch-envon", "fwd.patch.env", "in", "st", "conv_mfma_kernel[tile 17]", _f(N=2, H=64, W=128, srcs=((128, 0),), Cout=512, out_bf16=True), NOP2),
    ("fwd-patch-envoff", "fwd.patch.env", "out", "st", G8, _f(N=2, H=64, W=128, srcs=((128, 0),), Cout=512, out_bf16=True),
     {"HRV_CONV_P2": "0", "HRV_CONV_PATCH": "0"}),
    # ---- generic engine, the 1x1 tile 6
    ("fwd-tile6-Cout64", "fwd.tile6.Cout%64", "in", "st", "conv_mfma_kernel[tile 6]", _f(H=40, W=36, srcs=((64, 0),), Cout=64, K=1, pad=0), {}),
    ("fwd-tile6-Cout96", "fwd.tile6.Cout%64", "out", "st", G8, _f(H=40, W=36, srcs=((64, 0),), Cout=96, K=1, pad=0), {}),
    ("fwd-tile6-Cp128", "fwd.tile6.Cp<=128", "in", "st", "conv_mfma_kernel[tile 6]", _f(H=40, W=36, srcs=((128, 0),), Cout=64, K=1, pad=0, act=ACT_RELU), {}),
    ("fwd-tile6-Cp136", "fwd.tile6.Cp<=128", "out", "st", G9, _f(H=40, W=36, srcs=((136, 0),), Cout=64, K=1, pad=0, act=ACT_RELU), {}),
    # ---- generic engine, storage modes and epilogues that no gate above reaches
    ("fwd-f32-2src-up", "", "-", "f32", "conv_mfma_kernel[tile 5]", _f(N=2, H=24, W=20, srcs=((12, 0), (20, 1)), Cout=24, act=ACT_LRELU, res="f32"), {}),
    ("fwd-f32-s2-4x4", "", "-", "f32", "conv_mfma_kernel[tile 6]", _f(N=2, H=33, W=27, srcs=((16, 0),), Cout=40, K=4, stride=2, pad=2, act=ACT_LRELU), {}),
    ("fwd-f32-outup-slice", "", "-", "f32", "conv_mfma_kernel[tile 5]", _f(H=24, W=20, srcs=((16, 0),), Cout=20, out_up=1, out=(32, 8, False), act=ACT_RELU), {}),
    ("fwd-f32-wide", "", "-", "f32", "conv_mfma_kernel[tile 0]", _f(H=64, W=48, srcs=((64, 0),), Cout=128, res="f32"), {}),
    ("fwd-mb-2src-up", "", "-", "mb", G9, _f(N=2, H=24, W=20, srcs=((12, 0), (20, 1)), Cout=24, act=ACT_LRELU, res="f32"), {}),
    ("fwd-mb-outup-slice", "", "-", "mb", G9, _f(H=24, W=20, srcs=((16, 0),), Cout=20, out_up=1, out=(32, 8, False), act=ACT_RELU), {}),
    ("fwd-mb-s2-4x4", "", "-", "mb", G9, _f(N=2, H=33, W=27, srcs=((16, 0),), Cout=40, K=4, stride=2, pad=2), {}),
    ("fwd-st-bf16out-slice", "", "-", "st", G8, _f(H=40, W=36, srcs=((64, 0),), Cout=128, out=(144, 8, True), res="bf16", act=ACT_RELU), {}),
)

_DGRAD = (
    ("dgrad-cout1", "dgrad.cout1.res_mode", "in", "f32", COUT1, _d(H=20, W=17, Cout=1, cin=8, K=4, pad=2, add=True), {}),
    ("dgrad-cout1-mask", "dgrad.cout1.res_mode", "out", "f32", "conv_mfma_kernel[tile 5]", _d(H=20, W=17, Cout=1, cin=8, K=4, pad=2, mask="f32"), {}),
    ("dgrad-cout1-plain", "dgrad.cout1.Cout", "in", "mb", COUT1, _d(H=20, W=17, Cout=1, cin=8, K=4, pad=2), {}),
    ("dgrad-cout1-Cout2", "dgrad.cout1.Cout", "out", "mb", G9, _d(H=20, W=17, Cout=2, cin=8, K=4, pad=2), {}),
    # ---- conv_p2 modes 1 / 2 (bf16-stored dY); 64 columns = 1 pass: 192 tiles
    ("dgrad-p2-192", "dgrad.p2.tiles", "in", "st", P2M1, _d(H=192, W=256, Cout=64, cin=64, mask="bf16"), {}),
    ("dgrad-p2-176", "dgrad.p2.tiles", "out", "st", G9, _d(H=176, W=256, Cout=64, cin=64, mask="bf16"), {}),
    ("dgrad-p2-Cout80", "dgrad.p2.Cout%16", "in", "st", P2M1, _d(H=192, W=256, Cout=80, cin=32, out_bf16=True), {}),
    ("dgrad-p2-Cout72", "dgrad.p2.Cout%16", "out", "st", G9, _d(H=192, W=256, Cout=72, cin=32, out_bf16=True), {}),
    ("dgrad-p2-odd-Cout64", "dgrad.p2.odd.Cout>=64", "in", "st", P2M1, _d(H=192, W=256, Cout=64, cin=3), {}),
    ("dgrad-p2-odd-Cout48", "dgrad.p2.odd.Cout>=64", "out", "st", G9, _d(H=192, W=256, Cout=48, cin=3), {}),
    ("dgrad-p2-pair-mask", "dgrad.p2.mask_bf16", "in", "st", P2M2, _d(H=192, W=256, Cout=64, cin=64, pair=True, mask="bf16"), {}),
    ("dgrad-p2-pair-maskf32", "dgrad.p2.mask_bf16", "out", "st", G9, _d(H=192, W=256, Cout=64, cin=64, pair=True, mask="f32"), {}),
    ("dgrad-p2-noadd", "dgrad.p2.add", "in", "st", P2M1, _d(H=192, W=256, Cout=32, cin=64, out=(80, 8, False)), {}),
    ("dgrad-p2-add", "dgrad.p2.add", "out", "st", G9, _d(H=192, W=256, Cout=32, cin=64, out=(80, 8, False), add=True), {}),
    ("dgrad-p2-dyslice", "dgrad.p2.stride", "in", "st", P2M1, _d(H=192, W=256, Cout=32, cin=32, dy=(48, 16)), {}),
    ("dgrad-st-s2", "dgrad.p2.stride", "out", "st", G9, _d(H=192, W=256, Cout=32, cin=32, dy=(48, 16), stride=2, K=4, pad=2), {}),
    # ---- add_after: rides in conv_p2's epilogue behind the mask, else a separate add_slice pass
    ("dgrad-ride", "dgrad.ride.env", "in", "st", P2M1, _d(H=192, W=256, Cout=64, cin=64, mask="bf16", add_after=True), {}),
    ("dgrad-ride-envoff", "dgrad.ride.env", "out", "st", P2M1, _d(H=192, W=256, Cout=64, cin=64, mask="bf16", add_after=True), {"HRV_DGRAD_ADD_AFTER": "0"}),
    ("dgrad-ride-nomask", "dgrad.ride.p2", "in", "st", P2M1, _d(H=192, W=256, Cout=64, cin=32, add_after=True), {}),
    ("dgrad-noride-small", "dgrad.ride.p2", "out", "st", G9, _d(H=176, W=256, Cout=64, cin=32, add_after=True), {}),
    # ---- thin_conv mode 1 (conv_p2 off: it takes the layer first) and the patch tile
    ("dgrad-thin-65536", "dgrad.thin.pixels", "in", "st", THIN, _d(H=256, W=256, Cout=32, cin=80, mask="f32"), NOP2),
    ("dgrad-thin-65280", "dgrad.thin.pixels", "out", "st", G8, _d(H=255, W=256, Cout=32, cin=80, mask="f32"), NOP2),
    ("dgrad-patch-512", "dgrad.patch.tiles512", "in", "st", "conv_mfma_kernel[tile 17]", _d(H=128, W=128, Cout=128, cin=512), NOP2),
    ("dgrad-patch-480", "dgrad.patch.tiles512", "out", "st", G8, _d(H=120, W=128, Cout=128, cin=512), NOP2),
    # ---- stride 2: the four phases; odd extents; H == 1 / W == 1 leave a phase empty
    ("dgrad-f32-s2-odd", "dgrad.s2.phase", "in", "f32", "conv_mfma_kernel[tile 5]", _d(N=2, H=33, W=27, Cout=40, cin=16, K=4, stride=2, pad=2, mask="f32"), {}),
    ("dgrad-f32-s2-H1", "dgrad.s2.phase", "out", "f32", "conv_mfma_kernel[tile 5]", _d(N=2, H=1, W=27, Cout=40, cin=16, K=4, stride=2, pad=2, mask="f32"), {}),
    ("dgrad-mb-s2-W1", "", "-", "mb", G9, _d(N=2, H=33, W=1, Cout=40, cin=16, K=3, stride=2, pad=1, add=True), {}),
    ("dgrad-mb-s2-odd", "", "-", "mb", G9, _d(N=2, H=33, W=27, Cout=40, cin=16, K=3, stride=2, pad=1), {}),
    # ---- generic engine, stride 1
    ("dgrad-f32-mask-slice", "", "-", "f32", "conv_mfma_kernel[tile 5]", _d(N=2, H=24, W=20, Cout=24, cin=20, mask="f32", out=(32, 4, False)), {}),
    ("dgrad-f32-pair", "", "-", "f32", "conv_mfma_kernel[tile 5]", _d(N=2, H=24, W=20, Cout=32, cin=20, pair=True), {}),
    ("dgrad-mb-pair-add", "", "-", "mb", G9, _d(N=2, H=24, W=20, Cout=32, cin=20, pair=True, add=True), {}),
    ("dgrad-mb-addafter", "", "-", "mb", G9, _d(N=2, H=24, W=20, Cout=24, cin=20, mask="f32", add_after=True), {}),
    ("dgrad-f32-1x1", "", "-", "f32", "conv_mfma_kernel[tile 5]", _d(N=2, H=24, W=20, Cout=24, cin=20, K=1, pad=0), {}),
)

TR = "conv_wgrad_tr_kernel[class %d]"
WG_F32, WG_BF16, WG_ST, WG_XST = ("conv_wgrad_kernel[fp32]", "conv_wgrad_kernel[bf16]", "conv_wgrad_kernel[bf16 stored]",
                                  "conv_wgrad_kernel[bf16 x-stored]")
_C8 = dict(K=2, pad=1, C=48, Cout=64)         # the 2x2 class: PatchGAN's model0 over its space-to-depth image (Ho, Wo) == (H, W)

_WGRAD = (
    ("wgrad-cout1", "wgrad.cout1.Cout", "in", "f32", COUT1, _w(N=2, H=20, W=17, Cout=1, C=8, K=4, pad=2, Ho=21, Wo=18), {}),
    ("wgrad-cout2", "wgrad.cout1.Cout", "out", "f32", WG_F32, _w(N=2, H=20, W=17, Cout=2, C=8, K=4, pad=2, Ho=21, Wo=18), {}),
    # ---- every wgrad_tr class (bf16-stored dY and X)
    ("wgrad-tr0", "wgrad.tr.pixels", "in", "st", TR % 0, _w(H=64, W=128, Cout=40, C=128), {}),
    ("wgrad-tr0-8064", "wgrad.tr.pixels", "out", "st", WG_ST, _w(H=63, W=128, Cout=40, C=128), {}),
    ("wgrad-tr1", "wgrad.tr.storage", "in", "st", TR % 1, _w(H=64, W=128, Cout=32, C=80), {}),
    ("wgrad-tr1-xonly", "wgrad.tr.storage", "out", "st", WG_XST, _w(H=64, W=128, Cout=32, C=80, dy="f32"), {}),
    ("wgrad-tr2", "wgrad.tr.x_up", "in", "st", TR % 2, _w(N=2, H=64, W=64, Cout=24, C=32, ci_base=8, cin_tot=48, accumulate=True), {}),
    ("wgrad-tr2-xup", "wgrad.tr.x_up", "out", "st", WG_ST, _w(N=2, H=64, W=64, Cout=24, C=32, ci_base=8, cin_tot=48, accumulate=True, x_up=1), {}),
    ("wgrad-tr3", "", "-", "st", TR % 3, _w(H=64, W=128, Cout=16, C=72, K=1, pad=0, dbias_accumulate=True), {}),
    ("wgrad-tr4", "", "-", "st", TR % 4, _w(H=64, W=128, Cout=64, C=144), {}),
    ("wgrad-tr5", "wgrad.tr.Cout%64", "in", "st", TR % 5, _w(H=64, W=128, Cout=64, C=64), {}),
    ("wgrad-tr5-Cout60", "wgrad.tr.Cout%64", "out", "st", WG_ST, _w(H=64, W=128, Cout=60, C=64), {}),
    ("wgrad-tr5-slice", "wgrad.tr.Cp", "in", "st", TR % 5, _w(H=64, W=128, Cout=64, C=64, x=(192, 64), dbias=False), {}),
    ("wgrad-tr5-Cp72", "wgrad.tr.Cp", "out", "st", WG_ST, _w(H=64, W=128, Cout=64, C=68, x=(192, 64), dbias=False), {}),
    # ---- a bf16 slice on and off the 8-element (16-byte) granule: off it the LDS-DMA kernel declines and the generic kernel, which
    #      reads 4-channel groups, serves the layer
    ("wgrad-tr5-xcoff64", "wgrad.tr.x_granule", "in", "st", TR % 5, _w(H=64, W=128, Cout=64, C=64, x=(200, 64)), {}),
    ("wgrad-tr5-xcoff68", "wgrad.tr.x_granule", "out", "st", WG_ST, _w(H=64, W=128, Cout=64, C=64, x=(200, 68)), {}),
    ("wgrad-tr5-xcstride204", "wgrad.tr.x_granule", "out", "st", WG_ST, _w(H=64, W=128, Cout=64, C=64, x=(204, 64)), {}),
    ("wgrad-tr5-dycoff8", "wgrad.tr.dy_granule", "in", "st", TR % 5, _w(H=64, W=128, Cout=64, C=64, dyl=(80, 8)), {}),
    ("wgrad-tr5-dycoff4", "wgrad.tr.dy_granule", "out", "st", WG_ST, _w(H=64, W=128, Cout=64, C=64, dyl=(80, 4)), {}),
    # ---- widths that are not multiples of 4 on the 3x3 classes (the kernel masks the tail of a 64-pixel row segment per pixel)
    ("wgrad-tr0-W34", "", "-", "st", TR % 0, _w(H=241, W=34, Cout=40, C=128), {}),
    ("wgrad-tr4-W34", "", "-", "st", TR % 4, _w(H=241, W=34, Cout=64, C=144), {}),
    ("wgrad-tr5-W34", "", "-", "st", TR % 5, _w(H=241, W=34, Cout=64, C=64), {}),
    ("wgrad-tr6-W37", "", "-", "st", TR % 6, _w(H=222, W=37, Cout=64, C=272, dbias=False), {}),
    ("wgrad-tr7-W67", "", "-", "st", TR % 7, _w(H=123, W=67, Cout=64, C=256), {}),
    ("wgrad-tr6", "", "-", "st", TR % 6, _w(H=64, W=128, Cout=64, C=272), {}),
    ("wgrad-tr7", "", "-", "st", TR % 7, _w(H=64, W=128, Cout=64, C=256), {}),
    # ---- the 2x2 class and the cases where conv_wgrad's own predicate used to say yes and wgrad_tr_try no: the fallback's
    #      correct answer is expected, not an error
    ("wgrad-tr8-W32", "wgrad.tr.W>=32", "in", "st", TR % 8, _w(H=256, W=32, **_C8), {}),
    ("wgrad-tr8-W28", "wgrad.tr.W>=32", "out", "st", WG_ST, _w(H=293, W=28, **_C8), {}),
    ("wgrad-tr8-W33", "wgrad.tr.W>=32.odd", "in", "st", TR % 8, _w(H=249, W=33, **_C8), {}),
    ("wgrad-tr8-W31", "wgrad.tr.W>=32.odd", "out", "st", WG_ST, _w(H=265, W=31, **_C8), {}),
    ("wgrad-tr8-W34", "", "-", "st", TR % 8, _w(H=250, W=34, **_C8), {}),
    ("wgrad-tr8-W30", "", "-", "st", WG_ST, _w(H=280, W=30, **_C8), {}),
    ("wgrad-tr8-minpix-default", "wgrad.tr.min_pix_env", "in", "st", TR % 8, _w(H=129, W=65, **_C8), {}),
    ("wgrad-tr8-minpix-raised", "wgrad.tr.min_pix_env", "out", "st", WG_ST, _w(H=129, W=65, **_C8), {"HRV_WGRAD_TR_MIN_PIX": "16384"}),
    ("wgrad-tr8-envon", "wgrad.tr.env", "in", "st", TR % 8, _w(N=2, H=65, W=65, **_C8), {"HRV_WGRAD_TR": "1"}),
    ("wgrad-tr8-envoff", "wgrad.tr.env", "out", "st", WG_ST, _w(N=2, H=65, W=65, **_C8), {"HRV_WGRAD_TR": "0"}),
    # ---- wgrad_s2 (4x4 stride 2 pad 2, bf16-stored dY and X)
    ("wgrad-s2-c1", "wgrad.s2.pixels", "in", "st", "conv_wgrad_s2_kernel", _w(H=254, W=130, Cout=128, C=64, K=4, stride=2, pad=2), {}),
    ("wgrad-s2-c1-8184", "wgrad.s2.pixels", "out", "st", WG_ST, _w(H=246, W=130, Cout=128, C=64, K=4, stride=2, pad=2), {}),
    ("wgrad-s2-c2", "wgrad.s2.Wo>=32", "in", "st", "conv_wgrad_s2_kernel", _w(H=512, W=62, Cout=64, C=128, K=4, stride=2, pad=2), {}),
    ("wgrad-s2-c2-Wo31", "wgrad.s2.Wo>=32", "out", "st", WG_ST, _w(H=530, W=60, Cout=64, C=128, K=4, stride=2, pad=2), {}),
    ("wgrad-s2-Cout128", "wgrad.s2.Cout%128", "in", "st", "conv_wgrad_s2_kernel",
     _w(H=254, W=130, Cout=128, C=64, K=4, stride=2, pad=2, accumulate=True, dbias_accumulate=True), {}),
    ("wgrad-s2-Cout64", "wgrad.s2.Cout%128", "out", "st", WG_ST,
     _w(H=254, W=130, Cout=64, C=64, K=4, stride=2, pad=2, accumulate=True, dbias_accumulate=True), {}),
    ("wgrad-s2-xcoff64", "wgrad.s2.x_granule", "in", "st", "conv_wgrad_s2_kernel", _w(H=254, W=126, Cout=128, C=64, K=4, stride=2, pad=2, x=(200, 64)), {}),
    ("wgrad-s2-xcoff68", "wgrad.s2.x_granule", "out", "st", WG_ST, _w(H=254, W=126, Cout=128, C=64, K=4, stride=2, pad=2, x=(200, 68)), {}),
    ("wgrad-s2-envon", "wgrad.s2.env", "in", "st", "conv_wgrad_s2_kernel", _w(H=254, W=130, Cout=64, C=128, K=4, stride=2, pad=2), {"HRV_WGRAD_S2": "1"}),
    ("wgrad-s2-envoff", "wgrad.s2.env", "out", "st", WG_ST, _w(H=254, W=130, Cout=64, C=128, K=4, stride=2, pad=2), {"HRV_WGRAD_S2": "0"}),
    # ---- the generic kernels and both width-padding routes
    ("wgrad-st-Wo36", "wgrad.pad.bf16.Wo%4", "in", "st", WG_ST, _w(N=2, H=20, W=36, Cout=24, C=40), {}),
    ("wgrad-st-Wo37", "wgrad.pad.bf16.Wo%4", "out", "st", WG_ST, _w(N=2, H=20, W=37, Cout=24, C=40), {}),
    ("wgrad-mb-Wo36", "wgrad.pad.f32.Wo%4", "in", "mb", WG_BF16, _w(N=2, H=20, W=36, Cout=24, C=20), {}),
    ("wgrad-mb-Wo37", "wgrad.pad.f32.Wo%4", "out", "mb", WG_BF16, _w(N=2, H=20, W=37, Cout=24, C=20), {}),
    ("wgrad-mb-Wo33", "wgrad.pad.f32.Wo>=32", "in", "mb", WG_BF16, _w(N=2, H=20, W=33, Cout=24, C=20), {}),
    ("wgrad-mb-Wo31", "wgrad.pad.f32.Wo>=32", "out", "mb", WG_F32, _w(N=2, H=20, W=31, Cout=24, C=20, ref_round=False), {}),
    ("wgrad-f32-xup-slice", "", "-", "f32", WG_F32, _w(N=2, H=12, W=10, Cout=24, C=20, x_up=1, ci_base=12, cin_tot=40, accumulate=True), {}),
    ("wgrad-mb-xup-slice", "", "-", "mb", WG_BF16, _w(N=2, H=12, W=10, Cout=24, C=20, x_up=1, ci_base=12, cin_tot=40, dbias_accumulate=True), {}),
    ("wgrad-f32-s2-4x4", "", "-", "f32", WG_F32, _w(N=2, H=33, W=27, Cout=40, C=16, K=4, stride=2, pad=2), {}),
    ("wgrad-f32-1x1", "", "-", "f32", WG_F32, _w(N=2, H=24, W=20, Cout=24, C=20, K=1, pad=0, dbias=False), {}),
)


def _mk(rows, entry):
    out = []
    for cid, gate, side, mode, fam, p, env in rows:
        p = dict(p)
        p.pop("H_", None)
        out.append(Case(cid, entry, gate, side, mode, fam, p, dict(env)))
    return tuple(out)


FWD_CASES, DGRAD_CASES, WGRAD_CASES = _mk(_FWD, "fwd"), _mk(_DGRAD, "dgrad"), _mk(_WGRAD, "wgrad")
CASES = FWD_CASES + DGRAD_CASES + WGRAD_CASES
BY_ID = {c.id: c for c in CASES}

# every kernel family (with its variant) the three entry points can choose: each has to be expected by at least one case, and no case
# may expect another
FAMILIES = (COUT1, P2M0, P2M1, P2M2, THIN, G8, G9, "conv_mfma_kernel[tile 0]", "conv_mfma_kernel[tile 5]", "conv_mfma_kernel[tile 6]",
            "conv_mfma_kernel[tile 17]", "conv_mfma_kernel[tile 18]", "conv_wgrad_s2_kernel", WG_F32, WG_BF16, WG_ST,
            WG_XST) + tuple(TR % i for i in range(9))
# Launches next to the convolution that tell the two sides of a gate apart where both are served by the same family:
# case id -> ((record kind, record name or "" for any, count), ...) among the records of ops.profile_end
LAUNCHES = {
    "dgrad-ride": (("ew", "add_slice", 0), ("conv", "", 1)), "dgrad-ride-nomask": (("ew", "add_slice", 0), ("conv", "", 1)),
    "dgrad-ride-envoff": (("ew", "add_slice", 1), ("conv", "", 1)), "dgrad-noride-small": (("ew", "add_slice", 1), ("conv", "", 1)),
    "dgrad-mb-addafter": (("ew", "add_slice", 1),),
    "dgrad-f32-s2-odd": (("conv", "", 4),), "dgrad-f32-s2-H1": (("conv", "", 2),), "dgrad-mb-s2-W1": (("conv", "", 2),),
    "dgrad-mb-s2-odd": (("conv", "", 4),), "dgrad-st-s2": (("conv", "", 4),),
    "wgrad-st-Wo36": (("layout", "pad_width", 0),), "wgrad-st-Wo37": (("layout", "pad_width", 1),),
    "wgrad-mb-Wo36": (("layout", "pad_width", 0),), "wgrad-mb-Wo37": (("layout", "pad_width", 1),),
    "wgrad-mb-Wo33": (("layout", "pad_width", 1),), "wgrad-mb-Wo31": (("layout", "pad_width", 0),),
    "wgrad-tr8-W28": (("layout", "pad_width", 0),), "wgrad-tr8-W30": (("layout", "pad_width", 1),),
    "wgrad-tr8-W31": (("layout", "pad_width", 1),), "wgrad-tr8-minpix-raised": (("layout", "pad_width", 1),),
    "wgrad-tr8-envoff": (("layout", "pad_width", 1),), "wgrad-tr8-W33": (("layout", "pad_width", 0),),
    "wgrad-s2-c2-Wo31": (("layout", "pad_width", 1),), "wgrad-s2-c2": (("layout", "pad_width", 0),),
}
# the cases where conv_wgrad's own predicate said yes at the parent commit and the C launch path no
ACCEPT_THEN_DECLINE = ("wgrad-tr8-W30", "wgrad-tr8-W31", "wgrad-tr8-minpix-raised", "wgrad-tr8-envoff")


# ---------------------------------------------------------------------------------------------------------------------------------
# operands, rounding, reference
# ---------------------------------------------------------------------------------------------------------------------------------
def bf16_round(t):
    return t.to(torch.bfloat16).to(t.dtype)


def bf16_trunc(t):
    """the WRONG rounding (mutation check): the low 16 bits dropped"""
    return (t.to(torch.float32).contiguous().view(torch.int32) & -65536).view(torch.float32).to(t.dtype)


def _seed(c):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(c.id)) % (2 ** 31)


def out_hw(p):
    if p.get("Ho"):
        return p["Ho"], p["Wo"]
    return (p["H"] + 2 * p["pad"] - p["K"]) // p["stride"] + 1, (p["W"] + 2 * p["pad"] - p["K"]) // p["stride"] + 1


def wgrad_out_hw(p):
    """dY extent of a weight-gradient case: the convolution's own, except the 2x2 class, whose (Ho, Wo) == (H, W) (a 'same' 2x2 with
    the zero border on the top / left only)"""
    if p.get("Ho"):
        return p["Ho"], p["Wo"]
    H, W = p["H"] << p["x_up"], p["W"] << p["x_up"]
    if p["K"] == 2 and p["pad"] == 1:
        return H, W
    return (H + 2 * p["pad"] - p["K"]) // p["stride"] + 1, (W + 2 * p["pad"] - p["K"]) // p["stride"] + 1


def make_inputs(c):
    """fp32 CPU operands of a case (NCHW / OIHW), deterministic per case id.  Activations are post-ReLU randn, weights and dY randn:
    zero-mean products.  In mode "st" the stored tensors hold bf16 values already."""
    g = torch.Generator().manual_seed(_seed(c))
    p, st = c.p, c.mode == "st"
    rn = lambda *s: torch.randn(*s, generator=g)
    q = (lambda t: bf16_round(t)) if st else (lambda t: t)
    d = {}
    if c.entry == "fwd":
        cin = sum(ch for ch, _ in p["srcs"])
        Hf, Wf = p["H"] << p["srcs"][0][1], p["W"] << p["srcs"][0][1]      # (H, W: the FIRST source's own extent)
        d["xs"] = [q(rn(p["N"], ch, Hf >> up, Wf >> up).relu()) for ch, up in p["srcs"]]
        d["w"] = rn(p["Cout"], cin, p["K"], p["K"]) / math.sqrt(cin * p["K"] * p["K"])
        d["shift"] = rn(p["Cout"]) if p["shift"] else None
        H, W = p["H"] << p["srcs"][0][1], p["W"] << p["srcs"][0][1]
        Ho, Wo = (H + 2 * p["pad"] - p["K"]) // p["stride"] + 1, (W + 2 * p["pad"] - p["K"]) // p["stride"] + 1
        r = rn(p["N"], p["Cout"], Ho, Wo) if p["res"] else None
        d["res"] = bf16_round(r) if p["res"] == "bf16" else r
    elif c.entry == "dgrad":
        Ho, Wo = out_hw(p)
        d["dy"] = q(rn(p["N"], p["Cout"], Ho, Wo))
        sc = 1.0 / math.sqrt(p["Cout"] * p["K"] * p["K"])
        if p["pair"]:
            d["w"] = (rn(p["Cout"] // 2, p["cin"], p["K"], p["K"]) * sc, rn(p["Cout"] // 2, p["cin"], p["K"], p["K"]) * sc)
        else:
            d["w"] = rn(p["Cout"], p["cin"], p["K"], p["K"]) * sc
        shp = (p["N"], p["cin"], p["H"], p["W"])
        m = rn(*shp) if p["mask"] else None
        d["mask"] = bf16_round(m) if p["mask"] == "bf16" else m
        d["add"] = rn(*shp) if p["add"] else None
        d["add_after"] = rn(*shp) if p["add_after"] else None
    else:
        Ho, Wo = wgrad_out_hw(p)
        d["x"] = q(rn(p["N"], p["C"], p["H"], p["W"]).relu())
        dy = rn(p["N"], p["Cout"], Ho, Wo)
        d["dy"] = dy if p["dy"] == "f32" else q(dy)
        ct = p["cin_tot"] or p["C"]
        d["dw0"] = rn(p["Cout"], ct, p["K"], p["K"])          # prior contents of dW (accumulate) / poison pattern (else)
        d["db0"] = rn(p["Cout"])
    return d


def _rounder(c, trunc=False):
    if c.mode == "f32" or c.p.get("ref_round") is False:
        return lambda t: t
    return bf16_trunc if trunc else bf16_round


def _up(t, s):
    return t if s == 0 else t.repeat_interleave(1 << s, 2).repeat_interleave(1 << s, 3)


def _act64(y, act):
    if act == ACT_RELU:
        return y.clamp_min(0)
    if act == ACT_LRELU:
        return torch.where(y > 0, y, y * SLOPE)
    if act == ACT_TANH:
        return torch.tanh(y)
    return y


def _wgrad_xpad(p, x):
    """X of a weight-gradient case, upsampled and zero-bordered so that a pad-0 convolution yields exactly the case's dY extent"""
    x = _up(x, p["x_up"])
    H, W = x.shape[2], x.shape[3]
    Ho, Wo = wgrad_out_hw(p)
    pb = (Ho - 1) * p["stride"] + p["K"] - H - p["pad"]
    pr = (Wo - 1) * p["stride"] + p["K"] - W - p["pad"]
    return F.pad(x, (p["pad"], pr, p["pad"], pb))


def operands(c, d, trunc=False, dtype=torch.float64):
    """the operands of the case's convolution as the mode rounds them, in ``dtype``: fwd (x, w), dgrad (dy, w), wgrad (xpad, dy)"""
    r = _rounder(c, trunc)
    p = c.p
    if c.entry == "fwd":
        x = torch.cat([_up(r(t), up) for t, (_, up) in zip(d["xs"], p["srcs"])], 1)
        return x.to(dtype), r(d["w"]).to(dtype)
    if c.entry == "dgrad":
        w = torch.cat(d["w"], 0) if p["pair"] else d["w"]
        return r(d["dy"]).to(dtype), r(w).to(dtype)
    return _wgrad_xpad(p, r(d["x"])).to(dtype), r(d["dy"]).to(dtype)


def _lin(c, a, b):
    """the linear part of the case on operands (a, b) of one dtype"""
    p = c.p
    if c.entry == "fwd":
        return F.conv2d(a, b, None, p["stride"], p["pad"])
    if c.entry == "dgrad":
        return torch.nn.grad.conv2d_input((p["N"], p["cin"], p["H"], p["W"]), b, a, p["stride"], p["pad"])
    return torch.nn.grad.conv2d_weight(a, (p["Cout"], p["C"], p["K"], p["K"]), b, p["stride"], 0)


def k_terms(c):
    p = c.p
    if c.entry == "fwd":
        return sum(ch for ch, _ in p["srcs"]) * p["K"] ** 2
    if c.entry == "dgrad":
        return p["Cout"] * p["K"] ** 2
    Ho, Wo = wgrad_out_hw(p)
    return p["N"] * Ho * Wo


def epilogue(c, d, lin, A):
    """(ref64, A64) of the entry point's result from its linear part: bias / residual / activation / upsampled store (fwd); mask,
    addends (dgrad).  A scales with what multiplies the accumulated value."""
    p = c.p
    if c.entry == "fwd":
        y = lin
        if d["shift"] is not None:
            y = y + d["shift"].double().view(1, -1, 1, 1)
            A = A + d["shift"].double().abs().view(1, -1, 1, 1)
        if d["res"] is not None:
            y = y + d["res"].double()
            A = A + d["res"].double().abs()
        if p["act"] == ACT_LRELU:       # (a clearly negative pre-activation scales its error by the slope as well)
            A = torch.where(y < -LIMIT_U * U * A, A * SLOPE, A)
        y = _act64(y, p["act"])
        return _up(y, p["out_up"]), _up(A, p["out_up"])
    if c.entry == "dgrad":
        y = lin
        if d["mask"] is not None:
            f = torch.where(d["mask"].double() > 0, 1.0, SLOPE)
            y, A = y * f, A * f
        for k in ("add", "add_after"):
            if d[k] is not None:
                y = y + d[k].double()
                A = A + d[k].double().abs()
        return y, A
    return lin, A


def reference(c, d, trunc=False):
    """(ref64, A64[, dbias64, Adbias64]) of a case"""
    a, b = operands(c, d, trunc)
    ref, A = epilogue(c, d, _lin(c, a, b), _lin(c, a.abs(), b.abs()))
    if c.entry != "wgrad":
        return ref, A
    dyr = b
    return ref, A, dyr.sum((0, 2, 3)), dyr.abs().sum((0, 2, 3))


def limit(A, ref, K, bf16_out=False):
    """the per-element error allowance"""
    lim = min(LIMIT_U, 2.0 * K) * U * A
    return lim + BF16_OUT * ref.abs() if bf16_out else lim


def e_units(got, ref, A):
    """E / 2^-24 and the flat index of its worst element"""
    r = (got.double() - ref).abs() / A.clamp_min(1e-300)
    r = torch.where(A > 0, r, (got.double() - ref).abs() * 1e300)
    i = int(torch.argmax(r))
    return float(r.flatten()[i]) / U, i


def excess(got, ref, A, K, bf16_out=False):
    """max over elements of |got - ref| / allowance (<= 1 passes), and the flat index of the worst element"""
    lim = limit(A, ref, K, bf16_out)
    err = (got.double() - ref).abs()
    r = torch.where(lim > 0, err / lim.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    i = int(torch.argmax(r))
    return float(r.flatten()[i]), i


def output_is_bf16(c):
    p = c.p
    if c.entry == "wgrad" or c.mode != "st":
        return False
    if p["out"] is not None:
        return bool(p["out"][2])
    return bool(p["out_bf16"])


# ---------------------------------------------------------------------------------------------------------------------------------
# the case's operands as the entry point takes them (the GPU sweep launches with them; the CPU plan test asks conv_dispatch.plan_*)
# ---------------------------------------------------------------------------------------------------------------------------------
def act(nchw, bf16, layout=None, poison=SRC_POISON, device="cuda"):
    """NCHW fp32 CPU tensor -> NHWC Act on ``device``; ``layout`` = (cstride, coff): a channel slice of a wider tensor with ``poison``
    around it (the slice's own pad channels, up to its 16-byte group, are zero).  On the ``meta`` device only shape, storage type and
    slice layout exist."""
    from hr_viton_amd import ops
    N, C_, H, W = nchw.shape
    cp = ops._cpad(C_, bf16)
    cs, co = layout if layout else (cp, 0)
    dt = torch.bfloat16 if bf16 else torch.float32
    if device == "meta":
        return ops.Act(torch.empty((N, H, W, cs), dtype=dt, device="meta"), C_, co)
    t = torch.full((N, H, W, cs), poison, dtype=torch.float32)
    t[..., co:co + cp] = 0
    t[..., co:co + C_] = nchw.permute(0, 2, 3, 1)
    return ops.Act(t.to(dt).to(device), C_, co)


def _out_act(p, H, W, C_, device):
    """the caller's output slice of a case (poison all over), or None where the entry point allocates"""
    from hr_viton_amd import ops
    if p["out"] is None:
        return None
    cs, co, obf = p["out"]
    return ops.Act(torch.full((p["N"], H, W, cs), POISON, dtype=torch.bfloat16 if obf else torch.float32, device=device), C_, co)


def entry_kwargs(c, d, device="cuda"):
    """keyword arguments of the case's entry point (train_ops.conv_forward_dev / conv_dgrad / conv_wgrad) over the operands ``d`` of
    make_inputs"""
    p, st = c.p, c.mode == "st"
    if c.entry == "fwd":
        H, W = p["H"] << p["srcs"][0][1], p["W"] << p["srcs"][0][1]
        Ho, Wo = (H + 2 * p["pad"] - p["K"]) // p["stride"] + 1, (W + 2 * p["pad"] - p["K"]) // p["stride"] + 1
        return dict(w=d["w"].to(device),
                    srcs=[(act(x, st, p["src"] if i == 0 else None, device=device), up) for i, (x, (_, up)) in enumerate(zip(d["xs"], p["srcs"]))],
                    stride=p["stride"], pad=p["pad"], shift=None if d["shift"] is None else d["shift"].to(device),
                    residual=None if d["res"] is None else act(d["res"], p["res"] == "bf16", device=device), act=p["act"], slope=SLOPE,
                    out=_out_act(p, Ho << p["out_up"], Wo << p["out_up"], p["Cout"], device), out_up=p["out_up"], name=c.id, out_bf16=p["out_bf16"])
    if c.entry == "dgrad":
        return dict(dy=act(d["dy"], st, p["dy"], device=device), w=tuple(t.to(device) for t in d["w"]) if p["pair"] else d["w"].to(device),
                    H=p["H"], W=p["W"], stride=p["stride"], pad=p["pad"],
                    act_mask=None if d["mask"] is None else act(d["mask"], p["mask"] == "bf16", device=device), slope=SLOPE,
                    out=_out_act(p, p["H"], p["W"], p["cin"], device), name=c.id, out_bf16=p["out_bf16"],
                    add=None if d["add"] is None else act(d["add"], False, device=device),
                    add_after=None if d["add_after"] is None else act(d["add_after"], False, device=device))
    return dict(dy=act(d["dy"], st and p["dy"] != "f32", p["dyl"], device=device), x=act(d["x"], st, p["x"], device=device), x_up=p["x_up"],
                ci_base=p["ci_base"], cin_tot=p["cin_tot"] or p["C"], KH=p["K"], KW=p["K"], stride=p["stride"], pad=p["pad"],
                dw=d["dw0"].clone().to(device), accumulate=p["accumulate"], name=c.id, dbias=d["db0"].clone().to(device) if p["dbias"] else None,
                dbias_accumulate=p["dbias_accumulate"])


_PLAN = {"fwd": ("plan_forward", ("w", "srcs", "stride", "pad", "residual", "act", "out", "out_up", "out_bf16")),
         "dgrad": ("plan_dgrad", ("dy", "w", "H", "W", "stride", "pad", "act_mask", "out", "out_bf16", "add", "add_after")),
         "wgrad": ("plan_wgrad", ("dy", "x", "x_up", "ci_base", "cin_tot", "KH", "KW", "stride", "pad", "dw"))}


def plan(c, kw, mb=None):
    """conv_dispatch's plan for the entry point's arguments ``kw`` (``mb``: the engine mode; None = train_ops.MMA_BF16[0])"""
    from hr_viton_amd import conv_dispatch
    fn, keys = _PLAN[c.entry]
    return getattr(conv_dispatch, fn)(**{k: kw[k] for k in keys}, mb=mb)


def planned_launches(c, pl, kw):
    """what the plan says about the launches LAUNCHES counts: {(kind, name): count}"""
    if c.entry == "dgrad":
        return {("ew", "add_slice"): int(kw["add_after"] is not None and not pl.ride), ("conv", ""): len(pl.phases) or 1}
    if c.entry == "wgrad":
        return {("layout", "pad_width"): int(pl.pad != "")}
    return {("conv", ""): 1}


# ---------------------------------------------------------------------------------------------------------------------------------
# the least favourable legal summation: a strictly sequential fp32 chain (numpy.cumsum in float32) on a sample of output elements
# ---------------------------------------------------------------------------------------------------------------------------------
def chain_sample(c, d, n=256):
    """(flat indices into the LINEAR part's tensor, fp32 sequential-chain values at them)"""
    p = c.p
    a, b = operands(c, d, dtype=torch.float32)
    a, b = a.numpy(), b.numpy()
    rng = np.random.RandomState(_seed(c) % (2 ** 31 - 1))
    K, s, pad = p["K"], p["stride"], p["pad"]
    if c.entry == "fwd":
        shape = (a.shape[0], b.shape[0], (a.shape[2] + 2 * pad - K) // s + 1, (a.shape[3] + 2 * pad - K) // s + 1)
        ap = np.pad(a, ((0, 0), (0, 0), (pad, pad), (pad, pad)))
    elif c.entry == "dgrad":
        shape = (p["N"], p["cin"], p["H"], p["W"])
    else:
        shape = (p["Cout"], p["C"], K, K)
    total = int(np.prod(shape))
    idx = rng.choice(total, size=min(n, total), replace=False)
    vals = np.empty(len(idx), np.float32)
    for j, fi in enumerate(idx):
        i0, i1, i2, i3 = np.unravel_index(fi, shape)
        if c.entry == "fwd":
            terms = ap[i0, :, i2 * s:i2 * s + K, i3 * s:i3 * s + K].ravel() * b[i1].ravel()
        elif c.entry == "dgrad":
            ts = []
            for kh in range(K):
                for kw in range(K):
                    ho, wo = i2 + pad - kh, i3 + pad - kw
                    if ho % s or wo % s or not (0 <= ho // s < a.shape[2]) or not (0 <= wo // s < a.shape[3]):
                        continue
                    ts.append(a[i0, :, ho // s, wo // s] * b[:, i1, kh, kw])
            terms = np.concatenate(ts) if ts else np.zeros(1, np.float32)
        else:
            Ho, Wo = b.shape[2], b.shape[3]
            terms = (a[:, i1, i2:i2 + s * Ho:s, i3:i3 + s * Wo:s] * b[:, i0]).ravel()
        vals[j] = np.cumsum(terms.astype(np.float32), dtype=np.float32)[-1]
    return idx, vals


# ---------------------------------------------------------------------------------------------------------------------------------
# mutations of the REFERENCE (what a subtly wrong kernel would compute): each must exceed the limit
# ---------------------------------------------------------------------------------------------------------------------------------
MUTATIONS = ("tap_dropped_on_border_row", "bf16_truncated", "channel_groups_swapped", "slab_counted_twice", "dbias_last_column_missing")


def mutate(c, d, name):
    """the result tensor a kernel with this defect would return (float64), or for "dbias_last_column_missing" the bias gradient"""
    p = c.p
    a, b = operands(c, d)
    lin = _lin(c, a, b)
    A = _lin(c, a.abs(), b.abs())
    if name == "bf16_truncated":
        return reference(c, d, trunc=True)[0]
    if name == "tap_dropped_on_border_row":
        if c.entry == "wgrad":
            b1 = torch.zeros_like(b)
            b1[:, :, -1] = b[:, :, -1]                      # the last dY row's share of tap (0, 0)
            lin = lin.clone()
            lin[:, :, 0, 0] -= _lin(c, a, b1)[:, :, 0, 0]
        else:
            t = 0 if c.entry == "fwd" else -1               # the tap that reads image rows, not the zero border, on the last row
            w1 = torch.zeros_like(b)
            w1[:, :, t, t] = b[:, :, t, t]
            part = _lin(c, a, w1)
            lin = lin.clone()
            lin[:, :, -1] -= part[:, :, -1]
        return epilogue(c, d, lin, A)[0]
    if name == "slab_counted_twice":
        # one of 16 K-slabs (channel range of the source / of dY; image-row range for the weight gradient) added a second time
        if c.entry == "fwd":
            n = max(1, a.shape[1] // 16)
            lin = lin + F.conv2d(a[:, :n], b[:, :n], None, p["stride"], p["pad"])
        elif c.entry == "dgrad":
            n = max(1, a.shape[1] // 16)
            lin = lin + torch.nn.grad.conv2d_input((p["N"], p["cin"], p["H"], p["W"]), b[:n], a[:, :n], p["stride"], p["pad"])
        else:
            n = max(1, b.shape[2] // 16)
            b1 = torch.zeros_like(b)
            b1[:, :, :n] = b[:, :, :n]
            lin = lin + _lin(c, a, b1)
        return epilogue(c, d, lin, A)[0]
    if name == "channel_groups_swapped":
        y = epilogue(c, d, lin, A)[0].clone()
        ch = 0 if c.entry == "wgrad" else 1                 # the column dimension of the kernel's tile: Cout (fwd, wgrad) / Cin (dgrad)
        n = y.shape[ch]
        assert n >= 8
        i = n - 8 - (n % 4)
        sl = lambda lo: tuple(slice(lo, lo + 4) if k == ch else slice(None) for k in range(4))
        t = y[sl(i)].clone()
        y[sl(i)] = y[sl(i + 4)]
        y[sl(i + 4)] = t
        return y
    if name == "dbias_last_column_missing":
        assert c.entry == "wgrad"
        return b[:, :, :, :-1].sum((0, 2, 3))
    raise KeyError(name)


# one representative case per entry point for the mutation checks (mixed precision over fp32 tensors: the rounding mutation needs
# operands that are not bf16 values already)
MUTATION_CASES = ("fwd-mb-s2-4x4", "dgrad-mb-pair-add", "wgrad-mb-Wo36")
