"""Which kernel serves a convolution: the decisions of train_ops.conv_forward_dev / conv_dgrad / conv_wgrad as pure functions.

``plan_forward`` / ``plan_dgrad`` / ``plan_wgrad`` take what the entry points take and read only metadata -- shapes, storage types,
``cstride`` / ``coff``, ``data_ptr() % 16``, the HRV_* switches, the library's host predicates -- so they answer for ``Act`` views over
CPU or ``meta`` tensors as they do on the GPU (tests/test_conv_dispatch_plan_cpu.py walks tests/conv_dispatch_cases.py through them).
Nothing here allocates, packs or launches; the entry points run the plan they get.  Every gate is ONE predicate below, and its
docstring names the gate ids of ``conv_dispatch_cases.GATES`` it implements."""
from __future__ import annotations

import ctypes as C
import os
from typing import NamedTuple, Optional, Sequence, Tuple

from . import _lib
from ._lib import ACT_LRELU, ACT_NONE, ACT_RELU

# Mixed-precision training switch (the reference's --fp16 / apex-O1 role): when on, every training
# convolution (forward and data gradient) rounds its fp32 operands to bf16 while staging them and runs on
# v_mfma_f32_32x32x16_bf16 with fp32 accumulation; all tensors in HBM, the epilogues, the normalisations,
# the losses and the optimizer stay fp32.  The weight gradient has its own switch-aware kernel.
MMA_BF16 = [False]

COUT1, THIN, P2, ENGINE = "cout1_kernel", "thin_conv_kernel", "conv_p2_kernel", "conv_mfma_kernel"


class Plan(NamedTuple):
    """What an entry point runs.  ``f"{kernel}[{variant}]"`` is the family of the launch record (``family``)."""
    kernel: str             # as _Timed records it: COUT1 / THIN / P2 / "conv_mfma_kernel[tile N]" (stride-2 data gradient: the phases'
                            # kernels, distinct ones joined by "+") / "conv_wgrad_tr_kernel" / "conv_wgrad_s2_kernel" / "conv_wgrad_kernel"
    variant: str = ""       # conv_p2: "mode 0|1|2"; weight gradient: "class N" / "fp32" | "bf16" | "bf16 x-stored" | "bf16 stored"
    cfg: int = 0            # the generic engine's tile (forward, stride-1 data gradient), 0 for the other kernels
    out_bf16: bool = False  # storage type of the output (the caller's ``out``, or the one the entry point allocates)
    mb: bool = False        # the engine mode the plan was made for
    ride: bool = False      # dgrad: ``add_after`` rides in the kernel's epilogue; False with an ``add_after``: an add_slice pass follows
    phases: tuple = ()      # dgrad, stride 2 on the generic engine: (a, b, Hp, Wp, cfg) of every non-empty phase
    pad: str = ""           # wgrad: zero columns appended to dY up to a multiple of 4: "" none, "bf16" pad_width_bf16, "f32" F.pad
    desc: object = None     # wgrad: the hrv_conv2d_wgrad_t the route was asked with (wgrad_desc of the unpadded operands); conv_wgrad launches
                            # with it where dY needs no padding

    @property
    def family(self) -> str:
        return f"{self.kernel}[{self.variant}]" if self.variant else self.kernel


def _cpad(c: int, bf16: bool) -> int:
    """Channel padding of an NHWC tensor: one 16-byte gather group (4 fp32 / 8 bf16 channels)."""
    return (c + 7) // 8 * 8 if bf16 else (c + 3) // 4 * 4


# ---------------------------------------------------------------------------------------------------------------
# the generic engine's tile
# ---------------------------------------------------------------------------------------------------------------
def _bf16_tile(cout: int) -> int:
    """128-byte-row tile of the bf16 engine with the least column padding (cfg 8: 128 columns, cfg 9: 64)."""
    p64, p128 = (cout + 63) // 64 * 64, (cout + 127) // 128 * 128
    return 8 if p128 <= p64 else 9


_ALT_F32_TILE = {0: 7, 6: 4, 1: 2, 5: 3}      # 128-row fp32 tiles -> the 256-row tile of the same width


def _f32_tile(M: int, cout: int) -> int:
    """fp32-engine tile of a training convolution: hrv_conv2d_pick_tile, or -- HRV_CONV_TILE_TRAIN=bm256, a TEST knob -- the
    256-row tile of the same width (another block shape, wave layout and split-K geometry for the same convolution: the
    at-size self-consistency check of tests/test_gpu_fullsize_tocg.py)."""
    cfg = _lib.load().hrv_conv2d_pick_tile(M, cout)
    if os.environ.get("HRV_CONV_TILE_TRAIN") == "bm256":
        cfg = _ALT_F32_TILE.get(cfg, cfg)
    return cfg


def patch_tile(bf16_sources: bool, KH: int, KW: int, stride: int, pad: int, nsrc: int, up: int, C: int, cols: int,
               N: int, H: int, W: int, wide: bool = False, pad_w: Optional[int] = None) -> int:
    """Patch-mode tile of the conv engine (conv_f32.hip, VAR bit 6) for this layer, or 0.  Patch mode: 3x3 stride-1
    'same' convolution over ONE bf16-stored source with C % 128 == 0; the 8x16-pixel tile keeps its 10x18 halo
    patch resident in LDS and only the weight tiles stream (the implicit-GEMM gather re-reads every activation
    pixel from L2 once per tap).  tile_cfg 17: 128 columns, 18: 64 columns (column counts that are odd multiples
    of 64 -- the SPADE gamma|beta convs of the 80/144/272-channel blocks).  Needs enough tiles to fill the chip
    (else the gather tiles with split-K win).  HRV_CONV_PATCH=0 disables it, =16 selects the 16x16-pixel tile.
    ``pad_w``: the horizontal padding where the caller sets one (None: ``pad``); 'same' means 1 in BOTH directions.
    Gates: fwd.patch.tiles512, fwd.patch.c64pad, fwd.patch.C%128, fwd.patch.env, dgrad.patch.tiles512."""
    env = os.environ.get("HRV_CONV_PATCH", "1")
    if not (bf16_sources and KH == 3 and KW == 3 and stride == 1 and pad == 1 and pad_w in (None, 1) and nsrc == 1 and up == 0 and
            C % 128 == 0 and env != "0"):
        return 0
    # tile_cfg 19 (conv_patchw.hip): 16x16-pixel tiles x up to 192 columns per block, one block per CU, weights
    # streamed once per 256 pixels through 3 LDS stages.  Opt-in (HRV_CONV_PATCHW=1): measured in the training step
    # it is 5-10 % SLOWER than the 8x16 tiles below (up_4 gamma|beta 2.42 vs 2.25 ms) -- with one block per CU nothing
    # overlaps the SPADE epilogue's 246 KB of loads/stores per tile, which the two resident blocks of cfg 17/18 hide.
    # (``wide``: the caller's epilogue is one conv_patchw.hip implements -- the SPADE modulate sites)
    if wide and os.environ.get("HRV_CONV_PATCHW", "0") != "0" and N * ((H + 15) // 16) * ((W + 15) // 16) >= 256:
        return 19
    c64 = (cols + 63) // 64
    if c64 * 64 - cols > 32:
        return 0
    wide = c64 % 2 == 0
    if N * ((H + 7) // 8) * ((W + 15) // 16) * (c64 // 2 if wide else c64) < 512:
        return 0
    if env == "16" and wide:
        return 16
    return 17 if wide else 18


def engine_tile(engine: str, M: int, cols: int, bf16_src: bool, KH: int, KW: int, stride: int, pad: int, nsrc: int, up: int,
                C: int, N: int, H: int, W: int, c1x1: int = 0, wide: bool = False, base: Optional[int] = None,
                pad_w: Optional[int] = None) -> int:
    """tile_cfg of a layer on the generic engine (conv_f32.hip).  ``engine`` picks the tile a layer starts from unless the
    caller has one (``base``: the SPADE gamma|beta sites, whose column order fixes the tile width):
      "mb"    bf16 matrix cores, training (MMA_BF16) or inference over fp32 tensors: the least column padding (_bf16_tile);
      "f32"   the training fp32 engine: hrv_conv2d_pick_tile (_f32_tile: the HRV_CONV_TILE_TRAIN test knob);
      "serve" the inference engine: hrv_conv2d_pick_tile, and over bf16 sources its 128-byte-row twins 0 -> 8, 6 -> 9
              (128x128 tile +15-20 %, profiles/r01_conv_bench_bf16_rb.txt; the 128x64 tile stages by LDS-DMA,
              profiles/r01_conv_bench_bf16_glds.txt).
    Over bf16-stored sources two rules follow.  A 1x1 layer with at most 128 source channels (``c1x1``; 0 where the rule is not
    applied: data gradients, training layers with several sources) and 64-column multiples takes tile 6 -- one or two K-tiles,
    the block is all prologue and epilogue, so the small tile with 64-byte rows keeps more blocks resident (conv_shared as a 1x1
    over the 72 expanded taps: 0.39 vs 0.48 ms).  Then the LDS-resident patch tile where ``patch_tile`` has one.
    ``pad_w``: ops.ConvLayer's horizontal padding (None: ``pad``); only the patch tile's 'same' gate reads it -- no other rule here
    looks at the padding, and the tiles themselves take any (csrc/conv_f32.hip gathers with pad and pad_w separately).
    Gates: fwd.tile6.Cout%64, fwd.tile6.Cp<=128 (and patch_tile's)."""
    if base is not None:
        cfg = base
    elif engine == "mb":
        cfg = _bf16_tile(cols)
    elif engine == "f32":
        cfg = _f32_tile(M, cols)
    else:
        cfg = _lib.load().hrv_conv2d_pick_tile(M, cols)
        if bf16_src:
            cfg = {0: 8, 6: 9}.get(cfg, cfg)
    if not bf16_src:
        return cfg
    if KH == 1 and KW == 1 and 0 < c1x1 <= 128 and cols % 64 == 0:
        cfg = 6
    return patch_tile(True, KH, KW, stride, pad, nsrc, up, C, cols, N, H, W, wide, pad_w) or cfg


# ---------------------------------------------------------------------------------------------------------------
# the gates
# ---------------------------------------------------------------------------------------------------------------
def _thin_ok(mb: bool, a, KH: int, KW: int, stride: int, pad: int, cols: int, N: int, H: int, W: int) -> bool:
    """thin_conv.hip serves this layer: mixed precision, ONE bf16-stored source read at its own resolution, 3x3 / 1x1
    stride-1 'same', <= 96 channels on either side (the 1024x768 level), enough pixels for a persistent grid.
    Gates: fwd.thin.pixels, fwd.thin.supported, fwd.thin.env, fwd.thin.1x1.kb, dgrad.thin.pixels."""
    return (mb and a.bf16 and stride == 1 and KH == KW and pad == KH // 2 and N * H * W >= 65536 and
            os.environ.get("HRV_THIN_CONV", "1") != "0" and
            bool(_lib.load().hrv_thin_conv_supported(KH, KW, a.Cp, cols)))


def _cout1_ok(w, x_bf16: bool, x_C: int, x_cstride: int, x_coff: int, stride: int, pad: int, part: str = "fwd") -> bool:
    """conv_cout1.hip serves this layer: ONE output channel, K <= 4, stride 1, pad >= (K-1)/2, an fp32 source (``x_*``: its storage
    type, channels and slice layout) with 4-channel granules (PatchGAN's last convolution).  HRV_CONV_COUT1: "0" off, "fwd" the
    forward kernel only, default all three.
    Measured at 2 x 4 x 131 x 99 x 256: forward 0.233 -> 0.109 ms; the first data- / weight-gradient kernels (16 global dY
    loads per pixel) were no faster than the padded matrix-core path (0.099 / 0.72 ms against 0.094 / 0.19) and were
    rewritten with the dY rows of an input row staged in LDS.
    Gates: fwd.cout1.Cout, fwd.cout1.cin%4, fwd.cout1.pad, fwd.cout1.K<=4, fwd.cout1.env, dgrad.cout1.Cout, wgrad.cout1.Cout."""
    Cout, cin, KH, KW = w.shape
    mode = os.environ.get("HRV_CONV_COUT1", "1")
    return (Cout == 1 and KH == KW and KH <= 4 and stride == 1 and 0 <= pad < KH and 2 * pad >= KH - 1 and not x_bf16 and
            x_C == cin and cin % 4 == 0 and cin <= 2048 and x_cstride % 4 == 0 and x_coff % 4 == 0 and w.is_contiguous() and
            mode != "0" and (mode != "fwd" or part == "fwd"))


def conv_p2_ok(K: int, cols: int, N: int, H: int, W: int) -> bool:
    """hrv_conv_p2_supported (HRV_CONV_P2=0 switches the kernel off for A/B runs).
    Gates: fwd.p2.tiles, fwd.p2.min_tiles_env, fwd.p2.env, dgrad.p2.tiles."""
    if os.environ.get("HRV_CONV_P2", "1") == "0":
        return False
    return bool(_lib.load().hrv_conv_p2_supported(K, cols, N, H, W))


def _p2_odd() -> bool:
    """HRV_CONV_P2_ODD=0 (A/B): no conv_p2 for a K or a column count off its granule (the 3-channel image of VGG19 features.0)."""
    return os.environ.get("HRV_CONV_P2_ODD", "1") != "0"


def _p2_wide() -> bool:
    """HRV_CONV_P2_WIDE=0 (A/B): conv_p2 keeps to its round-4 mid range and the thin kernel goes first."""
    return os.environ.get("HRV_CONV_P2_WIDE", "1") != "0"


def _plain_act(a) -> bool:
    from .ops import Act        # (ops imports this module)
    return type(a) is Act


def _p2_fwd_ok(mb: bool, w, a0, stride: int, pad: int, out, out_is_bf16: bool, residual, act: int) -> bool:
    """csrc/conv_p2.hip serves this forward layer: 3x3 stride-1 'same' over ONE bf16-stored source read at its own resolution.
    Gates: fwd.p2.odd.Cout>=64, fwd.p2.Cout%oal, fwd.p2.act, fwd.p2.kernel3x3, fwd.p2.src_bf16 (and conv_p2_ok's; fwd.p2.nsrc,
    fwd.p2.up0, fwd.p2.out_up: plan_forward's ``plain``)."""
    Cout, cin, KH, KW = w.shape
    oal = 8 if out_is_bf16 else 4
    # a K that is not a multiple of 16 or a column count off the 16-byte store granule: only where it was measured to win -- a
    # 3-channel image into >= 64 columns (VGG19 features.0: the thin kernel's tile loop is latency-bound there)
    odd = cin % 16 != 0 or cin < 32 or Cout % oal != 0
    ok = (mb and (KH, KW, stride, pad) == (3, 3, 1, 1) and act in (ACT_NONE, ACT_RELU, ACT_LRELU) and a0.bf16 and a0.C == cin and
          (not odd or (Cout >= 64 and Cout % oal == 0 and _p2_odd())) and
          a0.cstride % 8 == 0 and a0.coff % 8 == 0 and a0.coff + (cin + 7) // 8 * 8 <= a0.cstride and w.is_contiguous() and
          (out is None or (out.cstride % oal == 0 and out.coff % oal == 0)) and
          (residual is None or (_plain_act(residual) and residual.C == Cout and residual.cstride % 4 == 0 and residual.coff % 4 == 0 and
                                residual.t.data_ptr() % 16 == 0)) and
          conv_p2_ok(cin, Cout, a0.N, a0.H, a0.W))
    if ok and not _p2_wide():      # (64-column multiples, thin kernel first)
        ok = Cout % 64 == 0 and residual is None and not _thin_ok(mb, a0, KH, KW, stride, pad, Cout, a0.N, a0.H, a0.W)
    return ok


def _p2_dgrad_ok(mb: bool, dy, w, pair: bool, Cout: int, cin: int, KH: int, KW: int, stride: int, pad: int, H: int, W: int,
                 o_bf16: bool, o_cstride: int, o_coff: int, mask, add) -> bool:
    """csrc/conv_p2.hip serves this data gradient: a stride-1 data gradient of a 3x3 'same' layer is a 3x3 'same' convolution over
    a bf16-stored dY.  (Columns off the 16-byte store granule: only the >= 64-channel gradient into a 3-channel image, VGG19
    features.0 -- the padded lanes of the output receive zeros.)
    Gates: dgrad.p2.Cout%16, dgrad.p2.odd.Cout>=64, dgrad.p2.mask_bf16, dgrad.p2.add, dgrad.p2.stride (and conv_p2_ok's)."""
    oal = 8 if o_bf16 else 4
    N = dy.N
    ok = (mb and stride == 1 and (KH, KW, pad) == (3, 3, 1) and (dy.H, dy.W) == (H, W) and dy.bf16 and add is None and dy.C == Cout and
          Cout % 16 == 0 and dy.cstride % 8 == 0 and dy.coff % 8 == 0 and
          (cin % oal == 0 or (not pair and Cout >= 64 and o_coff + (cin + oal - 1) // oal * oal <= o_cstride and _p2_odd())) and
          o_cstride % oal == 0 and o_coff % oal == 0 and
          (mask is None or (mask.bf16 and mask.C == cin and mask.cstride % 4 == 0 and mask.coff % 4 == 0)) and
          w.is_contiguous() and conv_p2_ok(Cout, cin, N, H, W))
    if ok and not _p2_wide():
        ok = Cout % 32 == 0 and cin % 64 == 0 and not (not pair and _thin_ok(mb, dy, KH, KW, 1, pad, cin, N, H, W))
    return ok


def _ride_ok(add_after, cin: int) -> bool:
    """``add_after`` of a data gradient that conv_p2 serves rides in its epilogue, behind the mask.  Gates: dgrad.ride.env (and,
    through plan_dgrad, dgrad.ride.p2)."""
    return (add_after.C == cin and add_after.cstride % 4 == 0 and add_after.coff % 4 == 0 and add_after.t.data_ptr() % 16 == 0 and
            add_after.coff + (cin + 3) // 4 * 4 <= add_after.cstride and os.environ.get("HRV_DGRAD_ADD_AFTER", "1") != "0")


def _wgrad_pad(mb: bool, dy, x, lds_dma: bool) -> str:
    """Zero columns for dY up to the next multiple of 4: the bf16 matrix-core kernel stages quads of 4 pixels of one image row, and
    the columns add nothing to dW or the bias gradient (the X taps they would pair with are never weighted).  "bf16": a dense
    bf16-stored dY that no LDS-DMA kernel takes (``lds_dma``: hrv_conv2d_wgrad_route's answer; the PatchGAN with bf16 feature maps); "f32": the odd-sized fp32 maps (the
    PatchGAN's 513 / 257 / 129 columns) instead of the fp32 kernel (60-100 TFLOP/s); "": none.
    Gates: wgrad.pad.bf16.Wo%4, wgrad.pad.f32.Wo%4, wgrad.pad.f32.Wo>=32."""
    if not mb or dy.W % 4 == 0 or dy.coff != 0:
        return ""
    if dy.bf16 and x.bf16 and dy.cstride == dy.C and dy.C % 8 == 0 and not lds_dma:
        return "bf16"
    if dy.W >= 32 and not (x.bf16 or dy.bf16) and dy.cstride == dy.Cp:
        return "f32"
    return ""


# ---------------------------------------------------------------------------------------------------------------
# the plans
# ---------------------------------------------------------------------------------------------------------------
def _hw(a, up: int) -> Tuple[int, int]:
    return (a.H << up, a.W << up) if up >= 0 else (a.H >> -up, a.W >> -up)


def plan_forward(w, srcs: Sequence[tuple], stride: int, pad: int, residual=None, act: int = ACT_NONE, out=None, out_up: int = 0,
                 out_bf16: bool = False, mb: Optional[bool] = None) -> Plan:
    """The kernel conv_forward_dev runs for these operands: cout1, else conv_p2 (mode 0), else thin_conv, else the generic engine."""
    if mb is None:
        mb = MMA_BF16[0]
    Cout, cin, KH, KW = w.shape
    a0, up0 = srcs[0]
    N = a0.N
    H, W = _hw(a0, up0)
    plain = len(srcs) == 1 and up0 == 0 and out_up == 0         # one source at its own resolution, no upsampled store
    if (plain and residual is None and act == ACT_NONE and out is None and      # (gate fwd.cout1.epilogue)
            _cout1_ok(w, a0.bf16, a0.C, a0.cstride, a0.coff, stride, pad)):
        return Plan(COUT1, mb=mb)           # (pad channels 1..3 are zero)
    p2_bf = out.bf16 if out is not None else (out_bf16 and Cout % 8 == 0)
    if plain and _p2_fwd_ok(mb, w, a0, stride, pad, out, p2_bf, residual, act):
        # plain 3x3 over one bf16 source: the two-blocks-per-CU kernel (VGG19's 128..512-channel layers; SPADEResBlock.conv_0 of
        # up_2 / up_3: 272 -> 128, 144 -> 64)
        return Plan(P2, "mode 0", 0, p2_bf, mb)
    if (plain and w.is_contiguous() and _thin_ok(mb, a0, KH, KW, stride, pad, Cout, N, H, W) and
            (out is None or out.cstride % 4 == 0)):
        return Plan(THIN, "", 0, out.bf16 if out is not None else (out_bf16 and Cout % 4 == 0), mb)
    Ho, Wo = (H + 2 * pad - KH) // stride + 1, (W + 2 * pad - KW) // stride + 1
    cfg = engine_tile("mb" if mb else "f32", N * Ho * Wo, Cout, mb and a0.bf16, KH, KW, stride, pad, len(srcs), up0, a0.Cp, N, H, W,
                      c1x1=a0.Cp if len(srcs) == 1 else 0)
    return Plan(f"{ENGINE}[tile {cfg}]", "", cfg, out.bf16 if out is not None else (out_bf16 and mb), mb)


def plan_dgrad(dy, w, H: int, W: int, stride: int, pad: int, act_mask=None, out=None, out_bf16: bool = False, add=None,
               add_after=None, mb: Optional[bool] = None) -> Plan:
    """The kernel conv_dgrad runs for these operands: cout1, else conv_p2 (mode 1, mode 2 for a weight pair), else thin_conv, else
    the generic engine (stride 2: one launch per non-empty phase).  An ``add_after`` that cannot ride in conv_p2's epilogue does not
    change the choice: the plan is that of the same call without it, and an add_slice pass follows."""
    if mb is None:
        mb = MMA_BF16[0]
    pair = isinstance(w, (tuple, list))
    if pair:
        w = w[0]
        Cout, cin, KH, KW = 2 * w.shape[0], w.shape[1], w.shape[2], w.shape[3]
    else:
        Cout, cin, KH, KW = w.shape
    N, Ho, Wo = dy.N, dy.H, dy.W
    if out is None:
        o_bf16 = out_bf16 and mb and cin % 8 == 0 and stride == 1
        o_cstride, o_coff = _cpad(cin, o_bf16), 0
    else:
        o_bf16, o_cstride, o_coff = out.bf16, out.cstride, out.coff
    if (not pair and act_mask is None and not dy.bf16 and not o_bf16 and (add is None or not add.bf16) and      # (gate dgrad.cout1.res_mode)
            (Ho, Wo) == (H + 2 * pad - KH + 1, W + 2 * pad - KW + 1) and
            _cout1_ok(w, o_bf16, cin, o_cstride, o_coff, stride, pad, "dgrad")):        # (x slot: the geometry of dX)
        return Plan(COUT1, "", 0, o_bf16, mb)
    if _p2_dgrad_ok(mb, dy, w, pair, Cout, cin, KH, KW, stride, pad, H, W, o_bf16, o_cstride, o_coff, act_mask, add):
        return Plan(P2, "mode 2" if pair else "mode 1", 0, o_bf16, mb, add_after is not None and _ride_ok(add_after, cin))
    if (add is None and not pair and stride == 1 and (Ho, Wo) == (H, W) and w.is_contiguous() and o_cstride % 4 == 0 and
            _thin_ok(mb, dy, KH, KW, 1, pad, cin, N, H, W)):
        return Plan(THIN, "", 0, o_bf16, mb)
    engine = "mb" if mb else "f32"
    if stride == 1:
        # (a stride-1 data gradient of a 3x3 pad-1 layer is a 'same' 3x3 convolution over dY: the patch tile's case)
        cfg = engine_tile(engine, N * H * W, cin, mb and dy.bf16, KH, KW, 1, KH - 1 - pad, 1, 0, dy.Cp, N, H, W)
        return Plan(f"{ENGINE}[tile {cfg}]", "", cfg, o_bf16, mb)
    assert stride == 2, "data gradient implemented for stride 1 and 2"
    phases = []
    for a in range(2):
        for b in range(2):
            Hp, Wp = (H - a + 1) // 2, (W - b + 1) // 2
            if Hp > 0 and Wp > 0:       # (gate dgrad.s2.phase)
                phases.append((a, b, Hp, Wp, engine_tile(engine, N * Hp * Wp, cin, False, KH, KW, 2, pad, 1, 0, dy.Cp, N, Hp, Wp)))
    kernels = []
    for ph in phases:
        k = f"{ENGINE}[tile {ph[4]}]"
        if k not in kernels:
            kernels.append(k)
    return Plan("+".join(kernels), "", 0, o_bf16, mb, False, tuple(phases))


def wgrad_desc(dy, x, x_up: int, ci_base: int, cin_tot: int, KH: int, KW: int, stride: int, pad: int,
               mma_bf16: bool) -> "_lib.hrv_conv2d_wgrad_t":
    """hrv_conv2d_wgrad's descriptor for these operands, metadata only: what hrv_conv2d_wgrad_route reads.  conv_wgrad adds the
    pointers and the workspace."""
    H, W = _hw(x, x_up)
    return _lib.hrv_conv2d_wgrad_t(
        dy_cstride=dy.cstride, dy_coff=dy.coff, Cout=dy.C, x_C=x.Cp, x_cstride=x.cstride, x_coff=x.coff, x_up_shift=x_up, x_C_real=x.C,
        ci_base=ci_base, CinTot=cin_tot, N=dy.N, H=H, W=W, Ho=dy.H, Wo=dy.W, KH=KH, KW=KW, stride=stride, pad=pad,
        mma_bf16=1 if mma_bf16 else 0, storage_flags=(1 if dy.bf16 else 0) | (2 if x.bf16 else 0))


def plan_wgrad(dy, x, x_up: int, ci_base: int, cin_tot: int, KH: int, KW: int, stride: int, pad: int, dw,
               mb: Optional[bool] = None) -> Plan:
    """The kernel conv_wgrad runs for these operands and the width padding dY gets first: cout1, else what hrv_conv2d_wgrad_route
    answers for the descriptor of the UNPADDED operands -- the C function hrv_conv2d_wgrad launches by (wgrad_route,
    csrc/conv_bwd.hip): an LDS-DMA kernel for bf16-stored operands where one takes the shape, else the generic kernel on bf16
    matrix cores (mixed precision, Wo % 4 == 0 after padding) or in fp32.
    Gates, all in C: wgrad.tr.storage, wgrad.tr.x_up (wgrad_route); wgrad.tr.pixels, wgrad.tr.W>=32, wgrad.tr.W>=32.odd,
    wgrad.tr.x_granule, wgrad.tr.dy_granule, wgrad.tr.Cout%64, wgrad.tr.Cp, wgrad.tr.min_pix_env, wgrad.tr.env (wgrad_tr_class);
    wgrad.s2.pixels, wgrad.s2.Wo>=32, wgrad.s2.x_granule, wgrad.s2.Cout%128, wgrad.s2.env (wgrad_s2_class)."""
    if mb is None:
        mb = MMA_BF16[0]
    Wo, x_bf16, dy_bf16 = dy.W, x.bf16, dy.bf16
    if dy.C == 1 and x_up == 0 and ci_base == 0 and cin_tot == x.C and not dy_bf16:
        H, W = _hw(x, x_up)
        if ((dy.H, Wo) == (H + 2 * pad - KH + 1, W + 2 * pad - KW + 1) and
                _cout1_ok(dw, x_bf16, x.C, x.cstride, x.coff, stride, pad, "wgrad")):
            return Plan(COUT1, mb=mb)
    d = wgrad_desc(dy, x, x_up, ci_base, cin_tot, KH, KW, stride, pad, mb)
    route = _lib.load().hrv_conv2d_wgrad_route
    if x_bf16 or dy_bf16:
        assert mb, "bf16-stored operands need the bf16 matrix-core weight gradient"
        assert x_bf16, "bf16 dY with an fp32 X is not built"
        code = route(C.byref(d))
        padded = _wgrad_pad(mb, dy, x, code >= _lib.WGRAD_S2)
        assert Wo % 4 == 0 or padded or code >= _lib.WGRAD_S2, "the generic bf16 matrix-core weight gradient needs Wo % 4 == 0"
    else:       # mixed precision: bf16 matrix cores (needs Wo % 4 == 0 after the padding: narrow odd-sized maps keep the fp32 kernel)
        padded = _wgrad_pad(mb, dy, x, False)
        d.mma_bf16 = 1 if mb and (Wo % 4 == 0 or padded) else 0
        code = route(C.byref(d))
    if code < 0:
        _lib.check(code, "hrv_conv2d_wgrad_route")
    if code >= _lib.WGRAD_TR:
        kernel, variant = "conv_wgrad_tr_kernel", f"class {code - _lib.WGRAD_TR}"
    elif code == _lib.WGRAD_S2:
        kernel, variant = "conv_wgrad_s2_kernel", ""
    elif code == _lib.WGRAD_BF16:
        kernel, variant = "conv_wgrad_kernel", "bf16 stored" if dy_bf16 else ("bf16 x-stored" if x_bf16 else "bf16")
    else:
        kernel, variant = "conv_wgrad_kernel", "fp32"
    return Plan(kernel, variant, mb=mb, pad=padded, desc=d)
