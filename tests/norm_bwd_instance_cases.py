"""The storage forms of the SPADE / InstanceNorm backward that have compile-time instances (csrc/norm_bwd.hip), as
descriptor recipes: one case per combination of a stage-1 and a stage-2 instance the training step meets, the two pair forms, and
descriptors outside the table.  ``hits``: the lines of hrv_diag_norm_bwd_instances() a case runs on.  Shared by the CPU test (the
table in C, the list in DESIGN.md and these cases name the same instances) and the GPU test (each instance against the generic
kernels, bit for bit)."""
from collections import namedtuple

# spade: a SPADE norm with [dgamma | dbeta] whose dout arrived in the dbeta half (bf16), 1 + gamma in ``g1p`` storage, noise;
# inorm: InstanceNorm + LeakyReLU (no 1 + gamma, no dgb, no noise) with dout / out in ``io`` storage.
# dx: "bf16" | "f32" | "acc" (fp32, accumulated into);  up: x = cat(up2(lo), hi);  route: hrv_diag_norm_bwd_route's answer
Case = namedtuple("Case", "id kind g1p io up dx pair route hits")

S1_SPADE16 = "single.stage1 dout_bf16+g1p+g1p_bf16+dnh_bf16+dgb+dgb_bf16+dbeta_in_place+noise"
S1_SPADE16_UP = S1_SPADE16 + "+up"
S1_SPADE32 = "single.stage1 dout_bf16+g1p+dnh_bf16+dgb+dgb_bf16+dbeta_in_place+noise"
S1_IN32 = "single.stage1 lrelu+dnh_bf16"
S1_IN16 = "single.stage1 lrelu+dout_bf16+out_bf16+dnh_bf16"
S2 = "single.stage2 dnh_bf16+noise"
S2_IN = "single.stage2 dnh_bf16+dx_bf16"
P1_UP = "pair.stage1 dout_bf16+g1p+g1p_bf16+dnh_bf16+dgb+dgb_bf16+dbeta_in_place+noise+up"
P1 = "pair.stage1 dout_bf16+g1p+dnh_bf16+dgb+dgb_bf16+dbeta_in_place+noise"
P2_UP = "pair.stage2 dnh_bf16+noise+up"
P2 = "pair.stage2 dnh_bf16+noise"

CASES = [
    Case("norm_1_fine", "spade", "bf16", None, False, "bf16", False, 3, (S1_SPADE16, S2 + "+dx_bf16")),
    Case("norm_0_fine", "spade", "bf16", None, True, "f32", False, 3, (S1_SPADE16_UP, S2 + "+up")),
    Case("norm_s_fine", "spade", "bf16", None, True, "acc", False, 3, (S1_SPADE16_UP, S2 + "+up+dx_acc")),
    Case("norm_0_coarse", "spade", "f32", None, False, "f32", False, 3, (S1_SPADE32, S2)),
    Case("norm_s_coarse", "spade", "f32", None, False, "acc", False, 3, (S1_SPADE32, S2 + "+dx_acc")),
    Case("patchgan_f32", "inorm", None, "f32", False, "bf16", False, 3, (S1_IN32, S2_IN)),
    Case("patchgan_bf16", "inorm", None, "bf16", False, "bf16", False, 3, (S1_IN16, S2_IN)),
    Case("pair_fine", "spade", "bf16", None, True, "f32", True, 3, (P1_UP, P2_UP)),
    Case("pair_coarse", "spade", "f32", None, False, "f32", True, 3, (P1, P2)),
    # outside the table: the generic kernels serve them, as before the instances existed
    Case("outside_patchgan_mixed_io", "inorm", None, "mixed", False, "bf16", False, 2, (S2_IN,)),     # bf16 dout, fp32 out: stage 1 generic
    Case("outside_up_bf16_dx", "spade", "bf16", None, True, "bf16", False, 1, (S1_SPADE16_UP,)),   # up + bf16 dx: stage 2 generic
    Case("outside_all_f32", "f32", "f32", "f32", False, "f32", False, 0, ()),                         # the fp32 engine's form
    Case("outside_pair_materialised_bf16_g1p", "spade", "bf16", None, False, "f32", True, 2, (P2,)),  # pair stage 1 generic
    Case("outside_pair_all_f32", "f32", "f32", "f32", False, "f32", True, 0, ()),
]

# (N, H, W, C): a small extent, and two whose H*W is not a multiple of the 128-pixel slab; H and W even (the up-sampled source)
EXTENTS = [(2, 16, 16, 64), (1, 18, 14, 80), (2, 34, 22, 128)]

# The pair pass against two sequential single calls (tests/test_gpu_spade_fused.py), N = 2: (H, W, up).  9x15 = 135 pixels are two
# slabs of 68 and 67 (norm_slabs does not divide H*W); 6x10 is even in both directions for the up-sampled source.  PAIR_CHANNELS:
# C/4 = 3 (85 pixel rows in flight: a thread walks one pixel at most, the tail alone) and C/4 = 65, one over NORM_GCAP: a second
# channel chunk with one live group, four rows, each thread walking 17 or 15 pixels at 9x15 -- the single's two-pixel stage-1
# loop runs and then takes its one-pixel tail (tests/test_norm_bwd_instances_cpu.py checks these properties).
PAIR_EXTENTS = [(9, 15, False), (6, 10, True)]
PAIR_CHANNELS = [12, 260]


def instance_lines():
    """every instance some case runs on, in no particular order"""
    return sorted({h for c in CASES for h in c.hits})
