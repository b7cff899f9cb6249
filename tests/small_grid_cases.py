"""The host scheduler of the persistent patch-pass kernels restated in plain Python, and the case tables of the exact tests on an
8-CU grid (tests/test_gpu_small_grid.py; this file needs no GPU, tests/test_small_grid_cases_cpu.py checks it).

Restated from csrc/patch_pass.h (patch_tiles, patch_pp, patch_pass_groups, PATCH_PASS_UNITS), csrc/hrv_common.h (xcd_remap) and the
column plans of the kernels (p2_plan, s2_plan, gf_plan, gb_plan): ``schedule(family, case, cus)`` gives, per launch, the grid and
whether it runs one (tile, pass) per unit (``pp``), and per block the units it works through in order.

HRV_RESERVE_CUS / hrv_set_reserved_cus never take the persistent grid below 8 CUs, so a reservation larger than the chip gives
exactly 8: a 60-tile tensor then sends a block of a two-per-CU kernel through 4 units, and 15 / 16 / 17 tiles lie around the pp
boundary (tiles < 2 x CUs).  With integer operands the float64 reference of such a tensor takes well under a second.

The shapes (N, H, W) of the tile grid, all counts at 8 CUs:
  15 tiles (1, 35, 77)    pp, one below the boundary
  16 tiles (1, 50, 61)    the first non-pp count: one unit per block of a two-per-CU kernel, two per block of spade_gb
  17 tiles (1, 10, 260)   ONE tile row (every tile touches the top and the bottom border); the smallest wrap; xcd_remap remainder 1
  60 tiles (2, 65, 81)    a deep loop with uneven remainders: 16 blocks = 12 x 4 + 4 x 3 units, 24 blocks (conv_p2's single-tile
                          passes, three per CU) = 12 x 3 + 12 x 2, 8 blocks (spade_gb) = 4 x 8 + 4 x 7
  60 tiles (15, 20, 20)   four tiles per image: EVERY block that takes three or more units changes image inside its run

About the image switch.  xcd_remap deals each XCD one contiguous range of tiles, and a grid that is a multiple of 8 keeps a block on
one XCD, so a block only ever sees tiles of its XCD's range.  At (2, 65, 81) the ranges are 0-7, 8-15, 16-23, 24-31, 32-38, ... and
the images meet at tile 30: the blocks of XCD 3 alone change image (spade_fused's c_n) inside a run.  The (15, 20, 20) cases are
there so that the others do too.

conv_s2 tiles its OUTPUT (forward, cells form) or ONE PHASE of dX (data gradient): its cases choose H x W so that this grid (s2_grid)
has the extents above.  The patch tiles 17 / 18 of the generic engine cut 8-row tiles (``engine_tiles``), so the same extents give
them other counts; their grid is 8 or 16 blocks (one or two per CU, by their LDS size)."""
from collections import namedtuple

import exact_cases as E
import spade_uniform_cases as U

CUS = 8

T15, T16, T17, T60, T60N = (1, 35, 77), (1, 50, 61), (1, 10, 260), (2, 65, 81), (15, 20, 20)


# ---------------------------------------------------------------------------------------------------------------
# the scheduler
# ---------------------------------------------------------------------------------------------------------------
def patch_tiles(N, H, W):
    return N * ((H + 15) // 16) * ((W + 15) // 16)


def patch_pp(tiles, cus):
    return tiles < 2 * cus


def xcd_remap(bid, nblk):
    xcd = bid & 7
    q, r = nblk >> 3, nblk & 7
    base = xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q
    return base + (bid >> 3)


def _plan_4_rem(NT):
    """conv_p2 / conv_s2: passes of 4 column tiles, then the remainder"""
    return [4] * (NT // 4) + ([NT % 4] if NT % 4 else [])


def _plan_4_2_5(NT):
    """spade_gb forward / spade_fused: passes of 4, then one of 2, then (an odd count: the 16-channel tail) one of 5"""
    n5 = NT & 1
    rest = NT - 5 * n5
    assert rest >= 0, NT
    n2 = 1 if rest % 4 == 2 else 0
    return [4] * ((rest - 2 * n2) // 4) + [2] * n2 + [5] * n5


def _gamma_beta_tiles(C):
    return 2 * (C // 32) + (1 if C % 32 else 0)


# family -> (pass widths of a case, blocks per CU by pass width, pp allowed, the tile grid (N, H, W) of a case)
def _s2_out(c, h, w):
    return (c[2], c[h] // 2 + 1, c[w] // 2 + 1)


FAMILIES = {
    "p2_fwd": (lambda c: _plan_4_rem((c[1] + 31) // 32), lambda ntp: 3 if ntp == 1 else 2, True, lambda c: c[2:5]),
    "p2_dgrad": (lambda c: _plan_4_rem((c[1] + 31) // 32), lambda ntp: 3 if ntp == 1 else 2, True, lambda c: c[2:5]),
    "p2_pair": (lambda c: _plan_4_rem(((c[6] if len(c) > 6 else 128) + 31) // 32), lambda ntp: 3 if ntp == 1 else 2, True, lambda c: c[1:4]),
    "gb_fwd": (lambda c: _plan_4_2_5(_gamma_beta_tiles(c[0])), lambda ntp: 1, False, lambda c: c[1:4]),
    "gb_dgrad": (lambda c: [4], lambda ntp: 1, False, lambda c: c[1:4]),
    "fused": (lambda c: _plan_4_2_5(_gamma_beta_tiles(c[0])), lambda ntp: 2, True, lambda c: c[1:4]),
    "s2_fwd": (lambda c: _plan_4_rem(c[1] // 32), lambda ntp: 2, True, lambda c: _s2_out(c, 3, 4)),
    "s2_dgrad": (lambda c: _plan_4_rem(4 * c[1] // 32), lambda ntp: 2, True, lambda c: (c[2], (c[3] + 1) // 2, (c[4] + 1) // 2)),
    "s2_cells": (lambda c: _plan_4_rem(c[1] // 32), lambda ntp: 2, True, lambda c: _s2_out(c, 3, 4)),
    "s2_split3_fwd": (lambda c: _plan_4_rem(c[1] // 32), lambda ntp: 2, True, lambda c: _s2_out(c, 3, 4)),
}

Unit = namedtuple("Unit", "u tile n passes")                  # unit number of the launch, tile after xcd_remap, its image, its passes
Launch = namedtuple("Launch", "pass0 pass1 ntp grid pp tiles blocks")      # blocks[b]: the Units of block b in order


def gb_chunks(case):
    """128-channel chunks of spade_gb's data-gradient source [dgamma | dbeta] (more than one: the patch is reloaded per pass)"""
    return (2 * case[0] + 127) // 128


def schedule_of(ntps, bpc, may_pp, grid_nhw, cus=CUS, tiles=None, tile_of=None):
    """patch_pass_groups + PATCH_PASS_UNITS.  ``tiles`` / ``tile_of``: a launch over a list (spade_fused's heavy list) instead of
    every tile of the grid; pp is the host's, from the whole grid."""
    N, H, W = grid_nhw
    total = patch_tiles(N, H, W)
    m = total if tiles is None else tiles
    per_image = total // N
    pp = may_pp and patch_pp(total, cus)
    out, a = [], 0
    while a < len(ntps):
        b = a
        while b < len(ntps) and ntps[b] == ntps[a]:
            b += 1
        npg = b - a
        units = m * npg if pp else m
        grid = min(total * npg if pp else total, bpc(ntps[a]) * cus)       # (the host sizes the grid from the whole tile count)
        blocks = []
        for blk in range(grid):
            run = []
            for u in range(blk, units, grid):
                bid = u // npg if pp else u
                t = xcd_remap(bid, m)
                t = t if tile_of is None else tile_of(t)
                run.append(Unit(u, t, t // per_image, (a + u % npg,) if pp else tuple(range(a, b))))
            blocks.append(run)
        out.append(Launch(a, b, ntps[a], grid, pp, m, blocks))
        a = b
    return out


def schedule(fam, case, cus=CUS):
    ntps, bpc, may_pp, grid = FAMILIES[fam]
    return schedule_of(ntps(case), bpc, may_pp, grid(case), cus)


def tiles_of(fam, case):
    return patch_tiles(*FAMILIES[fam][3](case))


def units_per_block(launch):
    n = [len(r) for r in launch.blocks]
    return min(n), max(n)


def image_switches(launch):
    """blocks of the launch whose run holds two consecutive units of different images"""
    return sum(1 for r in launch.blocks if any(x.n != y.n for x, y in zip(r, r[1:])))


def stale_toggles(launch):
    """blocks in which consecutive (tile, pass) steps differ in pass every time (c_pass never matches) and that take >= 2 steps"""
    k = 0
    for r in launch.blocks:
        steps = [p for un in r for p in un.passes]
        k += len(steps) >= 2 and all(x != y for x, y in zip(steps, steps[1:]))
    return k


def locate(fam, case, cus=CUS):
    """(n, y, x) of a pixel of the family's tile grid -> 'launch: tile, block, position in the block's run' for every launch"""
    N, H, W = FAMILIES[fam][3](case)
    tx, ty = (W + 15) // 16, (H + 15) // 16
    where = {}
    for li, L in enumerate(schedule(fam, case, cus)):
        for blk, run in enumerate(L.blocks):
            for pos, un in enumerate(run):
                where.setdefault(un.tile, []).append(
                    f"launch {li} (passes {L.pass0}..{L.pass1 - 1} x {L.ntp} tiles, grid {L.grid}{', pp' if L.pp else ''}): unit {un.u} pass "
                    f"{'/'.join(map(str, un.passes))} = block {blk}'s unit {pos + 1} of {len(run)}")
    half = 2 if fam == "s2_dgrad" else 1                 # (the data gradient tiles one phase of dX: pixel (y, x) is cell (y / 2, x / 2))

    def f(ix):
        n, y, x = ix[0], ix[1] // half, ix[2] // half
        t = (n * ty + y // 16) * tx + x // 16
        return f"tile {t} (image {n}, corner {16 * (y // 16)}, {16 * (x // 16)}): " + "; ".join(where.get(t, ["not scheduled"]))
    return f


def engine_tiles(case):
    """the 8-row x 16-column tiles of the patch tiles 17 / 18, and their column tiles (128 / 64 columns)"""
    _, cfg, Cin, Cout, k, N, H, W = case[:8]
    return N * ((H + 7) // 8) * ((W + 15) // 16), (Cout + (127 if cfg == 17 else 63)) // (128 if cfg == 17 else 64)


# ---------------------------------------------------------------------------------------------------------------
# the cases (tuples for the generators of exact_cases.py).  At the three boundary shapes: a layer with two equal passes and a tail
# launch, so that under pp a block takes two (tile, pass) units of different passes.  At 60 tiles, per family: a single pass, two
# equal passes in one launch, a tail launch of another width, and the family's own extras; both output storages and every epilogue.
# ---------------------------------------------------------------------------------------------------------------
def _at(shapes, f):
    return [f(*s) for s in shapes]


_B = (T15, T16, T17)

P2_FWD = (_at(_B, lambda N, H, W: (32, 272, N, H, W, True, "relu", None)) +
          _at(_B, lambda N, H, W: (80, 32, N, H, W, False, "lrelu", "f32")) +
          [(32, 128, 2, 65, 81, True, "relu", None),                # one pass of 4
           (32, 256, 2, 65, 81, False, "relu", None),               # two equal passes: the constants are stale at every step
           (32, 272, 2, 65, 81, True, "lrelu", "bf16"),             # + the single-tile tail launch, three blocks per CU
           (80, 32, 2, 65, 81, True, "relu", "f32"),                # a single-tile-pass layer (24 blocks); 3 K chunks, the last half empty
           (64, 96, 2, 65, 81, False, None, None),                  # one pass of 3
           (32, 160, 15, 20, 20, True, "relu", None)])              # 4 + 1, every block changes image
P2_DGRAD = (_at(_B, lambda N, H, W: (32, 272, N, H, W, True, 0.0, None)) +
            [(32, 128, 2, 65, 81, True, 0.0, None), (32, 256, 2, 65, 81, False, None, "before"), (32, 272, 2, 65, 81, True, 0.0, "after"),
             (64, 32, 2, 65, 81, True, 0.5, None), (64, 64, 2, 65, 81, False, 0.0, None)])
P2_PAIR = (_at(_B, lambda N, H, W: (16, N, H, W, 1, True, 272)) +
           [(16, 2, 65, 81, 1, True), (16, 2, 65, 81, 1, False, 256), (16, 2, 65, 81, 2, True, 272), (48, 2, 65, 81, 1, True, 32)])
GB_FWD = (_at(_B, lambda N, H, W: (144, N, H, W, 1, 1.0, True, "lrelu", True)) +
          [(64, 2, 65, 81, 1, 1.0, True, "lrelu", True),            # one pass of 4
           (128, 2, 65, 81, 2, 2.0, False, None, False),            # two equal passes
           (80, 2, 65, 81, 1, 1.0, True, None, True),               # the 5-tile tail alone
           (144, 2, 65, 81, 3, 2.0, True, "lrelu", True),           # 4 + 5
           (96, 2, 65, 81, 1, 1.0, False, "lrelu", False),          # 4 + 2
           (64, 15, 20, 20, 1, 1.0, True, "lrelu", True)])
GB_DGRAD = (_at(_B, lambda N, H, W: (80, N, H, W, 1, True)) +
            [(32, 2, 65, 81, 1, True),                              # one 64-channel chunk
             (80, 2, 65, 81, 2, True),                              # two chunks (128 + 32: the half-tile instance), repatch
             (96, 2, 65, 81, 1, False),                             # two chunks (128 + 64), fp32 out
             (64, 2, 65, 81, 1, False)])                            # one full chunk
FUSED = (_at(_B, lambda N, H, W: (144, N, H, W, 0, 1.0, True, "lrelu", True)) +
         [(64, 2, 65, 81, 0, 1.0, True, "lrelu", True), (128, 2, 65, 81, 1, 2.0, False, None, False), (80, 2, 65, 81, 0, 1.0, True, "lrelu", True),
          (144, 2, 65, 81, 1, 1.0, True, None, True), (96, 2, 65, 81, 0, 2.0, False, "lrelu", False),
          (64, 15, 20, 20, 0, 1.0, True, "lrelu", True), (128, 15, 20, 20, 0, 1.0, False, "lrelu", True)])
# conv_s2: the tile grid is the output (H / 2 + 1) or one phase of dX ((H + 1) / 2)
_S2F = ((1, 69, 152), (1, 98, 121), (1, 19, 518))
_S2D = ((1, 69, 154), (1, 100, 121), (1, 19, 520))
S2_FWD = (_at(_S2F, lambda N, H, W: (32, 192, N, H, W, True, "lrelu", 1.0, None)) +
          [(32, 128, 2, 129, 160, True, "lrelu", 1.0, None), (32, 256, 2, 129, 160, False, None, 1.0, None),
           (32, 192, 2, 129, 160, True, "lrelu", 4.0, 2.0), (64, 64, 2, 129, 160, False, "lrelu", 1.0, 0.5)])
S2_DGRAD = (_at(_S2D, lambda N, H, W: (32, 64, N, H, W, True, "both")) +
            [(64, 32, 2, 130, 161, True, "both"), (64, 64, 2, 130, 161, False, "none"), (32, 64, 2, 130, 161, True, "mask"),
             (32, 32, 2, 130, 161, True, "res32")])
S2_CELLS = (_at(((1, 68, 152), (1, 98, 120), (1, 18, 518)), lambda N, H, W: (3, 64, N, H, W, False)) +
            [(10, 64, 2, 128, 160, False), (12, 64, 2, 128, 160, True)])
S2_SPLIT3_FWD = [(32, 128, 2, 129, 160)]
ENGINE = [("cfg17_sg17", 17, 128, 128, 3, 1, 10, 260, True, "relu", None, 1.0, None),
          ("cfg18_sg17", 18, 128, 64, 3, 1, 10, 260, False, "lrelu", None, 1.0, None),
          ("cfg17_sg60", 17, 128, 125, 3, 2, 65, 81, False, "relu", None, 1.0, None),
          ("cfg18_sg60", 18, 128, 64, 3, 2, 65, 81, True, "lrelu", "bf16", 1.0, None)]
# (thin_conv: the dispatcher hands it layers of 65,536 pixels and more, so its existing 2 x 180 x 200 case is the small-grid case:
#  some 560 tiles over the 8-CU grid)

TABLES = {"p2_fwd": (P2_FWD, E.p2_fwd), "p2_dgrad": (P2_DGRAD, E.p2_dgrad), "p2_pair": (P2_PAIR, E.pair_dgrad), "gb_fwd": (GB_FWD, E.gb_fwd),
          "gb_dgrad": (GB_DGRAD, E.pair_dgrad), "fused": (FUSED, E.fused), "s2_fwd": (S2_FWD, E.s2_fwd), "s2_dgrad": (S2_DGRAD, E.s2_dgrad),
          "s2_cells": (S2_CELLS, E.s2_cells), "s2_split3_fwd": (S2_SPLIT3_FWD, E.s2_split3_fwd), "engine": (ENGINE, E.engine)}

# spade_uniform_cases.py (N = 2): (H, W, shift, map, C[, rstd, noise, act, save]).  Every tile on the border of an image is heavy
# (its 20 x 20 patch leaves the image), so 60 tiles of two images hold at most 2 x 12 interior tiles: at (2, 80, 96) 22 light ones
# after the two representatives.  A light list longer than the uniform kernel's 32 blocks needs more tiles: (2, 98, 98) has 98
# tiles, 2 x 25 interior, 48 light, 50 heavy -- the uniform kernel strides twice, and a block of the heavy launch (16 blocks,
# xcd_remap over the 50 entries of the heavy list) takes 3 or 4 of them.
UNIFORM_60 = (80, 96)
UNIFORM_98 = (98, 98)
UNIFORM_EXACT = [(80, 96, 0, "one_class", 64, 1.0, True, "lrelu", True), (98, 98, 0, "one_class", 32, 2.0, False, None, True),
                 (98, 98, 0, "edge3", 80, 1.0, True, "lrelu", True)]
# one shape per label map ("speckle" leaves light tiles only where the map is sampled at every other pixel)
UNIFORM_FORWARD = [(98, 98, 1 if m == "speckle" else 0, m, C) for m, C in zip(U.MAPS, (64, 80, 32, 64, 80, 32))]


def uniform_counts(H, W, shift, name):
    c = U.classify(U.label_map(name, H, W, shift), shift, 2, H, W)
    return len(c["heavy"]), len(c["light"])


def uniform_schedule(H, W, shift, name, C, cus=CUS):
    """the heavy launch(es) over the plan's heavy list, and the (grid, entries per block) of spade_uniform_kernel over the light list"""
    c = U.classify(U.label_map(name, H, W, shift), shift, 2, H, W)
    heavy = [e & 0xFFFFFF for e in c["heavy"]]
    L = schedule_of(_plan_4_2_5(_gamma_beta_tiles(C)), lambda ntp: 2, True, (2, H, W), cus, tiles=len(heavy), tile_of=lambda i: heavy[i])
    grid = min(patch_tiles(2, H, W), 4 * cus)
    return L, (grid, [len(range(b, len(c["light"]), grid)) for b in range(grid)])


def case_id(case):
    return "-".join(str(v) for v in case)
