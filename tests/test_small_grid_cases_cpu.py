"""tests/small_grid_cases.py on the CPU alone: the restated scheduler against what the kernels' host code is known to do, and every
new case against (a) the conditions of an exact comparison and (b) the property its table entry claims under that scheduler at 8
CUs -- pp or not, the units a block works through, uneven remainders, an image switch inside a block's run."""
import pytest

import exact_cases as E
import small_grid_cases as S
import spade_uniform_cases as U
from test_exact_cases_cpu import test_case_meets_the_conditions_of_an_exact_comparison as _exact_conditions

NEW = [(fam, case) for fam, (table, _) in S.TABLES.items() for case in table]
SCHED = [(fam, case) for fam, case in NEW if fam in S.FAMILIES]


def _ids(pairs):
    return [f"{f}:{E.case_id(c)}" for f, c in pairs]


# ---------------------------------------------------------------------------------------------------------------
# the restatement itself
# ---------------------------------------------------------------------------------------------------------------
def test_xcd_remap_is_a_bijection():
    """for every block count 1..600 the remap permutes [0, n); each XCD (block b lands on XCD b % 8) gets one contiguous range"""
    for n in range(1, 601):
        img = [S.xcd_remap(b, n) for b in range(n)]
        assert sorted(img) == list(range(n)), n
        for xcd in range(min(8, n)):
            mine = img[xcd::8]
            assert mine == list(range(mine[0], mine[0] + len(mine))), (n, xcd)


def test_column_plans():
    assert S._plan_4_rem(9) == [4, 4, 1] and S._plan_4_rem(1) == [1] and S._plan_4_rem(8) == [4, 4] and S._plan_4_rem(6) == [4, 2]
    # spade_gb / spade_fused: C = 64, 128, 80, 144, 96, 32, 272 norm channels
    want = {64: [4], 128: [4, 4], 80: [5], 144: [4, 5], 96: [4, 2], 32: [2], 272: [4, 4, 4, 5]}
    for C, p in want.items():
        assert S._plan_4_2_5(S._gamma_beta_tiles(C)) == p, C
        assert sum(p) == S._gamma_beta_tiles(C)


@pytest.mark.parametrize("fam", sorted(E.WRAP))
def test_wrap_cases_under_256_cus(fam):
    """What test_every_persistent_family_has_a_case_that_wraps_on_256_cus asserts, from the restated scheduler: the tile count of the
    family's grid is the one E.WRAP names, its tile count equals E.wrap_tiles and exceeds the resident blocks, the launch is not pp,
    and 32 of 512 blocks (spade_gb, one image: 16 of 256) take a second tile -- nobody a third."""
    case = E.WRAP[fam][0]
    per_cu = 1 if fam.startswith("gb_") else 2
    tiles = 272 * per_cu
    assert tuple(S.FAMILIES[fam][3](case)) == E.WRAP[fam][1:]
    assert S.tiles_of(fam, case) == E.wrap_tiles(fam) == tiles
    assert E.wrap_tiles(fam) > per_cu * 256
    for L in S.schedule(fam, case, 256):
        if L.ntp == 1 and fam.startswith("p2_"):
            assert L.grid == tiles          # (three per CU: 768 slots, every tile its own block)
            continue
        assert not L.pp and L.grid == per_cu * 256
        n = [len(r) for r in L.blocks]
        assert max(n) == 2 and n.count(2) == tiles - L.grid == 16 * per_cu


def test_reserve_16_gives_64_second_tiles():
    """the data-parallel setting (16 CUs reserved of 256): 480 blocks, 64 of them take a second tile"""
    for fam in ("p2_fwd", "fused", "s2_fwd"):
        L = S.schedule(fam, E.WRAP[fam][0], 240)[0]
        assert L.grid == 480 and [len(r) for r in L.blocks].count(2) == 64 and S.units_per_block(L) == (1, 2)


# ---------------------------------------------------------------------------------------------------------------
# every new case
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam,case", NEW, ids=_ids(NEW))
def test_new_case_meets_the_conditions_of_an_exact_comparison(fam, case, monkeypatch):
    monkeypatch.setitem(E.TABLES, fam, S.TABLES[fam])
    _exact_conditions(fam, case)


@pytest.mark.parametrize("case", S.UNIFORM_EXACT, ids=U.case_id)
def test_new_uniform_case_meets_the_conditions(case):
    d = U.exact(case)
    assert d["bound"] <= E.LIMIT
    for name, ref in d["want"].items():
        assert float(ref.abs().max()) <= d["bound"]
        if name != "actv":
            assert E.tie_share(ref) >= 0.01 and E.big_share(ref) >= 0.10, (name, E.tie_share(ref), E.big_share(ref))


def _shape_of(fam, case):
    return tuple(S.FAMILIES[fam][3](case))


@pytest.mark.parametrize("fam,case", SCHED, ids=_ids(SCHED))
def test_new_case_has_the_property_its_table_entry_claims(fam, case):
    shape, tiles = _shape_of(fam, case), S.tiles_of(fam, case)
    assert shape in (S.T15, S.T16, S.T17, S.T60, S.T60N), shape
    assert tiles == {S.T15: 15, S.T16: 16, S.T17: 17, S.T60: 60, S.T60N: 60}[shape]
    launches = S.schedule(fam, case)
    gb = fam.startswith("gb_")
    for L in launches:
        cap = S.FAMILIES[fam][1](L.ntp) * S.CUS
        assert L.grid <= cap and sorted(un.u for r in L.blocks for un in r) == list(range(L.tiles * (L.pass1 - L.pass0 if L.pp else 1)))
        lo, hi = S.units_per_block(L)
        if tiles == 15:
            assert L.pp == (not gb)
            if gb:
                assert (L.grid, lo, hi) == (8, 1, 2)
            else:                                      # 15 x passes (tile, pass) units over at most 16 (24) blocks
                assert L.grid == min(15 * (L.pass1 - L.pass0), cap) and hi == -(-15 * (L.pass1 - L.pass0) // L.grid)
        elif tiles == 16:
            assert not L.pp
            assert (L.grid, lo, hi) == ((8, 2, 2) if gb else (16, 1, 1))
        elif tiles == 17:
            assert not L.pp and shape[1] <= 16         # one tile row
            assert (L.grid, lo, hi) == ((8, 2, 3) if gb else ((16, 1, 2) if cap == 16 else (17, 1, 1)))
            assert 17 % 8 == 1
        else:
            assert not L.pp and 60 % L.grid != 0
            n = [len(r) for r in L.blocks]
            want = {16: (12, 4, 4, 3), 24: (12, 3, 12, 2), 8: (4, 8, 4, 7)}[L.grid]
            assert L.grid == cap and (n.count(want[1]), want[1], n.count(want[3]), want[3]) == want, n
            # an image switch inside a block's run: blocks of the one XCD whose tile range holds tile 30 and no others (see the
            # module's docstring), or -- four tiles per image -- every block that takes three units or more
            sw = [b for b, r in enumerate(L.blocks) if any(x.n != y.n for x, y in zip(r, r[1:]))]
            assert len(sw) == S.image_switches(L) >= 1
            if shape == S.T60N:
                assert set(sw) >= {b for b, r in enumerate(L.blocks) if len(r) >= 3}, (sw, L.grid)
            else:
                assert all(b & 7 == 3 for b in sw) and len(sw) >= min(2, L.grid // 8), (sw, L.grid)
    if tiles == 15 and not gb and launches[0].pass1 - launches[0].pass0 == 2:
        # pp with two equal passes: 30 (tile, pass) units over 16 blocks, 14 blocks take two.  The grid is even, so block b keeps
        # pass b % 2 over tiles b / 2 and b / 2 + 8: its constants stay fresh while the patch changes
        L = launches[0]
        assert (L.grid, S.units_per_block(L)) == (16, (1, 2)) and all(len({un.passes for un in r}) == 1 for r in L.blocks)
        assert all(r[0].tile != r[1].tile for r in L.blocks if len(r) == 2)


def _cases_60(fam):
    return [c for c in S.TABLES[fam][0] if _shape_of(fam, c) in (S.T60, S.T60N)]


@pytest.mark.parametrize("fam", sorted(S.FAMILIES))
def test_sixty_tile_cases_cover_what_the_family_has(fam):
    cases = _cases_60(fam)
    plans = [[L.ntp for L in S.schedule(fam, c)] for c in cases]
    passes = [[L.pass1 - L.pass0 for L in S.schedule(fam, c)] for c in cases]
    assert any(p == [1] for p in passes), "a single-pass layer"
    if fam not in ("gb_dgrad", "s2_cells", "s2_split3_fwd"):
        assert any(p[0] == 2 for p in passes), "two equal passes in one launch"
        # ... in which the constants in LDS are stale at every step of every block
        c = cases[[p[0] == 2 for p in passes].index(True)]
        L = S.schedule(fam, c)[0]
        assert S.stale_toggles(L) == L.grid
    if fam in ("p2_fwd", "p2_dgrad", "p2_pair"):
        assert any(p == [4, 1] and q == [2, 1] for p, q in zip(plans, passes)), "272 columns: 4 + 4 and a single-tile tail launch"
        assert any(p == [1] for p in plans), "a single-tile-pass layer (three blocks per CU)"
        assert S.schedule(fam, cases[plans.index([1])])[0].grid == 24
    if fam in ("gb_fwd", "fused"):
        assert [5] in plans and [4, 5] in plans, "80 and 144 channels: the 5-tile tail, 4 + 5"
    if fam in ("s2_fwd",):
        assert [4, 2] in plans
    if fam == "gb_dgrad":
        assert {S.gb_chunks(c) for c in cases} == {1, 2} and any(2 * c[0] % 128 == 32 for c in cases)
    # both output storages, every epilogue
    if fam == "p2_fwd":
        assert {c[5] for c in cases} == {True, False} and {c[7] for c in cases} == {None, "f32", "bf16"} and {c[6] for c in cases} >= {"relu", "lrelu", None}
    if fam == "p2_dgrad":
        assert {c[5] for c in cases} == {True, False} and {c[7] for c in cases} == {None, "before", "after"} and {c[6] for c in cases} == {None, 0.0, 0.5}
    if fam in ("p2_pair", "gb_dgrad"):
        assert {c[5] for c in cases} == {True, False}
    if fam in ("gb_fwd", "fused"):
        assert {c[-3] for c in cases} == {True, False} and {c[-1] for c in cases} == {True, False} and {c[-2] for c in cases} == {"lrelu", None}
    if fam == "s2_fwd":
        assert {c[5] for c in cases} == {True, False}
    if fam == "s2_dgrad":
        assert {c[5] for c in cases} == {True, False} and {c[6] for c in cases} == {"both", "none", "mask", "res32"}


def test_sixty_tile_references_stay_small():
    """pixels x K x columns of every new case stays below the existing wrap case's of its family: the float64 reference of the
    250 x 270 cases takes seconds, these a fraction"""
    def work(fam, c):
        N, H, W = S.FAMILIES[fam][3](c)
        k, cols = {"p2_fwd": (9 * c[0], c[1]), "p2_dgrad": (9 * c[0], c[1]), "gb_fwd": (9 * 128, 2 * c[0]), "fused": (9 * 128, 2 * c[0]),
                   "s2_fwd": (16 * c[0], c[1]), "s2_dgrad": (4 * c[0], 4 * c[1]), "s2_cells": (16 * c[0], c[1]), "s2_split3_fwd": (16 * c[0], c[1]),
                   "p2_pair": (18 * c[0], c[6] if len(c) > 6 else 128), "gb_dgrad": (18 * c[0], 128)}[fam]
        return N * H * W * k * cols
    for fam, case in SCHED:
        ref = E.WRAP[fam if fam in E.WRAP else "s2_fwd"][0]
        assert work(fam, case) <= work(fam if fam in E.WRAP else "s2_fwd", ref), (fam, case)


def test_engine_cases_are_single_column_tile_patch_launches():
    """the timeline check of the GPU test hands the kernel a buffer of tiles x 8 words: one column tile, so units = tiles"""
    for c in S.ENGINE:
        tiles, ncol = S.engine_tiles(c)
        assert c[1] in (17, 18) and c[2] % 128 == 0 and ncol == 1 and tiles > 16, c
    for c in E.ENGINE:
        if c[1] in (17, 18) and c[0] != "cfg18_split":
            assert S.engine_tiles(c)[1] == 1, c
    assert S.engine_tiles(E.ENGINE[-1])[0] == 32 * 17 and S.engine_tiles(S.ENGINE[2])[0] == 2 * 9 * 6


# ---------------------------------------------------------------------------------------------------------------
# the tile plan at 8 CUs
# ---------------------------------------------------------------------------------------------------------------
def test_uniform_shapes():
    # 60 tiles of two images: at most 24 interior tiles, so the light list cannot pass the uniform kernel's 32 blocks
    assert S.patch_tiles(2, *S.UNIFORM_60) == 60 and S.uniform_counts(*S.UNIFORM_60, 0, "one_class") == (38, 22)
    assert not S.patch_pp(60, S.CUS)
    # 98 tiles: 48 light entries over 32 blocks (16 blocks take two), 50 heavy entries over 16 blocks (3 or 4 each)
    assert S.patch_tiles(2, *S.UNIFORM_98) == 98 and S.uniform_counts(*S.UNIFORM_98, 0, "one_class") == (50, 48)
    L, (grid, per_block) = S.uniform_schedule(*S.UNIFORM_98, 0, "one_class", 64)
    assert grid == 32 and sorted(set(per_block)) == [1, 2] and per_block.count(2) == 16
    assert len(L) == 1 and not L[0].pp and L[0].grid == 16 and S.units_per_block(L[0]) == (3, 4)
    assert sorted(un.tile for r in L[0].blocks for un in r) == sorted(e & 0xFFFFFF for e in U.classify(
        U.label_map("one_class", 98, 98, 0), 0, 2, 98, 98)["heavy"])
    assert S.image_switches(L[0]) >= 1
    for H, W, shift, name, C in S.UNIFORM_FORWARD:
        heavy, light = S.uniform_counts(H, W, shift, name)
        assert heavy + light == 98 and (light == 0) == (name == "random"), (name, heavy, light)
    assert {c[3] for c in S.UNIFORM_FORWARD} == set(U.MAPS)
