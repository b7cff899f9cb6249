"""The zero-tolerance tests of the persistent kernels with the grid cut to 8 CUs (tests/small_grid_cases.py: why, and the restated
scheduler).  At the device's own grid a block of conv_p2 / conv_s2 / spade_fused / spade_gb works through one or two units in every
exact case; here a 60-tile tensor sends it through 3-4 (spade_gb: 7-8) and the 250 x 270 cases through 34, so what a block carries
from unit to unit -- the weight ring's stage, the prefetched patch, the stale-constants test, the hand-over at a unit's last pass
-- is compared bit for bit with float64.  The weight gradients run with one or two slabs, thin_conv and the patch tiles 17 / 18 with
8 or 16 persistent blocks.

The grid is cut through the environment only (HRV_RESERVE_CUS=4000 + reload; persistent_cus() never goes below 8): an explicit
hrv_set_reserved_cus would outlive every later reload in this process.  tests/conftest.py's autouse fixture reloads the environment
after each test, which restores the grid; the last test of this module checks that.

A failing comparison names the tile, the block and the unit's position in the block's run (small_grid_cases.locate)."""
import pytest
import torch

import exact_cases as E
import exact_runners as R
import small_grid_cases as S
import spade_uniform_cases as U

pytestmark = pytest.mark.gpu

_CUS0 = []            # hrv_persistent_cus() before this module changed anything


def _lib():
    import hr_viton_amd  # noqa: F401
    from hr_viton_amd import _lib as L
    return L


@pytest.fixture(scope="module", autouse=True)
def _device_cus():
    _CUS0.append(int(_lib().load().hrv_persistent_cus()))
    yield


@pytest.fixture
def grid8(monkeypatch):
    L = _lib()
    monkeypatch.setenv("HRV_RESERVE_CUS", "4000")
    L.reload_env()
    assert int(L.load().hrv_persistent_cus()) == S.CUS == 8
    yield
    R.LOCATE[0] = None


def _located(fam, case):
    R.LOCATE[0] = S.locate(fam, case) if fam in S.FAMILIES else None


RUN = {"p2_fwd": R.run_p2_fwd, "p2_dgrad": R.run_p2_dgrad, "p2_pair": R.run_p2_pair, "gb_fwd": R.run_gb_fwd, "gb_dgrad": R.run_gb_dgrad,
       "fused": R.run_fused, "s2_fwd": R.run_s2_fwd, "s2_dgrad": R.run_s2_dgrad, "s2_cells": R.run_s2_cells,
       "s2_split3_fwd": R.run_s2_split3_fwd}

NEW = [(f, c) for f in RUN for c in S.TABLES[f][0]]
OLD = [(f, c) for f in RUN for c in E.TABLES[f][0]]


def _ids(pairs):
    return [f"{f}:{E.case_id(c)}" for f, c in pairs]


# ---------------------------------------------------------------------------------------------------------------
# every new case, every existing case of the persistent families
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam,case", NEW, ids=_ids(NEW))
def test_new_case_on_8_cus(fam, case, grid8):
    _located(fam, case)
    RUN[fam](case)


@pytest.mark.parametrize("fam,case", OLD, ids=_ids(OLD))
def test_existing_case_on_8_cus(fam, case, grid8):
    """(the 250 x 270 cases: 544 tiles over 16 blocks, 34 units per block; their references are the cached ones)"""
    _located(fam, case)
    RUN[fam](case)


_ENGINE = [c for c in E.ENGINE if c[1] in (17, 18)] + S.ENGINE


@pytest.mark.parametrize("case", _ENGINE, ids=[c[0] for c in _ENGINE])
def test_patch_tiles_on_8_cus(case, grid8):
    R.run_engine(case, case[1])


@pytest.mark.parametrize("case", E.THIN, ids=E.case_id)
def test_thin_conv_on_8_cus(case, grid8, monkeypatch):
    """(the dispatcher gives thin_conv only layers of 65,536 pixels and more: the existing case, some 560 tiles over the 8-CU grid)"""
    R.run_thin(case, monkeypatch)


_WGRAD = [c for c in E.WGRAD if c[1].startswith("conv_wgrad_tr_kernel") or c[1] == "conv_wgrad_s2_kernel"]


@pytest.mark.parametrize("case", _WGRAD, ids=[c[0] for c in _WGRAD])
def test_weight_gradient_on_8_cus(case, grid8):
    """The slab count follows the CU count (wgrad_slabs: CUs / jobs): one or two slabs here -- the reduce tail over a single slab,
    accumulate=True on one slab, and grids larger than the CU count.  The kernel-name assertion is the runner's."""
    assert len(_WGRAD) == 11
    R.run_wgrad(case)


# ---------------------------------------------------------------------------------------------------------------
# the tile plan
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", U.EXACT + S.UNIFORM_EXACT, ids=U.case_id)
def test_exact_integer_with_plan_on_8_cus(case, grid8):
    H, W, shift, name = case[:4]
    assert R.run_uniform_exact(case) == S.uniform_counts(H, W, shift, name)


@pytest.mark.parametrize("case", S.UNIFORM_FORWARD, ids=U.case_id)
def test_plan_on_equals_plan_off_on_8_cus(case, grid8):
    """98 tiles: 48 light entries over the uniform kernel's 32 blocks ("one_class"), the heavy list over 16 blocks"""
    H, W, shift, name, C_ = case
    assert R.run_uniform_plan_on_equals_plan_off(case, wraps=True) == S.uniform_counts(H, W, shift, name)


# ---------------------------------------------------------------------------------------------------------------
# the loop ran as restated: the diagnostic timeline of the single-launch, non-pp cases
# ---------------------------------------------------------------------------------------------------------------
def _with_tlog(tiles, run):
    """``run()`` once more with the diagnostic timeline on a zeroed buffer of exactly tiles x 8 words: [tiles, 8] int64 on the CPU"""
    L = _lib()
    lib = L.load()
    tlog = torch.zeros(tiles * 8, dtype=torch.int64, device="cuda")
    L.check(lib.hrv_diag_set_tlog(tlog.data_ptr(), tiles), "hrv_diag_set_tlog")
    try:
        run()
        torch.cuda.synchronize()
    finally:
        L.check(lib.hrv_diag_set_tlog(None, 0), "hrv_diag_set_tlog")
    return tlog.cpu().view(tiles, 8)


_TL = [(f, c) for f, c in NEW + OLD if f in ("p2_fwd", "p2_dgrad", "p2_pair", "fused", "gb_fwd", "gb_dgrad") and
       len(S.schedule(f, c)) == 1 and not S.schedule(f, c)[0].pp and S.tiles_of(f, c) < 100]


@pytest.mark.parametrize("fam,case", _TL, ids=_ids(_TL))
def test_timeline_shows_the_restated_loop(fam, case, grid8):
    """slot 5 of unit u = the block that ran it = u % grid, slot 3 (stores drained) set for every unit; the outputs of the logged run
    are exact as well (the runner asserts them)"""
    (L,) = S.schedule(fam, case)
    assert L.tiles == S.tiles_of(fam, case) and not L.pp
    _located(fam, case)
    t = _with_tlog(L.tiles, lambda: RUN[fam](case))
    assert bool((t[:, 3] != 0).all()), ("units without a drained stamp", (t[:, 3] == 0).nonzero().flatten().tolist())
    assert t[:, 5].tolist() == [u % L.grid for u in range(L.tiles)], (L.grid, t[:, 5].tolist())
    for b, run in enumerate(L.blocks):
        assert [un.u for un in run] == [u for u in range(L.tiles) if int(t[u, 5]) == b]


# (one column tile, more tiles than the 16 blocks of a two-per-CU grid)
_TL_ENGINE = [c for c in _ENGINE if S.engine_tiles(c)[1] == 1 and 16 < S.engine_tiles(c)[0] < 200]


@pytest.mark.parametrize("case", _TL_ENGINE, ids=[c[0] for c in _TL_ENGINE])
def test_timeline_of_the_patch_tiles(case, grid8):
    """tiles 17 / 18 (8-row tiles, one column tile: units = tiles): the grid is one or two blocks per CU"""
    tiles, ncol = S.engine_tiles(case)
    assert ncol == 1 and tiles > 16
    t = _with_tlog(tiles, lambda: R.run_engine(case, case[1]))
    assert bool((t[:, 3] != 0).all())
    grid = int(t[:, 5].max()) + 1
    assert grid in (8, 16), grid
    assert t[:, 5].tolist() == [u % grid for u in range(tiles)]


# ---------------------------------------------------------------------------------------------------------------
# the production data-parallel setting: 16 CUs left to the collectives
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", sorted(E.WRAP))
def test_wrap_cases_with_16_reserved_cus(fam, monkeypatch):
    L = _lib()
    monkeypatch.setenv("HRV_RESERVE_CUS", "16")
    L.reload_env()
    cus = int(L.load().hrv_persistent_cus())
    assert cus == torch.cuda.get_device_properties(0).multi_processor_count - 16
    case = E.WRAP[fam][0]
    R.LOCATE[0] = S.locate(fam, case, cus)
    try:
        RUN[fam](case)
    finally:
        R.LOCATE[0] = None


def test_the_grid_is_back():
    """(last in the module) every test above changed the grid through the environment alone, so the reload after it restored it"""
    assert R.LOCATE[0] is None
    assert int(_lib().load().hrv_persistent_cus()) == _CUS0[0] >= 8
