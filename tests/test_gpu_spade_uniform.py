"""The fused SPADE forward with a tile plan (csrc/spade_tiles.hip, spade_uniform_kernel of csrc/spade_fused.hip): the classifier's
lists against the pure-Python reference, the forward with the plan against the forward without it bit for bit (out, 1 + gamma,
actv), and two cases in exact-integer form against float64 (tests/spade_uniform_cases.py).  Every forward case also asserts the
light count the reference gives: a run that sent every tile down the matrix path would pass the comparison alone."""
import pytest

import exact_runners as R
import spade_uniform_cases as U

pytestmark = pytest.mark.gpu

N = R.UN


def _mods():
    import hr_viton_amd  # noqa: F401
    from hr_viton_amd import ops, train_ops as T
    return ops, T


_seg = R._useg


@pytest.mark.parametrize("shape", U.SHAPES, ids=U.case_id)
@pytest.mark.parametrize("name", U.MAPS)
def test_classifier_lists(shape, name):
    _, T = _mods()
    H, W, shift = shape
    want = U.classify(U.label_map(name, H, W, shift), shift, N, H, W)
    plan = T.spade_tile_plan(_seg(name, H, W, shift), shift, N, H, W)
    heavy, light, rep = plan.lists()
    assert plan.counts() == (len(want["heavy"]), len(want["light"]))
    assert heavy == want["heavy"] and light == want["light"] and rep == want["rep"]


@pytest.mark.parametrize("case", U.FORWARD + U.WRAP, ids=U.case_id)
def test_plan_on_equals_plan_off(case):
    R.run_uniform_plan_on_equals_plan_off(case, wraps=case in U.WRAP)


@pytest.mark.parametrize("case", U.EXACT, ids=U.case_id)
def test_exact_integer_with_plan(case):
    R.run_uniform_exact(case)


def test_plan_is_cached_on_the_label_map(monkeypatch):
    ops, T = _mods()
    H, W, shift = U.SHAPES[0]
    seg = _seg("one_class", H, W, shift)
    monkeypatch.setenv("HRV_SPADE_UNIFORM_MIN_TILES", "1")
    monkeypatch.delenv("HRV_SPADE_UNIFORM", raising=False)
    p1 = T.spade_tile_plan_for(seg, shift, N, H, W)
    assert p1 is not None and T.spade_tile_plan_for(seg, shift, N, H, W) is p1
    assert T.spade_tile_plan_for(_seg("one_class", H, W, shift), shift, N, H, W) is not p1        # a new label map: a new plan
    monkeypatch.setenv("HRV_SPADE_UNIFORM_MIN_TILES", "100000")
    assert T.spade_tile_plan_for(seg, shift, N, H, W) is None
    monkeypatch.setenv("HRV_SPADE_UNIFORM_MIN_TILES", "1")
    monkeypatch.setenv("HRV_SPADE_UNIFORM", "0")
    assert T.spade_tile_plan_for(seg, shift, N, H, W) is None
