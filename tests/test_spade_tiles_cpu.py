"""The SPADE tile-classification rule on its pure-Python reference (tests/spade_uniform_cases.py), CPU only: what the GPU test
then holds the kernel's lists against."""
import pytest
import torch

import spade_uniform_cases as U

N = 2


def _plan(name, H, W, shift):
    return U.classify(U.label_map(name, H, W, shift), shift, N, H, W)


def _is_light(p, t):
    return any((e & 0xFFFFFF) == t for e in p["light"])


def _is_heavy(p, t):
    return any((e & 0xFFFFFF) == t for e in p["heavy"])


@pytest.mark.parametrize("shape", U.SHAPES, ids=U.case_id)
@pytest.mark.parametrize("name", U.MAPS)
def test_lists_partition_the_tiles(shape, name):
    H, W, shift = shape
    p = _plan(name, H, W, shift)
    m = N * ((H + 15) // 16) * ((W + 15) // 16)
    tiles = [e & 0xFFFFFF for e in p["heavy"]] + [e & 0xFFFFFF for e in p["light"]]
    assert sorted(tiles) == list(range(m))
    assert [e & 0xFFFFFF for e in p["heavy"]] == sorted(e & 0xFFFFFF for e in p["heavy"])
    assert [e & 0xFFFFFF for e in p["light"]] == sorted(e & 0xFFFFFF for e in p["light"])
    # one representative per class present among the light-classified tiles, the lowest of its class, flagged on the heavy list
    present = sorted({k for k in p["cls"] if k >= 0})
    assert [k for k in range(8) if p["rep"][k] >= 0] == present
    for k in present:
        assert p["rep"][k] == min(t for t, c in enumerate(p["cls"]) if c == k)
        assert p["rep"][k] | ((k + 1) << 24) in p["heavy"]
    assert sum(1 for e in p["heavy"] if e >> 24) == len(present)
    for e in p["light"]:
        assert p["cls"][e & 0xFFFFFF] == e >> 24 and p["rep"][e >> 24] != (e & 0xFFFFFF)


@pytest.mark.parametrize("shape", U.SHAPES, ids=U.case_id)
def test_border_and_partial_tiles_are_heavy(shape):
    H, W, shift = shape
    p = _plan("one_class", H, W, shift)          # every pixel of an image carries one class: only the position decides
    ty, tx = (H + 15) // 16, (W + 15) // 16
    for n in range(N):
        for r in range(ty):
            for c in range(tx):
                inside = r >= 1 and c >= 1 and 16 * r + 18 <= H and 16 * c + 18 <= W
                assert (p["cls"][(n * ty + r) * tx + c] >= 0) == inside, (n, r, c)
    # image 0 is class 1, image 1 class 3: two classes with light tiles
    assert {e >> 24 for e in p["light"]} == {1, 3}
    interior = sum(1 for k in p["cls"] if k >= 0)
    assert len(p["light"]) == interior - 2 and interior == N * sum(
        1 for r in range(1, ty) for c in range(1, tx) if 16 * r + 18 <= H and 16 * c + 18 <= W)


@pytest.mark.parametrize("shape", U.SHAPES, ids=U.case_id)
def test_two_pixel_halo(shape):
    H, W, shift = shape
    t = U.tile_index(N, H, W, 1, 16, 16)         # tile rows 16..31 of image 1; the other class starts at row 33 / 34
    assert _is_heavy(_plan("edge2", H, W, shift), t)
    assert _is_light(_plan("edge3", H, W, shift), t)
    # the tile below sees both classes either way
    assert _is_heavy(_plan("edge3", H, W, shift), U.tile_index(N, H, W, 1, 32, 16))


def test_not_one_hot_is_heavy():
    H, W, shift = 72, 56, 0
    p = _plan("multihot", H, W, shift)
    seg = U.bits(U.label_map("multihot", H, W, shift))
    # uniform patches all right -- and still heavy: two-hot at tile (16, 16), value 2.0 at tile (48, 32) of image 1
    for (y0, x0) in ((16, 16), (48, 32)):
        patch = seg[1, y0 - 2:y0 + 18, x0 - 2:x0 + 18].reshape(400, 8)
        assert bool((patch == patch[0]).all())
        assert p["cls"][U.tile_index(N, H, W, 1, y0, x0)] == -1
    assert [int(v) for v in seg[1, 16, 16]] == [0, U.ONE, U.ONE, 0, 0, 0, 0, 0]
    assert [int(v) for v in seg[1, 48, 32]] == [0, 0x4000, 0, 0, 0, 0, 0, 0]
    assert all(e >> 24 == 1 and (e & 0xFFFFFF) < 20 for e in p["light"]) and len(p["light"]) == 5      # image 0 only


def test_sampled_labels_under_seg_shift():
    H, W = 64, 48
    m1 = U.label_map("speckle", H, W, 1)
    assert bool((m1[:, 1::2, 1::2, 2] == 1).any())                 # the full-resolution map is not uniform ...
    p = U.classify(m1, 1, N, H, W)
    assert len(p["light"]) == 2 * 2 - 1                            # ... the sampled one is: every interior tile but the representative
    # the same speckle where it IS sampled (shift 0: odd level coordinates) leaves no uniform patch
    assert len(_plan("speckle", H, W, 0)["light"]) == 0
    # a label that only the sampled pixels carry: the classifier must not look at the full-resolution neighbours
    m2 = m1.clone()
    m2[:, 1::2, :, :] = 0
    m2[:, :, 1::2, :] = 0
    assert U.classify(m2, 1, N, H, W)["light"] == p["light"]


@pytest.mark.parametrize("shape", U.SHAPES, ids=U.case_id)
def test_random_map_has_no_light_tile(shape):
    H, W, shift = shape
    p = _plan("random", H, W, shift)
    assert p["light"] == [] and all(k < 0 for k in p["cls"])


def test_exact_cases_have_light_tiles():
    for case in U.EXACT:
        H, W, shift, name = case[:4]
        assert len(_plan(name, H, W, shift)["light"]) > 0, case
        d = U.exact(case)
        assert d["bound"] <= 2 ** 20
