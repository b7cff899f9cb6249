"""tests/diffaug_cases.py on the CPU alone: the restatement's fp32 decode against a pure-Python integer / fraction decode, what the
forced table guarantees to the GPU tests (no comparison of two all-zero or two untouched tensors), the restated backward against
torch's float64 autograd of the restated forward, the policy parser, the library's symbols and train_generator.py's flag."""
import os
import re

import numpy as np
import pytest
import torch

import diffaug_cases as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["hrv_diffaug_mean_f32", "hrv_diffaug_concat_f32", "hrv_diffaug_gsum_f32", "hrv_diffaug_bwd_f32"]
ALL_SHAPES = D.SHAPES + D.POW2_SHAPES + [(1, 1024, 768)]


@pytest.mark.parametrize("shape", ALL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_decode_equals_the_integer_decode(shape):
    _, H, W = shape
    g = torch.Generator().manual_seed(H * W)
    rows = [r for _, r in D.forced_rows(H, W)] + list(torch.rand(200, 8, generator=g).numpy())
    # uniforms next to every bin edge of both decodes: the fp32 product may round across the edge, and both sides must follow it
    for extent in (H, W):
        S = (extent + 4) // 8
        for bins in (2 * S + 1, extent + 1 - (extent // 2) % 2):
            for j in range(1, bins):
                e = np.float32(j / bins)
                for v in (np.nextafter(e, np.float32(0)), e, np.nextafter(e, np.float32(1))):
                    rows.append(np.full(8, v, dtype=np.float32))
    for r in rows:
        for flags in (D.GEOMETRY, D.TRANSLATION, D.CUTOUT, D.COLOR):
            got = D.decode(r, flags, H, W)[1]
            assert got == D.decode_geom_py(r, flags, H, W), (r, flags)
            ty, tx, y0, y1, x0, x1 = got
            assert abs(ty) <= (H + 4) // 8 and abs(tx) <= (W + 4) // 8 and 0 <= y0 <= y1 <= H and 0 <= x0 <= x1 <= W
            if flags == D.COLOR:
                assert got == (0, 0, 0, 0, 0, 0)


def test_decode_of_the_edges():
    H, W = 17, 13
    mid = np.asarray([0.5] * 8, dtype=np.float32)
    (beta, s, k), geom = D.decode(mid, D.ALL, H, W)
    assert (float(beta), float(s), float(k)) == (0.0, 1.0, 1.0) and geom[:2] == (0, 0)
    assert D.decode(mid, D.GEOMETRY, H, W)[0] == (0.0, 1.0, 1.0)
    top = np.asarray([D.TOP] * 8, dtype=np.float32)
    assert float(top[0]) == D.TOP < 1.0
    Sy, Sx = (H + 4) // 8, (W + 4) // 8
    assert int(np.float32(D.TOP) * np.float32(2 * Sy + 1)) == 2 * Sy              # the last bin, reached without the clamp ...
    assert D.decode(top, D.GEOMETRY, H, W)[1][:2] == (Sy, Sx)
    one = np.ones(8, dtype=np.float32)
    assert int(one[3] * np.float32(2 * Sy + 1)) == 2 * Sy + 1                      # ... which is for a u of exactly 1
    assert D.decode(one, D.GEOMETRY, H, W)[1] == (Sy, Sx, 13, 17, 10, 13)
    assert D.decode(np.zeros(8, dtype=np.float32), D.GEOMETRY, H, W)[1][:2] == (-Sy, -Sx)
    # box: ch = 8 rows (even: centres 0..17), cw = 6 columns
    assert D.box(0.0, 17) == (0, 4) and D.box(D.TOP, 17) == (13, 17) and D.box(0.0, 13) == (0, 3) and D.box(D.TOP, 13) == (10, 13)
    assert D.box(0.5, 1) == (0, 0) or D.box(0.5, 1)[0] == D.box(0.5, 1)[1]       # H = 1: no box


@pytest.mark.parametrize("shape", D.SHAPES + D.POW2_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_the_forced_table_zeroes_some_destinations_and_moves_some_pixels(shape):
    _, H, W = shape
    rows = D.forced_rows(H, W)
    names = [n for n, _ in rows]
    assert "identity" in names and "t=(+S,+S)" in names and "clamp" in names and sum(n.startswith("box") for n in names) >= 4
    idx = torch.arange(H * W, dtype=torch.float32).reshape(1, 1, H, W).repeat(1, 3, 1, 1) + 1.0      # every pixel its own value
    parse = torch.zeros(1, H, W, 8)
    plain = torch.cat((parse[..., :7], idx.permute(0, 2, 3, 1), torch.zeros(1, H, W, 2)), dim=3).double()
    for name, r in rows:
        V = D.valid_map(r, D.GEOMETRY, H, W)
        share = 1.0 - V.double().mean().item()
        assert 0.0 < share < 1.0, (name, share)
        ty, tx = D.decode(r, D.GEOMETRY, H, W)[1][:2]
        out = D.forward_ref(parse, 7, idx, torch.from_numpy(r)[None], D.GEOMETRY)
        if name.startswith("t="):
            assert (ty, tx) != (0, 0), name
            moved = V & (out[0, :, :, 7] != plain[0, :, :, 7])
            assert int(moved.sum()) >= 1 and int(moved.sum()) == int(V.sum()), name      # every surviving pixel comes from elsewhere
        if name == "identity":
            assert (ty, tx) == (0, 0) and torch.equal(out[0][V], plain[0][V])
        assert torch.equal(out[0][~V], torch.zeros_like(out[0][~V]))


@pytest.mark.parametrize("flags", [D.GEOMETRY, D.COLOR, D.ALL, D.TRANSLATION | D.COLOR])
def test_backward_ref_is_autograd_of_forward_ref(flags):
    N, H, W = 2, 17, 13
    parse, fake, _ = D.gauss_inputs(N, H, W, 7)
    gen = torch.Generator().manual_seed(3)
    for names, u in D.batches(D.forced_rows(H, W, seed=5), N)[::3]:
        u = u.clone()
        u[:, :3] = torch.rand(N, 3, generator=gen)          # a color transform that is not the identity
        x = fake.double().requires_grad_()
        out = D.forward_ref(parse, 7, x, u, flags)
        g = torch.randn(N, H, W, 12, generator=gen)
        (out * g.double()).sum().backward()
        want = D.backward_ref(g, 7, u, flags)
        scale = float(want.abs().max())
        assert scale > 0 and float((x.grad - want).abs().max()) <= 1e-13 * scale, names
        assert float((D.gsum_ref(g, 7, u, flags) - torch.stack([(o[..., 7:10] != 0).double().mul(gg[..., 7:10].double()).sum()
                                                                 for o, gg in zip(out.detach(), g)])).abs().max()) <= 1e-9


def test_forward_ref_selects_and_rounds_as_stated():
    N, H, W = 2, 16, 32
    parse, _, _ = D.gauss_inputs(N, H, W, 11)
    img = D.int_image(N, H, W, 12)
    M = D.mean_ref(img)
    assert torch.equal(M * 4, (M * 4).round()) and torch.equal(M.double(), img.double().mean(dim=(1, 2, 3)))
    u = torch.tensor([[0.75, 0.5, 0.0, 0.0, 0.5, 0.5, 0.0, 0.0], [0.0, 0.5, 0.5, 0.5, D.TOP, D.TOP, 0.5, 0.0]])
    out = D.forward_ref(parse, 7, img, u, D.ALL, mean=M)
    assert torch.equal(out.float().double(), out)            # exact in fp32: integers, s = 1, k and beta powers of two
    assert float(D.forward_bound(7, img, u, D.GEOMETRY, M).max()) == 0.0
    # a NaN behind a masked destination does not show
    V = D.valid_map(u[0].numpy(), D.GEOMETRY, H, W)
    bad = img.clone()
    ty, tx = D.decode(u[0].numpy(), D.GEOMETRY, H, W)[1][:2]
    ys, xs = torch.nonzero(~V, as_tuple=True)
    sy, sx = ys + ty, xs + tx
    ok = (sy >= 0) & (sy < H) & (sx >= 0) & (sx < W)
    used = torch.zeros(H, W, dtype=torch.bool)
    vy, vx = torch.nonzero(V, as_tuple=True)
    used[vy + ty, vx + tx] = True
    hide = torch.zeros(H, W, dtype=torch.bool)
    hide[sy[ok], sx[ok]] = True
    hide &= ~used
    assert int(hide.sum()) > 0
    bad[0, :, hide] = float("nan")
    assert torch.equal(D.forward_ref(parse, 7, bad, u, D.GEOMETRY)[0], D.forward_ref(parse, 7, img, u, D.GEOMETRY)[0])


def test_policy_parsing():
    import hr_viton_amd  # noqa: F401
    from hr_viton_amd import _lib, ops
    from hr_viton_amd.diffaug import DiffAugment, parse_policy
    assert (_lib.DIFFAUG_COLOR, _lib.DIFFAUG_TRANSLATION, _lib.DIFFAUG_CUTOUT) == (D.COLOR, D.TRANSLATION, D.CUTOUT)
    assert _lib.DIFFAUG_SLOTS == D.SLOTS
    assert parse_policy("color,translation,cutout") == D.ALL == parse_policy(" cutout , color,translation,")
    assert parse_policy("translation") == D.TRANSLATION and parse_policy("cutout,translation") == D.GEOMETRY
    assert parse_policy("") == 0 and parse_policy(None) == 0 and parse_policy(5) == 5
    for bad in ("flip", "color,rotation", "Color", "color translation", 8, -1, 1.5):
        with pytest.raises(ops.HrvError):
            parse_policy(bad)
    aug = DiffAugment("cutout,color")
    assert aug.flags == D.COLOR | D.CUTOUT and aug.names == ["color", "cutout"] and aug.color and "color,cutout" in repr(aug)
    u = aug.draw(3, "cpu")
    assert tuple(u.shape) == (3, 8) and u.dtype == torch.float32 and bool((u >= 0).all()) and bool((u < 1).all())


def test_symbols_constants_and_the_script_flag():
    import hr_viton_amd  # noqa: F401
    import train_generator as tg
    from hr_viton_amd import _lib
    from hr_viton_amd.diffaug import diffaug_from_opt
    with open(os.path.join(ROOT, "include", "hrviton_hip.h"), encoding="utf-8") as f:
        hdr = f.read()
    declared = set(re.findall(r"\b(hrv_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SYMBOLS, name
    assert re.search(r"#define\s+HRV_DIFFAUG_SLOTS\s+%d\b" % _lib.DIFFAUG_SLOTS, hdr)
    assert re.search(r"HRV_DIFFAUG_COLOR = 1, HRV_DIFFAUG_TRANSLATION = 2, HRV_DIFFAUG_CUTOUT = 4", hdr)
    opt = tg.get_opt(["--name", "t", "--synthetic"])
    assert not hasattr(opt, "diffaug") and diffaug_from_opt(opt) is None        # the option line of a plain run is the one it was
    opt = tg.get_opt(["--name", "t", "--synthetic", "--diffaug", "color,cutout"])
    assert diffaug_from_opt(opt).flags == D.COLOR | D.CUTOUT
    assert diffaug_from_opt(tg.get_opt(["--name", "t", "--synthetic", "--diffaug", ""])) is None
    with pytest.raises(_lib.HrvError):
        diffaug_from_opt(tg.get_opt(["--name", "t", "--synthetic", "--diffaug", "flip"]))


def test_the_step_rejects_augmentation_outside_the_pair_form():
    from argparse import Namespace
    import hr_viton_amd  # noqa: F401
    from hr_viton_amd import ops, pipeline
    from hr_viton_amd.diffaug import DiffAugment

    class NoPair:
        pass
    with pytest.raises(ops.HrvError, match="pair form"):
        pipeline.generator_train_step(Namespace(), None, NoPair(), None, None, None, None, None, None, None, None, aug=DiffAugment("color"))
    with pytest.raises(ops.HrvError, match="aug_u without aug"):
        pipeline.generator_train_step(Namespace(), None, NoPair(), None, None, None, None, None, None, None, None, aug_u=(None, None))
