"""tests/guard_cases.py on the CPU alone: the float64 restatement of the guarded Adam step is torch's clip_grad_norm_ followed by
torch.optim.Adam, the case tables meet the conditions the exact GPU comparisons (tests/test_gpu_grad_guard.py) rest on, and the
constants mirror the library's."""
import math
import os
import re

import numpy as np
import pytest
import torch

import guard_cases as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_constants_mirror_the_library():
    import hr_viton_amd  # noqa: F401
    from hr_viton_amd import _lib
    from hr_viton_amd import train_ops as T
    lib = _lib.load()
    assert lib.hrv_grad_guard_slots() == G.P
    with open(os.path.join(ROOT, "hr-viton_amd", "csrc", "grad_guard.hip"), encoding="utf-8") as f:
        src = f.read()
    assert int(re.search(r"constexpr int GUARD_SLOTS = (\d+);", src).group(1)) == G.P
    assert int(re.search(r"constexpr int GUARD_BLOCK = (\d+);", src).group(1)) == G.BLOCK
    with open(os.path.join(ROOT, "include", "hrviton_hip.h"), encoding="utf-8") as f:
        hdr = f.read()
    for name in ("NORM", "SCALE", "APPLY", "NONFINITE", "STEPS", "SKIPPED", "CLIPPED", "SUMSQ", "WORDS"):
        assert int(re.search(r"#define HRV_GUARD_%s (\d+)" % name, hdr).group(1)) == getattr(T, "GUARD_" + name), name
    assert T.GUARD_SUMSQ % 2 == 0 and T.GUARD_SUMSQ + 2 <= T.GUARD_WORDS      # the double is 8-byte aligned inside the record


def test_the_sizes_reach_the_edges_they_are_there_for():
    assert G.PASS == G.P * 1024 and G.SIZES[-4:] == [G.PASS - 1, G.PASS, G.PASS + 1, 2 * G.PASS + 7]
    assert {1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025} <= set(G.SIZES)
    assert max(G.SIZES) * 4 <= 8.5 * 2 ** 20                                  # "about 8 MB"
    for n in G.SIZES:
        for shift in (0, 1):
            pos = G.block_edge_positions(n, shift)
            assert pos[0] == 0 and pos[-1] == n - 1 and all(0 <= p < n for p in pos)
    # an unaligned view of 1030 elements: head 3, body 1024 (one block's trip exactly), tail 3
    assert G.block_edge_positions(1030, 1) == [0, 1026, 1027, 1029]
    assert G.block_edge_positions(1025, 0) == [0, 1023, 1024]                 # aligned: block 0's last element, then the tail


def test_banded_views_are_aligned_as_they_claim():
    for shift in (0, 1):
        buf, (o, n) = G.banded(torch.ones(5), shift)
        assert buf.data_ptr() % 16 == 0 and (buf.data_ptr() + 4 * o) % 16 == 4 * shift
        assert G.sumsq_ref(buf[o:o + n]) == (5.0, 0) and G.sumsq_ref(buf)[1] == 2 * G.BAND + shift


@pytest.mark.parametrize("n", G.SIZES)
def test_integer_gradients_sum_exactly_in_any_order(n):
    g = G.int_grads(n, n)
    assert set(g.unique().tolist()) <= {-2.0, -1.0, 0.0, 1.0, 2.0}
    ss, nf = G.sumsq_ref(g)
    assert nf == 0 and ss == float(int(ss)) and ss < 2 ** 24
    assert float((g * g).sum()) == ss and float((g.flip(0) * g.flip(0)).cumsum(0)[-1]) == ss      # fp32, two orders


def test_nonfinite_count_is_the_exponent_field():
    t = torch.tensor([0.0, -0.0, 1e-45, 3.4e38, float("inf"), float("-inf"), float("nan"), -float("nan")])
    assert G.sumsq_ref(t)[1] == 4


def test_finalize_ref_is_the_contract():
    r = G.finalize_ref(4096.0, 0, 1.0, 16.0)
    assert r == {"norm": 64.0, "scale": 0.25, "apply": 1}
    assert G.finalize_ref(4096.0, 0, 0.5, 64.0)["scale"] == 1.0 and G.finalize_ref(4096.0, 0, 0.5, 8.0)["scale"] == 0.25
    assert G.finalize_ref(4096.0, 0)["scale"] == 1.0
    # 1e30 in a small buffer: finite norm (fp32 squares would overflow); two elements of 3e38: the norm overflows fp32
    ss, nf = G.sumsq_ref(torch.tensor([1e30, 1.0, -2.0]))
    r = G.finalize_ref(ss, nf, skip_nonfinite=True)
    assert nf == 0 and r["apply"] == 1 and r["norm"] == float(np.float32(1e30))
    assert not math.isfinite(float((torch.tensor([1e30]) ** 2).sum()))
    ss, nf = G.sumsq_ref(torch.tensor([3e38, 3e38]))
    r = G.finalize_ref(ss, nf, skip_nonfinite=True)
    assert nf == 0 and math.isfinite(ss) and math.isinf(r["norm"]) and r["apply"] == 0
    assert G.finalize_ref(ss, nf, skip_nonfinite=False)["apply"] == 1
    # torch's behaviour with clipping on and skipping off: a NaN norm gives a NaN scale, an Inf norm a zero scale
    assert math.isnan(G.finalize_ref(float("nan"), 1, 1.0, 1.0)["scale"]) and G.finalize_ref(float("inf"), 1, 1.0, 1.0)["scale"] == 0.0


def test_square_gradients_meet_the_conditions_of_the_exact_comparison():
    for step in range(3):
        gr = G.square_grads(step)
        flat = torch.cat([g.reshape(-1) for g in gr])
        assert G.sumsq_ref(flat) == (G.SQUARE_NORM ** 2, 0) and [tuple(g.shape) for g in gr] == G.SHAPES
        for gscale in (1.0, 0.5):
            norm = np.float32(gscale * G.SQUARE_NORM)
            assert norm >= 32 and norm + np.float32(1e-6) == norm
            for k in (1, 3):
                assert G.finalize_ref(4096.0, 0, gscale, float(norm) / 2 ** k)["scale"] == 2.0 ** -k
    assert not torch.equal(G.square_grads(0)[0], G.square_grads(1)[0])
    assert any(math.prod(s) % 4 for s in G.SHAPES)


# ---------------------------------------------------------------------------------------------------------------
# the reference is shown right before it judges anything
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_norm", [None, 1.0, 5.0, 1e6])
def test_the_restatement_is_torch_clip_grad_norm_then_adam(max_norm):
    w0 = G.start_weights()
    steps = [G.gauss_grad_list(s) for s in range(3)]
    ref = G.adam_ref64(w0, steps, max_norm=max_norm)
    t64 = G.torch_clip_adam(w0, steps, max_norm, dtype=torch.float64)
    t32 = G.torch_clip_adam(w0, steps, max_norm)
    for s in range(3):
        # torch in float64 differs from the restatement only by the fp32 rounding of norm and scale (2^-24 relative each on a
        # gradient; Adam's update is scale-invariant up to eps) and by float64 rounding
        assert G.rel_err(t64[s], ref[s]["w"]) < 1e-7, (s, G.rel_err(t64[s], ref[s]["w"]))
        assert G.rel_err(t32[s], ref[s]["w"]) < 1e-6, (s, G.rel_err(t32[s], ref[s]["w"]))
    clipped = max_norm is not None and max_norm < 30                    # the norm of 1192 standard normals is about 34.5
    assert ref[-1]["rec"]["clipped"] == (3 if clipped else 0) and ref[-1]["step"] == 3
    if max_norm == 1.0:      # the clipped gradient's norm is max_norm
        flat = torch.cat([g.reshape(-1) for g in steps[0]]).double() * ref[0]["rec"]["scale"]
        assert abs(float(flat.norm()) - 1.0) < 1e-6


def test_a_skipped_step_is_no_step():
    w0 = G.start_weights()
    a, b, c = G.gauss_grad_list(0), G.poison(G.gauss_grad_list(1)), G.gauss_grad_list(2)
    three = G.adam_ref64(w0, [a, b, c], max_norm=5.0, skip_nonfinite=True)
    two = G.adam_ref64(w0, [a, c], max_norm=5.0, skip_nonfinite=True)
    assert three[1]["rec"]["apply"] == 0 and three[1]["rec"]["nonfinite"] == 1 and three[1]["step"] == 1
    for k in ("w", "m", "v"):
        assert all(torch.equal(x, y) for x, y in zip(three[0][k], three[1][k]))
        assert all(torch.equal(x, y) for x, y in zip(three[2][k], two[1][k]))
    assert three[2]["step"] == 2 and (three[2]["rec"]["steps"], three[2]["rec"]["skipped"]) == (3, 1)
    # without the skip the NaN spreads, as it does in torch
    bad = G.adam_ref64(w0, [a, b], max_norm=5.0)
    t32 = G.torch_clip_adam(w0, [a, b], 5.0)
    assert all(bool(torch.isnan(x).all()) for x in bad[1]["w"]) and all(bool(torch.isnan(x).all()) for x in t32[1])


def test_the_scripts_take_the_flags_and_print_the_old_options_without_them():
    import train_condition as tc
    import train_generator as tg
    from hr_viton_amd.optim import guard_kwargs
    for mod, argv in ((tc, []), (tg, ["--name", "x"])):
        o = mod.get_opt(argv)
        assert not any(k.startswith("max_grad_norm") or k == "skip_nonfinite" for k in vars(o))
        assert guard_kwargs(o, "G") == {} and guard_kwargs(o, "D") == {}
        o = mod.get_opt(argv + ["--max_grad_norm_G", "1.5", "--skip_nonfinite"])
        assert guard_kwargs(o, "G") == {"max_grad_norm": 1.5, "skip_nonfinite": True, "device_step": True}
        assert guard_kwargs(o, "D") == {"skip_nonfinite": True, "device_step": True}
        o = mod.get_opt(argv + ["--max_grad_norm_D", "2", "--max_grad_norm_G", "0"])
        assert guard_kwargs(o, "G") == {} and guard_kwargs(o, "D") == {"max_grad_norm": 2.0}
