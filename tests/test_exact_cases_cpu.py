"""tests/exact_cases.py on the CPU alone: the rounding helper is torch's own round-to-nearest-even bit for bit, the integer operands
are order-independent in fp32, and every case table of tests/test_gpu_exact_integer.py meets the conditions its zero-tolerance
comparison rests on -- the 2^20 bound, and for bf16-stored outputs enough exact ties and enough values at or above 256."""
import pytest
import torch
import torch.nn.functional as F

import exact_cases as E


def _bits(t):
    return t.view(torch.int16)


def test_to_bf16_rne_equals_torch_rounding_bit_for_bit():
    ints = torch.arange(-2100, 2101, dtype=torch.float64)                       # ties: odd in [256, 512), 2 mod 4 in [512, 1024), ...
    quarters = torch.arange(-1200, 1201, dtype=torch.float64) * 0.25           # values below 256, halves and quarters
    near = torch.tensor([257.0, 259.0, -257.0, -259.0, 255.0, 256.0, 258.0, 511.0, 513.0, 514.0, 1026.0, 1030.0, 65537.0 * 4,
                         0.0, -0.0, 1.0, -1.0, 0.5, 2.0 ** 20, 2.0 ** 20 - 1, -(2.0 ** 20 - 3)], dtype=torch.float64)
    sweep = torch.cat([ints, quarters, near, ints * 257.0])
    got = E.to_bf16_rne(sweep)
    want = sweep.float().to(torch.bfloat16)
    assert got.dtype == torch.bfloat16 and torch.equal(_bits(got), _bits(want))
    # the sweep holds what it is meant to hold: ties of both signs that round to even in both directions, and both zeros
    assert E.tie_share(sweep) > 0.05
    assert float(E.to_bf16_rne(torch.tensor([257.0], dtype=torch.float64))) == 256.0            # down to even
    assert float(E.to_bf16_rne(torch.tensor([259.0], dtype=torch.float64))) == 260.0            # up to even
    assert float(E.to_bf16_rne(torch.tensor([-259.0], dtype=torch.float64))) == -260.0
    z = _bits(E.to_bf16_rne(torch.tensor([0.0, -0.0], dtype=torch.float64)))
    assert z.tolist() == [0, -32768]
    with pytest.raises(AssertionError):
        E.to_bf16_rne(torch.tensor([1.0 + 2.0 ** -30], dtype=torch.float64))                    # not exact in fp32: refused


def test_tie_share_counts_exact_halves_only():
    t = torch.tensor([257.0, 258.0, 259.0, 256.5, 100.0, 101.0, 514.0, 516.0], dtype=torch.float64)
    assert E.tie_share(t) == 3 / 8                                                               # 257, 259, 514


def test_bound_refuses_a_case_beyond_2_to_20():
    assert E.bound(4608, 4, 4, 308) == 4608 * 16 + 308
    with pytest.raises(AssertionError):
        E.bound(4608, 16, 16)


@pytest.mark.parametrize("perm", [False, True], ids=["as_is", "channels_permuted"])
def test_fp32_convolution_of_the_operands_is_exact_in_any_order(perm):
    """fp32 F.conv2d / conv_transpose2d on the helper's operands equal the float64 reference exactly, also with the channels (the
    summation order) permuted: the operands are order-independent."""
    g = torch.Generator().manual_seed(3)
    m = E.pick_m(9 * 80)
    x, w = E.int_tensor((2, 33, 47, 80), -m, m, g), E.int_tensor((64, 80, 3, 3), -m, m, g)
    b = E.BIAS0 + E.int_tensor((64,), -8, 8, g)
    E.bound(9 * 80, m, m, E.BIAS0 + 8)
    p = torch.randperm(80, generator=g) if perm else torch.arange(80)
    ref = E.ref_conv64(x, w, b, act="lrelu", slope=0.5)
    got = F.leaky_relu(F.conv2d(x[..., p].permute(0, 3, 1, 2), w[:, p], b, padding=1), 0.5).permute(0, 2, 3, 1)
    assert torch.equal(got.double(), ref)
    dy = E.int_tensor((2, 33, 47, 64), -m, m, g)
    p = torch.randperm(64, generator=g) if perm else torch.arange(64)
    refd = E.ref_conv_transpose64(dy, w)
    gotd = F.conv_transpose2d(dy[..., p].permute(0, 3, 1, 2), w[p], padding=1).permute(0, 2, 3, 1)
    assert torch.equal(gotd.double(), refd)
    assert torch.equal(x.to(torch.bfloat16).float(), x) and torch.equal(w.to(torch.bfloat16).float(), w)      # exact in bf16


ALL = [(fam, case) for fam, (table, _) in E.TABLES.items() for case in table]


@pytest.mark.parametrize("fam,case", ALL, ids=[f"{f}:{E.case_id(c)}" for f, c in ALL])
def test_case_meets_the_conditions_of_an_exact_comparison(fam, case):
    d = E.TABLES[fam][1](case)
    assert d["bound"] <= E.LIMIT
    for name, ref in d["want"].items():
        assert ref.dtype == torch.float64 and float(ref.abs().max()) <= d["bound"], (name, float(ref.abs().max()), d["bound"])
        if d["bf16"][name] and d.get("rounds", {}).get(name, True):
            ties, big = E.tie_share(ref), E.big_share(ref)
            assert ties >= 0.01, (name, ties)
            assert big >= 0.10, (name, big)
    for k in ("x", "xall", "xs", "img", "seg", "actv_all", "dy", "dgb", "mask", "xin", "w", "w2", "wd", "wg", "wb", "wsh"):
        v = d.get(k)                # every matrix-core operand is an integer that bf16 holds (biases and fp32 addends need not be)
        if v is not None:
            assert torch.equal(v.to(torch.bfloat16).float(), v) and torch.equal(v.round(), v), k


@pytest.mark.parametrize("fam", sorted(E.WRAP))
def test_every_persistent_family_has_a_case_that_wraps_on_256_cus(fam):
    """More tiles than the resident blocks of an MI355X (256 CUs; two blocks per CU, spade_gb one): below that count conv_p2, conv_s2
    and spade_fused give each block one (tile, pass) unit and the persistent loop runs once.  (The GPU test asserts the same against
    the device's own hrv_persistent_cus().)"""
    case = E.WRAP[fam][0]
    assert case in E.TABLES[fam][0]
    assert E.wrap_tiles(fam) > (256 if fam.startswith("gb_") else 512)
