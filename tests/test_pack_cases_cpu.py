"""What tests/test_gpu_pack_exact.py rests on, proved without a GPU: the layout reference of tests/pack_cases.py equals the host packers
bit for bit, its geometry is the one hrv_conv2d_pack_weight_record returns (a host-only function: it runs on CPU tensor pointers), its
matrices ARE the convolutions they stand for (integer weights, float64 F.conv2d / F.conv_transpose2d, np.array_equal), the pair forms
equal the packs of the explicitly combined weights, the tables reach every path of the batched kernel and every edge they claim, and
the comparison rejects each seeded defect on every case the defect applies to."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pack_cases as P

IDS = dict(ids=lambda c: c.name)


@pytest.fixture(scope="module")
def lib():
    import hr_viton_amd  # noqa: F401
    from hr_viton_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from hr_viton_amd import build
        build.build(verbose=False)
    return _lib.load()


def _values(bits):
    """bit patterns -> the numbers they stand for (float32)"""
    bits = np.asarray(bits)
    return (bits.astype(np.uint32) << 16).view(np.float32) if bits.dtype == np.uint16 else bits.view(np.float32)


def test_tables_are_the_ones_the_issue_lists():
    assert [len(P.TABLES[k]) for k in ("forward", "mode1", "mode2", "pairs", "scale")] == [42, 42, 48, 12, 12]
    assert sorted(len(v) for v in P.LAUNCH_TABLES.values()) == sorted([42 + 6 + 6, 42 + 48 + 6 + 6])
    assert max(P.upper_bound_elems(c) for c in P.ALL) == 9 * 4 * 256 * 64        # [96,16,4] on the 256-column tile: 1.2 MB of bf16
    assert any(len(c.src_real) == P.MAX_SRC for c in P.FORWARD)


def test_tile_tables_are_the_librarys(lib):
    assert lib.hrv_conv2d_tile_bn(len(P.TILE_BN)) == -1
    for cfg in range(len(P.TILE_BN)):
        assert (lib.hrv_conv2d_tile_bn(cfg), lib.hrv_conv2d_tile_row_bytes(cfg)) == (P.TILE_BN[cfg], P.TILE_RB[cfg]), cfg


@pytest.mark.parametrize("c", [c for c in P.ALL if c.mode == 0 and c.pair_mode == 0], **IDS)
def test_forward_reference_equals_the_host_packer(lib, c):
    """raw bits; the host packers take no scale, so the scale cases are held to them at mul = 1"""
    w, _ = P.case_weights(c)
    r = P.case_pack(c, wscale=1.0, sigma=None)
    wt = torch.from_numpy(w.copy())
    n = len(c.src_pad)
    srcC, srcR = (C.c_int32 * n)(*c.src_pad), (C.c_int32 * n)(*c.src_real)
    if c.bf16:
        assert lib.hrv_conv2d_packed_elems_bf16(c.cout, c.k, c.k, n, srcC, c.cfg) == r["geom"][7]
        host = torch.full((r["geom"][7],), 0x7FC1, dtype=torch.int16)
        assert lib.hrv_conv2d_pack_weight_bf16(wt.data_ptr(), c.cout, c.k, c.k, n, srcC, srcR, c.cfg, host.data_ptr()) == 0
        assert P.same_bits(host.numpy().view(np.uint16), r["bits"])
    else:
        assert lib.hrv_conv2d_packed_elems(c.cout, c.k, c.k, n, srcC, c.cfg) == r["geom"][7]
        host = torch.full((r["geom"][7],), float("nan"))
        assert lib.hrv_conv2d_pack_weight_f32(wt.data_ptr(), c.cout, c.k, c.k, n, srcC, srcR, c.cfg, host.data_ptr()) == 0
        assert P.same_bits(host.numpy().view(np.uint32), r["bits"])


@pytest.mark.parametrize("c", P.ALL, **IDS)
def test_geometry_equals_the_record_functions(lib, c):
    w, w2 = (None if a is None else torch.from_numpy(a.copy()) for a in P.case_weights(c))
    n = len(c.src_pad)
    out = torch.zeros(16)
    rec = C.create_string_buffer(lib.hrv_conv2d_pack_record_bytes())
    geom, blocks = (C.c_int32 * 8)(), C.c_int32(-1)
    rc = lib.hrv_conv2d_pack_weight_record(w.data_ptr(), P.virtual_cout(c), c.k, c.k, n, (C.c_int32 * n)(*c.src_pad),
                                           (C.c_int32 * n)(*c.src_real), c.cfg, c.mode, c.stride, c.pad, c.phase[0], c.phase[1],
                                           c.wscale, None, 1 if c.bf16 else 0, None if w2 is None else w2.data_ptr(), c.pair_mode,
                                           c.cout if c.pair_mode else 0, out.data_ptr(), geom, rec, C.byref(blocks))
    assert rc == 0, lib.hrv_last_error()
    want = P.case_ref(c.name)[1]
    assert tuple(geom) == want
    assert blocks.value == P.blocks_of(c)
    # the wrappers' bound: reached unless a stride-2 phase keeps fewer taps than the kernel has
    assert want[7] <= P.upper_bound_elems(c) and (want[7] == P.upper_bound_elems(c)) == (c.mode != 2 or c.k == 1)
    assert len(P.case_ref(c.name)[0]) == want[7]


# ---------------------------------------------------------------------------------------------------------------
# the packed matrices are the convolutions they stand for
# ---------------------------------------------------------------------------------------------------------------
H, W, N = 5, 6, 2


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).double()


@pytest.mark.parametrize("c", P.ALL, **IDS)
def test_integer_packs_reproduce_float64_convolutions(c):
    w, w2 = P.case_int_weights(c)
    r = P.case_pack(c, w, w2, wscale=1.0, sigma=None)
    g = P.case_geometry(c)
    assert P.same_bits(_values(r["bits"]).view(np.uint32), r["raw32"]), "small integers survive the rounding to bf16"
    rs = np.random.RandomState(len(c.name))
    k, p = c.k, c.pad
    if c.mode == 0:
        x = rs.randint(-4, 5, (N, H, W, sum(c.src_real))).astype(np.float64)
        X = np.zeros((N, H, W, g["chunks"] * g["bke"]))
        for s, rc in enumerate(c.src_real):                      # every source starts on a chunk of its own
            X[..., g["chunk0"][s] * g["bke"]:g["chunk0"][s] * g["bke"] + rc] = x[..., g["base"][s]:g["base"][s] + rc]
        Ho, Wo = H + 2 * p - k + 1, W + 2 * p - k + 1
        got = P.engine(_values(r["bits"]), g, X, Ho, Wo)
        xt = _t(x).permute(0, 3, 1, 2)
        if c.pair_mode == 0:
            want = F.conv2d(xt, _t(w), padding=p).permute(0, 2, 3, 1).numpy()
        else:                                                    # columns 64 g + l: gamma[32 g + l] | beta[32 g + l - 32]
            ya, yb = (F.conv2d(xt, _t(a), padding=p).permute(0, 2, 3, 1).numpy() for a in (w, w2))
            want = np.zeros(got.shape)
            for co in range(c.cout):
                want[..., co // 32 * 64 + co % 32] = ya[..., co]
                want[..., co // 32 * 64 + 32 + co % 32] = yb[..., co]
        assert np.array_equal(got, want)
        return
    st = c.stride
    Ho, Wo = (H + 2 * p - k) // st + 1, (W + 2 * p - k) // st + 1
    CoutV = g["CoutV"]
    dy = rs.randint(-4, 5, (N, Ho, Wo, CoutV)).astype(np.float64)
    D = np.zeros((N, Ho, Wo, g["chunks"] * g["bke"]))
    D[..., :CoutV] = dy
    dyt = _t(dy).permute(0, 3, 1, 2)
    op = (H - ((Ho - 1) * st - 2 * p + k), W - ((Wo - 1) * st - 2 * p + k))
    assert all(0 <= o < st for o in op)
    if c.pair_mode == 0:
        full = F.conv_transpose2d(dyt, _t(w), stride=st, padding=p, output_padding=op)
    else:                                                        # dY = [dgamma | dbeta]
        full = (F.conv_transpose2d(dyt[:, :c.cout], _t(w), padding=p) + F.conv_transpose2d(dyt[:, c.cout:], _t(w2), padding=p))
    assert full.shape[2:] == (H, W)
    a, b = c.phase if c.mode == 2 else (0, 0)
    want = full[:, :, a::st, b::st].permute(0, 2, 3, 1).numpy()
    got = P.engine(_values(r["bits"]), g, D, want.shape[1], want.shape[2])
    assert np.array_equal(got, want)
    assert c.mode == 2 or np.abs(want).max() > 0


def test_a_phase_without_a_tap_is_all_zero():
    dead = [c for c in P.MODE2 if not P.has_tap(c)]
    assert {(c.k, c.phase) for c in dead} == {(1, (0, 1)), (1, (1, 0)), (1, (1, 1))} and len(dead) == 9
    for c in dead:
        bits, geom = P.case_ref(c.name)
        assert geom[0] * geom[1] == 1 and geom[2:4] == (0, 0) if c.phase == (1, 1) else geom[0] * geom[1] == 1
        assert not bits.any() and P.filled_count(c) == 0


# ---------------------------------------------------------------------------------------------------------------
# pairs
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", P.PAIRS, **IDS)
def test_pair_packs_equal_the_packs_of_the_combined_weight(c):
    w, w2 = P.case_weights(c)
    bits, geom = P.case_ref(c.name)
    if c.pair_mode == 1:
        groups = (c.cout + 31) // 32
        cat = np.zeros((groups * 64,) + w.shape[1:], np.float32)             # +0.0 rows where a group is short
        for g in range(groups):
            n = min(32, c.cout - 32 * g)
            cat[64 * g:64 * g + n] = w[32 * g:32 * g + n]
            cat[64 * g + 32:64 * g + 32 + n] = w2[32 * g:32 * g + n]
    else:
        cat = np.concatenate([w, w2])
    other, ogeom = P.ref_pack(cat, c.src_pad, c.src_real, c.cfg, c.mode, c.stride, c.pad, c.phase, 1.0, None, c.bf16)
    assert ogeom == geom and P.same_bits(other, bits)


def test_the_pair_edges_are_there():
    c = P.BY_NAME["pair2-re48-ci32-k3p1-bf16c9"]
    g = P.case_geometry(c)
    assert g["bke"] == 64 and g["CoutV"] == 96 and g["chunks"] == 2, "the [gamma | beta] split at 48 falls inside chunk 0"
    c = P.BY_NAME["pair1-re48-ci32-k3-bf16c9"]
    g = P.case_geometry(c)
    assert g["CoutV"] == 128 and int((~g["real"]).sum()) == 32 and not g["real"][64 + 16:64 + 32].any() and not g["real"][112:].any()
    assert [c.cout % 32 for c in P.PAIRS if c.pair_mode == 1].count(0) == 2


# ---------------------------------------------------------------------------------------------------------------
# coverage
# ---------------------------------------------------------------------------------------------------------------
def _paths(c, offset=0):
    return {n for blk in P.multi_path(c, offset) for n in blk}


def test_the_tables_reach_every_path_of_the_batched_kernel():
    for bf16 in (False, True):
        seen = set()
        for c in P.ALL:
            if c.bf16 == bf16:
                seen |= _paths(c)
        assert seen == {"lds", "col4", "col4_fast"}, (bf16, seen)
    for c in P.FORWARD:
        if c.src_real == (9,):                                   # odd CinTot: the alignment flips from row to row
            assert _paths(c) == {"col4", "col4_fast"}, c.name
            assert any(set(blk) == {"col4", "col4_fast"} for blk in P.multi_path(c)), "within one block"
    odd = [c for c in P.MODE1 if c.k == 3 and not c.bf16 and P.case_geometry(c)["rows_pad"] in (32, 96)]
    assert {P.case_geometry(c)["rows_pad"] for c in odd} == {32, 96}
    assert all(_paths(c) == {"col4"} for c in odd)
    assert all(_paths(c) == {"col4"} for c in P.ALL if c.k == 4), "4x4: neither the LDS transpose nor the float4 path"
    assert any(_paths(c) == {"lds"} for c in P.MODE2) and any(_paths(c) == {"col4"} for c in P.MODE2)
    assert any(_paths(c) == {"lds"} for c in P.PAIRS if not c.bf16) and any(_paths(c) == {"lds"} for c in P.PAIRS if c.bf16)


def test_a_shifted_weight_moves_the_float4_path():
    """+4 and +8 bytes: other 4-column groups are aligned, so the alignment test of the GPU file changes the path of some columns"""
    for c in P.FORWARD:
        if c.k == 3:
            at = [P.fast_groups(c, off).tolist() for off in (0, 4, 8)]
            if sum(c.src_real) % 4 == 0 and all(r % 4 == 0 for r in c.src_real):
                assert "col4_fast" in _paths(c, 0) and "col4_fast" not in _paths(c, 4) | _paths(c, 8), c.name
            else:
                assert any(at[0]) and any(at[1]) and any(at[2]) and at[0] != at[1] != at[2] != at[0], c.name
    assert any("col4_fast" in _paths(c, 4) for c in P.FORWARD) and any("col4_fast" in _paths(c, 8) for c in P.FORWARD)


def test_every_table_holds_a_record_of_one_block():
    for name in ("forward", "mode1", "mode2"):
        assert any(P.blocks_of(c) == 1 for c in P.TABLES[name]), name
    for name, cases in P.LAUNCH_TABLES.items():
        nb = [P.blocks_of(c) for c in P.shuffled(cases)]
        assert 1 in nb and max(nb) >= 16, name
        assert any(nb[i] == 1 and nb[i - 1] > 4 and nb[i + 1] > 4 for i in range(1, len(nb) - 1)), "a one-block record between large ones"
        assert len({c.bf16 for c in cases}) == 2
        big, one = P.two_records(name)
        assert P.blocks_of(big) > 4 and P.blocks_of(one) == 1 and big.bf16 and not one.bf16


@pytest.mark.parametrize("c", [c for c in P.ALL if c.bf16 and P.is_dyadic(c)], **IDS)
def test_bf16_cases_carry_the_ties(c):
    r = P.case_pack(c)
    raw = r["raw32"][r["filled"]]
    if not P.has_tap(c):                                          # nothing is filled: see test_a_phase_without_a_tap_is_all_zero
        assert raw.size == 0
        return
    assert raw.size == P.filled_count(c)
    tie = (raw & 0xFFFF) == 0x8000
    assert (tie & ((raw >> 16) & 1 == 0)).any() and (tie & ((raw >> 16) & 1 == 1)).any(), "a tie of each parity"
    assert (tie & (raw >> 31 == 1)).any() and (raw == P.NEG_ZERO).any()
    assert ((raw & 0xFFFF) == 0xFFFF).any() and (raw & 0x7F800000 != 0)[raw & 0x7FFFFFFF != 0].all(), "the carry; no denormal"
    got = r["bits"][r["filled"]]
    assert (got[raw == P.NEG_ZERO] == 0x8000).all()
    m = float(P.mul_of(c.wscale, c.sigma))
    for planted, want in ((P.TIE_EVEN, 0x3F80), (P.TIE_ODD, 0x3F82), (P.CARRY, 0x3F80)):
        prod = (np.array([planted], np.uint32).view(np.float32) * np.float32(m)).view(np.uint32)[0]
        scaled = (np.array([want << 16], np.uint32).view(np.float32) * np.float32(m)).view(np.uint32)[0] >> 16
        assert (got[raw == prod] == scaled).all() and (raw == prod).any()


def test_the_scale_table_has_both_kinds_of_multiplier():
    muls = {(c.wscale, c.sigma): P.mul_of(c.wscale, c.sigma) for c in P.SCALE}
    assert muls[(0.5, 4.0)] == np.float32(0.125) and muls[(0.7, None)] == np.float32(0.7)
    q = muls[(1.0, 1.7)]
    # the correctly rounded fp32 quotient, from the exact rational 1 / float32(1.7)
    from fractions import Fraction
    exact = Fraction(1) / Fraction(float(np.float32(1.7)))
    lo, hi = np.nextafter(q, np.float32(0)), np.nextafter(q, np.float32(2))
    assert abs(Fraction(float(q)) - exact) < min(abs(Fraction(float(lo)) - exact), abs(Fraction(float(hi)) - exact))
    assert all(P.is_dyadic(c) == (c.wscale == 0.5) for c in P.SCALE) and all(P.is_dyadic(c) for c in P.ALL if c.table != "scale")


# ---------------------------------------------------------------------------------------------------------------
# the comparison rejects seeded defects
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("defect", P.DEFECTS)
def test_the_comparison_rejects_the_defect_on_every_case_it_applies_to(defect):
    hit = [c for c in P.ALL if P.defect_applies(c, defect)]
    assert hit, defect
    for c in hit:
        bits, geom = P.case_ref(c.name)
        bad = P.case_pack(c, defect=defect)
        assert bad["geom"] == geom and not P.same_bits(bad["bits"], bits), (defect, c.name)
    assert all(P.same_bits(P.case_pack(c)["bits"], P.case_ref(c.name)[0]) for c in hit[:3])
    tables = {c.table for c in hit}
    want = dict(noflip={"mode1", "pairs", "scale"}, chunk0_real={"forward", "scale"}, cbase_padded={"forward"},
                interleave0={"pairs"}, split4={"pairs"}, truncate=set(P.TABLES), negzero_pad=set(P.TABLES),
                phase_reversed={"mode2"})[defect]
    assert tables == want, (defect, tables)


def test_same_bits_is_strict():
    bits, _ = P.case_ref(P.FORWARD[0].name)
    one = bits.copy()
    one[len(one) // 2] ^= 1
    assert P.same_bits(bits.copy(), bits) and not P.same_bits(one, bits) and not P.same_bits(bits[:-1], bits)
    assert not P.same_bits(bits.view(np.int32), bits)
    z = np.zeros(4, np.uint32)
    assert not P.same_bits(np.full(4, P.NEG_ZERO, np.uint32), z), "-0.0 is not +0.0"
