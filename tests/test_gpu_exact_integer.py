"""Bit-exact integer-operand tests of the bf16 matrix-core kernels: conv_p2, spade_gb, spade_fused, conv_s2, the weight-gradient
family, the bf16 tiles of the generic engine, thin_conv and conv_cout1 against float64 CPU references with torch.equal
(tests/exact_cases.py: why small integers make every summation order exact, the 2^20 bound, the tie / magnitude conditions that
tests/test_exact_cases_cpu.py proves for every case table below).  bf16-stored outputs are compared with the float64 result
rounded to nearest-even on the bit pattern, so a truncating store fails on every exact tie.

A kernel rewrite (a new main loop, another chunking, split-K) changes the accumulation order on purpose; it is accepted against
this file first: nothing here depends on the order.

The probe of the exactness assumption -- that the MFMA accumulation loses nothing on integer addends whose running sum stays far
below 2^24 -- is ``test_generic_tile_probe`` (conv_mfma_kernel, the tile conv_dispatch picks, 80 -> 64 channels, 2 x 33 x 47, fp32
out).  PROBE OUTCOME on the MI355X: bit-exact -- every one of the 2 x 33 x 47 x 64 outputs equals the float64 reference, and so
does every other comparison of this file (split-K partial sums and their reduce included), so the assumption holds for the rest."""
import pytest

import exact_cases as E
import exact_runners as R

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------------
# generic engine, bf16 tiles
# ---------------------------------------------------------------------------------------------------------------
def test_generic_tile_probe():
    """The probe of the module docstring: the plain generic bf16 tile at its default configuration."""
    R.run_engine_probe(E.ENGINE[0])


_ENGINE_RUNS = [(c, s) for c in E.ENGINE[1:] for s in (E.ENGINE_SPLITK if c[1] not in (17, 18) else (0,))]


@pytest.mark.parametrize("case,splitk", _ENGINE_RUNS, ids=[f"{c[0]}-splitk{s}" for c, s in _ENGINE_RUNS])
def test_generic_engine_bf16_tiles(case, splitk, monkeypatch):
    """Tiles 8-15 (gather) and 17 / 18 (LDS-resident patch) with split-K off / 2 / 5 (HRV_CONV_SPLITK; the patch tiles never split:
    they run once), bias, bf16 / fp32 residual and output, LeakyReLU 0.5, wscale and a device sigma as powers of two."""
    R.run_engine_splitk(case, splitk, monkeypatch)


# ---------------------------------------------------------------------------------------------------------------
# conv_p2.hip
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", E.P2_FWD, ids=E.case_id)
def test_conv_p2_forward(case):
    R.run_p2_fwd(case)


@pytest.mark.parametrize("case", E.P2_DGRAD, ids=E.case_id)
def test_conv_p2_data_gradient(case):
    """Mode 1: conv^T(dY) [+ g] [* act'(x)] [+ g behind the mask: conv_dgrad's add_after]."""
    R.run_p2_dgrad(case)


@pytest.mark.parametrize("case", E.P2_PAIR, ids=E.case_id)
def test_conv_p2_pair_data_gradient(case):
    R.run_p2_pair(case)


@pytest.mark.parametrize("case", E.P2_IMAGE, ids=E.case_id)
def test_conv_p2_three_channel_image_ends(case):
    R.run_p2_image(case)


# ---------------------------------------------------------------------------------------------------------------
# spade_gb.hip
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", E.GB_FWD, ids=E.case_id)
def test_spade_gb_forward(case):
    R.run_gb_fwd(case)


@pytest.mark.parametrize("case", E.GB_DGRAD, ids=E.case_id)
def test_spade_gb_data_gradient(case):
    R.run_gb_dgrad(case)


# ---------------------------------------------------------------------------------------------------------------
# spade_fused.hip
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", E.FUSED, ids=E.case_id)
def test_spade_fused_forward(case):
    R.run_fused(case)


# ---------------------------------------------------------------------------------------------------------------
# conv_s2.hip
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", E.S2_FWD, ids=E.case_id)
def test_conv_s2_forward(case):
    R.run_s2_fwd(case)


@pytest.mark.parametrize("case", E.S2_DGRAD, ids=E.case_id)
def test_conv_s2_data_gradient(case):
    """(conv^T(dY) [+ tap]) [* lrelu'(x)] with slope 0.5."""
    R.run_s2_dgrad(case)


@pytest.mark.parametrize("case", E.S2_CELLS, ids=E.case_id)
def test_conv_s2_cells_form(case):
    """The 2x2 form over the space-to-depth image, also with [hi | lo | hi] operands (split3): integers leave lo = 0, the three
    products must still sum to the exact result."""
    R.run_s2_cells(case)


@pytest.mark.parametrize("case", E.S2_SPLIT3_FWD, ids=E.case_id)
def test_conv_s2_split3_forward(case):
    R.run_s2_split3_fwd(case)


# ---------------------------------------------------------------------------------------------------------------
# weight gradients
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", E.WGRAD, ids=[c[0] for c in E.WGRAD])
def test_weight_gradient(case):
    """conv_wgrad_tr classes 0-8, wgrad_s2, the conv_wgrad_bf16 fallback at 528 source channels and the fp32 kernel, with the fused
    bias gradient, accumulate=True and channel slices; the launch record names the kernel the plan picked."""
    R.run_wgrad(case)


# ---------------------------------------------------------------------------------------------------------------
# thin_conv.hip, conv_cout1.hip
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", E.THIN, ids=E.case_id)
def test_thin_conv_forward_and_data_gradient(case, monkeypatch):
    R.run_thin(case, monkeypatch)


@pytest.mark.parametrize("case", E.COUT1, ids=E.case_id)
def test_conv_cout1_forward_and_data_gradient(case):
    R.run_cout1(case)
