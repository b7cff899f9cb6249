"""tests/span_stats_cases.py on the CPU alone: train_ops.span_pieces keeps its contract, the float64 restatement of a span record is
torch.linalg.vector_norm / isfinite / == 0 per parameter, its update direction is the step of the float64 Adam of
tests/guard_cases.py, the integer cases are exact in any order of summation, and the constants mirror the library's."""
import math
import os
import re

import numpy as np
import pytest
import torch

import guard_cases as G
import span_stats_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _T():
    import hr_viton_amd  # noqa: F401
    from hr_viton_amd import train_ops
    return train_ops


def test_the_constants_mirror_the_library():
    from hr_viton_amd import _lib
    T = _T()
    assert _lib.load().hrv_span_stats_piece() == S.PIECE == T.span_stats_piece()
    with open(os.path.join(ROOT, "hr-viton_amd", "csrc", "span_stats.hip"), encoding="utf-8") as f:
        assert int(re.search(r"constexpr int SPAN_PIECE = (\d+);", f.read()).group(1)) == S.PIECE
    with open(os.path.join(ROOT, "include", "hrviton_hip.h"), encoding="utf-8") as f:
        hdr = f.read()
    names = ("G_SUMSQ", "W_SUMSQ", "U_SUMSQ", "G_MAXABS", "W_MAXABS", "U_MAXABS", "G_NONFINITE", "W_NONFINITE", "U_NONFINITE", "G_ZEROS",
             "WORDS")
    for name in names:
        assert int(re.search(r"#define HRV_SPAN_%s (\d+)" % name, hdr).group(1)) == getattr(T, "SPAN_" + name), name
    assert T.SPAN_WORDS == S.WORDS and all(getattr(T, "SPAN_%s_SUMSQ" % x) % 2 == 0 for x in "GWU")      # 8-byte aligned doubles
    # the generator's 100.5 M elements give "a few thousand" pieces
    assert 2000 <= 100_481_987 // S.PIECE <= 9000


def test_bad_arguments_are_refused_by_the_library():
    from hr_viton_amd import _lib
    lib = _lib.load()
    assert lib.hrv_span_stats_f32(None, None, None, None, None, 1, None, 1.0, 0.0, None, None) != 0
    assert b"span_stats" in lib.hrv_last_error()
    assert lib.hrv_span_stats_finalize(None, None, 1, None, None) != 0
    assert b"span_stats_finalize" in lib.hrv_last_error()


def _module_spans():
    net = torch.nn.Sequential(torch.nn.Conv2d(3, 7, 3), torch.nn.InstanceNorm2d(7, affine=True), torch.nn.Conv2d(7, 5, 1, bias=False),
                              torch.nn.Linear(41, 1013))      # 41 * 1013 = 41 533 elements: three pieces
    ps = list(net.parameters())
    return ps, S.setup_spans([p.numel() for p in ps])


@pytest.mark.parametrize("name", S.TABLES + ("module",))
def test_span_pieces_tile_every_span(name):
    T = _T()
    spans = _module_spans()[1] if name == "module" else S.table(name)[0]
    pieces, first = T.span_pieces(spans, S.PIECE)
    S.check_pieces(spans, pieces, first)
    assert all(ln <= S.PIECE for _, ln in pieces) and sum(ln for _, ln in pieces) == sum(k for _, k in spans)
    # the optimizer's (parameter, offset, length) triples give the same table, and so does any other piece length its own
    assert T.span_pieces([(None, o, k) for o, k in spans], S.PIECE) == (pieces, first)
    p7, f7 = T.span_pieces(spans, 7)
    S.check_pieces(spans, p7, f7, 7)
    if name == "many":
        assert len(pieces) == 300 and first == list(range(301))
    if name == "one":
        assert pieces == [(0, S.PIECE), (S.PIECE, S.PIECE), (2 * S.PIECE, S.PIECE), (3 * S.PIECE, 5)]
    with pytest.raises(ValueError):
        T.span_pieces([(0, 0)], S.PIECE)


def test_the_tables_are_what_the_gpu_tests_rest_on():
    for name in S.TABLES:
        spans, shift = S.table(name)
        bufs, base = S.lay_out(spans, shift, S.int_data(spans, 1))
        assert all(b.data_ptr() % 16 == 0 for b in bufs) and base % 4 == shift
        inside = torch.zeros(bufs[0].numel(), dtype=torch.bool)
        for off, k in spans:
            assert not inside[base + off:base + off + k].any(), "spans overlap"
            inside[base + off:base + off + k] = True
        for b in bufs:      # NaN in all four arrays everywhere outside the spans: both bands and every gap
            assert torch.isnan(b[~inside]).all() and torch.isfinite(b[inside]).all()
        assert torch.isnan(bufs[0][:S.BAND]).all() and torch.isnan(bufs[0][-S.BAND:]).all()
        if name in ("edges", "many"):
            assert all(off % 4 == 0 for off, _ in spans) and int((~inside[base:base + S.extent(spans)]).sum()) > 0      # real gaps
        if name == "packed":
            assert all(a[0] + a[1] == b[0] for a, b in zip(spans, spans[1:])) and any(off % 4 for off, _ in spans)
    assert [k for _, k in S.table("edges")[0]] == S.EDGE_LENGTHS and len(S.table("many")[0]) == 300 > 256
    assert S.poison_positions(2 * S.PIECE + 3) == [0, S.PIECE - 1, S.PIECE, 2 * S.PIECE + 2] and S.poison_positions(1) == [0]


def test_the_restatement_is_vector_norm_and_the_counts_per_parameter():
    ps, spans = _module_spans()
    data = S.gauss_data(spans, 3)
    g, w, m, v = data[5]          # the 41 533-element weight
    g[5], g[17], w[0], g[40], g[41] = float("nan"), float("inf"), float("-inf"), 0.0, -0.0
    m[9] = float("nan")
    refs = S.records_ref(data, True, S.GAUSS_BC2_SQRT, S.GAUSS_EPS)
    for (g, w, m, v), r in zip(data, refs):
        fg, fw = torch.isfinite(g), torch.isfinite(w)
        for x, fin, key in ((g, fg, "g"), (w, fw, "w")):
            want = float(torch.linalg.vector_norm(x[fin].double()))
            assert abs(math.sqrt(r[key + "_sumsq"]) - want) <= 1e-14 * want
            assert r[key + "_maxabs"] == float(x[fin].abs().max()) and r[key + "_nonfinite"] == int((~fin).sum())
        assert r["g_zeros"] == int((g == 0).sum())
    assert (refs[5]["g_nonfinite"], refs[5]["w_nonfinite"], refs[5]["u_nonfinite"], refs[5]["g_zeros"]) == (2, 1, 1, 2)
    assert all(r["g_nonfinite"] == r["w_nonfinite"] == r["u_nonfinite"] == r["g_zeros"] == 0 for i, r in enumerate(refs) if i != 5)
    # without the moments the update fields are zero
    assert all(r["u_sumsq"] == 0.0 and r["u_maxabs"] == 0.0 and r["u_nonfinite"] == 0 for r in S.records_ref(data, False))
    # packing keeps every bit
    words = S.pack_records(refs)
    assert words.dtype == torch.int32 and words.shape == (len(refs), S.WORDS) and not words[:, 13:].any()
    assert words.view(torch.float64)[5, 0].item() == refs[5]["g_sumsq"] and words.view(torch.float32)[5, 8].item() == refs[5]["u_maxabs"]


@pytest.mark.parametrize("wd", [0.0, 0.01], ids=["plain", "weight_decay"])
def test_the_update_direction_is_the_step_of_the_float64_adam(wd):
    """(lr / bc1) u == w_before - w_after of guard_cases.adam_ref64, with the constants of the benchmark's optimizers (lr 1e-4,
    betas (0, 0.9), eps 1e-8).  u is formed here in float64 from the moments adam_ref64 returns, by the expression the restatement
    and the kernel round to fp32.  Start weights are scaled by 2^-4: w - delta is rounded to a double, half an ulp of |w| < 0.5 is
    2^-55, which against a step of 1e-4 is 3e-13 of it -- with weights of order 4 the subtraction alone would cost 4e-12."""
    lr, betas, eps = 1e-4, (0.0, 0.9), 1e-8
    w0 = [w / 16 for w in G.start_weights()]
    steps = [G.gauss_grad_list(s) for s in range(3)]
    ref = G.adam_ref64(w0, steps, lr=lr, betas=betas, eps=eps, wd=wd)
    before = [w.double() for w in w0]
    for t, st in enumerate(ref, 1):
        bc1, bc2 = 1.0 - betas[0] ** t, 1.0 - betas[1] ** t
        for wb, wa, m, v in zip(before, st["w"], st["m"], st["v"]):
            u = m / (v.sqrt() / math.sqrt(bc2) + eps)
            got, want = (lr / bc1) * u, wb - wa
            assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max()), (t, float((got - want).abs().max() / want.abs().max()))
            # and the fp32 form the kernel computes is that direction to fp32 accuracy: 4 operations of half an ulp each
            u32 = S.update_dir(m.float(), v.float(), np.float32(math.sqrt(bc2)), eps)
            assert float(((u32.double() - u) / u).abs().max()) < 2.0 ** -19
        before = st["w"]


@pytest.mark.parametrize("name", S.TABLES)
def test_the_integer_cases_are_exact(name):
    spans, _ = S.table(name)
    data = S.int_data(spans, 7)
    for (g, w, m, v), r in zip(data, S.records_ref(data)):
        u = S.update_dir(m, v, 1.0, 0.0)
        assert torch.equal(u, u.round()) and float(u.abs().max()) <= 8 and torch.equal(u * v.sqrt(), m)
        assert set(v.tolist()) <= {1.0, 4.0, 16.0, 64.0} and set(g.tolist()) | set(w.tolist()) <= {0.0, 1.0, -1.0, 2.0, -2.0}
        for key in ("g_sumsq", "w_sumsq", "u_sumsq"):
            assert r[key] == int(r[key]) and r[key] < 2.0 ** 40
        assert r["g_zeros"] >= 1 and r["g_nonfinite"] == r["w_nonfinite"] == r["u_nonfinite"] == 0
        # any order, any precision wide enough: fp32 sums of these integers agree while they stay below 2^24
        if g.numel() <= 4096:
            assert float((g * g).sum()) == r["g_sumsq"] and float((g.flip(0).double() ** 2).sum()) == r["g_sumsq"]
