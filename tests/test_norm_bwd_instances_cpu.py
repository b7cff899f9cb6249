"""The compile-time instances of the normalisation backward are named in three places that must agree: the table in csrc/norm_bwd.hip
(hrv_diag_norm_bwd_instances), the list in DESIGN.md 7h and the cases the GPU test runs (tests/norm_bwd_instance_cases.py)."""
import os
import re

import norm_bwd_instance_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _library_table():
    import hr_viton_amd  # noqa: F401
    from hr_viton_amd import train_ops as T
    return T.norm_bwd_instances()


def test_the_table_in_c_the_list_in_design_md_and_the_test_cases_agree():
    table = _library_table()
    assert len(table) == len(set(table)) and all(re.fullmatch(r"(single|pair)\.stage[12] [a-z0-9_+]+", l) for l in table), table
    with open(os.path.join(ROOT, "DESIGN.md"), encoding="utf-8") as f:
        doc = f.read()
    sec = doc[doc.index("## 7h."):]
    listed = re.findall(r"^((?:single|pair)\.stage[12] [a-z0-9_+]+)$", sec, re.M)
    assert sorted(listed) == sorted(table), (sorted(set(listed) ^ set(table)))
    assert K.instance_lines() == sorted(table), (sorted(set(K.instance_lines()) ^ set(table)))


def test_the_cases_cover_both_sides_of_the_table():
    ids = [c.id for c in K.CASES]
    assert len(ids) == len(set(ids))
    assert any(c.route == 0 for c in K.CASES) and any(c.route in (1, 2) for c in K.CASES)
    assert any(c.pair and c.route == 3 for c in K.CASES) and any(c.pair and c.route != 3 for c in K.CASES)
    for n, h, w, c in K.EXTENTS:
        assert h % 2 == 0 and w % 2 == 0 and c % 4 == 0
    assert sum((h * w) % 128 != 0 for _, h, w, _ in K.EXTENTS) >= 1 and {c for *_, c in K.EXTENTS} == {64, 80, 128}


def test_the_pair_extents_reach_the_tail_the_uneven_slab_and_both_sides_of_the_chunk_cap():
    """tests/test_gpu_spade_fused.py runs the pair pass against two single calls at K.PAIR_EXTENTS x K.PAIR_CHANNELS; the slab count
    is the library's (norm_slabs, through the workspace size), the chunk cap is read from hrv_common.h"""
    import hr_viton_amd  # noqa: F401
    from hr_viton_amd import _lib
    with open(os.path.join(ROOT, "hr-viton_amd", "csrc", "hrv_common.h"), encoding="utf-8") as f:
        gcap = int(re.search(r"constexpr int NORM_GCAP = (\d+);", f.read()).group(1))
    c4s = [c // 4 for c in K.PAIR_CHANNELS]
    assert min(c4s) < gcap and gcap + 1 in c4s
    uneven = up = tail_after_loop = False
    for h, w, is_up in K.PAIR_EXTENTS:
        hw = h * w
        up |= is_up and h % 2 == 0 and w % 2 == 0
        for c in K.PAIR_CHANNELS:
            nb = (_lib.load().hrv_norm_bwd_workspace_elems(2, h, w, c) - 2 * c * 2) // (2 * c * 2)
            uneven |= hw % nb != 0
            gb = min(c // 4, gcap)
            rows, pb = 256 // gb, -(-hw // nb)
            if c // 4 > gcap:
                assert rows * gb == 256 and rows == 4 and (c // 4) % gcap == 1      # the second chunk: one live group of 64
            else:
                assert 256 - rows * gb > 0                                           # idle threads past the last row
            slabs = [min(pb, hw - b * pb) for b in range(nb)]
            walked = [len(range(r, s, rows)) for s in slabs for r in range(rows)]
            assert any(n % 2 == 1 for n in walked), (h, w, c)                        # the one-pixel tail of the two-pixel loop
            tail_after_loop |= any(n % 2 == 1 and n >= 3 for n in walked)             # ... reached after the loop body ran
    assert uneven and up and tail_after_loop
