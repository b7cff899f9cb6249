"""The compile-time instances of the normalisation backward are named in three places that must agree: the table in csrc/train.hip
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
