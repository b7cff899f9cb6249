"""CPU (no GPU needed): the float64 restatement of precision / recall / density / coverage (tests/prdc_cases.py) on a hand example,
the margins of the Gaussian cases that let tests/test_gpu_prdc.py demand equality, the C interface of csrc/manifold.hip as far as
it goes without a device, and evaluate.py's --prdc flags, data path and output files with the GPU work stubbed."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

import fid_cases as Fc
import prdc_cases as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

NEW_SYMBOLS = ("hrv_row_sqnorm_f64", "hrv_sqdist_nt_f64", "hrv_row_kth_max", "hrv_row_kth_f64", "hrv_row_ball_f64")


def _evaluate():
    import importlib
    return importlib.import_module("evaluate")


# ---------------------------------------------------------------------------------------------------------- the restatement
def test_hand_example_in_one_dimension():
    """reals {0, 1, 2, 10}, fakes {0.5, 1.5, 20}, k = 1.  Squared radii: rR = (1, 1, 1, 64), rF = (1, 1, 342.25).
    cntF: 0.5 lies inside the balls of 0 and 1 (0.25 < 1), 1.5 inside those of 1 and 2, 20 inside none (100 > 64): (2, 2, 0) ->
    precision 2/3, density 4 / (1 * 3).  cntR: 0 lies in the ball of 0.5, 1 in those of 0.5 and 1.5, 2 in those of 1.5 and 20
    (324 < 342.25), 10 in that of 20: (1, 2, 2, 1), recall 1.  Nearest fakes at 0.25, 0.25, 0.25 and 72.25 against rR: coverage 3/4."""
    real = np.array([[0.0], [1.0], [2.0], [10.0]], np.float32)
    fake = np.array([[0.5], [1.5], [20.0]], np.float32)
    p = P.parts64(real, fake, 1)
    assert p["rR"].tolist() == [1.0, 1.0, 1.0, 64.0] and p["rF"].tolist() == [1.0, 1.0, 342.25]
    assert p["cntF"].tolist() == [2, 2, 0] and p["cntR"].tolist() == [1, 2, 2, 1] and p["minR"].tolist() == [0.25, 0.25, 0.25, 72.25]
    got = P.prdc64(real, fake, 1)
    assert got == {"precision": 2 / 3, "recall": 1.0, "density": 4 / 3, "coverage": 3 / 4, "k": 1, "n_real": 4, "n_fake": 3}


def test_restatement_excludes_the_index_not_the_value_and_compares_strictly():
    x = np.array([[0.0, 0.0], [0.0, 0.0], [3.0, 4.0]], np.float32)          # row 1 duplicates row 0
    assert P.radii64(x, 1).tolist() == [0.0, 0.0, 25.0] and P.radii64(x, 2).tolist() == [25.0, 25.0, 25.0]
    # a fake exactly on the sphere of a real's ball is outside it
    real, fake = np.array([[0.0], [2.0], [10.0]], np.float32), np.array([[4.0], [12.0], [30.0]], np.float32)
    p = P.parts64(real, fake, 1)
    assert p["rR"].tolist() == [4.0, 4.0, 64.0] and p["dRF"][1, 0] == 4.0 and p["dRF"][2, 1] == 4.0
    assert p["cntF"].tolist() == [1, 1, 0]          # 4 is inside the ball of 10 only (36 < 64; 4 < 4 is false), 12 too (4 < 64)


@pytest.mark.parametrize("case", P.CASES, ids=P.case_id)
def test_gaussian_cases_keep_every_comparison_outside_the_error_bound(case):
    """A comparison d2 < r of the GPU path has a rounding error on both sides, each below the bound of tests/prdc_cases.py's
    ``sqdist_bound``; with every |d2 - r| of the float64 restatement above twice the largest bound of the case no comparison can come
    out differently, and with the gap between the k-th and (k + 1)-th neighbour above it the radius is the same neighbour's."""
    real, fake = P.gaussian_case(case)
    k = case[3]
    margin, gap = P.margin64(real, fake, k)
    bound = P.max_bound(real, fake)
    print(f"{P.case_id(case)}: smallest |d2 - r| {margin:.3e}, smallest k / k+1 gap {gap:.3e}, largest error bound {bound:.3e}")
    assert margin > 2.0 * bound and gap > 2.0 * bound
    got = P.prdc64(real, fake, k)
    assert all(0.0 <= got[m] <= 1.0 for m in ("precision", "recall", "coverage")) and got["density"] >= 0.0


def test_the_case_table_covers_what_it_should():
    ks = {c[3] for c in P.CASES}
    assert ks == {1, 3, 5, 16} and {c[2] for c in P.CASES} == {1, 3, 4, 5, 17, 64}
    for k in ks:
        sizes = {n for c in P.CASES if c[3] == k for n in c[:2]}
        assert k + 1 in sizes and sizes <= {k + 1, 17, 63, 64, 65, 129}
    assert {n for c in P.CASES for n in c[:2]} >= {17, 63, 64, 65, 129} and P.SLAB_ROWS == [64, 4096]
    real, fake = P.integer_case((64, 65, 4, 1))
    assert np.abs(real).max() <= 3 and np.array_equal(real[-1], real[0]) and np.array_equal(fake[65 // 2], fake[1])
    # the mixture is not degenerate: somewhere in the Gaussian table each number lies strictly inside (0, 1)
    vals = [P.prdc64(*P.gaussian_case(c), c[3]) for c in P.CASES]
    for m in ("precision", "recall", "coverage"):
        assert any(0.0 < v[m] < 1.0 for v in vals), m


# ---------------------------------------------------------------------------------------------------------- the C interface
@pytest.fixture(scope="module")
def lib():
    import hr_viton_amd  # noqa: F401
    from hr_viton_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from hr_viton_amd import build
        build.build(verbose=False)
    return _lib.load()


def test_header_declares_and_library_exports_the_entry_points(lib):
    from hr_viton_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "hrviton_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
    # every launching entry point takes the stream last
    for name in NEW_SYMBOLS:
        if name != "hrv_row_kth_max":
            assert re.search(r"\b%s\s*\([^)]*hrv_stream_t stream\)" % name, hdr), name
    assert lib.hrv_row_kth_max() == 16 == _evaluate().PRDC_K_MAX


def test_null_and_bad_extent_calls_fail_before_launching(lib):
    """none of these reaches a launch: they return non-zero on a machine without a device (the pointers are never dereferenced)"""
    p = C.c_void_p(4096)
    sq, sd, kth, ball = lib.hrv_row_sqnorm_f64, lib.hrv_sqdist_nt_f64, lib.hrv_row_kth_f64, lib.hrv_row_ball_f64
    for args in ((None, 4, 8, 8, p), (p, 4, 8, 8, None), (p, 0, 8, 8, p), (p, 4, 0, 8, p), (p, 4, 8, 7, p)):
        assert sq(*args, None) != 0, args
    assert b"row_sqnorm" in lib.hrv_last_error()
    good = dict(X=p, Y=p, nx=4, ny=6, D=8, ldx=8, ldy=8, normX=p, normY=p, self_offset=-1, out=p, ldo=6)
    for bad in (dict(X=None), dict(Y=None), dict(normX=None), dict(normY=None), dict(out=None), dict(nx=0), dict(ny=0), dict(D=0),
                dict(ldx=7), dict(ldy=7), dict(ldo=5), dict(self_offset=-2), dict(self_offset=3), dict(nx=64 * 65535 + 1, ny=64 * 65535 + 1,
                                                                                                    ldo=64 * 65535 + 1)):
        a = dict(good, **bad)
        assert sd(*a.values(), None) != 0, bad
    assert b"sqdist" in lib.hrv_last_error()
    for args in ((None, 4, 8, 8, 1, p), (p, 4, 8, 8, 1, None), (p, 0, 8, 8, 1, p), (p, 4, 0, 8, 1, p), (p, 4, 8, 7, 1, p), (p, 4, 8, 8, 0, p),
                 (p, 4, 32, 32, 17, p), (p, 4, 8, 8, 9, p)):
        assert kth(*args, None) != 0, args
    assert b"row_kth" in lib.hrv_last_error()
    for args in ((None, p, 4, 8, 8, p, p), (p, None, 4, 8, 8, p, p), (p, p, 0, 8, 8, p, p), (p, p, 4, 0, 8, p, p), (p, p, 4, 8, 7, p, p),
                 (p, p, 4, 8, 8, None, None)):
        assert ball(*args, None) != 0, args
    assert b"row_ball" in lib.hrv_last_error()


# ---------------------------------------------------------------------------------------------------------- evaluate.py
def _tree(tmp_path, n_pred=4, n_gt=5, size=(48, 64)):
    from PIL import Image
    rng = np.random.default_rng(5)
    gt, pr = tmp_path / "gt", tmp_path / "pred"
    gt.mkdir()
    pr.mkdir()
    for i in range(n_gt):
        Image.fromarray(rng.integers(0, 256, (size[1], size[0], 3), dtype=np.uint8)).save(gt / f"{i:05d}_00.jpg")
    for i in range(n_pred):
        Image.fromarray(rng.integers(0, 256, (size[1], size[0], 3), dtype=np.uint8)).save(pr / f"{i:05d}_00_{(i + 1) % n_pred:05d}_00.png",
                                                                                          format="JPEG")
    return gt, pr


def _pair_stub(seen):
    def scorer(batch):
        seen.extend(batch)
        return [(0.5, 0.01, 0.2)] * len(batch)
    return scorer


class _FidStub:
    """stands in for evaluate.FidScorer as it was before --prdc: host banks of 12 block means per image, the restatement's FID /
    KID, and no ``prdc`` method"""

    def __init__(self):
        self.fills, self.banks = 0, []

    def bank(self, n):
        self.banks.append(np.full((n, 12), np.nan, np.float32))
        return self.banks[-1]

    def fill(self, bank, row0, batch):
        self.fills += 1
        for j, it in enumerate(batch):
            img = it["img"].astype(np.float64) / 255.0
            h, w = img.shape[0] // 2, img.shape[1] // 2
            bank[row0 + j] = [img[a * h:(a + 1) * h, b * w:(b + 1) * w, c].mean() for a in range(2) for b in range(2) for c in range(3)]

    def score(self, bank_pred, bank_gt, subsets, subset_size):
        return Fc.fid_kid64(bank_pred, bank_gt, subsets, subset_size)


class _PrdcStub(_FidStub):
    def prdc(self, bank_pred, bank_gt, k):
        return P.prdc64(bank_gt, bank_pred, k)


def _prdc_line(line):
    m = re.fullmatch(r"Precision : (\S+) / Recall : (\S+) / Density : (\S+) / Coverage : (\S+) / k : (\d+)", line)
    assert m, line
    return tuple(float(v) for v in m.groups()[:4]) + (int(m.group(5)),)


def test_evaluate_prdc_flags():
    ev = _evaluate()
    o = ev.get_opt([])
    assert o.prdc is False and o.prdc_k == 5
    o = ev.get_opt(["--prdc", "--prdc_k", "16", "--fid_only"])
    assert o.prdc is True and o.prdc_k == 16 and o.fid_only is True
    for bad in (["--prdc_k", "0"], ["--prdc_k", "17"], ["--prdc", "--prdc_k", "-1"]):
        with pytest.raises(SystemExit):
            ev.get_opt(bad)


@pytest.mark.parametrize("flags", [["--prdc"], ["--fid_only", "--prdc"], ["--fid", "--prdc"]], ids=lambda f: "".join(f))
def test_oversize_k_is_an_argparse_error_naming_both_counts(tmp_path, capsys, flags):
    ev = _evaluate()
    gt, pr = _tree(tmp_path, n_pred=4, n_gt=7)
    argv = ["--predict_dir", str(pr), "--ground_truth_dir", str(gt), "-j", "0", "--kid_subset_size", "4"] + flags
    for k in ("5", "4"):          # the default, and the smaller set's own size: k + 1 rows are needed
        with pytest.raises(SystemExit) as e:
            ev.main(argv + ["--prdc_k", k], scorer=_pair_stub([]), fid_scorer=_PrdcStub())
        assert e.value.code == 2
        err = capsys.readouterr().err
        assert "--prdc_k" in err and "4 predictions" in err and "7 ground truths" in err and "usage:" in err
    assert not (pr / "eval.txt").exists() or "Precision" not in (pr / "eval.txt").read_text()
    res = ev.main(argv + ["--prdc_k", "3"], scorer=_pair_stub([]), fid_scorer=_PrdcStub())
    assert res["prdc_k"] == 3


def test_without_prdc_a_stand_in_scorer_writes_what_it_wrote_before(tmp_path, capsys):
    """the scorer has no ``prdc`` method: --fid and --fid_only never call one, and eval.txt, stdout and the result are today's"""
    ev = _evaluate()
    gt, pr = _tree(tmp_path, n_pred=6, n_gt=8)
    stub = _FidStub()
    argv = ["--predict_dir", str(pr), "--ground_truth_dir", str(gt), "-j", "0", "-b", "4", "--kid_subsets", "3", "--kid_subset_size", "5",
            "--inception_weights", str(tmp_path / "none.pth")]
    res = ev.main(argv + ["--fid"], scorer=_pair_stub([]), fid_scorer=stub)
    fid, km, ks = (float(v) for v in Fc.fid_kid64(stub.banks[0], stub.banks[1], 3, 5))
    want = (f"SSIM : {sum([0.5] * 6) / 8} / MSE : {sum([0.01] * 6) / 8} / LPIPS : {sum([0.2] * 6) / 8}\nIS_mean : nan / IS_std : nan\n"
            f"FID : {fid} / KID_mean : {km} / KID_std : {ks}\n")
    assert (pr / "eval.txt").read_text() == want
    assert set(res) == {"ssim", "mse", "lpips", "is_mean", "is_std", "pairs", "timings", "fid", "kid_mean", "kid_std", "fid_images"}
    assert set(res["timings"]) == {"loader_wait_s", "gpu_s", "total_s", "fid_features_s", "fid_stats_s"}
    out = capsys.readouterr().out
    assert out.endswith("Calculate FID, KID...\nFID : %f / KID_mean : %f / KID_std : %f\n" % (fid, km, ks)) and "Precision" not in out
    res2 = ev.main(argv + ["--fid_only", "--fid_random_init"], fid_scorer=_FidStub())
    assert (pr / "eval.txt").read_text() == want + f"FID : {fid} / KID_mean : {km} / KID_std : {ks}\n" \
        "FID Inception weights : random init (plumbing only)\n"
    assert set(res2) == {"fid", "kid_mean", "kid_std", "fid_images", "timings"} and set(res2["timings"]) == {"fid_features_s", "fid_stats_s"}
    assert capsys.readouterr().out == ("Calculate FID, KID...\nFID : %f / KID_mean : %f / KID_std : %f\n" % (fid, km, ks)
                                       + "(FID / KID from randomly initialised weights: plumbing only)\n")
    # and a paired run without any of the flags: two lines, nothing of the unpaired path imported
    (tmp_path / "t3").mkdir()
    gt3, pr3 = _tree(tmp_path / "t3", n_pred=4, n_gt=4)
    before = set(sys.modules)
    res3 = ev.main(["--predict_dir", str(pr3), "--ground_truth_dir", str(gt3), "-j", "0", "--inception_weights", str(tmp_path / "none.pth")],
                   scorer=_pair_stub([]))
    assert (pr3 / "eval.txt").read_bytes() == b"SSIM : 0.5 / MSE : 0.01 / LPIPS : 0.2\nIS_mean : nan / IS_std : nan\n"
    assert set(res3) == {"ssim", "mse", "lpips", "is_mean", "is_std", "pairs", "timings"}
    assert not {m for m in set(sys.modules) - before if m.endswith(("feat_stats", "manifold"))}


def test_prdc_with_a_stand_in_scorer(tmp_path, capsys):
    ev = _evaluate()
    gt, pr = _tree(tmp_path, n_pred=6, n_gt=8)
    argv = ["--predict_dir", str(pr), "--ground_truth_dir", str(gt), "-j", "0", "-b", "4", "--kid_subsets", "3", "--kid_subset_size", "5",
            "--inception_weights", str(tmp_path / "none.pth"), "--prdc_k", "2"]
    # --prdc alone: its line after the paired run's two, no FID line; the ground truths are the real bank
    stub = _PrdcStub()
    seen = []
    res = ev.main(argv + ["--prdc"], scorer=_pair_stub(seen), fid_scorer=stub)
    lines = (pr / "eval.txt").read_text().splitlines()
    assert len(lines) == 3 and lines[0].startswith("SSIM : ") and lines[1] == "IS_mean : nan / IS_std : nan" and len(seen) == 6
    want = P.prdc64(stub.banks[1], stub.banks[0], 2)
    assert [b.shape for b in stub.banks] == [(6, 12), (8, 12)] and stub.fills == 4          # 6 and 8 images in batches of 4
    assert _prdc_line(lines[2]) == (want["precision"], want["recall"], want["density"], want["coverage"], 2)
    assert lines[2] == (f"Precision : {want['precision']} / Recall : {want['recall']} / Density : {want['density']} / "
                        f"Coverage : {want['coverage']} / k : 2")
    assert (res["precision"], res["recall"], res["density"], res["coverage"], res["prdc_k"]) == _prdc_line(lines[2])
    assert "fid" not in res and "prdc_s" in res["timings"] and "fid_stats_s" not in res["timings"] and "fid_features_s" in res["timings"]
    assert all(isinstance(res[m], float) for m in ("precision", "recall", "density", "coverage"))
    out = capsys.readouterr().out
    assert "Precision : %f / Recall : %f" % (want["precision"], want["recall"]) in out and "FID" not in out
    # --fid_only --prdc: the two unpaired lines, nothing paired, the banks filled once
    lp = (pr / "lpips.txt").read_bytes()
    stub2, seen2 = _PrdcStub(), []
    res2 = ev.main(argv + ["--fid_only", "--prdc", "--fid_random_init"], scorer=_pair_stub(seen2), fid_scorer=stub2)
    lines = (pr / "eval.txt").read_text().splitlines()
    assert len(lines) == 7 and lines[3].startswith("FID : ") and lines[5] == lines[2]
    assert lines[4] == lines[6] == "FID Inception weights : random init (plumbing only)"
    assert seen2 == [] and (pr / "lpips.txt").read_bytes() == lp and stub2.fills == 4 and len(stub2.banks) == 2
    assert set(res2) == {"fid", "kid_mean", "kid_std", "fid_images", "precision", "recall", "density", "coverage", "prdc_k", "timings"}
    assert set(res2["timings"]) == {"fid_features_s", "fid_stats_s", "prdc_s"}
    import json
    json.dumps(res2)
    # --fid --prdc: the paired lines, then both, again from one pair of banks
    stub3 = _PrdcStub()
    res3 = ev.main(argv + ["--fid", "--prdc"], scorer=_pair_stub([]), fid_scorer=stub3)
    lines = (pr / "eval.txt").read_text().splitlines()
    assert len(lines) == 11 and lines[9] == lines[3] and lines[10] == lines[2] and stub3.fills == 4 and len(stub3.banks) == 2
    assert res3["fid"] == res2["fid"] and res3["precision"] == res["precision"] and res3["pairs"] == 6


def test_prdc_without_weights_writes_nan(tmp_path, capsys):
    ev = _evaluate()
    gt, pr = _tree(tmp_path, n_pred=4, n_gt=4)
    argv = ["--predict_dir", str(pr), "--ground_truth_dir", str(gt), "-j", "0", "--prdc_k", "3", "--inception_weights", str(tmp_path / "no.pth"),
            "--fid_inception_weights", str(tmp_path / "none.pth")]
    res = ev.main(argv + ["--prdc"], scorer=_pair_stub([]))
    lines = (pr / "eval.txt").read_text().splitlines()
    assert lines == ["SSIM : 0.5 / MSE : 0.01 / LPIPS : 0.2", "IS_mean : nan / IS_std : nan",
                     "Precision : nan / Recall : nan / Density : nan / Coverage : nan / k : 3"]
    assert all(np.isnan(res[m]) for m in ("precision", "recall", "density", "coverage")) and res["prdc_k"] == 3 and "fid" not in res
    out = capsys.readouterr()
    assert "--fid_inception_weights" in out.err and "nothing is downloaded" in out.err and "precision / recall" in out.err
    assert "Precision : nan" in out.out
    ev.main(argv + ["--fid_only", "--prdc", "--kid_subset_size", "4"])
    assert (pr / "eval.txt").read_text().splitlines()[3:] == ["FID : nan / KID_mean : nan / KID_std : nan", lines[2]]
    assert "FID / KID / precision / recall / density / coverage: not computed" in capsys.readouterr().err


def test_product_modules_import_no_test_code():
    src = "".join(open(os.path.join(ROOT, *p)).read() for p in (("hr-viton_amd", "manifold.py"), ("evaluate.py",)))
    assert "prdc_cases" not in src and "from tests" not in src and "sklearn" not in src and "import oracle" not in src
