"""GPU: precision / recall / density / coverage on the HIP path (csrc/manifold.hip, hr_viton_amd/manifold.py) -- the four kernels,
``knn_radii`` and ``prdc`` at slab edges, and evaluate.py --prdc end to end -- against the float64 restatement of
tests/prdc_cases.py.

On the integer banks (values in -3 .. 3) all arithmetic is exact in fp64, so every output must equal the restatement.  On the
Gaussian banks a squared distance may differ from the restatement by the bound of ``prdc_cases.sqdist_bound``; tests/test_prdc_cpu.py
has shown that no comparison of those cases lies within twice that bound, so counts and metrics must still be equal.  Every test
prints its figures before it asserts.
"""
import os
import re
import sys

import numpy as np
import pytest
import torch

import fid_cases as Fc
import prdc_cases as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
INF = float("inf")


@pytest.fixture(scope="module")
def M():
    import hr_viton_amd  # noqa: F401
    from hr_viton_amd import manifold
    return manifold


def _dev(a, strided=False, pad=3, fill=77.0):
    """the array on the device: contiguous, or as a view of a wider buffer (row stride = columns + pad) whose padding holds junk"""
    t = torch.from_numpy(np.ascontiguousarray(a))
    if not strided:
        return t.cuda()
    wide = torch.full((t.shape[0], t.shape[1] + pad), fill, dtype=t.dtype)
    wide[:, :t.shape[1]] = t
    v = wide.cuda()[:, :t.shape[1]]
    assert v.stride(0) == t.shape[1] + pad and v.stride(1) == 1
    return v


_PARTS = {}


def _parts64(kind, case):
    """the restatement of a case, computed once and shared (read only)"""
    key = (kind, case)
    if key not in _PARTS:
        real, fake = (P.integer_case if kind == "int" else P.gaussian_case)(case)
        _PARTS[key] = (real, fake, P.parts64(real, fake, case[3]), P.prdc64(real, fake, case[3]))
    return _PARTS[key]


# ---------------------------------------------------------------------------------------------------------- integer banks: exact
@pytest.mark.parametrize("strided", [False, True], ids=["contiguous", "row-strided"])
@pytest.mark.parametrize("case", P.CASES, ids=P.case_id)
def test_kernels_on_integer_banks_are_exact(M, case, strided):
    nr, nf, D, k = case
    real, fake, want, _ = _parts64("int", case)
    R, F = _dev(real, strided), _dev(fake, strided)
    nR, nF = M.row_sqnorm(R), M.row_sqnorm(F)
    assert nR.dtype == torch.float64 and torch.equal(nR.cpu(), torch.from_numpy((real.astype(np.float64) ** 2).sum(-1)))
    assert torch.equal(nF.cpu(), torch.from_numpy((fake.astype(np.float64) ** 2).sum(-1)))
    # the cross block, with and without the norms handed in
    dRF = M.sqdist(R, F, nR, nF)
    assert dRF.shape == (nr, nf) and dRF.dtype == torch.float64 and torch.equal(dRF.cpu(), torch.from_numpy(want["dRF"]))
    assert torch.equal(M.sqdist(R, F), dRF) and torch.equal(M.sqdist(F, R, nF, nR), dRF.t())
    # inside a bank: duplicated rows are exactly 0 apart; slabs at rows 0 and 64 carry their own entries as +inf
    dRR = P.sqdist64(real, real)
    full = M.sqdist(R, R, nR, nR).cpu().numpy()
    assert np.array_equal(full, dRR) and (np.diag(full) == 0).all()
    if nr >= 4:
        assert full[nr - 1, 0] == 0.0 and full[nr // 2, 1] == 0.0
    for s0 in (0, 64):
        if s0 >= nr:
            continue
        s1 = min(s0 + 64, nr)
        slab = M.sqdist(R[s0:s1], R, nR[s0:s1], nR, self_offset=s0).cpu().numpy()
        ref = dRR[s0:s1].copy()
        ref[np.arange(s1 - s0), np.arange(s0, s1)] = INF
        assert np.array_equal(slab, ref), s0
        radii = M.row_kth(_dev(slab, strided), k).cpu().numpy()
        assert np.array_equal(radii, want["rR"][s0:s1]), s0
    # ball counts and minima from the restatement's block, as the metric asks for them
    d_fr, d_rf = _dev(np.ascontiguousarray(want["dRF"].T), strided), _dev(want["dRF"], strided)
    rR, rF = torch.from_numpy(want["rR"]).cuda(), torch.from_numpy(want["rF"]).cuda()
    cntF, none = M.row_ball(d_fr, rR, minimum=False)
    cntR, minR = M.row_ball(d_rf, rF)
    assert none is None and cntF.dtype == torch.int32 and torch.equal(cntF.cpu().long(), torch.from_numpy(want["cntF"]))
    assert torch.equal(cntR.cpu().long(), torch.from_numpy(want["cntR"])) and torch.equal(minR.cpu(), torch.from_numpy(want["minR"]))
    none, only_min = M.row_ball(d_rf, rF, count=False)
    assert none is None and torch.equal(only_min, minR)


@pytest.mark.parametrize("slab_rows", P.SLAB_ROWS)
@pytest.mark.parametrize("case", P.CASES, ids=P.case_id)
def test_prdc_on_integer_banks_is_exact(M, case, slab_rows):
    k = case[3]
    real, fake, want, want_m = _parts64("int", case)
    R, F = _dev(real), _dev(fake, strided=True)
    got = M.prdc_parts(R, F, k, slab_rows)
    for key in ("rR", "rF", "minR"):
        assert torch.equal(got[key].cpu(), torch.from_numpy(want[key])), key
    for key in ("cntF", "cntR"):
        assert got[key].dtype == torch.int32 and torch.equal(got[key].cpu().long(), torch.from_numpy(want[key])), key
    assert torch.equal(M.knn_radii(F, k, slab_rows).cpu(), torch.from_numpy(want["rF"]))
    res = M.prdc(R, F, k, slab_rows)
    print(f"{P.case_id(case)} integer, slabs of {slab_rows}: {res}")
    assert res == want_m and all(type(res[m]) is float for m in ("precision", "recall", "density", "coverage"))
    assert all(type(res[m]) is int for m in ("k", "n_real", "n_fake"))


# ---------------------------------------------------------------------------------------------------------- row_kth, row_ball
@pytest.mark.parametrize("strided", [False, True], ids=["contiguous", "row-strided"])
@pytest.mark.parametrize("rows,n", [(1, 1), (3, 16), (5, 17), (4, 63), (6, 64), (9, 65), (2, 129), (7, 300)])
def test_row_kth_order_statistics(M, rows, n, strided):
    rng = np.random.default_rng(rows * 1000 + n)
    d = rng.integers(0, 40, (rows, n)).astype(np.float64) / 4.0          # many ties
    d[rng.random((rows, n)) < 0.2] = INF
    d[0, :] = INF                                                         # a row without a finite entry
    if rows > 1:
        d[1, : min(n, 5)] = np.arange(min(n, 5))[::-1]                    # a row with exactly min(n, 5) finite entries ...
        d[1, min(n, 5):] = INF
    s = np.sort(d, axis=1)
    dev = _dev(d, strided)
    for k in sorted({1, 2, 5, 8, 9, 16, min(n, 5)}):
        if k > n:
            continue
        got = M.row_kth(dev, k).cpu().numpy()
        assert np.array_equal(got, s[:, k - 1]), k
    if rows > 1:      # ... whose k-th is its largest finite entry at k = their count, and +inf one further
        m = min(n, 5)
        assert M.row_kth(dev, m).cpu().numpy()[1] == m - 1
        if m < n:
            assert M.row_kth(dev, m + 1).cpu().numpy()[1] == INF
    assert np.isinf(M.row_kth(dev, 1).cpu().numpy()[0])
    from hr_viton_amd._lib import HrvError
    for bad in (0, 17, n + 1):
        with pytest.raises(HrvError):
            M.row_kth(dev, bad)


def test_row_ball_is_strict_and_serves_either_output_alone(M):
    from hr_viton_amd import _lib, ops
    rows, n = 9, 131
    rng = np.random.default_rng(3)
    r = rng.integers(1, 9, n).astype(np.float64)
    d = rng.integers(0, 9, (rows, n)).astype(np.float64)
    d[0] = r                          # every entry on its sphere: none counts
    d[1] = r - 0.5                    # every entry inside
    d[2] = np.nextafter(r, 0.0)       # one ulp inside
    d[3] = np.nextafter(r, INF)       # one ulp outside
    want_cnt, want_min = (d < r[None, :]).sum(1), d.min(1)
    assert want_cnt[:4].tolist() == [0, n, n, 0]
    dd, rr = torch.from_numpy(d).cuda(), torch.from_numpy(r).cuda()
    cnt, dmin = M.row_ball(dd, rr)
    assert torch.equal(cnt.cpu().long(), torch.from_numpy(want_cnt)) and torch.equal(dmin.cpu(), torch.from_numpy(want_min))
    # null cnt / null dmin at the C interface: the other output is written, and the same bits
    lib = _lib.load()
    c2 = torch.full((rows,), -5, dtype=torch.int32, device="cuda")
    m2 = torch.full((rows,), -5.0, dtype=torch.float64, device="cuda")
    assert lib.hrv_row_ball_f64(dd.data_ptr(), rr.data_ptr(), rows, n, n, c2.data_ptr(), None, ops._stream()) == 0
    assert lib.hrv_row_ball_f64(dd.data_ptr(), rr.data_ptr(), rows, n, n, None, m2.data_ptr(), ops._stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(c2, cnt) and torch.equal(m2, dmin)
    assert lib.hrv_row_ball_f64(dd.data_ptr(), rr.data_ptr(), rows, n, n, None, None, ops._stream()) != 0


# ---------------------------------------------------------------------------------------------------------- Gaussian banks
@pytest.mark.parametrize("case", P.CASES, ids=P.case_id)
def test_gaussian_banks_within_the_bound_and_metrics_equal(M, case):
    nr, nf, D, k = case
    real, fake, want, want_m = _parts64("gauss", case)
    R, F = _dev(real), _dev(fake)
    # squared distances, element by element, across and inside (the latter with their own entries replaced)
    worst = 0.0
    for (a, A), (b, B), ref in (((real, R), (fake, F), want["dRF"]), ((real, R), (real, R), P.sqdist64(real, real)),
                                ((fake, F), (fake, F), P.sqdist64(fake, fake))):
        got = M.sqdist(A, B).cpu().numpy()
        frac = np.abs(got - ref) / P.sqdist_bound(a, b)
        worst = max(worst, float(frac.max()))
        assert (got >= 0).all()
    # radii: an order statistic moves by no more than the largest error of its row
    fr = 0.0
    for x, X, key in ((real, R, "rR"), (fake, F, "rF")):
        got = M.knn_radii(X, k).cpu().numpy()
        fr = max(fr, float((np.abs(got - want[key]) / P.sqdist_bound(x, x).max(axis=1)).max()))
    print(f"{P.case_id(case)} Gaussian: worst sqdist error / bound {worst:.3e}, worst radius error / bound {fr:.3e}")
    assert worst <= 1.0 and fr <= 1.0
    parts = {s: M.prdc_parts(R, F, k, s) for s in P.SLAB_ROWS}
    for s, got in parts.items():
        for key in ("cntF", "cntR"):
            assert torch.equal(got[key].cpu().long(), torch.from_numpy(want[key])), (s, key)
        res = M.prdc(R, F, k, s)
        assert res == want_m, (s, res, want_m)
    # slabs of 64 and of 4096: the same bits; a second run: the same bits
    again = M.prdc_parts(R, F, k, 64)
    for key in ("rR", "rF", "cntF", "cntR", "minR"):
        assert torch.equal(parts[64][key], parts[4096][key]) and torch.equal(again[key], parts[64][key]), key
    print(f"  {want_m}")


# ---------------------------------------------------------------------------------------------------------- raising cases
def test_prdc_raises(M):
    from hr_viton_amd._lib import HrvError
    rng = np.random.default_rng(0)
    R, F = _dev(rng.standard_normal((20, 8)).astype(np.float32)), _dev(rng.standard_normal((18, 8)).astype(np.float32))
    assert M.kth_max() == 16
    for bad in (0, 17, -1, 2.5):
        with pytest.raises(ValueError):
            M.prdc(R, F, bad)
    with pytest.raises(ValueError):
        M.knn_radii(R, 17)
    for k in (3, 16):          # a bank of k rows, and of fewer
        with pytest.raises(ValueError):
            M.prdc(R[:k], F, k)
        with pytest.raises(ValueError):
            M.prdc(R, F[:k], k)
        with pytest.raises(ValueError):
            M.knn_radii(F[:k], k)
    assert M.prdc(R[:4], F[:4], 3)["n_real"] == 4          # k + 1 rows are enough
    for v in (float("nan"), INF):
        bad = R.clone()
        bad[7, 3] = v
        with pytest.raises(ValueError):
            M.prdc(bad, F, 3)
        with pytest.raises(ValueError):
            M.prdc(R, bad[:18], 3)
    with pytest.raises(HrvError):
        M.prdc(R, F[:, :7], 3)
    with pytest.raises(HrvError):
        M.prdc(R.cpu(), F.cpu(), 3)
    with pytest.raises(HrvError):
        M.prdc(R.double(), F.double(), 3)
    with pytest.raises(HrvError):
        M.sqdist(R[:4], R, self_offset=17)          # the slab would end past the bank


# ---------------------------------------------------------------------------------------------------------- evaluate.py
def _prdc_line(line):
    m = re.fullmatch(r"Precision : (\S+) / Recall : (\S+) / Density : (\S+) / Coverage : (\S+) / k : (\d+)", line)
    assert m, line
    return tuple(float(v) for v in m.groups()[:4]) + (int(m.group(5)),)


def test_evaluate_prdc_end_to_end(tmp_path):
    from PIL import Image
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import importlib
    ev = importlib.import_module("evaluate")

    class Recording(ev.FidScorer):
        fills, banks = 0, None

        def fill(self, bank, row0, batch):
            type(self).fills += 1
            return super().fill(bank, row0, batch)

        def prdc(self, bank_pred, bank_gt, k):
            type(self).banks = (bank_pred.cpu().numpy().copy(), bank_gt.cpu().numpy().copy())
            return super().prdc(bank_pred, bank_gt, k)

    def scorer():
        import hr_viton_amd  # noqa: F401
        from hr_viton_amd.inception import FIDInceptionV3
        torch.manual_seed(0)          # what load_fid_inception does under --fid_random_init with the default --seed
        Recording.fills, Recording.banks = 0, None
        return Recording(FIDInceptionV3().eval())

    gt_dir, pr_dir = tmp_path / "gt", tmp_path / "pred"
    gt_dir.mkdir()
    pr_dir.mkdir()
    pr_names = Fc.write_pngs(pr_dir, 12, 31)
    gt_names = Fc.write_pngs(gt_dir, 13, 32)
    argv = ["--predict_dir", str(pr_dir), "--ground_truth_dir", str(gt_dir), "--fid_only", "--fid_random_init", "--kid_subsets", "4",
            "--kid_subset_size", "8", "-j", "0", "--fid_inception_weights", str(tmp_path / "none.pth")]
    res0 = ev.main(argv)                                             # without --prdc: the FID line alone
    lines0 = (pr_dir / "eval.txt").read_text().splitlines()
    assert len(lines0) == 2 and lines0[0].startswith("FID : ")
    res = ev.main(argv + ["--prdc", "--prdc_k", "3"], fid_scorer=scorer())
    lines = (pr_dir / "eval.txt").read_text().splitlines()
    assert len(lines) == 6 and lines[2] == lines[0] and lines[3] == lines[1] == lines[5] == "FID Inception weights : random init (plumbing only)"
    assert res["fid"] == res0["fid"] and Recording.fills == 2          # 12 and 13 images in batches of 16: once per folder
    fp, fg = Recording.banks
    assert fp.shape == (12, 2048) and fg.shape == (13, 2048) and fp.dtype == np.float32
    want = P.prdc64(fg, fp, 3)
    margin, gap = P.margin64(fg, fp, 3)
    bound = P.max_bound(fg, fp)
    got = _prdc_line(lines[4])
    print(f"evaluate.py --fid_only --prdc: {lines[4]}; restatement {want}; smallest |d2 - r| {margin:.3e}, k / k+1 gap {gap:.3e}, "
          f"error bound {bound:.3e}")
    assert margin > 2.0 * bound, "the features put a comparison inside the error bound: the case cannot demand equality"
    assert got == (want["precision"], want["recall"], want["density"], want["coverage"], 3)
    assert (res["precision"], res["recall"], res["density"], res["coverage"], res["prdc_k"]) == got
    assert {"fid_features_s", "fid_stats_s", "prdc_s"} <= set(res["timings"])
    # --fid --prdc with the paired metrics on 12 + 13 images: the features are computed once for both
    gt2, pr2 = tmp_path / "gt2", tmp_path / "pred2"
    gt2.mkdir()
    pr2.mkdir()
    for i, nm in enumerate(pr_names):
        Image.open(pr_dir / nm).save(pr2 / f"{i:05d}_00_{(i + 1) % 12:05d}_00.png")
    for i, nm in enumerate(gt_names):
        Image.open(gt_dir / nm).convert("RGB").save(gt2 / f"{i:05d}_00.jpg", quality=95)
    res2 = ev.main(["--predict_dir", str(pr2), "--ground_truth_dir", str(gt2), "--fid", "--prdc", "--prdc_k", "3", "--fid_random_init",
                    "--kid_subsets", "4", "--kid_subset_size", "8", "-j", "0", "--lpips_random_init", "--lpips_weights",
                    str(tmp_path / "no.pth"), "--alexnet_weights", str(tmp_path / "no2.pth"), "--inception_weights",
                    str(tmp_path / "no3.pth"), "--fid_inception_weights", str(tmp_path / "none.pth")], fid_scorer=scorer())
    lines = (pr2 / "eval.txt").read_text().splitlines()
    assert len(lines) == 7, lines
    assert lines[0].startswith("SSIM : ") and lines[2] == "LPIPS weights : random init (plumbing only)" and lines[3].startswith("FID : ")
    assert _prdc_line(lines[5])[:4] == (res2["precision"], res2["recall"], res2["density"], res2["coverage"])
    assert lines[4] == lines[6] == "FID Inception weights : random init (plumbing only)"
    assert Recording.fills == 2 and res2["pairs"] == 12 and np.isfinite(res2["fid"])
    assert _prdc_line(lines[5])[:4] == tuple(P.prdc64(Recording.banks[1], Recording.banks[0], 3)[m]
                                             for m in ("precision", "recall", "density", "coverage"))
