"""CPU (no GPU needed): the FID Inception-v3's table and state-dict layout, the host half of FID / KID (hr_viton_amd/feat_stats.py:
the Frechet distance, torch-fidelity's subsets, the unbiased MMD^2) against the restatements of tests/fid_cases.py and scipy, and
evaluate.py's --fid flags, data path and output files with the GPU work stubbed."""
import os
import sys

import numpy as np
import pytest
import torch

import fid_cases as Fc
import inception_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _evaluate():
    import importlib
    return importlib.import_module("evaluate")


@pytest.fixture(scope="module")
def S():
    import hr_viton_amd  # noqa: F401
    from hr_viton_amd import feat_stats
    return feat_stats


# ---------------------------------------------------------------------------------------------------------- the network as data
def test_fid_module_matches_table():
    import hr_viton_amd  # noqa: F401
    from hr_viton_amd import inception as I
    torch.manual_seed(0)
    m = I.FIDInceptionV3()
    assert set(m.state_dict().keys()) == Fc.state_keys() == K.state_keys(aux=False)
    assert not any(k.startswith("AuxLogits.") for k in m.state_dict())
    assert tuple(m.fc.weight.shape) == (1008, 2048) and tuple(m.fc.bias.shape) == (1008,)
    units = dict(m.units())
    assert len(units) == 94
    for name, cin, cout, k, s, p in K.UNITS:
        conv, bn = units[name].conv, units[name].bn
        assert tuple(conv.weight.shape) == (cout, cin, *k) and conv.stride == (s, s) and conv.padding == p and bn.eps == 0.001, name
    assert not m.training and not any(p.requires_grad for p in m.parameters())
    # the variant is data: a pool step per block, in the pooled branch only; the unchanged blocks and torchvision's network keep theirs
    want = {"Mixed_5b": "avg_inside", "Mixed_5c": "avg_inside", "Mixed_5d": "avg_inside", "Mixed_6a": "max", "Mixed_6b": "avg_inside",
            "Mixed_6c": "avg_inside", "Mixed_6d": "avg_inside", "Mixed_6e": "avg_inside", "Mixed_7a": "max", "Mixed_7b": "avg_inside",
            "Mixed_7c": "max_same"}
    plain = I.Inception3()
    for name in K.BLOCKS:
        fb, pb = getattr(m, name).branches, getattr(plain, name).branches
        assert fb[-1][0] == want[name] and fb[:-1] == pb[:-1] and fb[-1][1:] == pb[-1][1:], name
        assert pb[-1][0] == ("max" if name in ("Mixed_6a", "Mixed_7a") else "avg"), name
        assert getattr(m, name).offsets() == getattr(plain, name).offsets()
    assert I.POOL_MODES == {"max": 0, "avg": 1, "avg_inside": 2, "max_same": 3}
    assert I.FIDInceptionV3.run_block is I.Inception3.run_block and I.FIDInceptionV3.stem is I.Inception3.stem
    assert I.FIDInceptionV3.features is I.Inception3.features and I.FIDInceptionV3.plan is I.Inception3.plan


def test_fid_state_dict_loading():
    import hr_viton_amd  # noqa: F401
    from hr_viton_amd.inception import FIDInceptionV3
    sd = Fc.fid_state_dict(K.raw_weights(4))
    assert set(sd) == Fc.state_keys()
    m = FIDInceptionV3()
    m.load_state_dict(sd)
    got = m.state_dict()
    for k in ("Mixed_6c.branch7x7dbl_3.conv.weight", "Mixed_7c.branch_pool.bn.running_var", "fc.weight", "Conv2d_1a_3x3.bn.weight"):
        assert torch.equal(got[k], sd[k]), k
    # the released file predates num_batches_tracked
    m.load_state_dict({k: v for k, v in sd.items() if not k.endswith("num_batches_tracked")}, strict=False)
    for gone in ("Mixed_5b.branch_pool.conv.weight", "Mixed_7c.branch3x3_2a.bn.running_mean", "fc.weight", "fc.bias"):
        with pytest.raises(KeyError) as e:
            FIDInceptionV3().load_state_dict({k: v for k, v in sd.items() if k != gone})
        assert gone in str(e.value) and "FIDInceptionV3" in str(e.value)
    with pytest.raises(NotImplementedError):
        m.train()
    from hr_viton_amd._lib import HrvError
    with pytest.raises(HrvError):
        m.features_u8(torch.zeros(1, 64, 48, 3, dtype=torch.uint8))


def test_prep_restatement_against_torch():
    """the float64 statement of the input path and torch's own fp32 interpolate are the same function: they differ by torch's fp32
    rounding of the source coordinate alone (below 512 here: half an ulp is 1.5e-5 on a weight, against a pixel step of at most 1 in
    x / 255, doubled by 2v - 1, on two axes: 6e-5; a wrong neighbour, clamp or half-pixel offset is off by 1e-2 and more)"""
    rng = np.random.default_rng(0)
    for H, W in Fc.PREP_SIZES[:4]:
        img = rng.integers(0, 256, (2, H, W, 3), dtype=np.uint8)
        err = np.abs(Fc.prep_torch32(img).astype(np.float64) - Fc.prep64(img)).max()
        assert Fc.prep64(img).shape == (2, 299, 299, 3) and err < 1e-4, (H, W, err)


# ---------------------------------------------------------------------------------------------------------- Frechet distance
def test_frechet_distance_against_scipy_sqrtm(S):
    m1, s1 = Fc.gaussian_moments(400, 32, 1, 0.0, 1.0)
    m2, s2 = Fc.gaussian_moments(400, 32, 2, 0.5, 1.7)
    assert max(np.linalg.cond(s1), np.linalg.cond(s2)) < 1e6
    got, want = S.frechet_distance(m1, s1, m2, s2), Fc.frechet_sqrtm(m1, s1, m2, s2)
    rel = abs(got - want) / abs(want)
    # two float64 algorithms (a Schur-based square root of a non-symmetric product; two symmetric eigen-decompositions).  Measured on
    # these inputs: 55.7274741494294 against 55.72747414942937, relative disagreement 5.1e-16.  The limit is 100 x that.
    MEASURED = 5.1e-16
    limit = 100 * MEASURED
    assert limit <= 1e-6
    print(f"frechet_distance {got!r}, sqrtm {want!r}, relative disagreement {rel:.3e} (limit {limit:.1e})")
    assert rel <= limit, (got, want, rel)
    assert isinstance(got, float)
    # torch tensors are accepted as they come from moments()
    assert S.frechet_distance(torch.from_numpy(m1), torch.from_numpy(s1), torch.from_numpy(m2), torch.from_numpy(s2)) == got


def test_frechet_distance_rank_deficient(S):
    m1, s1 = Fc.gaussian_moments(8, 32, 3, 0.0, 1.0)
    m2, s2 = Fc.gaussian_moments(8, 32, 4, 0.5, 1.7)
    assert np.linalg.matrix_rank(s1) == 7 and np.linalg.matrix_rank(s2) == 7
    a, b = S.frechet_distance(m1, s1, m2, s2), S.frechet_distance(m2, s2, m1, s1)
    print(f"rank-deficient: {a!r} / swapped {b!r}")
    assert isinstance(a, float) and np.isfinite(a) and np.isfinite(b)
    assert a >= -1e-9 * (np.trace(s1) + np.trace(s2))
    assert abs(a - b) <= 1e-10 * abs(a)
    for mu, s in ((m1, s1), (m2, s2), Fc.gaussian_moments(400, 32, 1, 0.0, 1.0)):
        assert abs(S.frechet_distance(mu, s, mu, s)) <= 1e-9 * np.trace(s)


def test_frechet_distance_against_the_singular_values_of_the_cross_matrix(S):
    """features of fewer rows than columns: tr sqrtm(S1 S2) is the nuclear norm of the small cross matrix of the centred rows, which
    takes no square root of a noisy zero; 12 and 14 rows of width 256"""
    rng = np.random.default_rng(5)
    fp = rng.standard_normal((12, 256)) * (0.5 + rng.random(256))
    fg = rng.standard_normal((14, 256)) * (0.5 + rng.random(256)) + 0.3
    got = S.frechet_distance(fp.mean(0), np.cov(fp, rowvar=False), fg.mean(0), np.cov(fg, rowvar=False))
    want = Fc.frechet_svd(fp, fg)
    assert abs(got - want) <= 1e-11 * abs(want), (got, want)
    assert abs(Fc.frechet_eig(fp.mean(0), np.cov(fp, rowvar=False), fg.mean(0), np.cov(fg, rowvar=False)) - want) <= 1e-11 * abs(want)


# ---------------------------------------------------------------------------------------------------------- KID
def test_kid_subsets_are_torch_fidelitys(S):
    ix, iy = S.kid_subsets(9, 11, 5, 3)
    assert ix.dtype == np.int32 and iy.dtype == np.int32 and ix.shape == (3, 5) and iy.shape == (3, 5)
    assert ix.tolist() == Fc.SUBSETS_9_11_5_3[0] == [[2, 4, 7, 1, 5], [1, 2, 8, 7, 4], [1, 0, 3, 2, 4]]
    assert iy.tolist() == Fc.SUBSETS_9_11_5_3[1] == [[6, 9, 7, 4, 5], [0, 3, 10, 6, 8], [5, 0, 9, 10, 6]]
    rng = np.random.RandomState(2020)
    for s in range(3):
        assert np.array_equal(ix[s], rng.choice(9, 5, replace=False)) and np.array_equal(iy[s], rng.choice(11, 5, replace=False))
    dx, dy = Fc.draw_subsets(9, 11, 5, 3)
    assert np.array_equal(dx, ix) and np.array_equal(dy, iy)
    for bad in ((9, 11, 10, 3), (12, 8, 9, 1)):
        with pytest.raises(ValueError) as e:
            S.kid_subsets(*bad)
        assert str(bad[0]) in str(e.value) and str(bad[1]) in str(e.value)
    assert S.KID_SUBSETS == 100 and S.KID_SUBSET_SIZE == 1000 and S.KID_SEED == 2020


def test_kid_against_direct_indexing(S):
    rng = np.random.default_rng(2)
    X, Y = rng.standard_normal((9, 64)), rng.standard_normal((11, 64)) + 0.2
    Kxx, Kyy, Kxy = Fc.poly64(X, X), Fc.poly64(Y, Y), Fc.poly64(X, Y)
    ix, iy = S.kid_subsets(9, 11, 5, 3)
    mean, std = S.kid(Fc.subset_sums64(Kxx, Kyy, Kxy, ix, iy), 5)
    want_mean, want_std = Fc.kid64(Kxx, Kyy, Kxy, ix, iy)
    assert mean == pytest.approx(want_mean, rel=1e-12, abs=1e-15) and std == pytest.approx(want_std, rel=1e-12, abs=1e-15)
    assert std > 0
    one = S.kid(Fc.subset_sums64(Kxx, Kyy, Kxy, ix[:1], iy[:1]), 5)
    assert one[1] == 0.0 and one[0] == pytest.approx(Fc.kid64(Kxx, Kyy, Kxy, ix[:1], iy[:1])[0], rel=1e-12)


# ---------------------------------------------------------------------------------------------------------- evaluate.py
def _tree(tmp_path, n_pred=4, n_gt=5, size=(48, 64)):
    from PIL import Image
    rng = np.random.default_rng(5)
    gt, pr = tmp_path / "gt", tmp_path / "pred"
    gt.mkdir()
    pr.mkdir()
    for i in range(n_gt):
        Image.fromarray(rng.integers(0, 256, (size[1], size[0], 3), dtype=np.uint8)).save(gt / f"{i:05d}_00.jpg")
    names = []
    for i in range(n_pred):
        nm = f"{i:05d}_00_{(i + 1) % n_pred:05d}_00.png"
        Image.fromarray(rng.integers(0, 256, (size[1], size[0], 3), dtype=np.uint8)).save(pr / nm, format="JPEG")
        names.append(nm)
    return gt, pr, names


def _pair_stub(seen):
    def scorer(batch):
        seen.extend(batch)
        return [(0.5, 0.01, 0.2)] * len(batch)
    return scorer


class _FidStub:
    """stands in for evaluate.FidScorer: the feature of an image is its 2 x 2 x 3 block means (12 numbers) in float32, the banks
    live on the host, and the statistics are the restatement's"""

    def __init__(self):
        self.seen, self.banks = [], []

    def bank(self, n):
        self.banks.append(np.full((n, 12), np.nan, np.float32))
        return self.banks[-1]

    def fill(self, bank, row0, batch):
        for j, it in enumerate(batch):
            self.seen.append(it)
            img = it["img"].astype(np.float64) / 255.0
            h, w = img.shape[0] // 2, img.shape[1] // 2
            bank[row0 + j] = [img[a * h:(a + 1) * h, b * w:(b + 1) * w, c].mean() for a in range(2) for b in range(2) for c in range(3)]

    def score(self, bank_pred, bank_gt, subsets, subset_size):
        return Fc.fid_kid64(bank_pred, bank_gt, subsets, subset_size)


def test_evaluate_fid_flags():
    ev = _evaluate()
    o = ev.get_opt([])
    assert o.fid is False and o.fid_only is False and o.fid_random_init is False
    assert (o.kid_subsets, o.kid_subset_size) == (100, 1000)
    assert o.fid_inception_weights.endswith(os.path.join("checkpoints", "pt_inception-2015-12-05-6726825d.pth"))
    o = ev.get_opt(["--fid", "--fid_only", "--fid_random_init", "--kid_subsets", "7", "--kid_subset_size", "33",
                    "--fid_inception_weights", "w.pth"])
    assert (o.fid, o.fid_only, o.fid_random_init, o.kid_subsets, o.kid_subset_size, o.fid_inception_weights) == \
        (True, True, True, 7, 33, "w.pth")
    for bad in (["--kid_subsets", "0"], ["--kid_subset_size", "1"]):
        with pytest.raises(SystemExit):
            ev.get_opt(bad)


@pytest.mark.parametrize("flag", ["--fid", "--fid_only"])
def test_oversize_subset_is_an_argparse_error_naming_both_counts(tmp_path, capsys, flag):
    ev = _evaluate()
    gt, pr, _ = _tree(tmp_path, n_pred=4, n_gt=7)
    argv = ["--predict_dir", str(pr), "--ground_truth_dir", str(gt), "-j", "0", flag]
    for extra in ([], ["--kid_subset_size", "5"]):       # the default of 1000, and one between the two counts
        with pytest.raises(SystemExit) as e:
            ev.main(argv + extra, scorer=_pair_stub([]), fid_scorer=_FidStub())
        assert e.value.code == 2
        err = capsys.readouterr().err
        assert "--kid_subset_size" in err and "4 predictions" in err and "7 ground truths" in err and "usage:" in err


def test_without_fid_eval_txt_has_exactly_todays_lines(tmp_path, capsys):
    ev = _evaluate()
    gt, pr, names = _tree(tmp_path, n_pred=4, n_gt=4)
    before = set(sys.modules)
    res = ev.main(["--predict_dir", str(pr), "--ground_truth_dir", str(gt), "-j", "0", "-b", "3",
                   "--inception_weights", str(tmp_path / "none.pth")], scorer=_pair_stub([]))
    assert (pr / "eval.txt").read_bytes() == b"SSIM : 0.5 / MSE : 0.01 / LPIPS : 0.2\nIS_mean : nan / IS_std : nan\n"
    assert (pr / "lpips.txt").read_text().splitlines() == [f"{nm} 0.2" for nm in sorted(names)]
    assert set(res) == {"ssim", "mse", "lpips", "is_mean", "is_std", "pairs", "timings"}
    assert set(res["timings"]) == {"loader_wait_s", "gpu_s", "total_s"}
    assert "FID" not in capsys.readouterr().out
    assert not {m for m in set(sys.modules) - before if m.endswith("feat_stats")}      # nothing new is imported


def _fid_line(line):
    parts = line.split(" / ")
    assert len(parts) == 3 and parts[0].startswith("FID : ") and parts[1].startswith("KID_mean : ") and \
        parts[2].startswith("KID_std : "), line
    return float(parts[0][6:]), float(parts[1][11:]), float(parts[2][10:])


def test_fid_with_a_stand_in_scorer_adds_one_line(tmp_path, capsys):
    from PIL import Image
    ev = _evaluate()
    gt, pr, names = _tree(tmp_path, n_pred=6, n_gt=8)
    (pr / "notes.txt").write_text("not an image")
    (gt / "notes.txt").write_text("not an image")
    stub = _FidStub()
    argv = ["--predict_dir", str(pr), "--ground_truth_dir", str(gt), "-j", "0", "-b", "4", "--kid_subsets", "3", "--kid_subset_size", "5",
            "--inception_weights", str(tmp_path / "none.pth")]
    res = ev.main(argv + ["--fid"], scorer=_pair_stub([]), fid_scorer=stub)
    lines = (pr / "eval.txt").read_text().splitlines()
    # (the paired averages keep the reference's division by the number of files in the ground-truth folder: 9 here)
    assert len(lines) == 3 and lines[0] == f"SSIM : {sum([0.5] * 6) / 9} / MSE : {sum([0.01] * 6) / 9} / LPIPS : {sum([0.2] * 6) / 9}"
    assert lines[1] == "IS_mean : nan / IS_std : nan"
    got = _fid_line(lines[2])
    assert got == (res["fid"], res["kid_mean"], res["kid_std"]) and res["fid_images"] == [6, 8] and res["pairs"] == 6
    assert "FID : %f / KID_mean : %f / KID_std : %f" % got in capsys.readouterr().out
    # every image of both folders, in sorted order, full size, decoded only (no resize at --resolution 1024), non-images skipped
    gt_names = sorted(f for f in os.listdir(gt) if f.endswith(".jpg"))
    assert [it["name"] for it in stub.seen] == sorted(names) + gt_names
    for it in stub.seen:
        folder = pr if it["name"] in names else gt
        assert np.array_equal(it["img"], np.asarray(Image.open(folder / it["name"]).convert("RGB"))) and it["img"].shape == (64, 48, 3)
    assert [b.shape for b in stub.banks] == [(6, 12), (8, 12)] and not np.isnan(stub.banks[0]).any() and not np.isnan(stub.banks[1]).any()
    want = Fc.fid_kid64(stub.banks[0], stub.banks[1], 3, 5)
    assert got == pytest.approx(want, rel=1e-12) and {"fid_features_s", "fid_stats_s"} <= set(res["timings"])
    import json
    json.dumps(res["timings"])
    # --fid_only: the one line (labelled under --fid_random_init), no pairing -- the pair scorer is never called --, lpips.txt untouched
    lp = (pr / "lpips.txt").read_bytes()
    seen_pairs, stub2 = [], _FidStub()
    res2 = ev.main(argv + ["--fid_only", "--fid_random_init"], scorer=_pair_stub(seen_pairs), fid_scorer=stub2)
    lines = (pr / "eval.txt").read_text().splitlines()
    assert len(lines) == 5 and lines[3] == lines[2] and lines[4] == "FID Inception weights : random init (plumbing only)"
    assert seen_pairs == [] and (pr / "lpips.txt").read_bytes() == lp
    assert set(res2) == {"fid", "kid_mean", "kid_std", "fid_images", "timings"} and res2["fid"] == res["fid"]
    # ground truths follow --resolution as in the paired path
    stub3 = _FidStub()
    ev.main(argv + ["--fid_only", "--resolution", "256"], fid_scorer=stub3)
    assert [it["img"].shape for it in stub3.seen] == [(64, 48, 3)] * 6 + [(256, 192, 3)] * 8


def test_fid_without_weights_writes_nan(tmp_path, capsys):
    ev = _evaluate()
    gt, pr, _ = _tree(tmp_path, n_pred=4, n_gt=4)
    res = ev.main(["--predict_dir", str(pr), "--ground_truth_dir", str(gt), "-j", "0", "--fid_only", "--kid_subset_size", "4",
                   "--fid_inception_weights", str(tmp_path / "none.pth")])
    assert (pr / "eval.txt").read_text() == "FID : nan / KID_mean : nan / KID_std : nan\n"
    assert all(np.isnan(res[k]) for k in ("fid", "kid_mean", "kid_std"))
    out = capsys.readouterr()
    assert "--fid_inception_weights" in out.err and "nothing is downloaded" in out.err and "FID : nan" in out.out
    assert not (pr / "lpips.txt").exists()


def test_product_modules_import_neither_tests_nor_scipy():
    src = "".join(open(os.path.join(ROOT, *p)).read() for p in (("hr-viton_amd", "feat_stats.py"), ("hr-viton_amd", "inception.py"),
                                                                  ("evaluate.py",)))
    assert "scipy" not in src.replace("scipy.stats.entropy", "") and "fid_cases" not in src and "from tests" not in src
    assert "import oracle" not in src and "from oracle" not in src
