"""CPU (no GPU needed): the Inception-v3 table and state-dict layout of hr_viton_amd/inception.py against the independent statement
of tests/inception_cases.py, ConvLayer's horizontal padding on the host side, the Inception Score against scipy, and evaluate.py's
Inception flags, data path and output files with the GPU work stubbed."""
import os
import sys

import numpy as np
import pytest
import torch

import inception_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _evaluate():
    import importlib
    return importlib.import_module("evaluate")


@pytest.fixture(scope="module")
def net():
    import hr_viton_amd  # noqa: F401
    from hr_viton_amd.inception import Inception3
    torch.manual_seed(0)
    return Inception3()


# ---------------------------------------------------------------------------------------------------------- the table
def test_table_counts():
    assert len(K.UNITS) == 94 and len({u[0] for u in K.UNITS}) == 94
    assert K.param_count() == 23_834_568
    assert K.param_count(aux=True) == 27_161_264          # the number torchvision documents for inception_v3
    assert K.param_count(aux=True) - K.param_count() == 3_326_696
    # every horizontal-padding unit is a 1xK / Kx1 pair member with 'same' output
    for name, _, _, (kh, kw), s, (ph, pw) in K.UNITS:
        if kh != kw:
            assert s == 1 and (ph, pw) == (kh // 2, kw // 2) and {kh, kw} in ({1, 7}, {1, 3}), name


def test_restatement_tap_shapes():
    """the float64 forward at 299x299: 35 / 35 / 17 / 8 with 192 / 288 / 768 / 2048 channels, logits [N, 1000]"""
    sd = K.raw_weights(1)
    taps = {}
    with torch.no_grad():
        logits = K.forward(sd, K.normalize_u8(K.images(1, 3)), torch.float64, taps=taps)
    assert tuple(logits.shape) == (1, 1000) and logits.dtype == torch.float64
    for name, (c, hw) in K.TAPS_299.items():
        assert tuple(taps[name].shape) == (1, c, hw, hw), (name, taps[name].shape)


def test_module_matches_table(net):
    assert set(net.state_dict().keys()) == K.state_keys()
    units = dict(net.units())
    assert len(units) == 94
    for name, cin, cout, k, s, p in K.UNITS:
        conv, bn = units[name].conv, units[name].bn
        assert tuple(conv.weight.shape) == (cout, cin, *k) and conv.bias is None, name
        assert conv.stride == (s, s) and conv.padding == p and bn.eps == 0.001, name
    assert tuple(net.fc.weight.shape) == (1000, 2048)
    assert sum(p.numel() for p in net.parameters()) == 23_834_568
    assert not net.training and not any(p.requires_grad for p in net.parameters())


def test_state_dict_loading(net):
    import hr_viton_amd  # noqa: F401
    from hr_viton_amd.inception import Inception3, inception_v3
    sd = K.raw_weights(2)
    assert set(sd) == K.state_keys()
    full = dict(sd)
    for name, cin, cout, (kh, kw), _, _ in K.AUX_UNITS:       # torchvision's file carries the AuxLogits branch
        full[f"{name}.conv.weight"] = torch.zeros(cout, cin, kh, kw)
        for k in K.BN_KEYS:
            full[f"{name}.bn.{k}"] = torch.zeros(cout) if k != "num_batches_tracked" else torch.tensor(0)
    full["AuxLogits.fc.weight"], full["AuxLogits.fc.bias"] = torch.zeros(1000, 768), torch.zeros(1000)
    assert set(full) == K.state_keys(aux=True)
    m = Inception3()
    m.load_state_dict(full)
    got = m.state_dict()
    for k in ("Mixed_6c.branch7x7dbl_3.conv.weight", "Mixed_7b.branch3x3_2b.bn.running_var", "fc.bias", "Conv2d_1a_3x3.bn.weight"):
        assert torch.equal(got[k], sd[k]), k
    for gone in ("Mixed_5b.branch1x1.conv.weight", "Mixed_7c.branch_pool.bn.running_mean", "fc.weight"):
        part = {k: v for k, v in full.items() if k != gone}
        with pytest.raises(KeyError) as e:
            Inception3().load_state_dict(part)
        assert gone in str(e.value)
    # BatchNorm folding: float64 on the host, y = conv * scale + shift
    u = dict(m.units())["Mixed_6c.branch7x7dbl_3"]
    w, scale, shift = u.folded()
    want = sd["Mixed_6c.branch7x7dbl_3.bn.weight"].double() / torch.sqrt(sd["Mixed_6c.branch7x7dbl_3.bn.running_var"].double() + 1e-3)
    assert torch.equal(scale, want.float()) and scale.dtype == torch.float32 and torch.equal(w, sd["Mixed_6c.branch7x7dbl_3.conv.weight"])
    # eval only; transform_input=True and pretrained=True are refused; CPU tensors raise
    with pytest.raises(NotImplementedError):
        m.train()
    assert m.eval() is m
    with pytest.raises(NotImplementedError):
        Inception3(transform_input=True)
    with pytest.raises(NotImplementedError):
        inception_v3(pretrained=True)
    from hr_viton_amd._lib import HrvError
    with pytest.raises(HrvError):
        m(torch.zeros(1, 3, 299, 299))
    with pytest.raises(HrvError):
        m.forward_u8(torch.zeros(1, 299, 299, 3, dtype=torch.uint8))


def test_block_slices_are_engine_aligned(net):
    """every branch offset of every block is a multiple of 4 (the fp32 engine's out_coff granule), widths as the table says"""
    want_out = {"Mixed_5b": 256, "Mixed_5c": 288, "Mixed_5d": 288, "Mixed_6a": 768, "Mixed_6b": 768, "Mixed_6c": 768, "Mixed_6d": 768,
                "Mixed_6e": 768, "Mixed_7a": 1280, "Mixed_7b": 2048, "Mixed_7c": 2048}
    for name in K.BLOCKS:
        blk = getattr(net, name)
        assert blk.cout == want_out[name] and all(o % 4 == 0 for o in blk.offsets()), (name, blk.offsets())
    assert net.Mixed_7b.widths == [320, 768, 768, 192] and net.Mixed_6a.widths == [384, 96, 288]


# ---------------------------------------------------------------------------------------------------------- ConvLayer(pad_w=...)
def test_convlayer_pad_w_host_side():
    import hr_viton_amd  # noqa: F401
    from hr_viton_amd import ops
    from hr_viton_amd.conv_dispatch import engine_tile, patch_tile
    w17, w71 = torch.zeros(8, 4, 1, 7), torch.zeros(8, 4, 7, 1)
    a = ops.ConvLayer(w17, [4], "cpu", pad=0, pad_w=3)
    b = ops.ConvLayer(w71, [4], "cpu", pad=3, pad_w=0)
    assert a.out_hw(17, 13) == (17, 13) and b.out_hw(17, 13) == (17, 13)
    assert ops.ConvLayer(w17, [4], "cpu", pad=0).out_hw(17, 13) == (17, 7)           # without it: pad in both directions
    assert a.flops(2, 17, 13) == 2.0 * 2 * 17 * 13 * 8 * 4 * 7
    sq = ops.ConvLayer(torch.zeros(8, 4, 3, 3), [4], "cpu", pad=1)
    assert sq.pad_w is None and sq.out_hw(9, 9) == ops.ConvLayer(torch.zeros(8, 4, 3, 3), [4], "cpu", pad=1, pad_w=1).out_hw(9, 9)
    # the one dispatch gate that reads "pad == 1" as 'same' in both directions: the LDS-resident patch tile
    args = (True, 3, 3, 1, 1, 1, 0, 128, 128, 4, 1024, 768)
    assert patch_tile(*args) == 17 and patch_tile(*args, pad_w=1) == 17 and patch_tile(*args, pad_w=0) == 0
    assert patch_tile(*args, pad_w=2) == 0
    e = ("serve", 4 * 1024 * 768, 128, True, 3, 3, 1, 1, 1, 0, 128, 4, 1024, 768)
    assert engine_tile(*e) == 17 and engine_tile(*e, pad_w=1) == 17 and engine_tile(*e, pad_w=0) not in (16, 17, 18, 19)
    # fp32 sources: the tile is hrv_conv2d_pick_tile's whatever the padding
    f = ("serve", 16 * 17 * 17, 192, False, 1, 7, 1, 0, 1, 0, 160, 16, 17, 17)
    assert engine_tile(*f) == engine_tile(*f, pad_w=3)


# ---------------------------------------------------------------------------------------------------------- the score
def _probs(rng, n, zeros=False):
    p = rng.random((n, 1000)) ** 6
    if zeros:
        p[0, :400] = 0.0
        p[:, 7] = 0.0            # a class nobody predicts: q == 0 there too
    return p / p.sum(axis=1, keepdims=True)


@pytest.mark.parametrize("splits", [1, 2])
def test_inception_score_matches_scipy(splits):
    entropy = pytest.importorskip("scipy.stats").entropy
    ev = _evaluate()
    rng = np.random.default_rng(4)
    for preds in (_probs(rng, 9), _probs(rng, 10, zeros=True), _probs(rng, 6) * 0.5):      # unnormalised rows: entropy normalises
        n = preds.shape[0] // splits
        want = []
        for k in range(splits):
            part = preds[k * n:(k + 1) * n]
            py = np.mean(part, axis=0)
            want.append(np.exp(np.mean([entropy(part[i], py) for i in range(part.shape[0])])))
        got = ev.inception_score(preds, splits)
        assert got[0] == pytest.approx(np.mean(want), rel=1e-12) and got[1] == pytest.approx(np.std(want), rel=1e-9, abs=1e-15)
        assert K.score64(preds, splits) == pytest.approx(got, rel=1e-12, abs=1e-15)
        assert np.isfinite(got[0]) and got[0] >= 1.0
    if splits == 1:
        assert ev.inception_score(_probs(rng, 5))[1] == 0.0
    assert all(np.isnan(v) for v in ev.inception_score(np.zeros((0, 1000)), splits))


# ---------------------------------------------------------------------------------------------------------- evaluate.py
def test_evaluate_inception_flags():
    ev = _evaluate()
    o = ev.get_opt([])
    assert o.inception_weights.endswith(os.path.join("checkpoints", "inception_v3_google-0cc3c7bd.pth"))
    assert o.inception_random_init is False and o.is_splits == 1 and o.seed == 0
    o = ev.get_opt(["--inception_weights", "w.pth", "--inception_random_init", "--is_splits", "3", "--seed", "7"])
    assert (o.inception_weights, o.inception_random_init, o.is_splits, o.seed) == ("w.pth", True, 3, 7)
    with pytest.raises(SystemExit):
        ev.get_opt(["--is_splits", "0"])
    assert ev.INCEPTION_FILES == ("inception_v3_google-0cc3c7bd.pth", "inception_v3_google-1a9a5a14.pth")


def test_default_inception_weights_prefers_the_file_that_exists(tmp_path, monkeypatch):
    ev = _evaluate()
    monkeypatch.setattr(torch.hub, "get_dir", lambda: str(tmp_path))
    (tmp_path / "checkpoints").mkdir()
    assert ev.get_opt([]).inception_weights == str(tmp_path / "checkpoints" / ev.INCEPTION_FILES[0])
    (tmp_path / "checkpoints" / ev.INCEPTION_FILES[1]).write_bytes(b"")
    assert ev.get_opt([]).inception_weights == str(tmp_path / "checkpoints" / ev.INCEPTION_FILES[1])
    (tmp_path / "checkpoints" / ev.INCEPTION_FILES[0]).write_bytes(b"")
    assert ev.get_opt([]).inception_weights == str(tmp_path / "checkpoints" / ev.INCEPTION_FILES[0])


def _tree(tmp_path, n=4, size=(48, 64), extra_gt=0):
    from PIL import Image
    rng = np.random.default_rng(5)
    gt, pr = tmp_path / "gt", tmp_path / "pred"
    gt.mkdir()
    pr.mkdir()
    names = []
    for i in range(n + extra_gt):
        Image.fromarray(rng.integers(0, 256, (size[1], size[0], 3), dtype=np.uint8)).save(gt / f"{i:05d}_00.jpg")
    for i in range(n):
        nm = f"{i:05d}_00_{(i + 1) % n:05d}_00.png"
        Image.fromarray(rng.integers(0, 256, (size[1], size[0], 3), dtype=np.uint8)).save(pr / nm, format="JPEG")
        names.append(nm)
    return gt, pr, names


def _pair_stub(seen):
    def scorer(batch):
        seen.extend(batch)
        return [(0.5, 0.01, 0.2)] * len(batch)
    return scorer


def test_evaluate_without_weights_writes_the_nan_line(tmp_path, capsys):
    ev = _evaluate()
    gt, pr, _ = _tree(tmp_path)
    seen = []
    res = ev.main(["--predict_dir", str(pr), "--ground_truth_dir", str(gt), "-j", "0", "-b", "3",
                   "--inception_weights", str(tmp_path / "none.pth")], scorer=_pair_stub(seen))
    assert (pr / "eval.txt").read_bytes().splitlines()[1] == b"IS_mean : nan / IS_std : nan"
    assert len((pr / "eval.txt").read_text().splitlines()) == 2
    assert all("pred299" not in it for it in seen) and len(seen) == 4        # the 299x299 resize is not paid for
    assert np.isnan(res["is_mean"]) and np.isnan(res["is_std"]) and "inception_preds" not in res["timings"]
    out = capsys.readouterr()
    assert "Inception" in out.err and "IS_mean : nan / IS_std : nan" in out.out


def test_evaluate_with_stubbed_inception_scorer(tmp_path, capsys):
    ev = _evaluate()
    from PIL import Image
    gt, pr, names = _tree(tmp_path, n=4, extra_gt=1)
    rng = np.random.default_rng(8)
    table = {nm: _probs(rng, 1)[0] for nm in names}
    seen, seen_is = [], []

    def is_scorer(batch):
        seen_is.extend(batch)
        return np.stack([table[it["name"]] for it in batch]).astype(np.float32)

    argv = ["--predict_dir", str(pr), "--ground_truth_dir", str(gt), "-j", "0", "-b", "3"]
    res = ev.main(argv + ["--inception_random_init"], scorer=_pair_stub(seen), is_scorer=is_scorer)
    assert [it["name"] for it in seen_is] == sorted(names)
    for it in seen_is:
        assert it["pred299"].shape == (299, 299, 3) and it["pred299"].dtype == np.uint8
        want = np.asarray(Image.open(pr / it["name"]).resize((299, 299), Image.BILINEAR))
        assert np.array_equal(it["pred299"], want)
    want_mean, want_std = K.score64(np.stack([table[nm] for nm in sorted(names)]).astype(np.float32), 1)
    assert res["is_mean"] == pytest.approx(want_mean, rel=1e-12) and res["is_std"] == 0.0 and want_std == 0.0
    lines = (pr / "eval.txt").read_text().splitlines()
    assert lines[1] == f"IS_mean : {res['is_mean']} / IS_std : 0.0" and float(lines[1].split(" / ")[0][10:]) == res["is_mean"]
    assert lines[2] == "Inception weights : random init (plumbing only)" and len(lines) == 3
    assert "inception_preds" not in res["timings"] and res["timings"]["inception_s"] >= 0.0
    import json
    json.dumps(res["timings"])                  # tools/eval_bench.py prints them
    err = capsys.readouterr().err
    assert "Inception Score is computed over the 4 predictions" in err and "(5)" in err
    # two splits, no label without the flag, no note when the counts agree
    (gt / "00004_00.jpg").unlink()
    res2 = ev.main(argv + ["--is_splits", "2"], scorer=_pair_stub([]), is_scorer=is_scorer)
    m2, s2 = K.score64(np.stack([table[nm] for nm in sorted(names)]).astype(np.float32), 2)
    assert res2["is_mean"] == pytest.approx(m2, rel=1e-12) and res2["is_std"] == pytest.approx(s2, rel=1e-9) and s2 > 0
    lines = (pr / "eval.txt").read_text().splitlines()
    assert lines[4] == f"IS_mean : {res2['is_mean']} / IS_std : {res2['is_std']}" and len(lines) == 5
    assert "Inception Score is computed over" not in capsys.readouterr().err


def test_evaluation_keeps_its_return_shape(tmp_path):
    """tools/eval_bench.py unpacks five values"""
    ev = _evaluate()
    gt, pr, names = _tree(tmp_path, n=2)
    opt = ev.get_opt(["--predict_dir", str(pr), "--ground_truth_dir", str(gt), "-j", "0"])
    out = ev.evaluation(opt, ev.list_predictions(str(pr)), sorted(os.listdir(gt)), _pair_stub([]))
    assert len(out) == 5 and set(out[4]) == {"loader_wait_s", "gpu_s"}
    out = ev.evaluation(opt, ev.list_predictions(str(pr)), sorted(os.listdir(gt)), _pair_stub([]),
                        is_scorer=lambda b: np.full((len(b), 1000), 1e-3))
    assert len(out) == 5 and out[4]["inception_preds"].shape == (2, 1000) and out[4]["inception_preds"].dtype == np.float64


def test_product_modules_import_neither_oracle_nor_tests():
    src = open(os.path.join(ROOT, "hr-viton_amd", "inception.py")).read() + open(os.path.join(ROOT, "evaluate.py")).read()
    assert "import oracle" not in src and "from oracle" not in src and "from tests" not in src and "import tests" not in src
    assert "inception_cases" not in src
