"""CPU (no GPU needed): the host side of the validation passes -- the case tables' own conditions, the IoU ratio, the schedule
predicate, the scalar log, the scripts' flags, and the C entry points' argument checks."""
import json
import math
import os
import sys
import types

import pytest
import torch
import torch.nn.functional as F

import validate_cases as VC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _validate():
    import hr_viton_amd  # noqa: F401
    from hr_viton_amd import validate
    return validate


# ----------------------------------------------------------------------------------------- the case tables
@pytest.mark.parametrize("comp", VC.COMPOSITIONS)
def test_small_case_keeps_its_margin_and_fp32_softmax_decides_alike(comp):
    _, seed, N, h, w = VC.SMALL
    seg, cm, label = VC.iou_inputs(seed, N, h, w)
    m = VC.margin64(seg, cm, comp)
    print(f"margin {comp}: {m:.3e}")
    assert m > VC.MARGIN
    # the figures the case table quotes (3.5e-4 / 7.2e-5 / 3.0e-4), to two digits
    want = {"no_composition": 3.5e-4, "detach": 7.2e-5, "warp_grad": 3.0e-4}[comp]
    assert abs(m - want) < 0.05 * want, (m, want)
    p32 = F.softmax(VC.compose64(seg, cm, comp).float(), dim=1)
    assert torch.equal(VC.counts_from_probs(p32, label), VC.iou_counts64(seg, cm, label, comp))


def test_large_case_seed_keeps_its_margin():
    _, seed, N, h, w = VC.LARGE
    seg, cm, label = VC.iou_inputs(seed, N, h, w)
    for comp in VC.COMPOSITIONS:
        m = VC.margin64(seg, cm, comp)
        print(f"margin {comp}: {m:.3e}")
        assert m > VC.MARGIN
    c = VC.iou_counts64(seg, cm, label, "warp_grad")
    assert (c[:, 0] > h * w // 4).all() and (c[:, 2] == h * w).all(), c       # the intersection is not near zero


def test_labels_are_one_hot_and_half_follow_the_argmax():
    _, seed, N, h, w = VC.SMALL
    seg, cm, label = VC.iou_inputs(seed, N, h, w)
    assert torch.equal(label.sum(1), torch.ones(N, h, w)) and set(label.unique().tolist()) == {0.0, 1.0}
    top = VC.compose64(seg, cm, "warp_grad").argmax(1)
    share = (label.argmax(1) == top).float().mean().item()
    assert 0.45 < share < 0.65, share          # 1/2 + 1/2 * 1/13 expected


def test_restatement_on_the_hand_case():
    seg, label, cm_keep, cm_drop = VC.hand_case()
    for comp in VC.COMPOSITIONS:
        assert VC.iou_counts64(seg, cm_keep, label, comp).tolist() == [[1, 1, 2]], comp
    assert VC.iou64(torch.tensor([[1, 1, 2]])).item() == pytest.approx(0.5, abs=1e-7)
    assert VC.iou_counts64(seg, cm_drop, label, "warp_grad").tolist() == [[0, 0, 2]]
    assert VC.iou_counts64(seg, cm_drop, label, "detach").tolist() == [[0, 0, 2]]
    assert VC.iou_counts64(seg, cm_drop, label, "no_composition").tolist() == [[1, 1, 2]]


def test_mutants_of_the_restatement_are_told_apart():
    seg, cm, label = VC.tie_case()
    strict = VC.iou_counts64(seg, cm, label, "warp_grad")
    loose = VC.iou_counts64(seg, cm, label, "warp_grad", strict=False)
    assert strict.tolist() == [[1, 1, 2]] and loose.tolist() == [[2, 3, 2]]         # '>=' counts both tied channels
    _, seed, N, h, w = VC.SMALL
    seg, cm, label = VC.iou_inputs(seed, N, h, w)
    full = VC.iou_counts64(seg, cm, label, "warp_grad")
    dropped = VC.iou_counts64(seg, cm, label, "warp_grad", composed=False)
    assert not torch.equal(full, dropped)
    assert torch.equal(dropped, VC.iou_counts64(seg, cm, label, "no_composition"))


def test_perfect_case_has_iou_one():
    seg, cm, label = VC.perfect_case()
    c = VC.iou_counts64(seg, cm, label, "warp_grad")
    assert torch.equal(c[:, 0], c[:, 1]) and torch.equal(c[:, 1], c[:, 2])
    assert torch.allclose(VC.iou64(c), torch.ones(2, dtype=torch.float64), atol=1e-12)


def test_resize_restatement_agrees_with_torch_fp32():
    """the float64 restatement and torch's fp32 CPU path are the same function: their distance is fp32 rounding, at every size"""
    for H, W in VC.RESIZE_SIZES:
        a, _ = VC.resize_inputs(1, H, W)
        d = (VC.prep_resized_torch_f32(a).double() - VC.prep_resized64(a)).abs().max().item()
        print(f"torch fp32 vs float64 at {H}x{W}: {d:.3e}")
        assert d < 5e-6, (H, W, d)          # values reach (1 + 0.188) / 0.448 = 2.7: a few ulp of 2^1


def test_tocg_case_oracle_alone_stays_inside_the_exempt_share():
    """the GPU test's condition on its case, checked with the oracle alone: fp32 against float64, tau = 8 x their largest
    probability difference, exempt share <= 0.5 %, and the case is decisive (thousands of predictions per sample)"""
    opt, m, batches = VC.tocg_case()
    assert m.training
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    for b in batches:
        p64 = VC.tocg_probs_oracle(sd, b, opt.clothmask_composition)
        p32 = VC.tocg_probs_oracle(sd, b, opt.clothmask_composition, torch.float32)
        tau, exempt, share = VC.exempt_stats(p32, p64, b["parse"])
        want = VC.counts_from_probs(p64, b["parse"])
        got = VC.counts_from_probs(p32, b["parse"])
        print(f"tau {tau:.3e} exempt {exempt.tolist()} share {share:.3e} counts {want.tolist()}")
        assert share <= VC.EXEMPT_SHARE and tau < 1e-3
        assert ((got - want).abs() <= exempt[:, None]).all() and (want[:, 1] > 1000).all()


# ----------------------------------------------------------------------------------------- seg_iou / validation_due
def test_seg_iou_on_hand_counts():
    import hr_viton_amd  # noqa: F401
    from hr_viton_amd.metrics import seg_iou
    got = seg_iou(torch.tensor([[1, 1, 2], [0, 5, 7], [0, 0, 4], [3, 3, 3], [0, 0, 0]]))
    assert got.dtype == torch.float64 and got.shape == (5,)
    want = [(1 + 1e-7) / (2 + 1e-7), 1e-7 / (12 + 1e-7), 1e-7 / (4 + 1e-7), 1.0, 1.0]
    assert got.tolist() == pytest.approx(want, rel=1e-12)
    assert torch.equal(got, VC.iou64(torch.tensor([[1, 1, 2], [0, 5, 7], [0, 0, 4], [3, 3, 3], [0, 0, 0]])))
    assert "fp32" in seg_iou.__doc__ and "reference" in seg_iou.__doc__


def test_validation_due_edges():
    due = _validate().validation_due
    assert not any(due(s, 0) for s in range(5)) and not due(0, -3)
    assert all(due(s, 1) for s in range(5))
    assert due(999, 1000) and not due(998, 1000) and not due(1000, 1000) and due(1999, 1000)
    assert due(1, 2) and not due(0, 2) and not due(2, 2)


# ----------------------------------------------------------------------------------------- ScalarLog
def test_scalar_log_writes_jsonl_and_nothing_before_the_first_record(tmp_path, monkeypatch):
    V = _validate()
    monkeypatch.setattr(V, "_summary_writer_class", lambda: None)
    d = tmp_path / "tb" / "run"
    log = V.ScalarLog(str(d))
    assert not d.exists()
    log.add_scalar("val/iou", 0.25, 2)
    log.add_scalar("test/LPIPS", torch.tensor(0.5), 4)
    log.close()
    V.ScalarLog(str(d)).add_scalar("val/iou", 0.75, 6)          # a resumed run appends
    lines = (d / "scalars.jsonl").read_text().splitlines()
    assert [json.loads(ln) for ln in lines] == [{"tag": "val/iou", "value": 0.25, "step": 2},
                                                {"tag": "test/LPIPS", "value": 0.5, "step": 4},
                                                {"tag": "val/iou", "value": 0.75, "step": 6}]
    assert V.read_scalars(str(d))[1]["tag"] == "test/LPIPS" and V.read_scalars(str(tmp_path / "none")) == []


def test_scalar_log_forwards_to_a_summary_writer(tmp_path, monkeypatch):
    V = _validate()
    calls = []

    class SummaryWriter(object):
        def __init__(self, log_dir=None):
            calls.append(("init", log_dir))

        def add_scalar(self, tag, value, step):
            calls.append(("scalar", tag, value, step))

        def close(self):
            calls.append(("close",))

    stand_in = types.ModuleType("tensorboardX")
    stand_in.SummaryWriter = SummaryWriter
    monkeypatch.setitem(sys.modules, "tensorboardX", stand_in)
    d = str(tmp_path / "run")
    log = V.ScalarLog(d)
    log.add_scalar("val/iou", 0.125, 10)
    log.add_scalar("test/LPIPS", 0.5, 20)
    log.close()
    assert calls == [("init", d), ("scalar", "val/iou", 0.125, 10), ("scalar", "test/LPIPS", 0.5, 20), ("close",)]
    assert len(V.read_scalars(d)) == 2


# ----------------------------------------------------------------------------------------- scripts
def test_train_condition_flags():
    import train_condition as tc
    base = tc.get_opt([])
    assert base.val_count == 1000 and base.val_items == 2000 and base.batch_size == 8 and base.tensorboard_dir == "tensorboard"
    assert base.test_dataroot == "./data/" and base.test_data_list == "test_pairs.txt" and base.clothmask_composition == "warp_grad"
    o = tc.get_opt(["--val_count", "2", "--val_items", "4"])
    assert (o.val_count, o.val_items) == (2, 4)
    changed = {k for k in vars(base) if getattr(base, k) != getattr(o, k)}
    assert changed == {"val_count", "val_items"}


def test_train_generator_flags():
    import train_generator as tg
    base = tg.get_opt(["--name", "x"])
    assert base.lpips_count == 1000 and base.val_items == 500 and base.val_batch_size == 1
    assert base.lpips_weights == "./eval_models/weights/v0.1/alex.pth" and base.alexnet_weights is None
    assert base.lpips_random_init is False and base.batch_size == 8 and base.fine_height == 1024 and base.ngf == 64
    o = tg.get_opt(["--name", "x", "--lpips_count", "2", "--val_items", "3", "--val_batch_size", "2", "--lpips_weights", "a.pth",
                    "--alexnet_weights", "b.pth", "--lpips_random_init"])
    changed = {k for k in vars(base) if getattr(base, k) != getattr(o, k)}
    assert changed == {"lpips_count", "val_items", "val_batch_size", "lpips_weights", "alexnet_weights", "lpips_random_init"}


def test_missing_lpips_weights_skip_with_one_note(tmp_path, capsys):
    import train_generator as tg
    V = _validate()
    opt = tg.get_opt(["--name", "x", "--lpips_weights", str(tmp_path / "no.pth"), "--alexnet_weights", str(tmp_path / "no2.pth")])
    assert V.load_validation_lpips(opt) is None
    out = capsys.readouterr().out
    assert out.count("test/LPIPS is skipped") == 1 and "nothing is downloaded" in out
    # the script asks once per run
    v = tg._Validation(opt, "cpu")
    assert v.run(None, None, 1) is None and v.run(None, None, 3) is None
    assert capsys.readouterr().out.count("test/LPIPS is skipped") == 1
    assert not os.path.exists(os.path.join(opt.tensorboard_dir, "x", "scalars.jsonl"))


def test_script_docstrings_name_the_validation_and_its_scope():
    import train_condition as tc
    import train_generator as tg
    assert "val/iou" in tc.__doc__ and "out of scope" in tc.__doc__ and "visualize_segmap" in tc.__doc__
    assert "test/LPIPS" in tg.__doc__ and "make_image_grid" in tg.__doc__
    V = _validate()
    for phrase in ("warped_cm_onehot", "--no_test_visualize", "min(limit, len)", "random variable", "rank 0", "image grids"):
        assert phrase in V.__doc__, phrase


# ----------------------------------------------------------------------------------------- C entry points (host checks only)
@pytest.fixture(scope="module")
def lib():
    import hr_viton_amd  # noqa: F401
    from hr_viton_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from hr_viton_amd import build
        build.build(verbose=False)
    return _lib.load()


def test_entry_points_refuse_bad_arguments(lib):
    import ctypes as C
    one = (C.c_float * 3)(1, 1, 1)
    buf = torch.zeros(64)
    p = buf.data_ptr()
    assert lib.hrv_seg_iou_nchw_f32(None, None, None, 1, 1, 1, 0, None, None) == -1
    assert b"seg_iou" in lib.hrv_last_error()
    assert lib.hrv_seg_iou_nchw_f32(p, None, p, 1, 1, 1, 2, p, None) == -1          # a composition without its mask
    assert lib.hrv_seg_iou_nchw_f32(p, p, p, 1, 1, 1, 3, p, None) == -1             # an unknown composition
    assert lib.hrv_seg_iou_nchw_f32(p, p, p, 0, 1, 1, 0, p, None) == -1
    assert lib.hrv_lpips_prep_resize_nchw_f32(p, None, 1, 1, 1, 128, 128, 0, one, one, p, None) == -1
    assert b"lpips_prep_resize" in lib.hrv_last_error()
    assert lib.hrv_lpips_prep_resize_nchw_f32(p, p, 1, 0, 1, 128, 128, 0, one, one, p, None) == -1
    assert lib.hrv_lpips_prep_resize_nchw_f32(p, p, 1, 4, 4, 128, 128, 0, one, one, p + 4, None) == -1    # float4 stores


def test_front_ends_refuse_cpu_tensors():
    import hr_viton_amd  # noqa: F401
    from hr_viton_amd import metrics
    from hr_viton_amd._lib import HrvError
    seg, cm, label = VC.tie_case()
    with pytest.raises(HrvError):
        metrics.seg_iou_counts(seg, cm, label, "warp_grad")
    with pytest.raises(ValueError):
        metrics.seg_iou_counts(seg, cm, label, "compose")
    assert math.isnan(_validate().condition_validation_iou(types.SimpleNamespace(), torch.nn.Linear(1, 1), [])["iou"])
