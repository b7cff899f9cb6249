"""The JSON line bench.py prints (driver contract).

Round 4's line had grown to 21.8 KB and the driver could not parse it (BENCH_r04.json: parsed = null).  Since round 5 the LAST stdout
line is a compact object under 4 KB (bench.compact_line) and everything else goes to gpurun_out/bench_detail.json.  These tests run the
REAL emit path (bench.summarize -> bench.roofline_obj -> bench.compact_line / bench.emit) on a synthetic full-size result -- the
per-launch records of a step, the largest parity / extra blocks a run has produced (taken from the committed round-4 line) -- and, when
the round's final run is committed (profiles/r05_final_bench_default.json + ..._detail.json), on that."""
import contextlib
import io
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import bench  # noqa: E402

CONTRACT = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
            "data", "config", "roofline", "cpu_baseline")


def _recs():
    """one training iteration's launch records, shaped like the headline's: (kind, name, flops, bytes, ms, kernel)"""
    r = []
    for i in range(31):
        r.append(("conv", f"up_4.norm_{i % 2}.gb.dgrad [spade_gb]", 2.8e11, 6.2e8, 0.31, "conv_p2_kernel"))      # (455 FLOP/B: the family's real ratio)
    for i in range(18):
        r.append(("conv", f"up_{i % 5}.norm_0.conv_shared+gamma|beta [spade_gb]", 5.2e11, 7.5e8, 0.49, "spade_fused_kernel"))
    for i in range(100):
        r.append(("conv", f"G_middle_{i % 2}.conv_{i % 2}", 3.0e10, 4.0e7, 0.05, "conv_mfma_kernel[tile 8]"))
    for i in range(70):
        r.append(("wgrad", f"up_{i % 5}.conv_0.wgrad", 6.0e10, 3.0e8, 0.08, "conv_wgrad_tr_kernel"))
    for i in range(62):
        r.append(("norm_bwd", "spade_norm_bwd", 0.0, 7.0e8, 0.127, "norm_bwd"))
    for i in range(40):
        r.append(("stats", "instnorm_stats", 0.0, 2.0e8, 0.047, "stats"))
    for i in range(800):
        r.append(("ew", "add_slice", 0.0, 1.0e7, 0.004, "ew"))
    r.append(("adam", "adam_f32", 0.0, 3.0e9, 0.6, "adam"))
    return r


def _full():
    recs = _recs()
    res = {"summary": bench.summarize(recs, bench.PEAK_BF16_MFMA_TFLOPS), "peak": bench.PEAK_BF16_MFMA_TFLOPS, "dt": 0.74, "steps": 10,
           "value": 54.0, "ms_per_step": 74.0}
    wl = {"B": 4, "flops_per_img": 8.8e12, "traffic_tag": "train_generator"}
    old = json.load(open(os.path.join(ROOT, "profiles", "r04_final_bench_default.json")))      # the blobs that broke the driver's parser
    full = {"metric": "1024x768 try-on images/sec (train_generator.py step: tocg+glue, G fwd/bwd, D fwd/bwd x2, VGG, Adam)", "value": 54.0,
            "unit": "images/s", "n_gpus": 1, "steps": 10, "warmup": 3, "ms_per_step": 74.0, "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "bf16", "data": "synthetic",
            "config": dict(old["config"]), "roofline": bench.roofline_obj(wl, res, north_star=True),
            "per_kind_ms": {k: {"launches": v[0], "ms": round(v[1], 2)} for k, v in res["summary"]["kinds"].items()},
            "cpu_baseline": old["cpu_baseline"], "parity": old["parity"], "extra": old["extra"]}
    return full


def test_the_line_is_one_line_under_4_kb_and_round_trips():
    full = _full()
    assert len(json.dumps(full)) > 15000          # the input really is a round-4 sized result
    txt = bench.compact_line(full, "gpurun_out/bench_detail.json")
    assert "\n" not in txt and len(txt.encode()) < 4096
    j = json.loads(txt)
    for k in CONTRACT:
        assert k in j, k
    assert j["dtype"] == "bf16" and j["unit"] == "images/s" and j["n_gpus"] == 1 and j["steps"] == 10 and j["warmup"] == 3
    assert j["higher_is_better"] is True and j["scaling"] == "weak" and j["vs_baseline"] is None and j["data"] == "synthetic"
    assert "configs[3]" in j["config"]["workload"] and "model" not in j["config"]
    for k in ("value", "unit", "cores", "kind", "sample", "seconds_per_step"):
        assert k in j["cpu_baseline"], k
    assert len(j["cpu_baseline"]["sample"]) <= 120 and j["cpu_baseline"]["kind"] == "port"
    assert j["detail"] == "gpurun_out/bench_detail.json"
    # worst parity numbers survive: the bf16 discriminator half is the weakest cosine of the round-4 line
    assert abs(j["parity"]["min_cosine"] - 0.9803) < 1e-3
    assert j["parity"]["fp32_engine_vs_oracle"]["image_max_rel_err"] < 1e-3
    for k, e in j["extra"].items():
        assert e["value"] > 0 and e["ms_per_step"] > 0, k


def test_roofline_names_the_kernel_with_the_largest_share_of_the_step():
    full = _full()
    r = full["roofline"]
    # conv_p2: 31 x 0.31 = 9.6 ms; spade_fused: 18 x 0.49 = 8.8 ms -- the best fraction is NOT the dominant kernel
    assert r["kernel"] == "hrv::conv_p2_kernel" and r["bound"] == "mfma" and r["unit"] == "TFLOP/s" and r["peak"] == 2500.0
    assert r["launches_per_step"] == 31 and abs(r["ms_per_step"] - 9.61) < 0.01
    avg_s = r["ms_per_step"] * 1e-3 / r["launches_per_step"]
    assert abs(r["achieved"] - r["algorithmic_flops_per_launch"] / avg_s / 1e12) < 0.01 * r["achieved"]
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3
    sib = {k["kernel"]: k for k in r["kernels"]}
    assert list(sib)[0] == "hrv::spade_fused_kernel" and sib["hrv::spade_fused_kernel"]["frac"] > r["frac"]
    assert sib["hrv::norm_bwd"]["bound"] == "hbm" and sib["hrv::norm_bwd"]["unit"] == "GB/s" and sib["hrv::norm_bwd"]["peak"] == 8000.0
    # the north-star aggregate stays at the top level
    assert r["north_star_set_frac"] == r["spade_3x3_set"]["frac"] > 0
    j = json.loads(bench.compact_line(full))
    assert j["roofline"]["kernel"] == "hrv::conv_p2_kernel" and "spade_fused_kernel" in j["roofline"]["kernels"]
    assert j["roofline"]["north_star_set_frac"] == r["north_star_set_frac"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "wasted_traffic_ratio", "algorithmic_flops_per_launch",
              "algorithmic_bytes_per_launch", "launches_per_step", "ms_per_step"):
        assert k in j["roofline"], k


def test_a_low_intensity_convolution_is_priced_against_hbm_and_rows_carry_the_measured_ceilings():
    # "any family with flops > 0 is MFMA-bound" mislabelled cout1 / thin_conv (tens of FLOP per byte)
    thin = bench.kernel_row(("thin_conv_kernel", 4, 0.9, 4 * 4.6e10, 4 * 9.0e8), 2500.0)
    assert thin["bound"] == "hbm" and thin["unit"] == "GB/s" and thin["peak"] == 8000.0 and thin["achievable_peak"] == 6300.0
    dense = bench.kernel_row(("conv_p2_kernel", 60, 15.0, 60 * 2.31e11, 60 * 5.08e8), 2500.0)
    assert dense["bound"] == "mfma" and dense["peak"] == 2500.0 and dense["achievable_peak"] == bench.ACHIEVABLE_BF16_TFLOPS
    assert abs(dense["frac_of_achievable"] - dense["achieved"] / bench.ACHIEVABLE_BF16_TFLOPS) < 1e-3
    j = json.loads(bench.compact_line(_full()))
    assert j["roofline"]["achievable_peak"] == bench.ACHIEVABLE_BF16_TFLOPS and 0 < j["roofline"]["frac_of_achievable"] < 1


def test_a_step_dominated_by_a_streaming_kernel_is_priced_against_hbm():
    recs = [("norm_bwd", "spade_norm_bwd", 0.0, 8.0e9, 2.0, "norm_bwd"), ("conv", "c", 1e12, 1e8, 1.0, "conv_mfma_kernel[tile 8]")]
    res = {"summary": bench.summarize(recs, 2500.0), "peak": 2500.0, "dt": 0.003, "steps": 1}
    r = bench.roofline_obj({"B": 1, "flops_per_img": 1e12, "traffic_tag": "none"}, res, north_star=False)
    assert r["kernel"] == "hrv::norm_bwd" and r["bound"] == "hbm" and r["unit"] == "GB/s" and abs(r["achieved"] - 4000.0) < 1 and r["frac"] == 0.5


def test_emit_prints_the_compact_line_last_and_writes_the_detail_file(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        bench.emit(_full())
    lines = buf.getvalue().splitlines()
    assert len(lines) == 1 and len(lines[0]) < 4096
    j = json.loads(lines[0])
    d = json.load(open(tmp_path / j["detail"]))
    assert d["roofline"]["hbm_kinds"] and d["parity"]["bf16_engine_vs_oracle"] and d["roofline"]["slowest_launches"]


def test_an_oversized_result_still_fits_by_shedding_optional_parts():
    full = _full()
    full["extra"] = {f"cfg{i}": dict(v, parity={"x" * 40 + str(j): {"max_rel_err": 1e-3} for j in range(60)})
                     for i, v in enumerate(list(full["extra"].values()) * 3)}
    txt = bench.compact_line(full)
    assert len(txt) < 4096 and json.loads(txt)["roofline"]["kernel"] == "hrv::conv_p2_kernel"


# ----------------------------------------------------------------------------------------------- the round's committed final run
def _final():
    p = os.path.join(ROOT, "profiles", "r05_final_bench_default.json")
    q = os.path.join(ROOT, "profiles", "r05_final_bench_detail.json")
    if not (os.path.exists(p) and os.path.exists(q)):
        pytest.skip("the round's final bench line is not committed yet")
    raw = open(p).read().strip()
    return raw, json.loads(raw), json.load(open(q))


def test_committed_final_line_is_the_headline_config_and_parses():
    raw, j, d = _final()
    assert "\n" not in raw and len(raw.encode()) < 4096
    for k in CONTRACT:
        assert k in j, k
    assert j["n_gpus"] == 1 and j["dtype"] == "bf16" and j["unit"] == "images/s" and j["vs_baseline"] is None
    cfg = j["config"]
    assert "configs[3]" in cfg["workload"] and "train_generator" in cfg["workload"]
    assert cfg["global_batch"] == 4 and (cfg["height"], cfg["width"]) == (1024, 768)
    assert cfg["rccl_ranks"] == 0 and cfg["world_size"] == 1 and cfg["persistent_grid_cus"] == 256
    assert abs(j["value"] - cfg["global_batch"] * 1e3 / j["ms_per_step"]) < 0.01 * j["value"]
    assert j["value"] >= 53.0                                             # round 4: 53.5-54.1
    r = j["roofline"]
    # the dominant kernel = the family with the largest summed time in the detail's own per-kernel table
    top = max([d["roofline"]] + d["roofline"]["kernels"], key=lambda k: k["ms_per_step"])
    assert r["kernel"] == top["kernel"] == d["roofline"]["kernel"]
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3 and r["north_star_set_frac"] >= 0.27
    assert r["traffic"] is not None and "r05" in r["traffic_source"]
    assert 0.5 * r["algorithmic_bytes_per_launch"] <= r["traffic"] <= 2.0 * r["algorithmic_bytes_per_launch"]
    c = j["cpu_baseline"]
    assert c["kind"] == "port" and c["cores"] >= 1 and c["seconds_per_step"] > 1.0


def test_committed_final_detail_holds_parity_within_the_stated_tolerances():
    _, j, d = _final()
    p = d["parity"]
    f, b = p["fp32_engine_vs_oracle"], p["bf16_engine_vs_oracle"]
    assert f["image_max_rel_err"] < 1e-3 and all(v < 1e-3 for v in f["loss_rel_err"].values()) and f["grad_worst_rel_err"] < 2e-2
    assert "1024x768" in f["size"] and "1024x768" in b["size"]
    assert b["image_mean_abs_err"] < 3e-3 and all(v < 2e-3 for v in b["loss_rel_err"].values()) and b["grad_min_cosine"] > 0.99
    df, db = p["discriminator_half_fp32_engine_vs_oracle"], p["discriminator_half_bf16_engine_vs_oracle"]
    assert all(v < 1e-3 for v in df["loss_rel_err"].values()) and df["grad_worst_rel_err"] < 2e-2
    assert all(v < 5e-3 for v in db["loss_rel_err"].values())
    # the D half is held to the fp32 oracle itself (round 4: only to the oracle's own bf16-operand evaluation, 0.983)
    assert db["grad_min_cosine"] > 0.99 > db["bf16_rounded_oracle_vs_fp32_oracle"]["grad_min_cosine"]
    e = d["extra"]
    c3 = e["config3_train_condition_f32_b8"]["parity"]
    assert "1024x768" in c3["size"] and all(v < 1e-3 for v in c3["false"]["loss_rel_err"].values())
    assert c3["false"]["tocg"]["min_cosine"] > 0.9999 and c3["false"]["D"]["min_cosine"] > 0.9999
    t, q = e["config5_tryon_infer_bf16_b16"], e["config2_tocg_infer_f32_b4"]
    assert t["batch"] == 16 and abs(t["value"] - 16e3 / t["ms_per_step"]) < 0.01 * t["value"] and t["value"] > 340
    assert all(t["parity"]["hipgraph_replay_vs_eager"]["bit_identical"].values())
    qp = q["parity"]
    assert qp["seg_max_rel_err"] < 1e-3 and qp["argmax_mismatch_pixels"] <= 2e-5 * qp["pixels"]
    assert all(m <= 1024 for m in qp["mismatch_top2_margin_ulps_of_logit"])
    # ... and the compact line carries the same worst numbers
    # (the engine's worst cosine: the oracle's own bf16-operand evaluation, a yardstick kept in the detail file, is not part of it)
    assert abs(j["parity"]["min_cosine"] - min(db["grad_min_cosine"], b["grad_min_cosine"], 1.0)) < 2e-3
    # the compact line IS bench.compact_line of the detail file
    assert json.loads(bench.compact_line(d, j.get("detail"))) == j


# ----------------------------------------------------------------------------------------------- --dump-outputs
def test_dump_outputs_names_every_returned_array_and_keeps_the_budget(tmp_path):
    """bench.named_arrays flattens what a step returns (dicts, lists, Act views: their real channels only); bench.dump_outputs writes
    float32 / float64 .npy files under the byte budget -- small arrays whole, large ones cut to the same seeded positions every time."""
    import numpy as np
    import torch
    import hr_viton_amd  # noqa: F401
    from hr_viton_amd.ops import Act
    g = torch.Generator().manual_seed(0)
    ret = {"output": torch.randn(2, 3, 64, 48, generator=g), "flow_list": [torch.randn(1, 8, 6, 2, generator=g)],
           "parse": Act(torch.arange(2 * 4 * 3 * 8, dtype=torch.float32).reshape(2, 4, 3, 8).to(torch.bfloat16), 7),
           "labels": torch.randint(0, 13, (2, 64, 48), generator=g), "loss": {"GAN": torch.tensor(1.5)},
           "params": torch.randn(200_000, generator=g, dtype=torch.float64)}
    arrays = bench.named_arrays(ret)
    assert {k: tuple(v.shape) for k, v in arrays.items()} == {
        "output": (2, 3, 64, 48), "flow_list_0": (1, 8, 6, 2), "parse": (2, 4, 3, 7), "labels": (2, 64, 48), "loss_GAN": (), "params": (200_000,)}
    whole = bench.dump_outputs(str(tmp_path / "whole"), arrays)
    assert all(s == list(arrays[k].shape) for k, s in whole.items())
    p = np.load(tmp_path / "whole" / "parse.npy")
    assert p.dtype == np.float32 and np.array_equal(p, ret["parse"].t[..., :7].float().numpy())
    assert np.load(tmp_path / "whole" / "params.npy").dtype == np.float64 and np.load(tmp_path / "whole" / "labels.npy").dtype == np.float32

    limit = 600_000
    for run in ("a", "b"):
        cut = bench.dump_outputs(str(tmp_path / run), arrays, limit=limit)
        assert sum(os.path.getsize(tmp_path / run / f) for f in os.listdir(tmp_path / run)) <= limit
    assert {k: s for k, s in cut.items() if k != "params"} == {k: s for k, s in whole.items() if k != "params"}   # the small ones whole
    assert len(cut["params"]) == 1 and 50_000 < cut["params"][0] < 200_000       # the large one fills the rest of the budget
    full = arrays["params"].numpy()
    for k in cut:
        a, b = np.load(tmp_path / "a" / f"{k}.npy"), np.load(tmp_path / "b" / f"{k}.npy")
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b), k
    assert np.isin(np.load(tmp_path / "a" / "params.npy"), full).all()       # a sample of the array's own elements


def test_a_read_only_checkout_still_gets_the_line(tmp_path, monkeypatch):
    """bench.py run from a tree it cannot write to: the side files (detail JSON, parity tables) are skipped, the line still goes out"""
    blocked = tmp_path / "file"
    blocked.write_text("")
    assert bench.writable_dir(str(blocked / "sub")) is None           # cannot be created (its parent is a file)
    assert bench.writable_dir(str(tmp_path / "a" / "b")) == str(tmp_path / "a" / "b") and (tmp_path / "a" / "b").is_dir()
    monkeypatch.setattr(bench, "ROOT", str(blocked))
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        bench.emit(_full())
    lines = buf.getvalue().splitlines()
    j = json.loads(lines[0])
    assert len(lines) == 1 and "detail" not in j and j["ms_per_step"] == 74.0 and all(k in j for k in CONTRACT)


# ----------------------------------------------------------------------------------------------- plain run / --full
def test_a_plain_run_does_only_the_headline_and_full_does_the_rest():
    """``bench.py --gpus 1 --steps K --warmup W`` stops after the timed steps; the profiled step, the CPU legs, the extra
    configurations and the detail file are --full's, trimmed there by --no-cpu-baseline / --no-extras as before."""
    p = bench.make_parser()

    def legs(argv, rank=0, world=1):
        return bench.planned_legs(p.parse_args(argv), rank, world)
    assert legs(["--gpus", "1", "--steps", "20", "--warmup", "5"]) == {
        "profiled_step": False, "cpu_legs": False, "extras": False, "detail_file": False}
    assert not any(legs(["--workload", "tocg_infer", "--no-cpu-baseline", "--no-extras"]).values())
    assert not any(legs(["--dump-outputs", "out"]).values())
    assert all(legs(["--full"]).values())
    assert legs(["--full", "--no-cpu-baseline"]) == {"profiled_step": True, "cpu_legs": False, "extras": True, "detail_file": True}
    assert legs(["--full", "--no-cpu-baseline", "--no-extras"]) == {
        "profiled_step": True, "cpu_legs": False, "extras": False, "detail_file": True}
    assert legs(["--full", "--workload", "tocg_infer"])["extras"] is False and legs(["--full", "--workload", "tocg_infer"])["cpu_legs"]
    # N > 1: every rank takes the profiled step (its collectives), no rank the CPU legs or the extras
    for rank in (0, 1):
        assert legs(["--full", "--gpus", "2"], rank, 2) == {"profiled_step": True, "cpu_legs": False, "extras": False, "detail_file": True}
    # --dump-launches asks for the profiled step by itself
    assert legs(["--dump-launches", "l.txt"]) == {"profiled_step": True, "cpu_legs": False, "extras": False, "detail_file": False}


def test_a_plain_run_line_carries_the_contract_keys_with_the_extra_measurements_null():
    full = _full()
    line = {k: v for k, v in full.items() if k not in ("extra", "per_kind_ms")}
    line.update(roofline=None, cpu_baseline=None, parity=None)
    j = json.loads(bench.compact_line(line))
    for k in CONTRACT:
        assert k in j, k
    assert j["roofline"] is None and j["cpu_baseline"] is None and j["parity"] is None and "extra" not in j and "detail" not in j
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert j[k] == full[k], k
