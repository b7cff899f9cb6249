"""GPU: a plain ``bench.py`` run (no --full) is the headline figure alone -- set-up, warm-up, the timed steps, the line -- and spends
little time outside its steps."""
import json
import os
import subprocess
import sys
import time

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUTSIDE_STEPS_BUDGET_S = 30.0


def test_a_plain_run_prints_the_headline_line_and_stays_within_its_budget():
    steps, warmup = 3, 2
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)],
                       capture_output=True, text=True, cwd=ROOT, timeout=300)
    wall = time.perf_counter() - t0
    assert r.returncode == 0, r.stderr[-2000:]
    j = json.loads(r.stdout.strip().splitlines()[-1])
    assert j["steps"] == steps and j["warmup"] == warmup and j["n_gpus"] == 1 and j["dtype"] == "bf16" and j["unit"] == "images/s"
    assert j["higher_is_better"] is True and "configs[3]" in j["config"]["workload"]
    assert abs(j["value"] - j["config"]["global_batch"] * 1e3 / j["ms_per_step"]) < 0.01 * j["value"]
    assert j["roofline"] is None and j["cpu_baseline"] is None and j["parity"] is None and "extra" not in j and "detail" not in j
    assert "cpu_baseline leg" not in r.stderr and "parity leg" not in r.stderr and "extra:" not in r.stderr
    outside = wall - (steps + warmup) * j["ms_per_step"] * 1e-3
    assert outside < OUTSIDE_STEPS_BUDGET_S, (outside, r.stderr[-2000:])
