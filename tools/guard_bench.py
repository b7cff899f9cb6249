"""Micro-benchmark of the guarded Adam step (csrc/grad_guard.hip) on flat buffers of the training run's sizes.

  python tools/guard_bench.py [--reps R] [--warmup W] [--burst K] [--out FILE]

For the generator's flat buffer (100 481 987 elements: the 402 MB the data-parallel reduce moves) and the PatchGAN's (1 339 522)
it times, with device events after warm-up and with the four launches alternating inside every repetition (every event pair spans
``--burst`` back-to-back launches behind one untimed launch of the same kind: the device is then busy while the host prepares the
next launch, and the pair measures the device, not the host's launch path):
  sumsq     hrv_grad_sumsq_f32        reads g once: 4 bytes per element
  finalize  hrv_grad_guard_finalize   one block over the 1024 partials
  adam      hrv_adam_f32              reads w, g, m, v and writes w, m, v: 28 bytes per element
  adam+g    hrv_adam_guarded_f32      the same bytes, plus the guard record
and prints the median time and the GB/s of those algorithmic bytes.  The yardstick for the reduction is the un-guarded Adam
launch IN THE SAME RUN ON THE SAME BUFFER: it moves one word per element where Adam moves seven, so its effective bandwidth should
be no lower than Adam's.  For context: about 6.3 TB/s is what a float4 copy achieves on an MI355X (8 TB/s spec).
A launch that finishes faster than the host issues the next one (``finalize``, everything on the PatchGAN's 5.4 MB buffer) shows the
host's launch interval, not the kernel; for kernel-only times run this under ``rocprofv3 --kernel-trace --stats`` in a run of its own."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import hr_viton_amd  # noqa: E402,F401
from hr_viton_amd import train_ops as T  # noqa: E402

BUFFERS = [("generator", 100_481_987), ("PatchGAN", 1_339_522)]
HBM_TBPS = 6.3


def bench(name, n, reps, warmup, burst):
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(n % 1000)
    w = torch.randn(n, device=dev, generator=gen)
    g = torch.randn(n, device=dev, generator=gen) * 1e-2
    m, v = torch.zeros_like(w), torch.zeros_like(w)
    rec, part, cnt = T.guard_alloc(dev)
    hyp = (1e-4, 0.0, 0.9, 1e-8, 0.0, 10)
    launches = [
        ("sumsq", 4.0 * n, lambda: T.grad_sumsq(g, part, cnt)),
        ("finalize", 12.0 * T.guard_slots(), lambda: T.grad_guard_finalize(part, cnt, rec, 1.0, 1.0, False)),
        ("adam", 28.0 * n, lambda: T.adam_step(w, g, m, v, *hyp, 1.0)),
        ("adam+g", 28.0 * n, lambda: T.adam_step_guarded(w, g, m, v, *hyp, 1.0, rec)),
    ]
    times = {k: [] for k, _, _ in launches}
    for it in range(warmup + reps):
        evs = []
        for k, _, fn in launches:
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            fn()                      # untimed: keeps the device busy while the host enqueues what follows
            s.record()
            for _ in range(burst):
                fn()
            e.record()
            evs.append((k, s, e))
        torch.cuda.synchronize()
        if it >= warmup:
            for k, s, e in evs:
                times[k].append(s.elapsed_time(e) * 1e-3 / burst)
    st = T.guard_read(rec)
    lines = ["%s flat buffer: %d elements (%.1f MB), %d repetitions of %d launches after %d warm-up; last record: norm %.4g scale %.4g"
             % (name, n, 4e-6 * n, reps, burst, warmup, st["norm"], st["scale"])]
    for k, nbytes, _ in launches:
        t = sorted(times[k])
        med = statistics.median(t)
        lines.append("  %-9s median %9.1f us  (min %9.1f, max %9.1f)  %8.1f GB/s" % (k, med * 1e6, t[0] * 1e6, t[-1] * 1e6, nbytes / med * 1e-9))
    med = {k: statistics.median(times[k]) for k in times}
    r = (4.0 * n / med["sumsq"]) / (28.0 * n / med["adam"])
    lines.append("  sumsq bandwidth / adam bandwidth (same run, same buffer): %.2f;  guarded / plain Adam time: %.3f;  "
                 "sumsq + finalize = %.1f %% of the plain Adam launch" % (r, med["adam+g"] / med["adam"],
                                                                         100.0 * (med["sumsq"] + med["finalize"]) / med["adam"]))
    return lines


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=30)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--burst", type=int, default=8, help="launches per event pair")
    p.add_argument("--out", type=str, default="")
    a = p.parse_args(argv)
    assert torch.cuda.is_available(), "guard_bench needs a GPU"
    lines = ["guard_bench: %s; reference point: a float4 copy achieves about %.1f TB/s on an MI355X" % (torch.cuda.get_device_name(0), HBM_TBPS)]
    for name, n in BUFFERS:
        lines += bench(name, n, a.reps, a.warmup, a.burst)
    text = "\n".join(lines)
    print(text, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
