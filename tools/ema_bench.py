"""Micro-benchmark of the Adam step that keeps a moving average of the weights (csrc/adam_ema.hip) on flat buffers of the training
run's sizes.

  python tools/ema_bench.py [--reps R] [--warmup W] [--burst K] [--out FILE]

For the generator's flat buffer (100 481 987 elements, 402 MB) and the PatchGAN's (1 339 522) it times, with device events after
warm-up and with the four kinds alternating inside every repetition (every event pair spans ``--burst`` back-to-back launches behind
one untimed launch of the same kind, so the pair measures the device and not the host's launch path):
  adam       hrv_adam_f32                     reads w, g, m, v and writes w, m, v: 28 bytes per element
  adam+ema   hrv_adam_ema_f32                 the same plus one read and one write of the average: 36 bytes per element
  adam,lerp  hrv_adam_f32, then ema.lerp_(w, 1 - d) on the flat buffer (the average kept outside the launch): 28 + 12 bytes
  swap       hrv_swap_f32                     reads and writes both buffers: 16 bytes per element
and prints the median time and the TB/s of those algorithmic bytes.  The claim under test is adam+ema <= adam,lerp in the same run;
from the bytes alone adam+ema should cost 36/28 of adam at equal bandwidth, less if its 16-byte accesses lift the rate.  For
context: about 6.3 TB/s is what a float4 copy achieves on an MI355X.  Everything on the PatchGAN's 5.4 MB buffer finishes faster
than the host issues the next launch: those rows show the launch interval, not the kernels."""
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
DECAY = 0.999


def bench(name, n, reps, warmup, burst):
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(n % 1000)
    w = torch.randn(n, device=dev, generator=gen)
    g = torch.randn(n, device=dev, generator=gen) * 1e-2
    m, v = torch.zeros_like(w), torch.zeros_like(w)
    ema, ema2 = w.clone(), w.clone()
    hyp = (1e-4, 0.0, 0.9, 1e-8, 0.0, 10)

    def unfused():
        T.adam_step(w, g, m, v, *hyp, 1.0)
        ema2.lerp_(w, 1.0 - DECAY)

    launches = [
        ("adam", 28.0 * n, lambda: T.adam_step(w, g, m, v, *hyp, 1.0)),
        ("adam+ema", 36.0 * n, lambda: T.adam_step_ema(w, g, m, v, ema, *hyp, 1.0, DECAY, False)),
        ("adam,lerp", 40.0 * n, unfused),
        ("swap", 16.0 * n, lambda: T.swap_(ema, ema2)),
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
    lines = ["%s flat buffer: %d elements (%.1f MB), %d repetitions of %d launches after %d warm-up" % (name, n, 4e-6 * n, reps, burst, warmup)]
    for k, nbytes, _ in launches:
        t = sorted(times[k])
        med = statistics.median(t)
        lines.append("  %-9s median %9.1f us  (min %9.1f, max %9.1f)  %6.2f TB/s" % (k, med * 1e6, t[0] * 1e6, t[-1] * 1e6, nbytes / med * 1e-12))
    med = {k: statistics.median(times[k]) for k in times}
    lines.append("  adam+ema / adam time: %.3f (bytes alone: %.3f);  adam+ema / (adam, then lerp) time: %.3f;  the average costs %.1f us "
                 "inside the launch, %.1f us outside it" % (med["adam+ema"] / med["adam"], 36.0 / 28.0, med["adam+ema"] / med["adam,lerp"],
                                                           (med["adam+ema"] - med["adam"]) * 1e6, (med["adam,lerp"] - med["adam"]) * 1e6))
    return lines


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=30)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--burst", type=int, default=8, help="launches per event pair")
    p.add_argument("--out", type=str, default="")
    a = p.parse_args(argv)
    assert torch.cuda.is_available(), "ema_bench needs a GPU"
    lines = ["ema_bench: %s; reference point: a float4 copy achieves about %.1f TB/s on an MI355X" % (torch.cuda.get_device_name(0), HBM_TBPS)]
    for name, n in BUFFERS:
        lines += bench(name, n, a.reps, a.warmup, a.burst)
    text = "\n".join(lines)
    print(text, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
