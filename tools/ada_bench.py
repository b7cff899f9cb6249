"""Micro-benchmark of the gated launches of adaptive discriminator augmentation (csrc/diffaug.hip) against their ungated twins and
the plain assembly, and of the controller launch, at the training run's shape.

  python tools/ada_bench.py [--batch N] [--height H] [--width W] [--reps R] [--warmup W] [--burst K] [--out FILE]

At N x H x W = 4 x 1024 x 768, policy color,translation,cutout, it times, with device events after warm-up and with the kinds
alternating inside every repetition (every event pair spans ``--burst`` back-to-back runs of a kind behind one untimed run of it, so
the pair measures the device and not the host's launch path):
  concat x2            the two plain assembly launches hrv_concat_nhwc_nchw_f32
  mean+aug x2          hrv_diffaug_mean_f32, then the two ungated augmenting launches
  mean+gated x2, p     the same with hrv_diffaug_concat_gated_f32, at p = 0, 0.5 and 1 (the mean runs at every p: the host does not know p)
  gated x2 alone, p=0  the two gated launches at p = 0 without the mean launch in front
  to_nchw slice        the plain extraction of d(fake)
  gsum+bwd             hrv_diffaug_gsum_f32, then hrv_diffaug_bwd_f32
  gsum+bwd gated, p    the gated pair at p = 0, 0.5 and 1
  ada_update           the controller launch alone (one thread; the time is the launch interval)
and prints the median time in us of each kind and the ratios the gates are judged by: p = 1 against the ungated twins, p = 0 against
the plain launches.  The uniforms are drawn once with a fixed seed; at p = 0.5 the line says which samples keep which transforms."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import hr_viton_amd  # noqa: E402,F401
from hr_viton_amd import _lib, ops  # noqa: E402
from hr_viton_amd import train_ops as T  # noqa: E402
from hr_viton_amd.diffaug import parse_policy  # noqa: E402
from hr_viton_amd.ops import Act  # noqa: E402

CA = 7
PS = (0.0, 0.5, 1.0)


def bench(N, H, W, reps, warmup, burst):
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(7)
    parse = Act(torch.randn((N, H, W, 8), device=dev, generator=gen), CA)
    fake = torch.randn((N, 3, H, W), device=dev, generator=gen)
    real = torch.randn((N, 3, H, W), device=dev, generator=gen)
    u = torch.rand((N, 8), device=dev, generator=gen)
    ug = torch.rand((N, 4), device=dev, generator=gen)
    a = torch.empty((2 * N, H, W, 12), device=dev)
    g = Act(torch.randn((N, H, W, 12), device=dev, generator=gen), CA + 3)
    full = parse_policy("color,translation,cutout")
    ps = {p: torch.tensor([p], dtype=torch.float64, device=dev) for p in PS}
    record = torch.zeros(_lib.DHEAD_WORDS, dtype=torch.float64, device=dev)
    state = torch.zeros(_lib.ADA_WORDS, dtype=torch.float64, device=dev)

    def plain():
        T.concat_nhwc_nchw(parse, fake, Act(a[:N], CA + 3))
        T.concat_nhwc_nchw(parse, real, Act(a[N:], CA + 3))

    def twins():
        mean = T.diffaug_mean(fake, real)
        T.diffaug_concat(parse, fake, u, mean[:N], full, Act(a[:N], CA + 3))
        T.diffaug_concat(parse, real, u, mean[N:], full, Act(a[N:], CA + 3))

    def gated(p):
        def run():
            mean = T.diffaug_mean(fake, real)
            T.diffaug_concat_gated(parse, fake, u, mean[:N], full, Act(a[:N], CA + 3), ug, ps[p])
            T.diffaug_concat_gated(parse, real, u, mean[N:], full, Act(a[N:], CA + 3), ug, ps[p])
        return run

    mean0 = T.diffaug_mean(fake, real)

    def gated_alone():      # the two gated launches at p = 0 behind a mean computed once: what the gates themselves cost over a copy
        T.diffaug_concat_gated(parse, fake, u, mean0[:N], full, Act(a[:N], CA + 3), ug, ps[0.0])
        T.diffaug_concat_gated(parse, real, u, mean0[N:], full, Act(a[N:], CA + 3), ug, ps[0.0])

    def gated_bwd(p):
        return lambda: T.diffaug_bwd_gated(g, CA, u, T.diffaug_gsum_gated(g, CA, u, full, ug, ps[p]), full, ug, ps[p])

    launches = [("concat x2", plain), ("mean+aug x2", twins)]
    launches += [("mean+gated x2, p=%g" % p, gated(p)) for p in PS]
    launches += [("gated x2 alone, p=0", gated_alone)]
    launches += [("to_nchw slice", lambda: ops.to_nchw(g, CA, 3)),
                 ("gsum+bwd", lambda: T.diffaug_bwd(g, CA, u, T.diffaug_gsum(g, CA, u, full), full))]
    launches += [("gsum+bwd gated, p=%g" % p, gated_bwd(p)) for p in PS]
    launches += [("ada_update", lambda: T.ada_update(record, 2, 0.6, 0.001, 4, 1.0, state))]
    times = {k: [] for k, _ in launches}
    for it in range(warmup + reps):
        evs = []
        for k, fn in launches:
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
    names = ("color", "translation", "cutout")
    kept = ["+".join(n for c, n in enumerate(names) if v[c] < 0.5) or "none" for v in ug.cpu().tolist()]
    lines = ["%d x %d x %d, policy color,translation,cutout, %d repetitions of %d runs after %d warm-up; at p = 0.5 the samples keep: %s" %
             (N, H, W, reps, burst, warmup, " | ".join(kept))]
    med = {}
    for k, _ in launches:
        t = sorted(times[k])
        med[k] = statistics.median(t)
        lines.append("  %-24s median %8.1f us  (min %8.1f, max %8.1f)" % (k, med[k] * 1e6, t[0] * 1e6, t[-1] * 1e6))
    lines.append("  assembly: gated p=1 / ungated twins %.3f;  gated p=0 / plain concat x2 %.3f with the mean launch, %.3f without it;  "
                 "gated p=0.5 / ungated twins %.3f" %
                 (med["mean+gated x2, p=1"] / med["mean+aug x2"], med["mean+gated x2, p=0"] / med["concat x2"],
                  med["gated x2 alone, p=0"] / med["concat x2"], med["mean+gated x2, p=0.5"] / med["mean+aug x2"]))
    lines.append("  d(fake):  gated p=1 / ungated gsum+bwd %.3f;  gated p=0 / to_nchw slice %.3f;  gated p=0.5 / ungated gsum+bwd %.3f" %
                 (med["gsum+bwd gated, p=1"] / med["gsum+bwd"], med["gsum+bwd gated, p=0"] / med["to_nchw slice"],
                  med["gsum+bwd gated, p=0.5"] / med["gsum+bwd"]))
    lines.append("  controller: %.1f us per discriminator step" % (med["ada_update"] * 1e6))
    return lines


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=4)
    p.add_argument("--height", type=int, default=1024)
    p.add_argument("--width", type=int, default=768)
    p.add_argument("--reps", type=int, default=30)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--burst", type=int, default=8, help="runs per event pair")
    p.add_argument("--out", type=str, default="")
    a = p.parse_args(argv)
    assert torch.cuda.is_available(), "ada_bench needs a GPU"
    lines = ["ada_bench: %s" % torch.cuda.get_device_name(0)]
    lines += bench(a.batch, a.height, a.width, a.reps, a.warmup, a.burst)
    text = "\n".join(lines)
    print(text, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
