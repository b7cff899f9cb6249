"""Micro-benchmark of DiffAugment inside the PatchGAN input assembly (csrc/diffaug.hip) against the plain launches it replaces, at the
training run's shape.

  python tools/diffaug_bench.py [--batch N] [--height H] [--width W] [--reps R] [--warmup W] [--burst K] [--out FILE]

At N x H x W = 4 x 1024 x 768 it times, with device events after warm-up and with the kinds alternating inside every repetition
(every event pair spans ``--burst`` back-to-back runs of a kind behind one untimed run of it, so the pair measures the device and not
the host's launch path):
  concat x2          the two plain assembly launches hrv_concat_nhwc_nchw_f32 (fake half, real half)
  mean+aug x2        hrv_diffaug_mean_f32 over both halves, then the two augmenting launches, policy color,translation,cutout
  aug x2 (geometry)  the two augmenting launches alone, policy translation,cutout (no reduction)
  to_nchw slice      the plain extraction of d(fake): hrv_nhwc_to_nchw_f32 over channels [7, 10) of the fake half's gradient
  gsum+bwd           hrv_diffaug_gsum_f32, then hrv_diffaug_bwd_f32, policy color,translation,cutout
  bwd (geometry)     hrv_diffaug_bwd_f32 alone, policy translation,cutout
  mean / gsum        the two reductions on their own
and prints the median time in us and the TB/s of each kind's own algorithmic bytes: an assembly launch reads 7 + 3 and writes 12
floats a pixel, the slice reads 3 and writes 3, the mean reads 3 floats a pixel and half (12 B), the gradient sum 3 floats a pixel.
The twins make the same accesses as the plain launches, shifted by whole pixels, minus what the mask skips (the box is a quarter of
the image), so the bytes predict a ratio near 1.  The uniforms are drawn once with a fixed seed."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import hr_viton_amd  # noqa: E402,F401
from hr_viton_amd import ops  # noqa: E402
from hr_viton_amd import train_ops as T  # noqa: E402
from hr_viton_amd.diffaug import parse_policy  # noqa: E402
from hr_viton_amd.ops import Act  # noqa: E402

HBM_TBPS = 6.3
CA = 7


def bench(N, H, W, reps, warmup, burst):
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(7)
    parse = Act(torch.randn((N, H, W, 8), device=dev, generator=gen), CA)
    fake = torch.randn((N, 3, H, W), device=dev, generator=gen)
    real = torch.randn((N, 3, H, W), device=dev, generator=gen)
    u = torch.rand((N, 8), device=dev, generator=gen)
    a = torch.empty((2 * N, H, W, 12), device=dev)
    g = Act(torch.randn((N, H, W, 12), device=dev, generator=gen), CA + 3)
    full, geom = parse_policy("color,translation,cutout"), parse_policy("translation,cutout")
    px = float(N * H * W)

    def plain():
        T.concat_nhwc_nchw(parse, fake, Act(a[:N], CA + 3))
        T.concat_nhwc_nchw(parse, real, Act(a[N:], CA + 3))

    def aug_full():
        mean = T.diffaug_mean(fake, real)
        T.diffaug_concat(parse, fake, u, mean[:N], full, Act(a[:N], CA + 3))
        T.diffaug_concat(parse, real, u, mean[N:], full, Act(a[N:], CA + 3))

    def aug_geom():
        T.diffaug_concat(parse, fake, u, None, geom, Act(a[:N], CA + 3))
        T.diffaug_concat(parse, real, u, None, geom, Act(a[N:], CA + 3))

    cat_bytes = 2 * 4.0 * px * (CA + 3 + 12)
    launches = [
        ("concat x2", cat_bytes, plain),
        ("mean+aug x2", cat_bytes + 2 * 12.0 * px, aug_full),
        ("aug x2 (geometry)", cat_bytes, aug_geom),
        ("to_nchw slice", 24.0 * px, lambda: ops.to_nchw(g, CA, 3)),
        ("gsum+bwd", 24.0 * px + 12.0 * px, lambda: T.diffaug_bwd(g, CA, u, T.diffaug_gsum(g, CA, u, full), full)),
        ("bwd (geometry)", 24.0 * px, lambda: T.diffaug_bwd(g, CA, u, None, geom)),
        ("mean (both halves)", 2 * 12.0 * px, lambda: T.diffaug_mean(fake, real)),
        ("gsum", 12.0 * px, lambda: T.diffaug_gsum(g, CA, u, full)),
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
    lines = ["%d x %d x %d (%.1f M pixels a half), %d repetitions of %d runs after %d warm-up; u = %s" %
             (N, H, W, px * 1e-6, reps, burst, warmup, " | ".join(" ".join("%.3f" % v for v in r) for r in u.cpu().tolist()))]
    for k, nbytes, _ in launches:
        t = sorted(times[k])
        med = statistics.median(t)
        lines.append("  %-19s median %8.1f us  (min %8.1f, max %8.1f)  %6.2f TB/s of its own %.1f MB" %
                     (k, med * 1e6, t[0] * 1e6, t[-1] * 1e6, nbytes / med * 1e-12, nbytes * 1e-6))
    med = {k: statistics.median(times[k]) for k in times}
    lines.append("  assembly: (mean + aug x2) / (concat x2) time %.3f (bytes alone: %.3f);  aug x2 geometry-only / concat x2 time %.3f" %
                 (med["mean+aug x2"] / med["concat x2"], (cat_bytes + 24.0 * px) / cat_bytes, med["aug x2 (geometry)"] / med["concat x2"]))
    lines.append("  d(fake):  (gsum + bwd) / (to_nchw slice) time %.3f (bytes alone: %.3f);  bwd geometry-only / to_nchw slice time %.3f" %
                 (med["gsum+bwd"] / med["to_nchw slice"], 36.0 / 24.0, med["bwd (geometry)"] / med["to_nchw slice"]))
    lines.append("  per discriminator call with color,translation,cutout: %+.1f us in the assembly, %+.1f us in the extraction of d(fake)" %
                 ((med["mean+aug x2"] - med["concat x2"]) * 1e6, (med["gsum+bwd"] - med["to_nchw slice"]) * 1e6))
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
    assert torch.cuda.is_available(), "diffaug_bench needs a GPU"
    lines = ["diffaug_bench: %s; reference point: a float4 copy achieves about %.1f TB/s on an MI355X" % (torch.cuda.get_device_name(0), HBM_TBPS)]
    lines += bench(a.batch, a.height, a.width, a.reps, a.warmup, a.burst)
    text = "\n".join(lines)
    print(text, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
