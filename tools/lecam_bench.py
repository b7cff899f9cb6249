"""Micro-benchmark of the discriminator step's fused loss head (csrc/dhead.hip, hr_viton_amd.lecam) against the four GANLoss calls
it replaces, at the training run's logit shapes.

  python tools/lecam_bench.py [--reps R] [--warmup W] [--burst K] [--out FILE]

The run's PatchGAN (n_layers_D = 3, num_D = 2, batch 4 at 1024x768) ends in logit maps of 4x1x259x195 and 4x1x131x99 per half; the
real half sits n floats behind the fake half (the first line of the output says where that leaves its pointer).  In one process, with the
kinds alternating inside every repetition and device events around ``--burst`` back-to-back runs behind one untimed run, it times
forward + backward of
  GANLoss x4          D_Fake and D_Real at both scales: per call loss_kernel + loss_final_kernel forward and scale_kernel backward
                      (12 launches, plus torch's additions and divisions of the [1] tensors)
  head, weight 0      dhead_reduce + dhead_finalize forward, dhead_grad backward (3 launches): statistics only
  head, paper / relu  the same with the LeCam regulariser on, both forms
and prints the medians and the launches ``ops.profile_*`` records for one forward + backward of each kind (a ``loss_f32`` record is
loss_kernel + loss_final_kernel, and scale_kernel is not a recorded launch: the four-call path runs 12 launches where the count
shows 4), then the time between events around each single recorded launch.  Both paths move about 2 MB; in eager mode the time of
either is the host's: autograd nodes and launch calls, not the kernels."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import hr_viton_amd  # noqa: E402,F401
from hr_viton_amd import ops  # noqa: E402
from hr_viton_amd.lecam import LeCam  # noqa: E402
from hr_viton_amd.losses import GANLoss  # noqa: E402

SHAPES = [(4, 1, 259, 195), (4, 1, 131, 99)]


def bench(reps, warmup, burst):
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(7)
    leaves = []
    for s in SHAPES:
        n = s[0] * s[2] * s[3]
        buf = torch.randn(2 * n, device=dev, generator=gen)
        leaves.append((buf[:n].view(s).detach().requires_grad_(), buf[n:].view(s).detach().requires_grad_()))
    fake, real = [[f] for f, _ in leaves], [[r] for _, r in leaves]
    crit = GANLoss("hinge")
    heads = {"head, weight 0": LeCam(0.0), "head, paper 0.3": LeCam(0.3, form="paper"), "head, relu 0.3": LeCam(0.3, form="relu")}

    def four():
        d = {"D_Fake": crit(fake, False, for_discriminator=True), "D_Real": crit(real, True, for_discriminator=True)}
        sum(d.values()).mean().backward()

    def head(h):
        def run():
            sum(h.d_losses(fake, real).values()).mean().backward()
        return run

    kinds = [("GANLoss x4", four)] + [(k, head(h)) for k, h in heads.items()]
    counts = {}
    for k, fn in kinds:
        fn()
        ops.profile_begin()
        fn()
        names = [r[1] for r in ops.profile_end()]
        counts[k] = (len(names), sorted(set(names)))
    per_launch = {}      # kind -> {recorded name: median ms between the events around that one launch}
    for k, fn in kinds:
        seen = {}
        for _ in range(20):
            ops.profile_begin()
            fn()
            for r in ops.profile_end():
                seen.setdefault(r[1], []).append(r[4])
        per_launch[k] = {n: statistics.median(v) for n, v in seen.items()}
    times = {k: [] for k, _ in kinds}
    for it in range(warmup + reps):
        evs = []
        for k, fn in kinds:
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            fn()
            s.record()
            for _ in range(burst):
                fn()
            e.record()
            evs.append((k, s, e))
        torch.cuda.synchronize()
        if it >= warmup:
            for k, s, e in evs:
                times[k].append(s.elapsed_time(e) * 1e3 / burst)
    total = sum(2 * f.numel() for f, _ in leaves)
    lines = ["logits %s per half (%d floats in all; real halves at byte offsets %s mod 16), %d repetitions of %d runs after %d warm-up" %
             (" and ".join("x".join(map(str, s)) for s in SHAPES), total, "/".join(str(r.data_ptr() % 16) for _, r in leaves), reps, burst,
              warmup)]
    med = {k: statistics.median(v) for k, v in times.items()}
    for k, _ in kinds:
        t = sorted(times[k])
        lines.append("  %-16s forward + backward median %7.1f us  (min %7.1f, max %7.1f)  %2d recorded launches: %s" %
                     (k, med[k], t[0], t[-1], counts[k][0], ", ".join(counts[k][1])))
    for k in heads:
        lines.append("  %s / GANLoss x4: %.3f" % (k, med[k] / med["GANLoss x4"]))
    lines.append("  events around single launches (median of 20, us; a pair around one launch includes the launch interval):")
    for k, _ in kinds:
        lines.append("    %-16s %s" % (k, ", ".join("%s %.1f" % (n, v * 1e3) for n, v in sorted(per_launch[k].items()))))
    return lines


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=30)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--burst", type=int, default=8, help="runs per event pair")
    p.add_argument("--out", type=str, default="")
    a = p.parse_args(argv)
    assert torch.cuda.is_available(), "lecam_bench needs a GPU"
    lines = ["lecam_bench: %s" % torch.cuda.get_device_name(0)] + bench(a.reps, a.warmup, a.burst)
    text = "\n".join(lines)
    print(text, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
