"""Benchmark of the lazy R1 phase (hr_viton_amd.r1, csrc/r1.hip) against the plain discriminator step, at the training run's size.

  python tools/r1_bench.py [--batch 4] [--height 1024] [--width 768] [--ndf 64] [--fp16] [--reps R] [--warmup W] [--out FILE]

The script's PatchGAN (n_layers_D = 3, num_D = 2, spectral norm on).  In one process, alternating inside every repetition, with
device events around each:
  plain D step   forward_pair over [fake ; real] (2 x batch images), the two hinge terms, backward, fused Adam step
  R1 phase       opt_d.zero_grad(), R1.phase on the real half (batch images, fp32 operands also under --fp16), fused Adam step
then, from ``ops.profile_*`` records of one phase, the time of every launch kind of the phase and -- for the two new InstanceNorm
launches and the seed alone -- the achieved rate over the bytes they move (stats: c, f, t, df read; bwd: the same read, tbar and cbar
written, plus the incoming adjoint where there is one; r1_seed: d_in read, v written, its finalize block included).  The per-iteration cost at ``--interval`` is phase / interval."""
import argparse
import os
import statistics
import sys
from argparse import Namespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import hr_viton_amd  # noqa: E402,F401
from hr_viton_amd import ops  # noqa: E402
from hr_viton_amd import train_ops as T  # noqa: E402
from hr_viton_amd.losses import GANLoss  # noqa: E402
from hr_viton_amd.network_generator import MultiscaleDiscriminator  # noqa: E402
from hr_viton_amd.optim import Adam  # noqa: E402
from hr_viton_amd.r1 import R1  # noqa: E402


def bench(a):
    dev = torch.device("cuda", 0)
    opt = Namespace(cuda=True, gen_semantic_nc=7, ndf=a.ndf, norm_D="spectralinstance", n_layers_D=3, num_D=2, no_ganFeat_loss=False)
    torch.manual_seed(0)
    D = MultiscaleDiscriminator(opt)
    D.init_weights("xavier", 0.02)
    D.to(dev).train()
    od = Adam(D.parameters(), lr=4e-4, betas=(0.0, 0.9))
    N, H, W = a.batch, a.height, a.width
    g = torch.Generator().manual_seed(1)
    lab = torch.randint(0, 7, (N, 1, H // 32, W // 32), generator=g).repeat_interleave(32, 2).repeat_interleave(32, 3)
    parse = torch.zeros(N, 8, H, W).scatter_(1, lab, 1.0).permute(0, 2, 3, 1).contiguous().to(dev)
    parse7 = ops.Act(parse, 7)
    fake = (torch.rand(N, 3, H, W, generator=g) * 2 - 1).to(dev)
    real = (torch.rand(N, 3, H, W, generator=g) * 2 - 1).to(dev)
    crit = GANLoss("hinge")
    r1 = R1(a.gamma, a.interval)

    def plain():
        pf, pr = D.forward_pair(parse7, fake, real)
        loss = crit(pf, False, for_discriminator=True) + crit(pr, True, for_discriminator=True)
        od.zero_grad()
        loss.mean().backward()
        od.step()

    def phase():
        od.zero_grad()
        r1.phase(D, parse7, real)
        od.step()

    kinds = [("plain D step", plain), ("R1 phase", phase)]
    for _ in range(a.warmup):
        for _, fn in kinds:
            fn()
    times = {k: [] for k, _ in kinds}
    for _ in range(a.reps):
        evs = []
        for k, fn in kinds:
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn()
            e.record()
            evs.append((k, s, e))
        torch.cuda.synchronize()
        for k, s, e in evs:
            times[k].append(s.elapsed_time(e))
    by_kind, new = {}, {}
    for _ in range(5):
        ops.profile_begin()
        phase()
        recs = ops.profile_end()
        tot = {}
        for kind, name, _fl, nbytes, ms in recs:
            tot[kind] = tot.get(kind, 0.0) + ms
            if name.startswith("instnorm_jvp") or name == "r1_seed":
                new.setdefault((name, int(nbytes)), []).append(ms)
        for kind, ms in tot.items():
            by_kind.setdefault(kind, []).append(ms)
    med = {k: statistics.median(v) for k, v in times.items()}
    lines = ["D: ndf %d, num_D 2, n_layers_D 3, spectral norm; batch %d at %dx%d; %s operands in the plain step, fp32 in the phase; "
             "%d repetitions after %d warm-up" % (a.ndf, N, H, W, "bf16" if T.MMA_BF16[0] else "fp32", a.reps, a.warmup)]
    for k, _ in kinds:
        t = sorted(times[k])
        lines.append("  %-13s median %8.3f ms  (min %8.3f, max %8.3f)" % (k, med[k], t[0], t[-1]))
    lines.append("  R1 phase / plain D step: %.2f;  per iteration at interval %d: %.3f ms (%.1f%% of a plain D step)" %
                 (med["R1 phase"] / med["plain D step"], a.interval, med["R1 phase"] / a.interval,
                  100.0 * med["R1 phase"] / a.interval / med["plain D step"]))
    lines.append("  the phase by launch kind (sum of the events around each recorded launch, median of 5 phases, ms):")
    lines.append("    " + ", ".join("%s %.3f" % (k, statistics.median(v)) for k, v in sorted(by_kind.items(), key=lambda kv: -statistics.median(kv[1]))))
    lines.append("  the new launches alone (median over their calls; bytes as the wrappers count them; r1_seed: d_in read, v written):")
    for (name, nbytes), v in sorted(new.items(), key=lambda kv: (-kv[0][1], kv[0][0])):
        ms = statistics.median(v)
        lines.append("    %-20s %10.2f MB  %8.1f us  %6.2f TB/s" % (name, nbytes / 1e6, ms * 1e3, nbytes / ms / 1e9))
    return lines


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=4)
    p.add_argument("--height", type=int, default=1024)
    p.add_argument("--width", type=int, default=768)
    p.add_argument("--ndf", type=int, default=64)
    p.add_argument("--gamma", type=float, default=10.0)
    p.add_argument("--interval", type=int, default=16)
    p.add_argument("--fp16", action="store_true", help="the plain step on bf16 matrix cores, as train_generator.py --fp16")
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--out", type=str, default="")
    a = p.parse_args(argv)
    assert torch.cuda.is_available(), "r1_bench needs a GPU"
    if a.fp16:
        T.MMA_BF16[0] = True
    lines = ["r1_bench: %s" % torch.cuda.get_device_name(0)] + bench(a)
    text = "\n".join(lines)
    print(text, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
