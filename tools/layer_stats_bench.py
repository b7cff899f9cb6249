"""Micro-benchmark of the per-parameter statistics (csrc/span_stats.hip; optim.Adam.layer_stats) on the generator's REAL span table.

  python tools/layer_stats_bench.py [--reps R] [--warmup W] [--burst K] [--out FILE]      (default FILE: profiles/layer_stats_bench.txt)

It builds SPADEGenerator at the benchmark's configuration (train_generator.py's defaults), lets optim.Adam lay its parameters into the
flat buffers (``opt._flat[0]``), fills gradient and moments with random data, and times in ONE run, with device events after warm-up
and the launches alternating inside every repetition (every event pair spans ``--burst`` back-to-back launches behind one untimed
launch of the same kind, as tools/guard_bench.py does: the pair then measures the device, not the host's launch path):
  stats      hrv_span_stats_f32        reads g, w, m, v over every parameter's elements: 16 bytes per element
  finalize   hrv_span_stats_finalize   one wave per parameter over its pieces' partials
  both       the two launches of one report
  sumsq      hrv_grad_sumsq_f32        the guard's reduction of the same gradient buffer: 4 bytes per element -- the yardstick
  adam       hrv_adam_f32              on copies of w, m, v: 28 bytes per element
and, in wall-clock time with one synchronisation at the end, the host loop a report replaces: per parameter
torch.linalg.vector_norm of gradient and weight plus an isfinite count of the gradient (3 of the report's 10 numbers)."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import hr_viton_amd  # noqa: E402,F401
from hr_viton_amd import train_ops as T  # noqa: E402


def build_optimizer(dev):
    import train_generator as tg
    from hr_viton_amd.network_generator import SPADEGenerator
    from hr_viton_amd.optim import Adam
    opt = tg.get_opt(["--name", "bench", "--synthetic", "-b", "4"])
    torch.manual_seed(0)
    gen = SPADEGenerator(opt, 9)
    gen.init_weights("xavier", 0.02)
    gen.to(dev).train()
    og = Adam(gen.parameters(), lr=opt.G_lr, betas=(0.0, 0.9))
    og.prepare_layer_stats()
    return gen, og


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--burst", type=int, default=8, help="launches per event pair")
    p.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "layer_stats_bench.txt"))
    a = p.parse_args(argv)
    assert torch.cuda.is_available(), "layer_stats_bench needs a GPU"
    dev = torch.device("cuda", 0)
    gen, og = build_optimizer(dev)
    st = og._flat[0]
    ws = st["span_ws"]
    n_el = sum(k for _, _, k in st["spans"])
    g, w, m, v = st["g"], st["w"], st["m"], st["v"]
    rng = torch.Generator(device=dev).manual_seed(1)
    g.copy_(torch.randn(g.numel(), device=dev, generator=rng) * 1e-2)
    m.copy_(torch.randn(g.numel(), device=dev, generator=rng) * 1e-3)
    v.copy_(torch.rand(g.numel(), device=dev, generator=rng) * 1e-4 + 1e-12)
    for _, off, k in st["spans"]:          # the padding between spans is zero in the optimizer's buffers
        pad = (k + 3) // 4 * 4 - k
        if pad:
            for t in (g, m, v):
                t[off + k:off + k + pad].zero_()
    w2, m2, v2 = w.clone(), m.clone(), v.clone()
    rec, part, cnt = T.guard_alloc(dev)
    lib = T._lib.load()

    def stats():
        T._lib.check(lib.hrv_span_stats_f32(g.data_ptr(), w.data_ptr(), m.data_ptr(), v.data_ptr(), ws["pieces"].data_ptr(), ws["n_pieces"],
                                            None, 0.5, 1e-8, ws["part"].data_ptr(), T._stream()), "hrv_span_stats_f32")

    def finalize():
        T._lib.check(lib.hrv_span_stats_finalize(ws["part"].data_ptr(), ws["span_first"].data_ptr(), ws["n_spans"], ws["records"].data_ptr(),
                                                 T._stream()), "hrv_span_stats_finalize")

    launches = [
        ("stats", 16.0 * n_el, stats),
        ("finalize", 64.0 * (ws["n_pieces"] + ws["n_spans"]), finalize),
        ("both", 16.0 * n_el, lambda: T.span_stats(ws, g, w, m, v, None, 0.5, 1e-8)),
        ("sumsq", 4.0 * g.numel(), lambda: T.grad_sumsq(g, part, cnt)),
        ("adam", 28.0 * g.numel(), lambda: T.adam_step(w2, g, m2, v2, 1e-4, 0.0, 0.9, 1e-8, 0.0, 10, 1.0)),
    ]
    times = {k: [] for k, _, _ in launches}
    for it in range(a.warmup + a.reps):
        evs = []
        for k, _, fn in launches:
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            fn()                      # untimed: keeps the device busy while the host enqueues what follows
            s.record()
            for _ in range(a.burst):
                fn()
            e.record()
            evs.append((k, s, e))
        torch.cuda.synchronize()
        if it >= a.warmup:
            for k, s, e in evs:
                times[k].append(s.elapsed_time(e) * 1e-3 / a.burst)

    def host_loop():
        out = []
        for p, off, k in st["spans"]:
            gv = g[off:off + k]
            out.append((torch.linalg.vector_norm(gv), torch.linalg.vector_norm(w[off:off + k]), (~torch.isfinite(gv)).sum()))
        torch.cuda.synchronize()
        return out

    host = []
    for it in range(2 + 5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host_loop()
        if it >= 2:
            host.append(time.perf_counter() - t0)
    report = []
    for it in range(2 + 5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        og.layer_stats()
        if it >= 2:
            report.append(time.perf_counter() - t0)

    med = {k: statistics.median(times[k]) for k in times}
    lines = ["layer_stats_bench: %s; generator flat buffer: %d parameters, %d elements (%d with padding, %.1f MB per array), %d pieces of "
             "at most %d; %d repetitions of %d launches after %d warm-up"
             % (torch.cuda.get_device_name(0), ws["n_spans"], n_el, g.numel(), 4e-6 * g.numel(), ws["n_pieces"], T.span_stats_piece(),
                a.reps, a.burst, a.warmup)]
    for k, nbytes, _ in launches:
        t = sorted(times[k])
        lines.append("  %-9s median %9.1f us  (min %9.1f, max %9.1f)  %8.1f GB/s" % (k, med[k] * 1e6, t[0] * 1e6, t[-1] * 1e6,
                                                                                      nbytes / med[k] * 1e-9))
    bw = lambda k: dict((x, b) for x, b, _ in launches)[k] / med[k]  # noqa: E731
    lines.append("  both launches: %.2f TB/s of 16 B/element = %.2f of the guard's reduction (%.2f TB/s of 4 B/element) and %.2f of the "
                 "Adam launch (%.2f TB/s of 28 B/element), same run, same buffers"
                 % (bw("both") * 1e-12, bw("both") / bw("sumsq"), bw("sumsq") * 1e-12, bw("both") / bw("adam"), bw("adam") * 1e-12))
    lines.append("  one report, wall clock with its read-back (Adam.layer_stats()): median %.2f ms;  the host loop it replaces (%d x "
                 "[vector_norm(grad), vector_norm(weight), isfinite count], one synchronisation): median %.2f ms  -> %.1f x"
                 % (statistics.median(report) * 1e3, ws["n_spans"], statistics.median(host) * 1e3,
                    statistics.median(host) / statistics.median(report)))
    text = "\n".join(lines)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
