"""GPU: per-parameter statistics of the optimizer's flat buffers (csrc/span_stats.hip; train_ops.span_stats; optim.Adam.layer_stats,
optim.layer_report; --layer_stats_count of the scripts) against the float64 restatement of tests/span_stats_cases.py, which
tests/test_span_stats_cases_cpu.py holds against torch: exactly on integer data over every span table (NaN in every gap), one
non-finite element anywhere, Gaussian data within the bounds of the number formats, independence of the spans, the guard's totals,
the optimizer on both step-count paths, a skipped step, capture in a hipGraph, the real backward, the scripts."""
import functools
import json
import math
import os

import numpy as np
import pytest
import torch

import guard_cases as G
import span_stats_cases as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _T():
    import hr_viton_amd  # noqa: F401
    from hr_viton_amd import train_ops
    return train_ops


@functools.lru_cache(maxsize=None)
def _case(name, kind):
    """one table with one kind of data: the CPU data and its restatement (never modified), the workspace"""
    spans, shift = S.table(name)
    data = S.int_data(spans, 11) if kind == "int" else S.gauss_data(spans, 12)
    bufs, base = S.lay_out(spans, shift, data)
    return {"spans": spans, "shift": shift, "data": data, "bufs": bufs, "base": base, "ws": _T().span_stats_alloc(spans, "cuda")}


def _views(case):
    """fresh device copies of the four storages and their views (the storages keep the NaN bands and gaps around them)"""
    n = S.extent(case["spans"])
    dev = [b.cuda() for b in case["bufs"]]
    views = [d[case["base"]:case["base"] + n] for d in dev]
    assert all(v.data_ptr() % 16 == 4 * case["shift"] for v in views)
    return dev, views


def _run(case, views, with_mv=True, hyper=None, bc2_sqrt=1.0, eps=0.0):
    ws = case["ws"]
    ws["part"].fill_(-1)            # every word of every partial and record is written by every call
    ws["records"].fill_(-1)
    g, w, m, v = views
    rec = _T().span_stats(ws, g, w, m if with_mv else None, v if with_mv else None, hyper, bc2_sqrt, eps)
    return rec.cpu()


def test_the_piece_length_is_the_mirrored_constant():
    assert _T().span_stats_piece() == S.PIECE


# ---------------------------------------------------------------------------------------------------------------
# 1, 2: exact on integers; nothing outside the spans is read
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_mv", [True, False], ids=["gwmv", "gw"])
@pytest.mark.parametrize("name", S.TABLES)
def test_every_word_is_exact_on_integer_data_and_the_nan_gaps_are_not_read(name, with_mv):
    case = _case(name, "int")
    _, views = _views(case)
    got = _run(case, views, with_mv)
    want = S.pack_records(S.records_ref(case["data"], with_mv))
    assert not got[:, 9:12].any(), "a read outside the spans met a NaN band or gap"
    assert torch.equal(got, want), (got != want).nonzero()[:8].tolist()
    assert all(r["g_zeros"] >= 1 for r in _T().span_stats_read(got))


# ---------------------------------------------------------------------------------------------------------------
# 3: one non-finite element
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", S.TABLES)
def test_one_nonfinite_element_is_counted_left_out_and_stays_in_its_span(name):
    case = _case(name, "int")
    _, views = _views(case)
    base = _run(case, views)
    assert torch.equal(base, S.pack_records(S.records_ref(case["data"])))
    rows = torch.arange(base.shape[0])
    for j, (off, k) in enumerate(case["spans"]):
        for pos in S.poison_positions(k):
            for a, word in ((0, 9), (1, 10), (2, 11)):          # g, then w, then m
                keep = float(case["data"][j][a][pos])
                for kind, val in S.POISONS.items():
                    views[a][off + pos] = val
                    got = _run(case, views)
                    arrs = [x.clone() if i == a else x for i, x in enumerate(case["data"][j])]
                    arrs[a][pos] = val
                    want = S.pack_records([S.record_ref(*arrs)])[0]
                    assert got[j, word] == 1 and int(got[j, 9:12].sum()) == 1, (j, pos, a, kind, got[j].tolist())
                    assert torch.equal(got[j], want), (j, pos, a, kind, got[j].tolist(), want.tolist())
                    assert torch.equal(got[rows != j], base[rows != j]), (j, pos, a, kind)
                views[a][off + pos] = keep
    assert torch.equal(_run(case, views), base)


# ---------------------------------------------------------------------------------------------------------------
# 4: Gaussian data
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", S.TABLES)
def test_gaussian_data_within_the_bounds_of_the_formats(name):
    """g_sumsq, w_sumsq within len * 2^-52 * S of float64 (the squares are exact in double: only the order of the additions
    differs); the maxima exactly; u_sumsq within 2^-19 * S (four fp32 operations per element, each allowed 4 ulp, doubled by the
    square); u_maxabs within 2^-20 relative.  Measured on an MI355X, worst fraction of each bound over the four tables:
    g_sumsq 0.198, w_sumsq 0.181 (both on the 300 spans of 1 .. 7 elements, where the bound is a few ulp), u_sumsq 0.104,
    u_maxabs 0.105; the test prints them per table."""
    case = _case(name, "gauss")
    _, views = _views(case)
    got = _T().span_stats_read(_run(case, views, True, None, S.GAUSS_BC2_SQRT, S.GAUSS_EPS))
    want = S.records_ref(case["data"], True, S.GAUSS_BC2_SQRT, S.GAUSS_EPS)
    worst = {"g_sumsq": 0.0, "w_sumsq": 0.0, "u_sumsq": 0.0, "u_maxabs": 0.0}
    fails = []
    for j, ((_, k), r, x) in enumerate(zip(case["spans"], got, want)):
        bounds = {"g_sumsq": k * 2.0 ** -52 * x["g_sumsq"], "w_sumsq": k * 2.0 ** -52 * x["w_sumsq"], "u_sumsq": 2.0 ** -19 * x["u_sumsq"],
                  "u_maxabs": 2.0 ** -20 * x["u_maxabs"]}
        for key, b in bounds.items():
            frac = abs(r[key] - x[key]) / b
            worst[key] = max(worst[key], frac)
            if frac > 1.0:
                fails.append((j, key, r[key], x[key], frac))
        if (r["g_maxabs"], r["w_maxabs"]) != (x["g_maxabs"], x["w_maxabs"]):
            fails.append((j, "maxabs", r["g_maxabs"], x["g_maxabs"], r["w_maxabs"], x["w_maxabs"]))
        if (r["g_nonfinite"], r["w_nonfinite"], r["u_nonfinite"], r["g_zeros"]) != (0, 0, 0, 0):
            fails.append((j, "counts", r))
    print("span_stats %s: worst fraction of the bound: %s" % (name, ", ".join("%s %.3g" % kv for kv in worst.items())))
    assert not fails, fails[:8]


# ---------------------------------------------------------------------------------------------------------------
# 5: independence and determinism
# ---------------------------------------------------------------------------------------------------------------
def test_runs_are_bit_identical_spans_are_independent_and_hyper_dev_is_the_scalar():
    case = _case("edges", "gauss")
    _, views = _views(case)
    a = _run(case, views, True, None, S.GAUSS_BC2_SQRT, S.GAUSS_EPS)
    b = _run(case, views, True, None, S.GAUSS_BC2_SQRT, S.GAUSS_EPS)
    assert torch.equal(a, b)
    hyper = torch.tensor([1e-4, 0.5, S.GAUSS_BC2_SQRT], dtype=torch.float32, device="cuda")
    assert torch.equal(_run(case, views, True, hyper, 123.0, S.GAUSS_EPS), a), "hyper_dev[2] replaces the scalar"
    assert not torch.equal(_run(case, views, True, None, 0.5, S.GAUSS_EPS)[:, 4:6], a[:, 4:6])
    rows = torch.arange(a.shape[0])
    gen = torch.Generator().manual_seed(99)
    for j in (0, 5, 11, 14):          # 1 element, 63, PIECE - 1, 2 PIECE + 3
        off, k = case["spans"][j]
        keep = [v[off:off + k].clone() for v in views]
        for v in views:
            v[off:off + k] = (torch.rand(k, generator=gen) + 0.5).cuda()
        c = _run(case, views, True, None, S.GAUSS_BC2_SQRT, S.GAUSS_EPS)
        assert torch.equal(c[rows != j], a[rows != j]) and not torch.equal(c[j], a[j]), j
        for v, x in zip(views, keep):
            v[off:off + k] = x
    assert torch.equal(_run(case, views, True, None, S.GAUSS_BC2_SQRT, S.GAUSS_EPS), a)


# ---------------------------------------------------------------------------------------------------------------
# 6: against the guard
# ---------------------------------------------------------------------------------------------------------------
def test_the_spans_add_up_to_the_guards_totals():
    T = _T()
    case = _case("edges", "int")
    n = (S.extent(case["spans"]) + 3) // 4 * 4
    flat = [torch.zeros(n) for _ in range(4)]          # _setup's layout: zero padding between the spans
    for (off, k), arrs in zip(case["spans"], case["data"]):
        for f, x in zip(flat, arrs):
            f[off:off + k] = x
    dev = [f.cuda() for f in flat]
    rec, part, cnt = T.guard_alloc("cuda")

    def both():
        T.grad_sumsq(dev[0], part, cnt)
        T.grad_guard_finalize(part, cnt, rec, 1.0, None, False)
        return T.guard_read(rec), T.span_stats_read(T.span_stats(case["ws"], *dev))

    guard, spans = both()
    assert sum(r["g_sumsq"] for r in spans) == guard["sumsq"] == float((flat[0].double() ** 2).sum()) and guard["nonfinite"] == 0
    off, k = case["spans"][12]
    dev[0][off + 7], dev[0][off + k - 1], dev[0][0] = float("nan"), float("inf"), float("-inf")
    guard, spans = both()
    assert sum(r["g_nonfinite"] for r in spans) == guard["nonfinite"] == 3
    assert (spans[0]["g_nonfinite"], spans[12]["g_nonfinite"]) == (1, 2)


# ---------------------------------------------------------------------------------------------------------------
# 7: through optim.Adam
# ---------------------------------------------------------------------------------------------------------------
class _World:
    """what optim.Adam asks of a grad_sync: the gradients are multiplied by 1 / world inside the fused launch"""

    def __init__(self, world):
        self.world = world

    def wait(self):
        pass

    def grad_of(self, p):
        return p.grad


def _make(device_step=False, world=1, **kw):
    from hr_viton_amd.optim import Adam
    ps = [torch.nn.Parameter(w.cuda()) for w in G.start_weights()]
    opt = Adam(ps, lr=G.LR, betas=G.BETAS, eps=G.EPS, device_step=device_step, grad_sync=_World(world) if world > 1 else None, **kw)
    return ps, opt


def _step(ps, opt, grads):
    for p, g in zip(ps, grads):
        p.grad = None if g is None else g.cuda()
    opt.step()


def _bits(opt):
    st = opt._flat[0]
    return {k: st[k].clone().view(torch.int32) for k in ("w", "m", "v", "g")}


def _same(a, b, keys=("w", "m", "v", "g")):
    return all(torch.equal(a[k], b[k]) for k in keys)


def _bc2_sqrt(t):
    return float(np.sqrt(np.float32(1.0) - np.power(np.float32(G.BETAS[1]), np.float32(t))))


def _check_report(opt, rep, t, world=1):
    """layer_stats() against the restatement on the read-back flat buffers"""
    st = opt._flat[0]
    g, w, m, v = (st[k].cpu() for k in ("g", "w", "m", "v"))
    step_size = G.LR / (1.0 - G.BETAS[0] ** t)
    assert [e["param"] for e in rep] == [p for p, _, _ in st["spans"]]
    for e, (p, off, k) in zip(rep, st["spans"]):
        sl = slice(off, off + k)
        x = S.record_ref(g[sl], w[sl], m[sl], v[sl], _bc2_sqrt(t), G.EPS)
        assert e["numel"] == k == p.numel()
        assert abs(e["grad_norm"] - math.sqrt(x["g_sumsq"]) / world) <= k * 2.0 ** -52 * e["grad_norm"]
        assert abs(e["weight_norm"] - math.sqrt(x["w_sumsq"])) <= k * 2.0 ** -52 * e["weight_norm"]
        assert e["grad_maxabs"] == x["g_maxabs"] / world and e["weight_maxabs"] == x["w_maxabs"]
        assert (e["grad_nonfinite"], e["weight_nonfinite"], e["update_nonfinite"], e["grad_zeros"]) == (
            x["g_nonfinite"], x["w_nonfinite"], x["u_nonfinite"], x["g_zeros"])
        want = step_size * math.sqrt(x["u_sumsq"])
        assert abs(e["update_norm"] - want) <= 2.0 ** -19 * want, (e["update_norm"], want)
        assert abs(e["update_ratio"] - want / math.sqrt(x["w_sumsq"])) <= 2.0 ** -18 * e["update_ratio"]


@pytest.mark.parametrize("wd", [0.0, 0.01], ids=["plain", "weight_decay"])
@pytest.mark.parametrize("device_step", [False, True], ids=["host_count", "device_step"])
def test_layer_stats_of_the_optimizer_is_the_restatement_and_touches_nothing(device_step, wd):
    pa, oa = _make(device_step, weight_decay=wd)
    pn, on = _make(device_step, weight_decay=wd)          # the run that never asks
    for s in range(3):
        before = [p.detach().double().cpu() for p in pa]
        _step(pa, oa, G.gauss_grad_list(s))
        _step(pn, on, G.gauss_grad_list(s))
        bits = _bits(oa)
        rep = oa.layer_stats()
        assert _same(_bits(oa), bits), "layer_stats wrote to w, m, v or g"
        _check_report(oa, rep, s + 1)
        for e, wb, p in zip(rep, before, pa):
            moved = float(torch.linalg.vector_norm(wb - p.detach().double().cpu()))
            assert abs(e["update_norm"] - moved) <= 1e-5 * moved, (s, e["update_norm"], moved)
    assert "span_ws" in oa._flat[0] and "span_ws" not in on._flat[0]
    _step(pa, oa, G.gauss_grad_list(3))
    _step(pn, on, G.gauss_grad_list(3))
    assert _same(_bits(oa), _bits(on))


def test_the_world_factor_and_a_parameter_without_a_gradient():
    p1, o1 = _make()
    p2, o2 = _make(world=2)
    grads = G.gauss_grad_list(0)
    _step(p1, o1, grads)
    _step(p2, o2, grads)
    r1, r2 = o1.layer_stats(), o2.layer_stats()
    for a, b in zip(r1, r2):
        assert b["grad_norm"] == 0.5 * a["grad_norm"] and b["grad_maxabs"] == 0.5 * a["grad_maxabs"] and a["grad_norm"] > 0
    _check_report(o2, r2, 1, world=2)
    # host-count path: parameter 1 has no gradient in the second iteration; its own step count falls behind the group's
    grads = G.gauss_grad_list(1)
    _step(p1, o1, [grads[0], None, grads[2]])
    rep = o1.layer_stats()
    assert rep[1]["update_norm"] is None and rep[1]["update_ratio"] is None and rep[1]["grad_zeros"] == rep[1]["numel"]
    assert all(rep[i]["update_norm"] > 0 and rep[i]["update_ratio"] > 0 for i in (0, 2))
    assert rep[1]["weight_norm"] > 0 and rep[1]["grad_norm"] == 0.0
    # a weight of norm zero has no ratio
    o1._flat[0]["w"][:300].zero_()
    rep = o1.layer_stats()
    assert rep[0]["weight_norm"] == 0.0 and rep[0]["update_ratio"] is None and rep[0]["update_norm"] > 0


# ---------------------------------------------------------------------------------------------------------------
# 8: a skipped step
# ---------------------------------------------------------------------------------------------------------------
def test_the_report_after_a_skipped_step_names_the_poisoned_parameter():
    ps, opt = _make(True, skip_nonfinite=True)
    _step(ps, opt, G.gauss_grad_list(0))
    before = _bits(opt)
    _step(ps, opt, G.poison(G.gauss_grad_list(1), "nan"))
    assert opt.guard_stats()["apply"] == 0
    rep = opt.layer_stats()
    assert [e["grad_nonfinite"] for e in rep] == [0, 1, 0]
    assert all(e["weight_nonfinite"] == 0 and e["update_nonfinite"] == 0 for e in rep)
    assert _same(_bits(opt), before, ("w", "m", "v"))
    # the poisoned tensor still reports the norm of its finite elements, and the update is the stale moments' direction
    g1 = G.poison(G.gauss_grad_list(1), "nan")[1].reshape(-1)
    want = float(torch.linalg.vector_norm(g1[torch.isfinite(g1)].double()))
    assert abs(rep[1]["grad_norm"] - want) <= 1e-12 * want and all(e["update_norm"] > 0 for e in rep)


def test_the_scripts_log_reports_a_skipped_step_at_once(tmp_path, capsys):
    """optim.LayerStatsLog with on_skip (what --layer_stats_on_skip builds) over a three-parameter module: nothing on an applied
    step, one line that names the poisoned parameter right after a skipped one"""
    from hr_viton_amd.optim import Adam, LayerStatsLog

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.a, self.b, self.c = (torch.nn.Parameter(w.cuda()) for w in G.start_weights())

    net = Net()
    ps = [net.a, net.b, net.c]
    opt = Adam(ps, lr=G.LR, betas=G.BETAS, eps=G.EPS, device_step=True, skip_nonfinite=True)
    path = str(tmp_path / "run" / "layer_stats.jsonl")
    log = LayerStatsLog(path, 0, 2, True, [("G", opt, net)])
    _step(ps, opt, G.gauss_grad_list(0))
    assert log.after_step(1) == "" and not os.path.exists(path)
    _step(ps, opt, G.poison(G.gauss_grad_list(1), "ninf"))
    text = log.after_step(2)
    assert "nonfinite_G: b(g1/w0/u0)" in text and text.count("=") == 2 and "layers_G: " in text
    out = capsys.readouterr().out
    assert "optimizer G skipped its step" in out and "nonfinite_G: b(g1/w0/u0)" in out
    lines = _read_jsonl(path)
    assert len(lines) == 1 and (lines[0]["step"], lines[0]["opt"]) == (2, "G") and list(lines[0]["params"]) == ["a", "b", "c"]
    assert [e["grad_nonfinite"] for e in lines[0]["params"].values()] == [0, 1, 0]
    _step(ps, opt, G.gauss_grad_list(2))
    assert log.after_step(3) == "" and len(_read_jsonl(path)) == 1


# ---------------------------------------------------------------------------------------------------------------
# 9: capture
# ---------------------------------------------------------------------------------------------------------------
def test_a_captured_report_follows_the_eager_one_and_allocates_nothing():
    ps, opt = _make(True)
    _step(ps, opt, G.gauss_grad_list(9))
    opt.prepare_layer_stats()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        opt.layer_stats(read=False)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    count = lambda: torch.cuda.memory_stats()["allocation.all.allocated"]  # noqa: E731
    with torch.cuda.graph(graph):      # (counted inside: beginning a capture allocates the generator's state itself)
        n0 = count()
        rec = opt.layer_stats(read=False)
        n1 = count()
    assert n1 == n0, "the captured layer_stats(read=False) allocated device memory"
    assert rec.data_ptr() == opt._flat[0]["span_ws"]["records"].data_ptr()
    for s in range(2):
        _step(ps, opt, G.gauss_grad_list(s))
        rec.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        replayed = rec.clone()
        rec.fill_(-1)
        eager = opt.layer_stats(read=False).clone()
        assert torch.equal(replayed, eager), s
        _check_report(opt, opt.layer_stats(), s + 2)


# ---------------------------------------------------------------------------------------------------------------
# 10: through the real backward (the setup of tests/test_gpu_grad_guard.py)
# ---------------------------------------------------------------------------------------------------------------
def _gen_setup(seed, H=256, W=128):
    from argparse import Namespace
    from hr_viton_amd.network_generator import MultiscaleDiscriminator, SPADEGenerator
    opt = Namespace(cuda=True, norm_G="spectralaliasinstance", gen_semantic_nc=7, ngf=8, num_upsampling_layers="most",
                    fine_height=H, fine_width=W, ndf=8, norm_D="spectralinstance", n_layers_D=3, num_D=2,
                    no_ganFeat_loss=False, lambda_feat=10.0, lambda_vgg=10.0, no_vgg_loss=True)
    torch.manual_seed(seed)
    gen = SPADEGenerator(opt, 9)
    gen.init_weights("xavier", 0.02)
    dis = MultiscaleDiscriminator(opt)
    dis.init_weights("xavier", 0.02)
    return opt, gen, dis


def _gen_batch(seed, H=256, W=128, N=1):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(N, 9, H, W, generator=g) * 2 - 1
    lab = torch.randint(0, 7, (N, 1, H // 16, W // 16), generator=g).repeat_interleave(16, 2).repeat_interleave(16, 3)
    seg = torch.zeros(N, 7, H, W).scatter_(1, lab, 1.0)
    real = torch.rand(N, 3, H, W, generator=g) * 2 - 1
    return x, seg, real


def test_the_report_of_a_real_generator_step():
    import hr_viton_amd  # noqa: F401
    from hr_viton_amd import ops, pipeline
    from hr_viton_amd.losses import GANLoss, L1Loss
    from hr_viton_amd.optim import Adam, layer_report
    opt, gen, dis = _gen_setup(5)
    gen.cuda().train()
    dis.cuda().train()
    og = Adam(gen.parameters(), lr=1e-4, betas=(0.0, 0.9), max_grad_norm=1.0, device_step=True)
    od = Adam(dis.parameters(), lr=4e-4, betas=(0.0, 0.9), max_grad_norm=1.0, device_step=True)
    x, seg, real = _gen_batch(6, N=2)
    seen = {}
    for name, o, mod in (("G", og, gen), ("D", od, dis)):
        def capture(o=o, mod=mod, name=name, real_step=o.step):          # the gradients as step() receives them
            seen[name] = {n: (None if p.grad is None else float(torch.linalg.vector_norm(p.grad.detach().double())))
                          for n, p in mod.named_parameters()}
            return real_step()
        o.step = capture
    try:
        pipeline.generator_train_step(opt, gen, dis, GANLoss("hinge"), L1Loss(), None, og, od, x.cuda(), ops.to_nhwc(seg.cuda()), real.cuda())
    finally:
        del og.step, od.step
    for name, o, mod in (("G", og, gen), ("D", od, dis)):
        rep = layer_report(o, mod)
        trainable = [n for n, p in mod.named_parameters() if p.requires_grad]
        assert sorted(rep) == sorted(trainable) and set(trainable) <= set(mod.state_dict())
        assert any(n.endswith("weight_orig") for n in rep) and len(rep) == len(o._flat[0]["spans"])
        assert all(set(e) == {"numel", "grad_norm", "grad_maxabs", "grad_nonfinite", "grad_zeros", "weight_norm", "weight_maxabs",
                              "weight_nonfinite", "update_norm", "update_ratio", "update_nonfinite"} for e in rep.values())
        for n, e in rep.items():
            want = seen[name][n] or 0.0
            assert abs(e["grad_norm"] - want) <= G.ulp32(want), (name, n, e["grad_norm"], want)
            assert e["grad_nonfinite"] == e["weight_nonfinite"] == e["update_nonfinite"] == 0
        total = math.sqrt(sum(e["grad_norm"] ** 2 for e in rep.values()))
        guard = o.guard_stats()["norm"]
        assert total > 0 and abs(total - guard) <= G.ulp32(guard), (name, total, guard)
        st = o._flat[0]
        names = {id(p): n for n, p in mod.named_parameters()}
        never = {names[id(st["spans"][i][0])] for i in st.get("never", ())}
        assert never == {n for n, nrm in seen[name].items() if nrm is None and n in rep}
        for n in never:
            assert rep[n]["grad_zeros"] == rep[n]["numel"] and rep[n]["grad_norm"] == 0.0 and rep[n]["update_norm"] == 0.0
        assert any(e["grad_zeros"] < e["numel"] for e in rep.values())


# ---------------------------------------------------------------------------------------------------------------
# 11: the scripts
# ---------------------------------------------------------------------------------------------------------------
GEN_ARGV = ["--synthetic", "-b", "2", "--fine_height", "256", "--fine_width", "192", "--num_upsampling_layers", "more", "--ngf", "8",
            "--ndf", "8", "--tocg_ngf", "8", "--max_steps", "2", "--num_test_visualize", "0", "--no_vgg_loss", "--board",
            "--tensorboard_count", "1", "--display_count", "1"]
COND_ARGV = ["--synthetic", "-b", "2", "--ngf", "8", "--max_steps", "2", "--num_test_visualize", "0", "--display_count", "1"]
FIELDS = {"numel", "grad_norm", "grad_maxabs", "grad_nonfinite", "grad_zeros", "weight_norm", "weight_maxabs", "weight_nonfinite",
          "update_norm", "update_ratio", "update_nonfinite"}
LAYER_TAGS = ["Layers/%s/%s" % (o, k) for o in "GD" for k in ("update_ratio_max", "update_ratio_min", "nonfinite_params", "zero_grad_params")]


def _read_jsonl(path):
    with open(path) as f:
        return [json.loads(line) for line in f]


def _check_lines(lines, modules):
    assert [(ln["step"], ln["opt"]) for ln in lines] == [(1, "G"), (1, "D"), (2, "G"), (2, "D")]
    for ln in lines:
        assert set(ln) == {"step", "opt", "params"} and ln["params"]
        if modules is not None:
            assert list(ln["params"]) and set(ln["params"]) == modules[ln["opt"]]
        for n, e in ln["params"].items():
            assert set(e) == FIELDS, (n, set(e) ^ FIELDS)
            assert all(v is None or math.isfinite(v) for v in e.values()), (n, e)
            assert e["grad_nonfinite"] == e["weight_nonfinite"] == e["update_nonfinite"] == 0
            # no ratio for a weight of norm zero (biases start there) or a parameter that has never had a gradient
            assert (e["update_ratio"] is None) == (e["weight_norm"] == 0.0 or e["update_norm"] is None)
        assert any(e["grad_norm"] > 0 and e["update_ratio"] for e in ln["params"].values())


def test_train_generator_reports_only_when_asked_and_trains_the_same_bits(tmp_path, capsys):
    import train_generator as tg
    from hr_viton_amd import validate as V

    def run(name, extra):
        torch.manual_seed(0)
        tg.main(["--name", name, "--checkpoint_dir", str(tmp_path / "ck"), "--tensorboard_dir", str(tmp_path / "tb")] + GEN_ARGV + extra)
        sd = {k: torch.load(str(tmp_path / "ck" / name / f), map_location="cpu") for k, f in
              (("gen", "gen_model_final.pth"), ("dis", "dis_model_final.pth"))}
        return sd, V.read_scalars(str(tmp_path / "tb" / name)), capsys.readouterr().out

    sd_a, recs, out = run("a", ["--layer_stats_count", "1", "--layer_stats_top", "3"])
    lines = _read_jsonl(str(tmp_path / "tb" / "a" / "layer_stats.jsonl"))
    _check_lines(lines, None)
    for ln in lines:          # the names are state-dict keys, and every weight and bias of the state dict is reported
        sd = sd_a["gen" if ln["opt"] == "G" else "dis"]
        assert {k for k in sd if k.endswith(("weight", "bias", "weight_orig"))} <= set(ln["params"]) <= set(sd)
        assert any(n.endswith("weight_orig") for n in ln["params"])
    printed = [ln for ln in out.splitlines() if "layers_G: " in ln]
    assert len(printed) == 2 and all("layers_D: " in ln and "nonfinite_" not in ln for ln in printed)
    for ln in printed:
        for tag in "GD":
            named = ln.split("layers_%s: " % tag)[1].split(", ")[0].split()
            assert len(named) == 3 and all("=" in x for x in named), ln
    for step in (1, 2):
        got = {r["tag"]: r["value"] for r in recs if r["step"] == step and r["tag"].startswith("Layers/")}
        assert list(got) == LAYER_TAGS and all(math.isfinite(v) for v in got.values()), got
        assert got["Layers/G/update_ratio_max"] >= got["Layers/G/update_ratio_min"] > 0 and got["Layers/G/nonfinite_params"] == 0
    sd_p, recs_p, out_p = run("p", [])
    assert not os.path.exists(str(tmp_path / "tb" / "p" / "layer_stats.jsonl"))
    assert "layers_G:" not in out_p and "layers_D:" not in out_p and "layer_stats" not in out_p and not any(r["tag"].startswith("Layers/") for r in recs_p)
    for k in ("gen", "dis"):
        assert list(sd_a[k]) == list(sd_p[k]) and all(torch.equal(sd_a[k][n], sd_p[k][n]) for n in sd_p[k]), k


def test_train_condition_writes_its_reports(tmp_path, capsys):
    import train_condition as tc
    torch.manual_seed(0)
    tc.main(["--name", "c", "--checkpoint_dir", str(tmp_path / "ck"), "--tensorboard_dir", str(tmp_path / "tb")] + COND_ARGV
            + ["--layer_stats_count", "1"])
    _check_lines(_read_jsonl(str(tmp_path / "tb" / "c" / "layer_stats.jsonl")), None)
    assert "layers_G: " in capsys.readouterr().out


def test_on_skip_without_the_skip_is_refused():
    import train_condition as tc
    import train_generator as tg
    for mod, argv in ((tg, GEN_ARGV), (tc, COND_ARGV)):
        with pytest.raises(SystemExit, match="--layer_stats_on_skip needs --skip_nonfinite"):
            mod.main(["--name", "x"] + argv + ["--layer_stats_on_skip"])
