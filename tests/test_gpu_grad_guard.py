"""GPU: the guarded Adam step (csrc/grad_guard.hip; optim.Adam(max_grad_norm=, skip_nonfinite=)) against the float64 restatement of
tests/guard_cases.py, which tests/test_guard_cases_cpu.py holds against torch's clip_grad_norm_ + Adam: the reduction exactly on
integer data at every edge of its geometry and from aligned and 4-byte-aligned pointers, non-finite detection, clipping exactly
(power-of-two scales) on both step-count paths, skipping, capture in a hipGraph, the real backward, two ranks, the script."""
import functools
import math
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import guard_cases as G

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _T():
    import hr_viton_amd  # noqa: F401
    from hr_viton_amd import train_ops
    return train_ops


def _reduce(view, gscale=1.0, max_norm=None, skip=False):
    T = _T()
    rec, part, cnt = T.guard_alloc(view.device)
    part.fill_(float("nan"))          # every slot is written by every launch
    cnt.fill_(-1)
    T.grad_sumsq(view, part, cnt)
    T.grad_guard_finalize(part, cnt, rec, gscale, max_norm, skip)
    return T.guard_read(rec), part, cnt


@functools.lru_cache(maxsize=None)
def _int_case(n):
    g = G.int_grads(n, n)
    return g, G.sumsq_ref(g)


@functools.lru_cache(maxsize=None)
def _gauss_case(n):
    g = G.gauss_grads(n, n + 1)
    return g, G.sumsq_ref(g)


def _view(vals, shift):
    buf, (o, n) = G.banded(vals, shift)
    dbuf = buf.cuda()
    v = dbuf[o:o + n]
    assert v.data_ptr() % 16 == 4 * shift
    return dbuf, v


# ---------------------------------------------------------------------------------------------------------------
# the reduction
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "buf[1:]"])
@pytest.mark.parametrize("n", G.SIZES)
def test_sumsq_is_exact_on_integer_gradients(n, shift):
    vals, (ss, nf) = _int_case(n)
    _, v = _view(vals, shift)
    rec, part, cnt = _reduce(v, skip=True)
    assert rec["nonfinite"] == 0 == nf and int(cnt.sum()) == 0, "a read outside [0, n) met the NaN band"
    assert rec["sumsq"] == ss and float(part.sum()) == ss
    assert rec["norm"] == float(np.float32(math.sqrt(ss))) and rec["scale"] == 1.0 and rec["apply"] == 1
    assert (rec["steps"], rec["skipped"], rec["clipped"]) == (1, 0, 0)


@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "buf[1:]"])
@pytest.mark.parametrize("n", G.SIZES)
def test_norm_of_gaussian_gradients_within_one_ulp_and_bit_identical_between_runs(n, shift):
    vals, (ss, nf) = _gauss_case(n)
    _, v = _view(vals, shift)
    rec, part, cnt = _reduce(v)
    want = G.finalize_ref(ss, nf)["norm"]
    # fp64 accumulation leaves ~n 2^-53 of relative error; what remains is the double rounding of sqrt and the cast
    assert abs(rec["norm"] - want) <= G.ulp32(want), (rec["norm"], want)
    assert rec["nonfinite"] == 0
    rec2, part2, cnt2 = _reduce(v)
    assert torch.equal(part.view(torch.int64), part2.view(torch.int64)) and torch.equal(cnt, cnt2)
    assert rec2 == rec


@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "buf[1:]"])
@pytest.mark.parametrize("n", G.SIZES)
def test_one_nonfinite_element_anywhere_is_counted_and_skips(n, shift):
    vals, _ = _int_case(n)
    _, v = _view(vals, shift)
    pos = G.block_edge_positions(n, shift)
    for p in pos:
        keep = float(vals[p])
        for kind, val in G.POISONS.items():
            v[p] = val
            rec, _, cnt = _reduce(v, skip=True)
            assert rec["nonfinite"] == 1 and int(cnt.sum()) == 1 and rec["apply"] == 0 and rec["skipped"] == 1, (p, kind, rec)
            assert _reduce(v, skip=False)[0]["apply"] == 1
        v[p] = keep
    for i, p in enumerate(pos):
        v[p] = list(G.POISONS.values())[i % 3]
    rec, _, _ = _reduce(v, skip=True)
    assert rec["nonfinite"] == len(pos) and rec["apply"] == 0


def test_squares_are_taken_in_fp64_and_a_norm_beyond_fp32_counts_as_nonfinite():
    vals = G.int_grads(1025, 3)
    vals[517] = 1e30
    _, v = _view(vals, 1)
    rec, _, _ = _reduce(v, skip=True)
    want = G.finalize_ref(*G.sumsq_ref(vals), skip_nonfinite=True)
    assert rec["nonfinite"] == 0 and math.isfinite(rec["norm"]) and rec["apply"] == 1
    assert abs(rec["norm"] - want["norm"]) <= G.ulp32(want["norm"]) and rec["norm"] >= 9.99e29
    vals = torch.zeros(1025)
    vals[3] = vals[1024] = 3e38
    _, v = _view(vals, 0)
    rec, _, _ = _reduce(v, skip=True)
    assert rec["nonfinite"] == 0 and math.isinf(rec["norm"]) and rec["apply"] == 0 and rec["skipped"] == 1
    assert math.isfinite(rec["sumsq"]) and rec["sumsq"] == G.sumsq_ref(vals)[0]
    # clipping on, skipping off: torch's clip_grad_norm_(error_if_nonfinite=False) -- an Inf norm gives scale 0, a NaN norm NaN
    rec, _, _ = _reduce(v, max_norm=1.0)
    assert rec["apply"] == 1 and rec["scale"] == 0.0 and rec["clipped"] == 1
    v[7] = float("nan")
    rec, _, _ = _reduce(v, max_norm=1.0)
    assert rec["apply"] == 1 and math.isnan(rec["scale"]) and math.isnan(rec["norm"]) and rec["clipped"] == 0


# ---------------------------------------------------------------------------------------------------------------
# the optimizer
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


def _step(ps, opt, grads, mul=1.0):
    for p, g in zip(ps, grads):
        p.grad = (g * mul).cuda()
    opt.step()


def _state(opt):
    st = opt._flat[0]
    out = {k: st[k].clone() for k in ("w", "m", "v")}
    if "step_dev" in st:
        out["step_dev"] = st["step_dev"].clone()
    return out


def _same(a, b, keys=("w", "m", "v")):
    return all(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for k in keys)


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("world", [1, 2], ids=["gscale1", "gscale0.5"])
@pytest.mark.parametrize("device_step", [False, True], ids=["host_count", "device_step"])
def test_clipping_by_a_power_of_two_is_the_unguarded_kernel_on_prescaled_gradients(device_step, world, k):
    norm = G.SQUARE_NORM / world
    pg, og = _make(device_step, world, max_grad_norm=norm / 2 ** k)
    pp, op = _make(device_step, world)
    for s in range(3):
        gr = G.square_grads(s)
        _step(pg, og, gr)
        _step(pp, op, gr, 2.0 ** -k)
        if s in (0, 2):
            assert _same(_state(og), _state(op)), s
            assert all(torch.equal(a, b) for a, b in zip(pg, pp))
    st = og.guard_stats()
    assert st["norm"] == norm and st["scale"] == 2.0 ** -k and (st["steps"], st["clipped"], st["skipped"]) == (3, 3, 0)
    assert not torch.equal(pg[0].detach().cpu(), G.start_weights()[0])
    assert op.guard_stats() is None


@pytest.mark.parametrize("device_step", [False, True], ids=["host_count", "device_step"])
def test_inactive_clipping_is_bitwise_the_unguarded_optimizer(device_step):
    pg, og = _make(device_step, max_grad_norm=1e6)
    pp, op = _make(device_step)
    for s in range(3):
        gr = G.gauss_grad_list(s)
        _step(pg, og, gr)
        _step(pp, op, gr)
        assert _same(_state(og), _state(op)), s
        assert og.guard_stats()["scale"] == 1.0
    assert og.guard_stats()["clipped"] == 0


@pytest.mark.parametrize("device_step", [False, True], ids=["host_count", "device_step"])
def test_clipping_against_torch(device_step):
    """fp32 clip_grad_norm_ + torch.optim.Adam on the CPU; the bound is twice torch fp32's own error against the float64
    restatement on the same case (the project's rule for its torch comparisons)."""
    max_norm = 5.0
    w0 = G.start_weights()
    steps = [G.gauss_grad_list(s) for s in range(3)]
    ref = G.adam_ref64(w0, steps, max_norm=max_norm)
    t32 = G.torch_clip_adam(w0, steps, max_norm)
    pg, og = _make(device_step, max_grad_norm=max_norm)
    for s in range(3):
        _step(pg, og, steps[s])
        torch_err = G.rel_err(t32[s], ref[s]["w"])
        got = [p.detach().cpu() for p in pg]
        hip_vs_torch = G.rel_err(got, [t.double() for t in t32[s]])
        hip_err = G.rel_err(got, ref[s]["w"])
        print("step %d: torch fp32 vs float64 %.3e | HIP vs torch fp32 %.3e | HIP vs float64 %.3e" % (s + 1, torch_err, hip_vs_torch, hip_err))
        assert hip_vs_torch <= 2 * torch_err, "step %d: HIP vs torch fp32 %.3e > 2 x (torch fp32 vs float64 %.3e); HIP vs float64 %.3e" % (
            s + 1, hip_vs_torch, torch_err, hip_err)
    st = og.guard_stats()
    want = ref[2]["rec"]
    assert abs(st["norm"] - want["norm"]) <= G.ulp32(want["norm"]) and st["clipped"] == 3
    assert abs(st["scale"] - want["scale"]) <= 2 * G.ulp32(want["scale"])


def test_a_poisoned_step_is_skipped_whole():
    pg, og = _make(True, max_grad_norm=5.0, skip_nonfinite=True)
    pp, op = _make(True, max_grad_norm=5.0, skip_nonfinite=True)
    a, b, c = G.gauss_grad_list(0), G.poison(G.gauss_grad_list(1), "pinf"), G.gauss_grad_list(2)
    _step(pg, og, a)
    s1 = _state(og)
    assert int(s1["step_dev"]) == 1
    _step(pg, og, b)
    s2 = _state(og)
    assert _same(s1, s2) and int(s2["step_dev"]) == 1
    st = og.guard_stats()
    assert (st["apply"], st["nonfinite"], st["steps"], st["skipped"]) == (0, 1, 2, 1)
    _step(pg, og, c)
    _step(pp, op, a)
    _step(pp, op, c)
    assert _same(_state(og), _state(op)) and int(_state(og)["step_dev"]) == 2
    assert all(bool(torch.isfinite(p).all()) for p in pg)
    sd = og.state_dict()
    assert all(int(sd["state"][i]["step"]) == 2 for i in range(len(pg)))
    st = og.guard_stats()
    assert (st["apply"], st["steps"], st["skipped"], st["clipped"]) == (1, 3, 1, 2)
    # the float64 restatement takes the same decisions
    ref = G.adam_ref64(G.start_weights(), [a, b, c], max_norm=5.0, skip_nonfinite=True)
    assert ref[2]["step"] == 2 and {k: ref[2]["rec"][k] for k in ("steps", "skipped", "clipped")} == {k: st[k] for k in ("steps", "skipped", "clipped")}
    assert G.rel_err([p.detach().cpu() for p in pg], ref[2]["w"]) < 1e-5


def test_skip_nonfinite_needs_the_device_step_count():
    from hr_viton_amd.ops import HrvError
    from hr_viton_amd.optim import Adam
    with pytest.raises(HrvError, match="device_step=True"):
        Adam([torch.nn.Parameter(torch.zeros(4, device="cuda"))], skip_nonfinite=True)
    with pytest.raises(HrvError):
        Adam([torch.nn.Parameter(torch.zeros(4, device="cuda"))], max_grad_norm=-1.0)


def test_the_default_optimizer_has_no_guard():
    ps, opt = _make()
    _step(ps, opt, G.gauss_grad_list(0))
    assert not opt.guarded and opt.guard_record is None and opt.guard_stats() is None and opt.guard_records() == [None]
    assert not any(k.startswith("guard") for k in opt._flat[0])
    ps, opt = _make(max_grad_norm=1.0)
    _step(ps, opt, G.gauss_grad_list(0))
    assert opt.guard_record.dtype == torch.int32 and opt.guard_record.is_cuda and opt.guard_record.numel() == _T().GUARD_WORDS


def test_device_step_leaves_a_never_trained_parameter_alone():
    """A parameter that never receives a gradient (a block the configured generator does not use: train_generator.py with
    --num_upsampling_layers more) rides along in the device-step launch: zero gradient on zero moments is an exact no-op.  One that
    joins later would need its own step count and is refused."""
    from hr_viton_amd.ops import HrvError
    from hr_viton_amd.optim import Adam
    kw = dict(lr=G.LR, betas=G.BETAS, eps=G.EPS, device_step=True, max_grad_norm=5.0, skip_nonfinite=True)
    ps = [torch.nn.Parameter(w.cuda()) for w in G.start_weights()]
    idle = torch.nn.Parameter(torch.randn(7, generator=torch.Generator().manual_seed(1)).cuda())
    idle0 = idle.detach().clone()
    opt = Adam(ps[:1] + [idle] + ps[1:], **kw)
    pp, op = _make(True, max_grad_norm=5.0, skip_nonfinite=True)
    for s in range(2):
        _step(ps, opt, G.gauss_grad_list(s))
        _step(pp, op, G.gauss_grad_list(s))
    assert all(torch.equal(a, b) for a, b in zip(ps, pp)) and torch.equal(idle.detach(), idle0)
    a, b = opt.guard_stats(), op.guard_stats()      # (the spans sit elsewhere in the buffer: the float64 sum may differ in its last bit)
    assert all(a[k] == b[k] for k in ("norm", "scale", "apply", "steps", "skipped", "clipped")) and a["steps"] == 2
    # like torch.optim.Adam, state_dict() holds no state for the parameter that was never stepped; a fresh optimizer that loads it
    # goes on bit-identically
    sd = opt.state_dict()
    assert sorted(sd["state"]) == [0, 2, 3] and all(int(e["step"]) == 2 for e in sd["state"].values())
    ps2 = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    idle2 = torch.nn.Parameter(idle0.clone())
    opt2 = Adam(ps2[:1] + [idle2] + ps2[1:], **kw)
    opt2.load_state_dict(sd)
    _step(ps, opt, G.gauss_grad_list(2))
    _step(ps2, opt2, G.gauss_grad_list(2))
    assert all(torch.equal(a, b) for a, b in zip(ps, ps2)) and torch.equal(idle2.detach(), idle0)
    assert int(opt2.state_dict()["state"][0]["step"]) == 3
    idle.grad = torch.ones(7, device="cuda")
    with pytest.raises(HrvError, match="every parameter needs a gradient"):
        opt.step()


def test_a_captured_step_follows_the_eager_sequence():
    """opt.step() captured once (one stream, no parallel branches) over static gradient tensors; between replays three
    gradients are written into them: finite, poisoned, finite"""
    kw = dict(max_grad_norm=5.0, skip_nonfinite=True)
    pe, oe = _make(True, **kw)
    pc, oc = _make(True, **kw)
    warm = G.gauss_grad_list(9)
    seq = [G.gauss_grad_list(0), G.poison(G.gauss_grad_list(1)), G.gauss_grad_list(2)]
    static = [torch.zeros(s, device="cuda") for s in G.SHAPES]
    for p, t in zip(pc, static):
        p.grad = t

    def load(grads):
        for t, g in zip(static, grads):
            t.copy_(g.cuda())

    _step(pe, oe, warm)
    load(warm)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        oc.step()                      # eager: the flat buffers, the device scalars, the guard record and workspace
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert _same(_state(oe), _state(oc))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        oc.step()
    for i, grads in enumerate(seq):
        _step(pe, oe, grads)
        load(grads)
        oc.push_lr()
        graph.replay()
        torch.cuda.synchronize()
        assert _same(_state(oe), _state(oc), ("w", "m", "v", "step_dev")), i
        assert torch.equal(oe.guard_record, oc.guard_record), (i, oe.guard_stats(), oc.guard_stats())
    st = oc.guard_stats()
    assert (st["steps"], st["skipped"]) == (4, 1) and int(_state(oc)["step_dev"]) == 3


# ---------------------------------------------------------------------------------------------------------------
# through the real backward
# ---------------------------------------------------------------------------------------------------------------
def _gen_setup(seed, H=256, W=128, N=1):
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


def test_the_norm_of_a_real_generator_step_and_the_zero_padding_of_the_flat_buffer():
    """One generator train step (ngf = ndf = 8, 256x128) with clipping on: the record's norm is the norm of the parameters'
    gradients gathered on the host in float64, to one fp32 ulp -- which also needs the padding between the spans of the flat
    gradient buffer to be zero, asserted here directly (the reduction runs over the whole buffer)."""
    import hr_viton_amd  # noqa: F401
    from hr_viton_amd import ops, pipeline
    from hr_viton_amd.losses import GANLoss, L1Loss
    from hr_viton_amd.optim import Adam
    opt, gen, dis = _gen_setup(5)
    gen.cuda().train()
    dis.cuda().train()
    og = Adam(gen.parameters(), lr=1e-4, betas=(0.0, 0.9), max_grad_norm=1.0)
    od = Adam(dis.parameters(), lr=4e-4, betas=(0.0, 0.9), max_grad_norm=1.0)
    x, seg, real = _gen_batch(6, N=2)
    seen = {}
    for it in range(2):          # the second iteration produces every gradient directly in its slot of the flat buffer
        for name, o, mod in (("G", og, gen), ("D", od, dis)):
            def capture(o=o, mod=mod, name=name, real_step=o.step):
                seen[name] = sum(float((p.grad.detach().double() ** 2).sum()) for p in mod.parameters() if p.grad is not None)
                return real_step()
            o.step = capture
        try:
            pipeline.generator_train_step(opt, gen, dis, GANLoss("hinge"), L1Loss(), None, og, od, x.cuda(), ops.to_nhwc(seg.cuda()),
                                          real.cuda())
        finally:
            del og.step, od.step
        for name, o in (("G", og), ("D", od)):
            st, flat = o.guard_stats(), o._flat[0]
            want = float(np.float32(math.sqrt(seen[name])))
            assert seen[name] > 0 and abs(st["norm"] - want) <= G.ulp32(want), (it, name, st["norm"], want)
            assert st["nonfinite"] == 0 and st["steps"] == it + 1
            pads = [flat["g"][off + k:off + (k + 3) // 4 * 4] for _, off, k in flat["spans"] if k % 4]
            assert pads or name == "D"
            assert all(float(p.abs().max()) == 0.0 for p in pads), (it, name)
    assert og.guard_stats()["clipped"] >= 1


# ---------------------------------------------------------------------------------------------------------------
# two ranks
# ---------------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_worker(rank, world, port, q):
    try:
        sys.path.insert(0, ROOT)
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        os.environ.update(RANK=str(rank), LOCAL_RANK="0", WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                          MASTER_PORT=str(port), HRV_DIST_BACKEND="gloo")
        import faulthandler
        from conftest import diag_path
        _wd = open(diag_path(f"dp_guard_rank{rank}_stacks.txt"), "w")
        faulthandler.dump_traceback_later(90, repeat=False, file=_wd, exit=False)
        import torch.distributed as dist
        import hr_viton_amd  # noqa: F401
        from hr_viton_amd import dist as hdist
        from hr_viton_amd import ops
        from hr_viton_amd.gen_train import attach_grad_sync
        from hr_viton_amd.losses import GANLoss, L1Loss
        from hr_viton_amd.optim import Adam
        from hr_viton_amd.parallel import broadcast_module
        from hr_viton_amd.pipeline import generator_train_step
        hdist.init_from_env()
        dev = torch.device("cuda", 0)
        torch.cuda.set_device(0)
        opt, gen, dis = _gen_setup(200 + rank)
        gen.to(dev).train()
        dis.to(dev).train()
        broadcast_module(gen)
        broadcast_module(dis)
        og = Adam(gen.parameters(), lr=1e-4, betas=(0.0, 0.9), device_step=True, skip_nonfinite=True)
        od = Adam(dis.parameters(), lr=4e-4, betas=(0.0, 0.9), device_step=True, skip_nonfinite=True)
        sg, sd = og.make_grad_sync(bucket_mb=0.25), od.make_grad_sync(bucket_mb=4.0)
        attach_grad_sync(sg)
        attach_grad_sync(sd)
        w0 = torch.cat([p.detach().flatten() for p in gen.parameters()]).clone()
        after = []
        for step in range(3):
            x, seg, real = _gen_batch(1000 + 10 * step + rank)
            if step == 1 and rank == 1:
                x[0, 4, 100, 50] = float("inf")            # one rank's input image holds one Inf
            torch.manual_seed(77 + rank + step)
            generator_train_step(opt, gen, dis, GANLoss("hinge"), L1Loss(), None, og, od, x.to(dev), ops.to_nhwc(seg.to(dev)),
                                 real.to(dev), sg, sd)
            after.append(torch.cat([p.detach().flatten() for p in gen.parameters()]).clone())
        torch.cuda.synchronize()
        wg = after[-1]
        wd = torch.cat([p.detach().flatten() for p in dis.parameters()])
        sums = torch.stack([t.double().sum() for t in (wg, wd)] + [t.double().abs().sum() for t in (wg, wd)]).cpu()
        gathered = [torch.zeros_like(sums) for _ in range(world)]
        dist.all_gather(gathered, sums)
        sg_, sd_ = og.guard_stats(), od.guard_stats()
        q.put((rank, [t.tolist() for t in gathered], float((wg - w0).abs().max()), bool(torch.isfinite(wg).all() and torch.isfinite(wd).all()),
               bool(torch.equal(after[0], after[1])), bool(torch.equal(after[1], after[2])),
               {k: (sg_[k], sd_[k]) for k in ("steps", "skipped", "apply")}, int(og.state_dict()["state"][0]["step"])))
        dist.barrier()
        dist.destroy_process_group()
    except Exception:  # noqa: BLE001
        import traceback
        q.put((rank, "ERROR: " + traceback.format_exc()))


def test_two_ranks_skip_the_step_one_of_them_poisoned():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=150) for _ in range(2))
    for p in procs:
        p.join(60)
    for r in res:
        assert len(r) == 8, r
    (_, g0, moved0, fin0, same01_0, same12_0, st0, n0), (_, g1, moved1, fin1, same01_1, same12_1, st1, n1) = res
    assert g0 == g1 and g0[0] == g0[1], ("replica weight checksums differ", g0, g1)      # bitwise identical replicas
    assert fin0 and fin1 and moved0 > 1e-6 and moved0 == moved1
    assert same01_0 and same01_1 and not same12_0 and not same12_1      # step 2 moved nothing on either rank, step 3 did
    for st in (st0, st1):
        assert st["steps"] == (3, 3) and st["skipped"] == (1, 1) and st["apply"] == (1, 1), st
    assert n0 == n1 == 2


# ---------------------------------------------------------------------------------------------------------------
# the script
# ---------------------------------------------------------------------------------------------------------------
GEN_ARGV = ["--synthetic", "-b", "2", "--fine_height", "256", "--fine_width", "192", "--num_upsampling_layers", "more", "--ngf", "8",
            "--ndf", "8", "--tocg_ngf", "8", "--max_steps", "2", "--num_test_visualize", "0", "--no_vgg_loss", "--board",
            "--tensorboard_count", "1", "--display_count", "1"]
GRAD_TAGS = ["Grad/norm_G", "Grad/norm_D", "Grad/skipped_G", "Grad/skipped_D", "Grad/clipped_G", "Grad/clipped_D"]


def test_train_generator_records_the_guard_only_when_asked(tmp_path, capsys):
    import train_generator as tg
    from hr_viton_amd import validate as V

    def run(name, extra):
        torch.manual_seed(0)
        tg.main(["--name", name, "--checkpoint_dir", str(tmp_path / "ck"), "--tensorboard_dir", str(tmp_path / "tb")] + GEN_ARGV + extra)
        return V.read_scalars(str(tmp_path / "tb" / name)), capsys.readouterr().out

    recs, out = run("g", ["--max_grad_norm_G", "1", "--skip_nonfinite"])
    for step in (1, 2):
        got = {r["tag"]: r["value"] for r in recs if r["step"] == step and r["tag"].startswith("Grad/")}
        assert list(got) == GRAD_TAGS and all(np.isfinite(v) for v in got.values()), got
        assert got["Grad/norm_G"] > 0 and got["Grad/norm_D"] > 0 and got["Grad/skipped_G"] == 0 == got["Grad/skipped_D"]
        assert got["Grad/norm_G"] > 1 and got["Grad/clipped_D"] == 0 and got["Grad/clipped_G"] == step      # clipped at every step
    assert out.count("gnorm_G:") == 2 and "skipped_D: 0" in out and "skip_nonfinite=True" in out
    recs, out = run("p", [])
    assert recs and not any(r["tag"].startswith("Grad/") for r in recs)
    assert "gnorm" not in out and "skip_nonfinite" not in out and "max_grad_norm" not in out
