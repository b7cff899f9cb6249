"""GPU: the data-parallel TRAINING path end to end with two ranks (both on cuda:0, gloo carrying the CUDA
tensors -- RCCL refuses two ranks on one device; the collective calls, bucket logic, in-place flat-buffer
reduction, fused Adam and replica broadcast are the ones the 8-GPU RCCL run uses)."""
import os
import socket
import sys

import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _watchdog(tag, rank):
    """a hung rank writes its Python stacks to test_diagnostics/ instead of dying silently with the parent's timeout"""
    import faulthandler
    from conftest import diag_path
    f = open(diag_path(f"dp_{tag}_rank{rank}_stacks.txt"), "w")
    faulthandler.dump_traceback_later(90, repeat=False, file=f, exit=False)
    return f


def _worker(rank, world, port, q):
    try:
        sys.path.insert(0, ROOT)
        _wd = _watchdog("cond", rank)
        os.environ.update(RANK=str(rank), LOCAL_RANK="0", WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                          MASTER_PORT=str(port), HRV_DIST_BACKEND="gloo")
        import torch.distributed as dist
        import torch.nn as nn
        import hr_viton_amd  # noqa: F401
        from hr_viton_amd import dist as hdist
        from hr_viton_amd.gen_train import attach_grad_sync
        from hr_viton_amd.losses import L1Loss
        from hr_viton_amd.networks import ConditionGenerator, GANLoss, define_D
        from hr_viton_amd.optim import Adam
        from hr_viton_amd.parallel import broadcast_module
        from hr_viton_amd.pipeline import condition_train_step
        import train_condition as tc
        hdist.init_from_env()
        dev = torch.device("cuda", 0)
        torch.cuda.set_device(0)
        opt = tc.get_opt(["--synthetic", "--Ddownx2", "--lasttvonly", "--interflowloss", "-b", "2", "--fine_height", "128",
                          "--fine_width", "96", "--ngf", "8", "--no_vgg_loss"])
        torch.manual_seed(100 + rank)                   # replicas start different; broadcast makes them equal
        tocg = ConditionGenerator(opt, 4, 16, 13, ngf=8, norm_layer=nn.BatchNorm2d).to(dev).train()
        D = define_D(input_nc=33, Ddownx2=True, Ddropout=False, n_layers_D=3, spectral=False, num_D=2).to(dev).train()
        broadcast_module(tocg)
        broadcast_module(D)
        w0 = torch.cat([p.detach().flatten() for p in tocg.parameters()]).clone()
        og = Adam(tocg.parameters(), lr=2e-4, betas=(0.5, 0.999))
        od = Adam(D.parameters(), lr=2e-4, betas=(0.5, 0.999))
        sg, sd = og.make_grad_sync(bucket_mb=0.25), od.make_grad_sync(bucket_mb=4.0)
        attach_grad_sync(sg)
        attach_grad_sync(sd)
        assert len(sg.buckets) >= 2
        losses = None
        for step in range(2):
            batch = tc.synthetic_batch(opt, 1, 50 + 10 * step + rank, dev)      # a different sample per rank
            losses = condition_train_step(opt, tocg, D, L1Loss(), None, GANLoss(use_lsgan=True), og, od, batch, sg, sd)
        torch.cuda.synchronize()
        wg = torch.cat([p.detach().flatten() for p in tocg.parameters()])
        wd = torch.cat([p.detach().flatten() for p in D.parameters()])
        sums = torch.stack([wg.double().sum(), wg.double().abs().sum(), wd.double().sum(), wd.double().abs().sum()]).cpu()
        gathered = [torch.zeros_like(sums) for _ in range(world)]
        dist.all_gather(gathered, sums)
        moved = float((wg - w0).abs().max())
        q.put((rank, [g.tolist() for g in gathered], moved, float(losses["loss_G"].detach()), float(losses["loss_D"].detach())))
        dist.barrier()
        dist.destroy_process_group()
    except Exception:  # noqa: BLE001
        import traceback
        q.put((rank, "ERROR: " + traceback.format_exc()))


def test_two_rank_condition_training_keeps_replicas_identical():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=150) for _ in range(2))
    for p in procs:
        p.join(60)
    for r in res:
        assert len(r) == 5, r
    (_, g0, moved0, lg0, ld0), (_, g1, moved1, lg1, ld1) = res
    assert g0 == g1 and g0[0] == g0[1], ("replica weight checksums differ", g0, g1)      # bitwise identical replicas
    assert moved0 > 1e-5 and moved0 == moved1
    assert all(map(lambda v: v == v and abs(v) < 1e6, (lg0, ld0, lg1, ld1)))
    assert lg0 != lg1                                   # the ranks really saw different data


def _gen_worker(rank, world, port, q):
    """Two ranks of train_generator.py's iteration (G step + D step): SPADE generator + PatchGAN, spectral norm in
    training mode (one power iteration per forward on every rank -- u, v are buffers, never all-reduced), per-rank
    data and SPADE noise, gradients summed by GradSync from inside the backward plans, fused Adam."""
    try:
        sys.path.insert(0, ROOT)
        os.environ.update(RANK=str(rank), LOCAL_RANK="0", WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                          MASTER_PORT=str(port), HRV_DIST_BACKEND="gloo")
        _wd = _watchdog("gen", rank)
        from argparse import Namespace
        import torch.distributed as dist
        import hr_viton_amd  # noqa: F401
        from hr_viton_amd import dist as hdist
        from hr_viton_amd import ops
        from hr_viton_amd.gen_train import attach_grad_sync
        from hr_viton_amd.losses import GANLoss, L1Loss
        from hr_viton_amd.network_generator import MultiscaleDiscriminator, SPADEGenerator
        from hr_viton_amd.optim import Adam
        from hr_viton_amd.parallel import broadcast_module
        from hr_viton_amd.pipeline import generator_train_step
        hdist.init_from_env()
        dev = torch.device("cuda", 0)
        torch.cuda.set_device(0)
        H, W = 256, 128
        opt = Namespace(cuda=True, norm_G="spectralaliasinstance", gen_semantic_nc=7, ngf=8, num_upsampling_layers="most",
                        fine_height=H, fine_width=W, ndf=8, norm_D="spectralinstance", n_layers_D=3, num_D=2,
                        no_ganFeat_loss=False, lambda_feat=10.0, lambda_vgg=10.0, no_vgg_loss=True)
        torch.manual_seed(200 + rank)                   # replicas start different (weights AND u, v); broadcast equalises
        gen = SPADEGenerator(opt, 9)
        gen.init_weights("xavier", 0.02)
        dis = MultiscaleDiscriminator(opt)
        dis.init_weights("xavier", 0.02)
        gen.to(dev).train()
        dis.to(dev).train()
        broadcast_module(gen)
        broadcast_module(dis)
        og = Adam(gen.parameters(), lr=1e-4, betas=(0.0, 0.9))
        od = Adam(dis.parameters(), lr=4e-4, betas=(0.0, 0.9))
        sg, sd = og.make_grad_sync(bucket_mb=0.25), od.make_grad_sync(bucket_mb=4.0)
        attach_grad_sync(sg)
        attach_grad_sync(sd)
        assert len(sg.buckets) >= 2
        w0 = torch.cat([p.detach().flatten() for p in gen.parameters()]).clone()
        losses = None
        for step in range(2):
            g = torch.Generator().manual_seed(1000 + 10 * step + rank)     # a different sample per rank
            x = (torch.rand(1, 9, H, W, generator=g) * 2 - 1).to(dev)
            lab = torch.randint(0, 7, (1, 1, H // 16, W // 16), generator=g).repeat_interleave(16, 2).repeat_interleave(16, 3)
            seg = torch.zeros(1, 7, H, W).scatter_(1, lab, 1.0).to(dev)
            real = (torch.rand(1, 3, H, W, generator=g) * 2 - 1).to(dev)
            torch.manual_seed(77 + rank + step)                            # per-rank SPADE noise draws
            losses, _ = generator_train_step(opt, gen, dis, GANLoss("hinge"), L1Loss(), None, og, od, x, ops.to_nhwc(seg),
                                             real, sg, sd)
        torch.cuda.synchronize()
        wg = torch.cat([p.detach().flatten() for p in gen.parameters()])
        wd = torch.cat([p.detach().flatten() for p in dis.parameters()])
        uv = torch.cat([b.detach().flatten() for n, b in list(gen.named_buffers()) + list(dis.named_buffers())
                        if n.endswith(("weight_u", "weight_v"))])
        sums = torch.stack([t.double().sum() for t in (wg, wd, uv)] + [t.double().abs().sum() for t in (wg, wd, uv)]).cpu()
        gathered = [torch.zeros_like(sums) for _ in range(world)]
        dist.all_gather(gathered, sums)
        q.put((rank, [t.tolist() for t in gathered], float((wg - w0).abs().max()), float(losses["GAN_Feat"].detach()),
               float(losses["D_Fake"].detach())))
        dist.barrier()
        dist.destroy_process_group()
    except Exception:  # noqa: BLE001
        import traceback
        q.put((rank, "ERROR: " + traceback.format_exc()))


def test_two_rank_generator_training_keeps_replicas_identical():
    """train_generator.py's DP iteration (train_generator.py:171-178 -> one process per GPU + gradient all-reduce):
    after two iterations on different per-rank data the generator, the PatchGAN AND the spectral-norm (u, v)
    buffers are bitwise identical on both ranks."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_gen_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=150) for _ in range(2))
    for p in procs:
        p.join(60)
    for r in res:
        assert len(r) == 5, r
    (_, g0, moved0, lf0, ld0), (_, g1, moved1, lf1, ld1) = res
    assert g0 == g1 and g0[0] == g0[1], ("replica checksums (G weights, D weights, spectral u/v) differ", g0, g1)
    assert moved0 > 1e-6 and moved0 == moved1
    assert all(map(lambda v: v == v and abs(v) < 1e6, (lf0, ld0, lf1, ld1)))
    assert lf0 != lf1                                   # the ranks really saw different data


# ------------------------------------------------------------------------------------------------------------------
# "replicas are right", not only "replicas agree": two ranks x one sample == one process x the two samples
# ------------------------------------------------------------------------------------------------------------------
def _eq_setup(dev):
    """identical on every caller: SPADE generator + PatchGAN (ngf = ndf = 8, 256x128), two samples, two noise sets"""
    from argparse import Namespace
    from hr_viton_amd.network_generator import MultiscaleDiscriminator, SPADEGenerator
    H, W = 256, 128
    opt = Namespace(cuda=True, norm_G="spectralaliasinstance", gen_semantic_nc=7, ngf=8, num_upsampling_layers="most",
                    fine_height=H, fine_width=W, ndf=8, norm_D="spectralinstance", n_layers_D=3, num_D=2,
                    no_ganFeat_loss=False, lambda_feat=10.0, lambda_vgg=10.0, no_vgg_loss=True)
    torch.manual_seed(300)
    gen = SPADEGenerator(opt, 9)
    gen.init_weights("xavier", 0.02)
    dis = MultiscaleDiscriminator(opt)
    dis.init_weights("xavier", 0.02)
    g = torch.Generator().manual_seed(301)
    with torch.no_grad():
        for n_, p in list(gen.named_parameters()) + list(dis.named_parameters()):
            if n_.endswith("noise_scale"):
                p.copy_(0.2 * torch.randn(p.shape, generator=g))
            elif n_.endswith("weight") or n_.endswith("weight_orig"):
                p.mul_(8.0)
    gen.to(dev).train()
    dis.to(dev).train()
    x = torch.rand(2, 9, H, W, generator=g) * 2 - 1
    lab = torch.randint(0, 7, (2, 1, H // 16, W // 16), generator=g).repeat_interleave(16, 2).repeat_interleave(16, 3)
    seg = torch.zeros(2, 7, H, W).scatter_(1, lab, 1.0)
    real = torch.rand(2, 3, H, W, generator=g) * 2 - 1
    noises = []
    for _ in range(2):                       # G step, D step
        nz = {}
        for j, name in enumerate(gen._blocks()):
            h, w = gen.sh << j, gen.sw << j
            k = 3 if getattr(gen, name).learned_shortcut else 2
            nz[name] = [torch.randn(2, w, h, 1, generator=g) for _ in range(k)]
        noises.append(nz)
    return opt, gen, dis, x, seg, real, noises


def _eq_run(opt, gen, dis, x, seg, real, noises, sl, dev, sync):
    """one full iteration on the samples ``sl``; returns the gradients as the optimizers saw them (mean over the global
    batch) and the post-step weights"""
    from hr_viton_amd import ops
    from hr_viton_amd.gen_train import attach_grad_sync
    from hr_viton_amd.losses import GANLoss, L1Loss
    from hr_viton_amd.optim import Adam
    from hr_viton_amd.pipeline import generator_train_step
    og = Adam(gen.parameters(), lr=1e-4, betas=(0.0, 0.9))
    od = Adam(dis.parameters(), lr=4e-4, betas=(0.0, 0.9))
    sg = sd = None
    world = 1
    if sync:
        import torch.distributed as dist
        world = dist.get_world_size()
        sg, sd = og.make_grad_sync(bucket_mb=0.25), od.make_grad_sync(bucket_mb=0.05)
        attach_grad_sync(sg)
        attach_grad_sync(sd)
        assert len(sg.buckets) >= 2 and len(sd.buckets) >= 2      # gradients cross bucket boundaries
    grads = {}
    step_g, step_d = og.step, od.step

    def cap(mod, tag, stepfn):
        def f():
            if sg is not None:
                (sg if tag == "G" else sd).wait()     # the optimizer waits too; here the summed gradients are read first
            grads.update({tag + "." + n: p.grad.detach().float().cpu().clone() / world for n, p in mod.named_parameters()
                          if p.grad is not None})
            return stepfn()
        return f
    og.step, od.step = cap(gen, "G", step_g), cap(dis, "D", step_d)
    pick = lambda nz: {k: [z[sl].to(dev).contiguous() for z in v] for k, v in nz.items()}      # noqa: E731
    generator_train_step(opt, gen, dis, GANLoss("hinge"), L1Loss(), None, og, od, x[sl].to(dev), ops.to_nhwc(seg[sl].to(dev)),
                         real[sl].to(dev), sg, sd, noise=pick(noises[0]), noise_d=pick(noises[1]))
    torch.cuda.synchronize()
    weights = {"G." + n: p.detach().float().cpu().clone() for n, p in gen.named_parameters()}
    weights.update({"D." + n: p.detach().float().cpu().clone() for n, p in dis.named_parameters()})
    return grads, weights


def _eq_worker(rank, world, port, q):
    try:
        sys.path.insert(0, ROOT)
        os.environ.update(RANK=str(rank), LOCAL_RANK="0", WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                          MASTER_PORT=str(port), HRV_DIST_BACKEND="gloo")
        _wd = _watchdog("eq", rank)
        import torch.distributed as dist
        import hr_viton_amd  # noqa: F401
        from hr_viton_amd import dist as hdist
        hdist.init_from_env()
        dev = torch.device("cuda", 0)
        torch.cuda.set_device(0)
        setup = _eq_setup(dev)
        grads, weights = _eq_run(*setup, slice(rank, rank + 1), dev, True)
        if rank == 0:       # numpy: pickled by value (torch tensors travel as shared-memory handles that die with this process)
            q.put((rank, {k: v.numpy() for k, v in grads.items()}, {k: v.numpy() for k, v in weights.items()}))
        else:
            q.put((rank, None, None))
        dist.barrier()
        dist.destroy_process_group()
    except Exception:  # noqa: BLE001
        import traceback
        q.put((rank, "ERROR: " + traceback.format_exc(), None))


def test_two_rank_iteration_equals_the_single_process_iteration_on_the_concatenated_batch():
    """train_generator.py:171-178 -> DP: InstanceNorm is per sample and every loss is a mean over the batch, so two ranks
    with one sample each (gradients all-reduced in buckets from inside the backward, 1/world folded into the fused Adam)
    must produce the single-process iteration on the two-sample batch: every G and D gradient within fp32 reassociation
    (a wrong 1/world factor, a bucket reduced twice or not at all would be off by a factor), post-step weights equal
    wherever the gradient is not ~0 (Adam's first step is -lr * sign-like)."""
    import hr_viton_amd  # noqa: F401
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_eq_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=200) for _ in range(2)), key=lambda r: r[0])
    for p in procs:
        p.join(60)
    assert not isinstance(res[0][1], str) and not isinstance(res[1][1], str), (res[0][1], res[1][1])
    g2 = {k: torch.from_numpy(v) for k, v in res[0][1].items()}
    w2 = {k: torch.from_numpy(v) for k, v in res[0][2].items()}
    dev = torch.device("cuda", 0)
    g1, w1 = _eq_run(*_eq_setup(dev), slice(0, 2), dev, False)
    assert set(g1) == set(g2) and len(g1) > 100
    worst = 0.0
    for tag in ("G.", "D."):
        gmax = max(float(v.abs().max()) for k, v in g1.items() if k.startswith(tag))
        for k, v in g1.items():
            if k.startswith(tag):
                err = float((g2[k] - v).abs().max()) / max(float(v.abs().max()), 1e-3 * gmax)
                worst = max(worst, err)
                # measured: worst parameter 1.9e-4 (split-K factors and tile shapes depend on the batch size: reassociation);
                # a wrong 1/world factor or a bucket reduced twice / never is off by >= 0.5
                assert err < 1e-3, (k, err)
    gmx = {tag: max(float(v.abs().max()) for k, v in g1.items() if k.startswith(tag)) for tag in ("G.", "D.")}
    for k, v in w1.items():
        g = g1.get(k)
        if g is None:
            continue
        # (a bias in front of an InstanceNorm has an analytically zero gradient: pure round-off, its Adam step is noise)
        big = g.abs() > 1e-3 * gmx[k[:2]]
        if big.any():
            assert float((w2[k] - v)[big].abs().max()) < 2e-6, k
    print("worst relative gradient difference 2 ranks vs 1 process:", worst)


# ------------------------------------------------------------------------------------------------------------------
# the hipGraph-captured iteration under data parallelism: three graph segments, the gradient all-reduces between them
# ------------------------------------------------------------------------------------------------------------------
def _graph_dp_worker(rank, world, port, q):
    try:
        sys.path.insert(0, ROOT)
        os.environ.update(RANK=str(rank), LOCAL_RANK="0", WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                          MASTER_PORT=str(port), HRV_DIST_BACKEND="gloo")
        _wd = _watchdog("graphdp", rank)
        import torch.distributed as dist
        import hr_viton_amd  # noqa: F401
        from hr_viton_amd import dist as hdist
        from hr_viton_amd import gen_train, ops
        from hr_viton_amd.gen_train import attach_grad_sync
        from hr_viton_amd.graph import GraphedIteration, GraphedTrainStep
        from hr_viton_amd.losses import GANLoss, L1Loss
        from hr_viton_amd.optim import Adam
        from hr_viton_amd.parallel import GraphGradSync
        from hr_viton_amd.pipeline import generator_train_step
        hdist.init_from_env()
        dev = torch.device("cuda", 0)
        torch.cuda.set_device(0)

        def build(graph):
            opt, gen, dis, x, seg, real, noises = _eq_setup(dev)      # identical replicas; per-rank sample and noise below
            og = Adam(gen.parameters(), lr=1e-3, betas=(0.0, 0.9), device_step=True)
            od = Adam(dis.parameters(), lr=2e-3, betas=(0.0, 0.9), device_step=True)
            sg, sd = og.make_grad_sync(bucket_mb=0.25, graph=graph), od.make_grad_sync(bucket_mb=0.05, graph=graph)
            attach_grad_sync(sg)
            attach_grad_sync(sd)
            sl = slice(rank, rank + 1)
            pick = lambda nz: {k: [z[sl].to(dev).contiguous() for z in v] for k, v in nz.items()}      # noqa: E731
            inputs = {"x": x[sl].to(dev), "parse7": ops.to_nhwc(seg[sl].to(dev)).t, "im": real[sl].to(dev)}
            return opt, gen, dis, og, od, sg, sd, inputs, pick(noises[0]), pick(noises[1])

        def snapshot(gen, dis, og, od):
            torch.cuda.synchronize()
            sd_ = {"G." + k: v.detach().cpu().clone() for k, v in gen.state_dict().items()}
            sd_.update({"D." + k: v.detach().cpu().clone() for k, v in dis.state_dict().items()})
            for tag, o in (("og", og), ("od", od)):
                st = o._flat[0]
                sd_[tag + ".m"], sd_[tag + ".v"] = st["m"].detach().cpu().clone(), st["v"].detach().cpu().clone()
                sd_[tag + ".step"] = st["step_dev"].detach().cpu().clone()
            return sd_
        # ---- eager data parallel (bucketed GradSync, collectives started from inside the backward): four iterations
        opt, gen, dis, og, od, sg, sd, inputs, nz, nzd = build(False)
        assert len(sg.buckets) >= 2
        for _ in range(4):
            le, _o = generator_train_step(opt, gen, dis, GANLoss("hinge"), L1Loss(), None, og, od, inputs["x"],
                                          ops.Act(inputs["parse7"], 7), inputs["im"], sg, sd, noise=nz, noise_d=nzd)
        want = snapshot(gen, dis, og, od)
        want_l = {k: float(v) for k, v in le.items()}
        # ---- the same start, captured: two eager warm-up iterations (GraphGradSync reduces eagerly there) + two replays
        opt, gen, dis, og, od, sg, sd, inputs, nz, nzd = build(True)
        assert isinstance(sg, GraphGradSync) and isinstance(sd, GraphGradSync)
        gs = GraphedTrainStep(opt, gen, dis, GANLoss("hinge"), L1Loss(), None, og, od, inputs, noise=nz, noise_d=nzd, warmup=2)
        n_graphs, n_cuts = len(gs._it.graphs), len(gs._it.cuts)
        for _ in range(2):
            lg, _o = gs(inputs)
        got = snapshot(gen, dis, og, od)
        bad = [k for k in want if not torch.equal(want[k], got[k])]
        got_l = {k: float(v) for k, v in lg.items()}
        # the bucketed GradSync inside a capture is refused
        refused = False
        try:
            o2 = Adam([torch.nn.Parameter(torch.zeros(64, device=dev))], lr=1e-3, device_step=True)
            o2.make_grad_sync()
            GraphedIteration(lambda: None, (o2,), warmup=1)
        except ops.HrvError:
            refused = True
        wg = torch.cat([p.detach().flatten() for p in gen.parameters()])
        sums = torch.stack([wg.double().sum(), wg.double().abs().sum()]).cpu()
        gathered = [torch.zeros_like(sums) for _ in range(world)]
        dist.all_gather(gathered, sums)
        q.put((rank, n_graphs, n_cuts, bad, want_l == got_l, refused, [t.tolist() for t in gathered], int(got["og.step"]),
               want_l["GAN_Feat"]))
        dist.barrier()
        dist.destroy_process_group()
    except Exception:  # noqa: BLE001
        import traceback
        q.put((rank, "ERROR: " + traceback.format_exc()))


def test_two_rank_graph_segments_equal_the_eager_data_parallel_iterations():
    """graph.GraphedTrainStep under data parallelism (optimizer.make_grad_sync(graph=True)): the iteration is captured as three
    hipGraph segments cut where an optimizer waits for its gradients -- [G forward/backward, D pass of the G step] | all-reduce
    of G's flat gradient buffer | [Adam(G), D-step forward/backward] | all-reduce of D's buffer | [Adam(D)].  Two warm-up
    iterations + two replays end in bit-identical weights, spectral-norm buffers, Adam moments and step counts as four eager
    data-parallel iterations (bucketed GradSync) from the same start, on both ranks, with different data per rank."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_graph_dp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=240) for _ in range(2))
    for p in procs:
        p.join(60)
    for r in res:
        assert len(r) == 9, r
    for rank, n_graphs, n_cuts, bad, same_losses, refused, sums, step, _lf in res:
        assert n_graphs == 3 and n_cuts == 2, (n_graphs, n_cuts)
        assert bad == [], bad[:5]
        assert same_losses and refused and step == 4
        assert sums[0] == sums[1]                       # replicas identical
    assert res[0][8] != res[1][8]                       # the ranks saw different data
