"""GPU: the R1 phase under data parallelism, two ranks of one image each (both on cuda:0, gloo carrying the CUDA tensors, as
tests/test_gpu_lecam_dp.py) against one process on the two images: every rank takes the penalty over its local N, the gradient
all-reduce and the 1 / world of the optimizer step average the phase like any other step."""
import os
import socket
import sys

import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE = "d2_2x64x48"


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
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        _wd = _watchdog("r1", rank)
        os.environ.update(RANK=str(rank), LOCAL_RANK="0", WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                          MASTER_PORT=str(port), HRV_DIST_BACKEND="gloo")
        import torch.distributed as dist
        import hr_viton_amd  # noqa: F401
        import r1_cases as R
        from hr_viton_amd import dist as hdist
        from hr_viton_amd import ops
        from hr_viton_amd.gen_train import attach_grad_sync
        from hr_viton_amd.optim import Adam
        from hr_viton_amd.r1 import R1
        hdist.init_from_env()
        torch.cuda.set_device(0)
        cs = R.PHASE_CASES[CASE]
        D = R.build_d(cs["num_D"], cs["seed"]).cuda().train()
        parse, real = R.phase_inputs(cs)
        parse, real = parse[rank:rank + 1], real[rank:rank + 1]
        parse7 = torch.cat((parse.permute(0, 2, 3, 1), torch.zeros(1, cs["H"], cs["W"], 1)), dim=3).contiguous().cuda()
        od = Adam(D.parameters(), lr=1e-3, betas=(0.0, 0.9))
        sync = od.make_grad_sync(bucket_mb=0.05)
        attach_grad_sync(sync)
        sync.begin()
        od.zero_grad()
        out = R1(R.GAMMA, R.INTERVAL).phase(D, ops.Act(parse7, 7), real.cuda())
        sync.wait()
        torch.cuda.synchronize()
        grads = {n: (sync.grad_of(p) / sync.world).cpu().tolist() for n, p in D.named_parameters()}
        q.put((rank, grads, float(out["r1_penalty"])))
        dist.barrier()
        dist.destroy_process_group()
    except Exception:  # noqa: BLE001
        import traceback
        q.put((rank, "ERROR: " + traceback.format_exc()))


def test_two_ranks_of_one_image_average_to_the_phase_on_two_images():
    from test_gpu_r1 import _phase, _reference
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=150) for _ in range(2)), key=lambda r: r[0])
    for p in procs:
        p.join(60)
    for r in res:
        assert len(r) == 3, r
    out, single = _phase(CASE)
    ref = _reference(CASE)
    # the mean of the two local penalties is the penalty of the two images: inside the scalar's limit of tests/test_gpu_r1.py
    f64, f32 = ref["f64"], ref["f32"]
    dg = float((f32["g"].double() - f64["g"]).abs().max())
    pen_limit = 4.0 * 2.0 * float(f64["g"].abs().sum()) * dg / 2 + 2.0 ** -22 * f64["r1_penalty"]
    assert abs(0.5 * (res[0][2] + res[1][2]) - float(out["r1_penalty"])) <= 2 * pen_limit
    for n, want in single.items():
        limit = 4.0 * float((ref["f32"]["grads"][n].double() - ref["f64"]["grads"][n]).abs().max())
        a, b = torch.tensor(res[0][1][n]), torch.tensor(res[1][1][n])
        assert torch.equal(a, b), n                                 # both ranks hold the same all-reduced gradient
        assert float((a.double() - want.double()).abs().max()) <= limit, (n, limit)
