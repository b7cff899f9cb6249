"""GPU: the discriminator step's loss head under data parallelism, two ranks (both on cuda:0, gloo carrying the CUDA tensors, as
tests/test_gpu_dp.py): the fp64 sums are all-reduced between reduce and finalize, so both ranks hold the anchors a single process
computes on the concatenated batch; the captured iteration refuses world > 1."""
import os
import socket
import sys

import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(2, 1, 16, 8), (2, 1, 9, 5)]       # per rank: n = 256 and 90 (not a multiple of 4)
STEPS = 3


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


def _logits(step, rank):
    g = torch.Generator().manual_seed(1000 + 10 * step + rank)
    return [(torch.randint(-8, 9, s, generator=g).float(), torch.randint(-8, 9, s, generator=g).float()) for s in SHAPES]


def _steps(head, batches):
    for pairs in batches:
        leaves = [(f.cuda().requires_grad_(), r.cuda().requires_grad_()) for f, r in pairs]
        out = head.d_losses([[f] for f, _ in leaves], [[r] for _, r in leaves])
        sum(out.values()).sum().backward()
    torch.cuda.synchronize()
    return head.stats().cpu(), [float(v.detach()) for v in out.values()], [(f.grad.cpu(), r.grad.cpu()) for f, r in leaves]


def _worker(rank, world, port, q):
    try:
        sys.path.insert(0, ROOT)
        _wd = _watchdog("lecam", rank)
        os.environ.update(RANK=str(rank), LOCAL_RANK="0", WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                          MASTER_PORT=str(port), HRV_DIST_BACKEND="gloo")
        from argparse import Namespace
        import torch.distributed as dist
        import hr_viton_amd  # noqa: F401
        from hr_viton_amd import dist as hdist
        from hr_viton_amd.graph import GraphedTrainStep
        from hr_viton_amd.lecam import LeCam
        from hr_viton_amd.ops import HrvError
        hdist.init_from_env()
        torch.cuda.set_device(0)
        head = LeCam(0.25, 0.5, start=1)
        rec, losses, grads = _steps(head, [_logits(s, rank) for s in range(STEPS)])
        refused = ""
        try:
            o = Namespace(device_step=True)
            GraphedTrainStep(None, None, None, None, None, None, o, o, {}, lecam=head)
        except HrvError as e:
            refused = str(e)
        q.put((rank, rec.tolist(), losses, [[g.tolist() for g in pair] for pair in grads], refused))
        dist.barrier()
        dist.destroy_process_group()
    except Exception:  # noqa: BLE001
        import traceback
        q.put((rank, "ERROR: " + traceback.format_exc()))


def test_two_ranks_hold_the_anchors_of_the_concatenated_batch_and_capture_is_refused():
    import hr_viton_amd  # noqa: F401
    from hr_viton_amd import _lib
    from hr_viton_amd.lecam import LeCam
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
        assert len(r) == 5, r
    # the single process on the concatenated batch
    both = [[(torch.cat((a[0], b[0])), torch.cat((a[1], b[1]))) for a, b in zip(_logits(s, 0), _logits(s, 1))] for s in range(STEPS)]
    rec, losses, grads = _steps(LeCam(0.25, 0.5, start=1), both)
    keep = [_lib.DHEAD_COUNT, _lib.DHEAD_LAMBDA] + [_lib.DHEAD_STATE + _lib.DHEAD_SCALE_WORDS * k + j for k in range(len(SHAPES))
                                                   for j in (_lib.DHEAD_ANCHOR_REAL, _lib.DHEAD_ANCHOR_FAKE, _lib.DHEAD_RT_AVG,
                                                             _lib.DHEAD_MEAN_REAL, _lib.DHEAD_MEAN_FAKE)]
    keep += list(range(_lib.DHEAD_SUMS, _lib.DHEAD_SUMS + _lib.DHEAD_SCALE_WORDS * len(SHAPES)))
    want = rec[keep]
    assert float(rec[_lib.DHEAD_COUNT]) == STEPS and float(rec[_lib.DHEAD_LAMBDA]) == 0.25
    for rank, rrec, rlosses, rgrads, refused in res:
        got = torch.tensor(rrec, dtype=torch.float64)[keep]
        assert torch.equal(got.view(torch.int64), want.view(torch.int64)), (rank, got, want)
        assert rlosses == losses, (rank, rlosses, losses)            # paper form: the losses are the global batch's on every rank
        assert "LeCam" in refused and "data-parallel" in refused, refused
        # the gradient of a rank's logits is its slice of the single process's, times the world (GradSync averages over the ranks)
        for k, (gf, gr) in enumerate(rgrads):
            N = SHAPES[k][0]
            assert torch.equal(torch.tensor(gf), 2 * grads[k][0][rank * N:(rank + 1) * N])
            assert torch.equal(torch.tensor(gr), 2 * grads[k][1][rank * N:(rank + 1) * N])
