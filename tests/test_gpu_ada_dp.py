"""GPU: adaptive discriminator augmentation under data parallelism, two ranks (both on cuda:0, gloo carrying the CUDA tensors, as
tests/test_gpu_lecam_dp.py): the loss head's sums are all-reduced, so every rank computes the same r and the same p without a
collective of the controller's own -- bitwise the state a single process computes on the concatenated batch, and under the same
injected uniforms each rank's gated assembly is its slice of that process's."""
import os
import socket
import sys

import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(2, 1, 16, 8), (2, 1, 9, 5)]       # logits per rank and scale: n = 256 and 90 (not a multiple of 4)
STEPS = 4
N, H, W, CA = 2, 17, 13, 7                   # the assembled batch per rank
POLICY = "color,translation,cutout"
# global batch 4, interval 2, kimg 0.064: step = 4 * 2 / 64 = 1/8; integer logits in [-8, 8] have r_t near 0, above the target
ADA = dict(target=-0.5, kimg=0.064, interval=2, p_init=0.125)


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
    g = torch.Generator().manual_seed(2000 + 10 * step + rank)
    return [(torch.randint(-8, 9, s, generator=g).float(), torch.randint(-8, 9, s, generator=g).float()) for s in SHAPES]


def _images(step, rank):
    """(parse [N,H,W,8], image [N,3,H,W], u [N,8], ug [N,4]) of one rank: the injected uniforms included"""
    g = torch.Generator().manual_seed(3000 + 10 * step + rank)
    parse = torch.randn(N, H, W, 8, generator=g)
    parse[..., CA:] = 0
    return parse, torch.randn(N, 3, H, W, generator=g), torch.rand(N, 8, generator=g), torch.rand(N, 4, generator=g)


def _steps(head, aug, logits, images, world):
    """per step: the gated assembly under the p of the step before, the head's forward, the controller -> (state, [outputs])"""
    from hr_viton_amd import diffaug, ops
    outs = []
    for pairs, (parse, img, u, ug) in zip(logits, images):
        gate = (ug.cuda(), aug.p_tensor("cuda"))
        outs.append(diffaug.diffaug_concat(ops.Act(parse.cuda(), CA), img.cuda(), u.cuda(), aug, gate=gate).t.cpu())
        head.d_losses([[f.cuda()] for f, _ in pairs], [[r.cuda()] for _, r in pairs])
        aug.update(head, pairs[0][0].shape[0] * world)
    torch.cuda.synchronize()
    return aug.state().cpu(), outs


def _worker(rank, world, port, q):
    try:
        sys.path.insert(0, ROOT)
        _wd = _watchdog("ada", rank)
        os.environ.update(RANK=str(rank), LOCAL_RANK="0", WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                          MASTER_PORT=str(port), HRV_DIST_BACKEND="gloo")
        import torch.distributed as dist
        import hr_viton_amd  # noqa: F401
        from hr_viton_amd import dist as hdist
        from hr_viton_amd.diffaug import AdaptiveAugment
        from hr_viton_amd.lecam import LeCam
        hdist.init_from_env()
        torch.cuda.set_device(0)
        state, outs = _steps(LeCam(0.0), AdaptiveAugment(POLICY, **ADA), [_logits(s, rank) for s in range(STEPS)],
                             [_images(s, rank) for s in range(STEPS)], world)
        q.put((rank, state.tolist(), [o.tolist() for o in outs]))
        dist.barrier()
        dist.destroy_process_group()
    except Exception:  # noqa: BLE001
        import traceback
        q.put((rank, "ERROR: " + traceback.format_exc()))


def test_two_ranks_hold_the_p_and_the_state_of_the_concatenated_batch():
    import hr_viton_amd  # noqa: F401
    from hr_viton_amd import _lib
    from hr_viton_amd.diffaug import AdaptiveAugment
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
        assert len(r) == 3, r
    # the single process on the concatenated batch, under the same uniforms
    logits = [[(torch.cat((a[0], b[0])), torch.cat((a[1], b[1]))) for a, b in zip(_logits(s, 0), _logits(s, 1))] for s in range(STEPS)]
    images = [tuple(torch.cat((a, b)) for a, b in zip(_images(s, 0), _images(s, 1))) for s in range(STEPS)]
    aug = AdaptiveAugment(POLICY, **ADA)
    assert aug.step_size(4) == 0.125
    state, outs = _steps(LeCam(0.0), aug, logits, images, 1)
    assert state[_lib.ADA_STEPS] == STEPS and state[_lib.ADA_UPDATES] == 2 and state[_lib.ADA_P] == 0.375      # p moved twice
    for rank, rstate, routs in res:
        got = torch.tensor(rstate, dtype=torch.float64)
        assert torch.equal(got.view(torch.int64), state.view(torch.int64)), (rank, got, state)
        for s in range(STEPS):
            mine = torch.tensor(routs[s], dtype=torch.float32)
            assert torch.equal(mine.view(torch.int32), outs[s][rank * N:(rank + 1) * N].view(torch.int32)), (rank, s)
    # (the gates did select under the moving p: a step's assembly is neither the plain copy nor the full transform for every sample)
    from hr_viton_amd import diffaug, ops
    parse, img, u, ug = images[-1]
    full = diffaug.diffaug_concat(ops.Act(parse.cuda(), CA), img.cuda(), u.cuda(), POLICY).t.cpu()
    none = diffaug.diffaug_concat(ops.Act(parse.cuda(), CA), img.cuda(), u.cuda(), 0).t.cpu()
    assert not torch.equal(outs[-1], full) and not torch.equal(outs[-1], none)
