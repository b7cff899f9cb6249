"""GPU: the Adam step that keeps an exponential moving average of the weights (csrc/adam_ema.hip; optim.Adam(ema_decay=,
ema_warmup=)) against the restatements of tests/ema_cases.py, which tests/test_ema_cases_cpu.py holds against a plain float64 loop:
the weights keep the bits of the plain / guarded / device-count kernels at every edge of the geometry and from aligned and
4-byte-aligned pointers, the average is exact where it can be and within the derived bound elsewhere, a skipped step leaves it
alone, capture in a hipGraph, the host-count path, the in-place swap, the checkpoint, two ranks, the script."""
import functools
import hashlib
import math
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import ema_cases as E
import guard_cases as G

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR, (B1, B2), EPS = E.LR, E.BETAS, E.EPS


def _T():
    import hr_viton_amd  # noqa: F401
    from hr_viton_amd import train_ops
    return train_ops


class _Dev:
    """some arrays of one length on the device, each between two NaN bands, all at the same ``shift``"""

    def __init__(self, tensors, shift):
        self.bufs, self.views = [], []
        for t in tensors:
            buf, (o, n) = E.banded(t, shift)
            d = buf.cuda()
            assert d[o:o + n].data_ptr() % 16 == 4 * shift
            self.bufs.append(d)
            self.views.append(d[o:o + n])
        self.o, self.n = o, n

    def clone(self):
        c = object.__new__(_Dev)
        c.bufs = [b.clone() for b in self.bufs]
        c.o, c.n = self.o, self.n
        c.views = [b[c.o:c.o + c.n] for b in c.bufs]
        assert all(a.data_ptr() % 16 == b.data_ptr() % 16 for a, b in zip(c.views, self.views))
        return c

    def bands_intact(self):
        nan = torch.full((E.BAND + 1,), float("nan")).view(torch.int32)[0].item()
        return all(bool((b[:self.o].view(torch.int32) == nan).all()) and bool((b[self.o + self.n:].view(torch.int32) == nan).all())
                   for b in self.bufs)


def _bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@functools.lru_cache(maxsize=2)
def _gauss_case(n):
    return E.gauss_state(n, 1000 + n % 977)


@functools.lru_cache(maxsize=2)
def _int_case(n):
    return E.int_values(n, n % 991), E.int_values(n, n % 991 + 1)


def _record(scale):
    T = _T()
    rec = torch.zeros(T.GUARD_WORDS, dtype=torch.int32)
    rec[T.GUARD_APPLY] = 1
    rec[T.GUARD_SCALE] = int(np.float32(scale).view(np.int32))
    return rec.cuda()


def _hyper(t):
    """what hrv_adam_hyper_f32 leaves behind at count t, formed on the host: the pairs below read ONE such tensor"""
    return torch.tensor([LR, 1.0 - B1 ** t, math.sqrt(1.0 - B2 ** t)], dtype=torch.float32).cuda()


# ---------------------------------------------------------------------------------------------------------------
# 1. the weights keep their bits
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("shift", E.SHIFTS, ids=["aligned", "buf[1:]"])
@pytest.mark.parametrize("n", E.SIZES)
def test_weights_and_moments_keep_the_bits_of_the_kernels_without_the_average(n, shift, wd):
    T = _T()
    base = _Dev(_gauss_case(n), shift)
    t, gscale, decay = 3, 0.5, 0.999
    rec, hyper = _record(0.75), _hyper(t)
    step_dev = torch.tensor([t], dtype=torch.int32).cuda()
    pairs = {
        "plain": (lambda w, g, m, v: T.adam_step(w, g, m, v, LR, B1, B2, EPS, wd, t, gscale),
                  lambda w, g, m, v, e: T.adam_step_ema(w, g, m, v, e, LR, B1, B2, EPS, wd, t, gscale, decay, True)),
        "guarded": (lambda w, g, m, v: T.adam_step_guarded(w, g, m, v, LR, B1, B2, EPS, wd, t, gscale, rec),
                    lambda w, g, m, v, e: T.adam_step_guarded_ema(w, g, m, v, e, LR, B1, B2, EPS, wd, t, gscale, rec, decay, False)),
        "dev": (lambda w, g, m, v: T.adam_step_dev(w, g, m, v, torch.tensor([t - 1], dtype=torch.int32).cuda(),
                                                   torch.tensor([LR]).cuda(), torch.zeros(3).cuda(), B1, B2, EPS, wd, gscale),
                lambda w, g, m, v, e: T.adam_step_dev_ema(w, g, m, v, e, torch.tensor([t - 1], dtype=torch.int32).cuda(),
                                                          torch.tensor([LR]).cuda(), torch.zeros(3).cuda(), B1, B2, EPS, wd, gscale,
                                                          decay, True)),
        "dev_guarded": (lambda w, g, m, v: T.adam_step_dev_guarded(w, g, m, v, hyper, B1, B2, EPS, wd, gscale, rec),
                        lambda w, g, m, v, e: T.adam_step_dev_guarded_ema(w, g, m, v, e, hyper, B1, B2, EPS, wd, gscale, rec, step_dev,
                                                                          decay, False)),
    }
    for name, (plain, fused) in pairs.items():
        a, b = base.clone(), base.clone()
        plain(*a.views[:4])
        fused(*b.views)
        torch.cuda.synchronize()
        for k, key in enumerate("wmv"):
            i = (0, 2, 3)[k]
            assert _bits(a.views[i], b.views[i]), (name, key)
        assert _bits(a.views[1], b.views[1]) and _bits(b.views[1], base.views[1]), name      # the gradient is read only
        assert not _bits(b.views[0], base.views[0]) and not _bits(b.views[4], base.views[4]), name
        assert bool(torch.isfinite(b.views[4]).all()), name
        assert b.bands_intact() and a.bands_intact(), (name, "a write outside [0, n), or a read that met the NaN band")


# ---------------------------------------------------------------------------------------------------------------
# 2. the average is exact where it can be
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", E.SHIFTS, ids=["aligned", "buf[1:]"])
@pytest.mark.parametrize("n", E.SIZES)
def test_the_average_is_exact_on_integers_with_power_of_two_weights(n, shift):
    """g = m = v = 0 without weight decay: w' == w bitwise; integer w, e in [-64, 64] and 1 - d in {1/2, 1/4, 1/8}: every
    intermediate of the average is exact, so e' has the bits of the fp32 restatement"""
    T = _T()
    w, e = _int_case(n)
    z = torch.zeros(n)
    base = _Dev((w, z, z, z, e), shift)
    for decay in (0.5, 0.75, 0.875):
        d = base.clone()
        T.adam_step_ema(*d.views, LR, B1, B2, EPS, 0.0, 2, 1.0, decay, False)
        _, omd = E.schedule(decay, False, 2)
        assert _bits(d.views[0], base.views[0]) and _bits(d.views[2], base.views[2]) and _bits(d.views[3], base.views[3])
        assert _bits(d.views[4].cpu(), E.ema_ref32(w, e, omd)), decay
        assert d.bands_intact()


@pytest.mark.parametrize("shift", E.SHIFTS, ids=["aligned", "buf[1:]"])
@pytest.mark.parametrize("n", [5, 1025, E.PASS + 1])
def test_the_entry_point_below_the_decay_under_warmup_and_at_decay_zero(n, shift):
    T = _T()
    base = _Dev(_gauss_case(n), shift)
    for t in (1, 5):            # d = 2/11, 6/15: far below 0.999
        d = base.clone()
        T.adam_step_ema(*d.views, LR, B1, B2, EPS, 0.0, t, 1.0, 0.999, True)
        dd, omd = E.schedule(0.999, True, t)
        assert float(dd) < 0.5
        wn, e0 = d.views[0].cpu(), base.views[4].cpu()
        e64 = E.ema_ref64(wn, e0, omd)
        err, bound = (d.views[4].cpu().double() - e64).abs(), E.ema_bound(wn, e0, omd, e64)
        print("n %d shift %d t %d: worst error / bound %.3f" % (n, shift, t, float((err / bound).max())))
        assert bool((err <= bound).all()), (t, float((err / bound).max()))
    d = base.clone()            # decay 0: omd == 1 and e' IS w'
    T.adam_step_ema(*d.views, LR, B1, B2, EPS, 0.0, 1, 1.0, 0.0, False)
    assert _bits(d.views[4], d.views[0]) and not _bits(d.views[0], base.views[0]) and d.bands_intact()


# ---------------------------------------------------------------------------------------------------------------
# 3. the average within the derived bound
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("warmup", [False, True], ids=["fixed", "warmup"])
@pytest.mark.parametrize("decay", [0.999, 0.9999])
@pytest.mark.parametrize("shift", E.SHIFTS, ids=["aligned", "buf[1:]"])
@pytest.mark.parametrize("n", [5, 1025, E.PASS + 1])
def test_three_chained_steps_stay_within_the_bound_and_repeat_bit_for_bit(n, shift, decay, warmup):
    T = _T()
    base = _Dev(_gauss_case(n), shift)
    runs = []
    for rep in range(2):
        d, trail = base.clone(), []
        for t in (1, 2, 3):
            e0 = d.views[4].cpu()
            T.adam_step_ema(*d.views, LR, B1, B2, EPS, 0.0, t, 1.0, decay, warmup)
            trail.append((e0, d.views[0].cpu(), d.views[4].cpu()))
        runs.append(trail)
        assert d.bands_intact()
    for t, ((e0, wn, e1), (f0, wm, f1)) in enumerate(zip(*runs), 1):
        assert _bits(e1, f1) and _bits(wn, wm), t
        _, omd = E.schedule(decay, warmup, t)
        e64 = E.ema_ref64(wn, e0, omd)
        err, bound = (e1.double() - e64).abs(), E.ema_bound(wn, e0, omd, e64)
        print("n %d shift %d decay %g warmup %d t %d: worst error / bound %.3f" % (n, shift, decay, warmup, t, float((err / bound).max())))
        assert bool((err <= bound).all()), (t, float((err / bound).max()))
        assert not _bits(e1, e0)


# ---------------------------------------------------------------------------------------------------------------
# the optimizer
# ---------------------------------------------------------------------------------------------------------------
def _make(device_step=False, **kw):
    from hr_viton_amd.optim import Adam
    ps = [torch.nn.Parameter(w.cuda()) for w in G.start_weights()]
    return ps, Adam(ps, lr=G.LR, betas=G.BETAS, eps=G.EPS, device_step=device_step, **kw)


def _step(ps, opt, grads):
    for p, g in zip(ps, grads):
        p.grad = None if g is None else g.cuda()
    opt.step()


def _state(opt):
    st = opt._flat[0]
    out = {k: st[k].clone() for k in ("w", "m", "v", "ema")}
    if "step_dev" in st:
        out["step_dev"] = st["step_dev"].clone()
    return out


def _same(a, b, keys=("w", "m", "v", "ema")):
    return all(_bits(a[k], b[k]) for k in keys)


def _within(e1, wn, e0, decay, warmup, t):
    _, omd = E.schedule(decay, warmup, t)
    e64 = E.ema_ref64(wn.cpu(), e0.cpu(), omd)
    return bool(((e1.cpu().double() - e64).abs() <= E.ema_bound(wn.cpu(), e0.cpu(), omd, e64)).all())


def test_the_average_is_off_by_default_and_starts_at_the_weights():
    ps, opt = _make()
    _step(ps, opt, G.gauss_grad_list(0))
    assert opt.ema_decay is None and "ema" not in opt._flat[0]
    assert all("ema" not in ent for ent in opt.state_dict()["state"].values())
    ps, opt = _make(ema_decay=0.9)
    assert _bits(opt.ema_buffer(), opt._flat[0]["w"]) and opt.ema_buffer().data_ptr() != opt._flat[0]["w"].data_ptr()
    pp, op = _make()
    for s in range(2):
        _step(ps, opt, G.gauss_grad_list(s))
        _step(pp, op, G.gauss_grad_list(s))
    assert _same(_state(opt), {**{k: op._flat[0][k] for k in "wmv"}}, ("w", "m", "v"))      # the optimizer without it, bit for bit
    assert not _bits(opt.ema_buffer(), opt._flat[0]["w"])


def test_a_skipped_step_leaves_the_average_alone_and_the_next_uses_the_applied_count():
    kw = dict(skip_nonfinite=True, ema_decay=0.9, ema_warmup=True)
    pg, og = _make(True, **kw)
    pp, op = _make(True, **kw)
    a, b, c = G.gauss_grad_list(0), G.poison(G.gauss_grad_list(1), "nan"), G.gauss_grad_list(2)
    _step(pg, og, a)
    s1 = _state(og)
    assert int(s1["step_dev"]) == 1 and not _bits(s1["ema"], s1["w"])
    _step(pg, og, b)
    s2 = _state(og)
    assert _same(s1, s2) and int(s2["step_dev"]) == 1 and og.guard_stats()["apply"] == 0
    _step(pg, og, c)
    s3 = _state(og)
    _step(pp, op, a)
    _step(pp, op, c)
    assert _same(s3, _state(op)) and int(s3["step_dev"]) == 2
    # under warm-up the decay of that step is the one of count 2 (3/12), not of the third call (4/13)
    assert _within(s3["ema"], s3["w"], s2["ema"], 0.9, True, 2) and not _within(s3["ema"], s3["w"], s2["ema"], 0.9, True, 3)
    assert not _bits(s3["ema"], s2["ema"])


@pytest.mark.parametrize("guarded", [False, True], ids=["plain", "guarded"])
def test_a_captured_step_follows_the_eager_sequence_with_the_average(guarded):
    kw = dict(ema_decay=0.9, ema_warmup=True, **(dict(max_grad_norm=5.0, skip_nonfinite=True) if guarded else {}))
    pe, oe = _make(True, **kw)
    pc, oc = _make(True, **kw)
    warm = G.gauss_grad_list(9)
    seq = [G.gauss_grad_list(0), G.poison(G.gauss_grad_list(1)) if guarded else G.gauss_grad_list(1), G.gauss_grad_list(2)]
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
        oc.step()                      # eager: the flat buffers, the average, the device scalars, the guard record and workspace
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert _same(_state(oe), _state(oc))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        oc.step()
    before = _state(oc)
    for i, grads in enumerate(seq):
        _step(pe, oe, grads)
        load(grads)
        oc.push_lr()
        graph.replay()
        torch.cuda.synchronize()
        assert _same(_state(oe), _state(oc), ("w", "m", "v", "ema", "step_dev")), i
    assert int(_state(oc)["step_dev"]) == (3 if guarded else 4) and not _bits(before["ema"], _state(oc)["ema"])


def test_host_count_a_parameter_without_a_gradient_keeps_its_average_and_counts_differ():
    decay = 0.9
    ps, opt = _make(ema_decay=decay, ema_warmup=True)
    spans = [(off, k) for _, off, k in (opt._flat.get(0) or opt._setup(0, opt.param_groups[0]))["spans"]]
    _step(ps, opt, G.gauss_grad_list(0))
    s1 = _state(opt)
    g1 = G.gauss_grad_list(1)
    g1[1] = None
    _step(ps, opt, g1)
    s2 = _state(opt)
    off, k = spans[1]
    assert all(_bits(s1[key][off:off + k], s2[key][off:off + k]) for key in ("w", "m", "v", "ema"))
    for i in (0, 2):
        o, kk = spans[i]
        assert all(not _bits(s1[key][o:o + kk], s2[key][o:o + kk]) for key in ("w", "m", "v", "ema")), i
    assert opt._flat[0]["steps"] == [2, 1, 2]
    _step(ps, opt, G.gauss_grad_list(2))          # counts 3, 2, 3: three launches, each with its own decay (4/13, 3/12, 4/13)
    s3 = _state(opt)
    assert opt._flat[0]["steps"] == [3, 2, 3]
    for i, (t, other) in enumerate([(3, 2), (2, 3), (3, 2)]):
        o, kk = spans[i]
        sl = slice(o, o + kk)
        assert _within(s3["ema"][sl], s3["w"][sl], s2["ema"][sl], decay, True, t), i
        assert not _within(s3["ema"][sl], s3["w"][sl], s2["ema"][sl], decay, True, other), i
    # weights and moments are those of the optimizer without the average, fed the same gradients
    pp, op = _make()
    for grads in (G.gauss_grad_list(0), g1, G.gauss_grad_list(2)):
        _step(pp, op, grads)
    assert all(_bits(s3[key], op._flat[0][key]) for key in ("w", "m", "v"))


# ---------------------------------------------------------------------------------------------------------------
# 7. the swap
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", E.SHIFTS, ids=["aligned", "buf[1:]"])
@pytest.mark.parametrize("n", E.SIZES)
def test_swap_exchanges_exactly_and_stays_inside(n, shift):
    T = _T()
    w, g, _, _, _ = _gauss_case(n)
    base = _Dev((w, g), shift)
    d = base.clone()
    T.swap_(d.views[0], d.views[1])
    assert _bits(d.views[0], base.views[1]) and _bits(d.views[1], base.views[0]) and d.bands_intact()
    assert not _bits(d.views[0], base.views[0])


def test_swap_refuses_overlapping_buffers():
    from hr_viton_amd.ops import HrvError
    buf = torch.zeros(64, device="cuda")
    with pytest.raises(HrvError, match="overlap"):
        _T().swap_(buf[:40], buf[8:48])


def test_swap_ema_exchanges_restores_bumps_the_epochs_and_refuses_a_step():
    from hr_viton_amd import ops
    from hr_viton_amd.ops import HrvError
    ps, opt = _make(ema_decay=0.5)
    _step(ps, opt, G.gauss_grad_list(0))
    s0 = _state(opt)
    raw = [p.detach().clone() for p in ps]
    ep0, pe0 = ops.WEIGHTS_EPOCH[0], [p._hrv_epoch for p in ps]
    with opt.swap_ema() as o:
        assert o is opt
        s1 = _state(opt)
        assert _bits(s1["w"], s0["ema"]) and _bits(s1["ema"], s0["w"])
        assert all(not torch.equal(p.detach(), r) for p, r in zip(ps, raw))          # the parameters now show the averaged weights
        for p, (_, off, k) in zip(ps, opt._flat[0]["spans"]):
            assert torch.equal(p.detach().reshape(-1), s0["ema"][off:off + k])
        assert ops.WEIGHTS_EPOCH[0] == ep0 + 1 and [p._hrv_epoch for p in ps] == [e + 1 for e in pe0]
        with pytest.raises(HrvError, match="swap_ema"):
            opt.step()
        with pytest.raises(HrvError, match="already inside"):
            with opt.swap_ema():
                pass
    assert _same(_state(opt), s0) and all(torch.equal(p.detach(), r) for p, r in zip(ps, raw))
    assert ops.WEIGHTS_EPOCH[0] == ep0 + 2 and [p._hrv_epoch for p in ps] == [e + 2 for e in pe0]
    _step(ps, opt, G.gauss_grad_list(1))          # and the optimizer steps again
    with pytest.raises(HrvError, match="without ema_decay"):
        with _make()[1].swap_ema():
            pass


# ---------------------------------------------------------------------------------------------------------------
# 8. checkpoints
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


def test_ema_state_dict_has_the_modules_keys_and_loads_into_a_fresh_generator(tmp_path):
    import hr_viton_amd  # noqa: F401
    from hr_viton_amd.checkpoint import load_checkpoint_G, save_checkpoint
    from hr_viton_amd.network_generator import SPADEGenerator
    from hr_viton_amd.optim import Adam
    gopt, gen, _ = _gen_setup(5)
    gen.cuda().train()
    opt = Adam(gen.parameters(), lr=1e-2, betas=(0.0, 0.9), ema_decay=0.5)
    rng = torch.Generator(device="cuda").manual_seed(3)
    for p in gen.parameters():
        p.grad = torch.randn(p.shape, device="cuda", generator=rng)
    opt.step()
    sd, live = opt.ema_state_dict(gen), gen.state_dict()
    assert list(sd) == list(live) and getattr(sd, "_metadata", None) == getattr(live, "_metadata", None)
    params = dict(gen.named_parameters())
    where = {id(p): (off, k) for p, off, k in opt._flat[0]["spans"]}
    assert params and set(params) < set(sd)          # there are buffers too (spectral norm's u, v)
    for name, val in sd.items():
        if name in params:
            off, k = where[id(params[name])]
            assert torch.equal(val.reshape(-1), opt.ema_buffer()[off:off + k]), name
            assert not torch.equal(val, live[name]) and val.data_ptr() != live[name].data_ptr(), name
            # e' = w0 + (w' - w0) / 2 at decay 0.5
        else:
            assert torch.equal(val, live[name]), name
    path = str(tmp_path / "gen_ema.pth")
    save_checkpoint(gen, path, gopt, state_dict=sd)
    torch.manual_seed(99)
    fresh = SPADEGenerator(gopt, 9)
    fresh.init_weights("xavier", 0.02)
    load_checkpoint_G(fresh, path, gopt)          # strict
    got = fresh.state_dict()
    assert all(torch.equal(got[k].cpu(), sd[k].cpu()) for k in sd)
    # the optimizer's own state round-trips the average bit for bit; a state without it leaves the average at the weights
    osd = opt.state_dict()
    assert all("ema" in ent for ent in osd["state"].values())
    _, gen2, _ = _gen_setup(6)
    gen2.cuda().train()
    gen2.load_state_dict(gen.state_dict())
    opt2 = Adam(gen2.parameters(), lr=1e-2, betas=(0.0, 0.9), ema_decay=0.5)
    opt2.load_state_dict(osd)
    assert _bits(opt2.ema_buffer(), opt.ema_buffer()) and _bits(opt2._flat[0]["m"], opt._flat[0]["m"])
    for ent in osd["state"].values():
        del ent["ema"]
    opt2.load_state_dict(osd)
    assert _bits(opt2.ema_buffer(), opt2._flat[0]["w"]) and _bits(opt2._flat[0]["w"], opt._flat[0]["w"])
    # ... and load_ema_state_dict seeds it from the file
    opt2.load_ema_state_dict(gen2, torch.load(path, map_location="cpu"))
    assert _bits(opt2.ema_buffer(), opt.ema_buffer())


def test_save_training_state_moves_the_average_to_the_cpu(tmp_path):
    from hr_viton_amd.checkpoint import load_training_state, save_training_state
    ps, opt = _make(ema_decay=0.5)
    _step(ps, opt, G.gauss_grad_list(0))
    path = str(tmp_path / "state.pth")
    mod = torch.nn.ParameterList(ps)
    save_training_state(path, {"m": mod}, {"o": opt}, step=1)
    blob = torch.load(path, map_location=None, weights_only=False)
    ents = list(blob["optimizers"]["o"]["state"].values())
    assert ents and all(not ent[k].is_cuda for ent in ents for k in ("exp_avg", "exp_avg_sq", "ema"))
    want = _state(opt)
    _step(ps, opt, G.gauss_grad_list(1))
    load_training_state(path, {"m": mod}, {"o": opt})
    assert _same(_state(opt), want)


# ---------------------------------------------------------------------------------------------------------------
# 9. two ranks
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
        _wd = open(diag_path(f"dp_ema_rank{rank}_stacks.txt"), "w")
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
        og = Adam(gen.parameters(), lr=1e-4, betas=(0.0, 0.9), ema_decay=0.9, ema_warmup=True)
        od = Adam(dis.parameters(), lr=4e-4, betas=(0.0, 0.9))
        sg, sd = og.make_grad_sync(bucket_mb=0.25), od.make_grad_sync(bucket_mb=4.0)
        attach_grad_sync(sg)
        attach_grad_sync(sd)
        e0 = og.ema_buffer().clone()
        for step in range(3):
            x, seg, real = _gen_batch(1000 + 10 * step + rank)
            torch.manual_seed(77 + rank + step)
            generator_train_step(opt, gen, dis, GANLoss("hinge"), L1Loss(), None, og, od, x.to(dev), ops.to_nhwc(seg.to(dev)),
                                 real.to(dev), sg, sd)
        torch.cuda.synchronize()
        ema, w = og.ema_buffer(), og._flat[0]["w"]
        digest = [hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest() for t in (ema, w)]
        q.put((rank, digest, bool(torch.isfinite(ema).all()), float((ema - e0).abs().max()), float((ema - w).abs().max())))
        dist.barrier()
        dist.destroy_process_group()
    except Exception:  # noqa: BLE001
        import traceback
        q.put((rank, "ERROR: " + traceback.format_exc()))


def test_two_ranks_hold_the_same_average_bit_for_bit():
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
        assert len(r) == 5, r
    (_, d0, fin0, moved0, gap0), (_, d1, fin1, moved1, gap1) = res
    assert d0 == d1, "the replicas' averages (or weights) differ"
    assert fin0 and fin1 and moved0 == moved1 and moved0 > 1e-7 and gap0 > 0


# ---------------------------------------------------------------------------------------------------------------
# 10. the script
# ---------------------------------------------------------------------------------------------------------------
GEN_ARGV = ["--synthetic", "-b", "1", "--fine_height", "256", "--fine_width", "192", "--num_upsampling_layers", "more", "--ngf", "8",
            "--ndf", "8", "--tocg_ngf", "8", "--max_steps", "3", "--num_test_visualize", "1", "--no_vgg_loss", "--board",
            "--tensorboard_count", "3", "--display_count", "1", "--lpips_count", "3", "--val_items", "2", "--save_count", "2"]


def test_train_generator_writes_the_averaged_checkpoints_only_when_asked(tmp_path, capsys):
    import train_generator as tg
    from hr_viton_amd import validate as V
    from hr_viton_amd.network_generator import SPADEGenerator

    def run(name, extra):
        torch.manual_seed(0)
        tg.main(["--name", name, "--checkpoint_dir", str(tmp_path / "ck"), "--tensorboard_dir", str(tmp_path / "tb")] + GEN_ARGV + extra)
        return V.read_scalars(str(tmp_path / "tb" / name)), capsys.readouterr().out

    recs_e, out_e = run("e", ["--ema_decay", "0.5", "--ema_eval"])
    recs_p, out_p = run("p", [])
    ck = tmp_path / "ck"
    for f in ("gen_ema_model_final.pth", "gen_ema_step_000002.pth", "gen_model_final.pth", "gen_step_000002.pth"):
        assert (ck / "e" / f).exists(), f
    assert sorted(f.name for f in (ck / "p").iterdir() if "ema" in f.name) == []
    assert "ema_decay=0.5" in out_e and "ema_eval=True" in out_e and "ema_" not in out_p
    raw_e = torch.load(str(ck / "e" / "gen_model_final.pth"), map_location="cpu")
    raw_p = torch.load(str(ck / "p" / "gen_model_final.pth"), map_location="cpu")
    ema = torch.load(str(ck / "e" / "gen_ema_model_final.pth"), map_location="cpu")
    # the average changes nothing about the training run, evaluation under the swapped weights included
    assert list(raw_e) == list(raw_p) == list(ema) and all(_bits(raw_e[k], raw_p[k]) if raw_e[k].dtype == torch.float32
                                                            else torch.equal(raw_e[k], raw_p[k]) for k in raw_e)
    opt = tg.get_opt(["--name", "e"] + GEN_ARGV)
    gen = SPADEGenerator(opt, 9)
    gen.load_state_dict(ema, strict=True)
    names = {n for n, p in gen.named_parameters()}
    moved = [k for k in ema if k in names and not torch.equal(ema[k], raw_e[k])]
    assert moved and all(torch.equal(ema[k], raw_e[k]) for k in ema if k not in names)          # buffers are the live ones
    assert all(bool(torch.isfinite(v).all()) for v in ema.values() if v.is_floating_point())
    # the test/LPIPS pass ran in both, on different weights
    lp_e = [r["value"] for r in recs_e if r["tag"] == "test/LPIPS"]
    lp_p = [r["value"] for r in recs_p if r["tag"] == "test/LPIPS"]
    assert len(lp_e) == len(lp_p) == 1 and np.isfinite(lp_e[0]) and lp_e[0] != lp_p[0]
