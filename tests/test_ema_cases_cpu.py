"""tests/ema_cases.py on the CPU alone: the restatements of the averaged Adam step against a plain float64 EMA loop, the warm-up
schedule, the constants and symbols of the library, the optimizer's argument checks and train_generator.py's flags."""
import os
import re

import numpy as np
import pytest
import torch

import ema_cases as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["hrv_adam_ema_f32", "hrv_adam_dev_ema_f32", "hrv_adam_guarded_ema_f32", "hrv_adam_dev_guarded_ema_f32", "hrv_swap_f32"]


@pytest.mark.parametrize("warmup", [False, True], ids=["fixed", "warmup"])
@pytest.mark.parametrize("decay", [0.9, 0.999])
def test_ref64_is_a_plain_float64_ema_loop(decay, warmup):
    ws = [E.gauss(1000, 40 + s) for s in range(5)]
    e0 = E.gauss(1000, 39)
    want = E.ema_loop64(ws, decay, warmup, e0)
    e = e0.double()
    for t, w in enumerate(ws, 1):
        _, omd = E.schedule(decay, warmup, t)
        e = E.ema_ref64(w, e, omd)          # (chained in float64: the restatement itself, no fp32 rounding between the steps)
        assert float((e - want[t - 1]).abs().max()) <= 1e-14 * float(want[t - 1].abs().max()), t
    assert float((e - e0.double()).abs().max()) > 1e-3


def test_ref32_is_ref64_rounded_once_and_exact_on_the_integer_cases():
    w, e = E.int_values(4099, 1), E.int_values(4099, 2)
    for decay in (0.5, 0.75, 0.875):
        d, omd = E.schedule(decay, False, 3)
        assert float(d) == decay and float(omd) == 1.0 - decay
        r32, r64 = E.ema_ref32(w, e, omd), E.ema_ref64(w, e, omd)
        assert torch.equal(r32.double(), r64)          # every intermediate is exact: no rounding anywhere
        assert not torch.equal(r32, w) and not torch.equal(r32, e)
    assert torch.equal(E.ema_ref32(w, e, 1.0), w) and torch.equal(E.ema_ref64(w, e, 1.0), w.double())
    # Gaussian data: one rounding of t and one of the result
    w, e = E.gauss(4099, 3), E.gauss(4099, 4)
    _, omd = E.schedule(0.999, False, 1)
    r32, r64 = E.ema_ref32(w, e, omd), E.ema_ref64(w, e, omd)
    assert bool(((r32.double() - r64).abs() <= E.ema_bound(w, e, omd, r64)).all())


def test_the_warmup_schedule():
    for decay in (0.9, 0.999, 0.9999):
        t0 = E.warmup_reaches_decay_at(decay)
        for t in (1, 2, 10, 100, t0 - 1, t0, t0 + 1, 10 * t0):
            d, omd = E.schedule(decay, True, t)
            want = min(decay, (1.0 + t) / (10.0 + t))
            assert abs(float(d) - want) <= 2.0 ** -23 * want, (decay, t)
            assert omd == np.float32(1.0) - d and d.dtype == np.float32 and omd.dtype == np.float32
            assert E.schedule(decay, False, t)[0] == np.float32(decay)
        assert (1.0 + t0) / (10.0 + t0) >= decay > t0 / (9.0 + t0)
        assert E.schedule(decay, True, t0 // 2)[0] < np.float32(decay)
        assert E.schedule(decay, True, t0)[0] == np.float32(decay) == E.schedule(decay, True, t0 + 1)[0]
    assert E.warmup_reaches_decay_at(0.9) == 80 and E.warmup_reaches_decay_at(0.999) == 8990
    assert float(E.schedule(0.999, True, 1)[0]) == float(np.float32(2.0) / np.float32(11.0))


def test_the_sizes_and_constants_mirror_the_kernel():
    with open(os.path.join(ROOT, "hr-viton_amd", "csrc", "adam_ema.hip"), encoding="utf-8") as f:
        src = f.read()
    assert int(re.search(r"constexpr int EMA_BLOCK = (\d+);", src).group(1)) == E.BLOCK
    assert int(re.search(r"constexpr int EMA_CAP = (\d+);", src).group(1)) == E.CAP
    assert E.PASS == E.CAP * E.BLOCK * 4
    assert E.SIZES == [1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, E.PASS - 1, E.PASS, E.PASS + 1, 2 * E.PASS + 7]
    for shift in E.SHIFTS:
        buf, (o, n) = E.banded(torch.ones(5), shift)
        assert (buf.data_ptr() + 4 * o) % 16 == 4 * shift and n == 5
        assert bool(torch.isnan(buf[:o]).all()) and bool(torch.isnan(buf[o + n:]).all()) and o >= 64 and buf.numel() - o - n == 64


def test_the_header_declares_the_new_symbols_and_the_binding_lists_them():
    from hr_viton_amd import _lib
    with open(os.path.join(ROOT, "include", "hrviton_hip.h"), encoding="utf-8") as f:
        hdr = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = set(re.findall(r"\b(hrv_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SYMBOLS, name
    # five arrays, then n; the device-count variants take the count's address as their last argument before the stream
    for name in NEW_SYMBOLS[:4]:
        args = _lib.SYMBOLS[name][1]
        assert args[:6] == [_lib._vp] * 5 + [_lib._i64] and args[-1] is _lib._vp
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert getattr(lib, name) is not None


@pytest.mark.parametrize("bad", [1.0, -0.1, 1.5])
def test_a_decay_outside_the_open_interval_is_refused_without_a_gpu(bad):
    from hr_viton_amd.ops import HrvError
    from hr_viton_amd.optim import Adam
    p = torch.nn.Parameter(torch.zeros(4))
    with pytest.raises(HrvError, match="ema_decay"):
        Adam([p], ema_decay=bad)
    for off in (None, 0, 0.0):
        assert Adam([p], ema_decay=off).ema_decay is None
    on = Adam([p], ema_decay=0.5, ema_warmup=True)
    assert on.ema_decay == 0.5 and on.ema_warmup is True
    with pytest.raises(HrvError, match="without ema_decay"):
        Adam([p]).ema_buffer()


def test_train_generator_takes_the_flags_and_leaves_them_out_when_not_given():
    import train_generator as tg
    from hr_viton_amd.optim import ema_kwargs
    opt = tg.get_opt(["--name", "t", "--synthetic"])
    for k in ("ema_decay", "ema_warmup", "ema_eval", "ema_checkpoint"):
        assert not hasattr(opt, k), k
    assert ema_kwargs(opt) == {} and "ema_" not in str(opt)
    opt = tg.get_opt(["--name", "t", "--synthetic", "--ema_decay", "0.999", "--ema_warmup", "--ema_eval", "--ema_checkpoint", "x.pth"])
    assert opt.ema_decay == 0.999 and opt.ema_warmup is True and opt.ema_eval is True and opt.ema_checkpoint == "x.pth"
    assert ema_kwargs(opt) == {"ema_decay": 0.999, "ema_warmup": True}
    assert ema_kwargs(tg.get_opt(["--name", "t", "--synthetic", "--ema_decay", "0.5"])) == {"ema_decay": 0.5, "ema_warmup": False}
    assert ema_kwargs(tg.get_opt(["--name", "t", "--synthetic", "--ema_decay", "0"])) == {}
