"""tests/ada_cases.py on the CPU alone: the controller's restatement on hand-worked sequences, the gate mask at its edges, what the
gate tables guarantee to the GPU tests, the library's symbols and constants, AdaptiveAugment's host side and train_generator.py's
flags."""
import os
import re

import numpy as np
import pytest
import torch

import ada_cases as A
import diffaug_cases as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["hrv_diffaug_concat_gated_f32", "hrv_diffaug_gsum_gated_f32", "hrv_diffaug_bwd_gated_f32", "hrv_ada_update_f64"]
IDS = lambda s: "x".join(map(str, s))  # noqa: E731


# ------------------------------------------------------------------ the controller
def test_the_restated_controller_follows_the_hand_worked_sequence():
    states = A.run_sequence(A.HAND, A.HAND_SEQ)
    assert len(states) >= 14
    for i, (st, (_, _, p, seen, updates)) in enumerate(zip(states, A.HAND_SEQ)):
        assert (st[A.P], st[A.SEEN], st[A.UPDATES], st[A.STEPS]) == (p, seen, updates, i + 1), (i, st)
    ps = [st[A.P] for st in states]
    # a window closing above, below and at the target; a run into each clamp; the poisoned step left the window alone
    assert ps[1] > 0.0 and ps[10] < ps[9] and ps[8] == ps[7] and states[8][A.UPDATES] == states[7][A.UPDATES] + 1
    assert ps[6] == A.HAND["p_max"] and states[6][A.RT_WINDOW] == 1.0 and ps[14] == 0.0 and states[14][A.RT_WINDOW] == -1.0
    assert states[3][A.ACC] == states[2][A.ACC] == 1.0 and states[3][A.RT_LAST] == 1.0 and states[3][A.STEPS] == 4.0
    assert states[4][A.RT_WINDOW] == 0.75
    assert states[15][A.ACC] == (0.1 + 0.3) / 2.0 and states[15][A.RT_LAST] == states[15][A.ACC]


def test_the_rounded_sequence_exercises_what_it_is_for():
    seq = A.rounded_seq()
    states = A.run_sequence(A.ROUNDED, seq)
    assert len(states) >= 14 and [i for i, s in enumerate(seq) if s[1]] == [7]
    ps = [st[A.P] for st in states]
    assert states[2][A.P] == 0.05 + 0.1 and states[2][A.RT_WINDOW] == (0.9 + 0.7 + 0.95) / 3.0      # the header's order, one rounding each
    assert states[7][A.SEEN] == states[6][A.SEEN] == 1.0 and states[7][A.ACC] == 0.8 and states[7][A.STEPS] == 8.0
    assert states[9][A.RT_WINDOW] == (0.8 + 0.9 + 0.7) / 3.0 and ps[9] == A.ROUNDED["p_max"] == ps[12]
    assert ps[15] == 0.2 - 0.1 and ps[18] == 0.0 == ps[21] and states[21][A.RT_WINDOW] == -1.0
    assert states[-1][A.UPDATES] == 7.0 and states[-1][A.SEEN] == 0.0 and states[-1][A.STEPS] == 22.0


def test_the_step_size_is_stylegan2_adas():
    import hr_viton_amd  # noqa: F401
    from hr_viton_amd.diffaug import AdaptiveAugment
    aug = AdaptiveAugment("color", target=0.6)
    assert aug.step_size(64) == 64 * 4 / (500 * 1000.0)
    assert AdaptiveAugment("color", target=0.6, kimg=0.008, interval=2).step_size(2) == 0.5


# ------------------------------------------------------------------ the gates
def test_gate_mask_at_its_edges():
    row = np.asarray([0.0, 0.5, D.TOP, 0.0], dtype=np.float32)
    assert A.gate_mask(row, 0.0) == 0                         # p = 0 applies nothing, not even under ug = 0
    assert A.gate_mask(row, 1.0) == D.ALL                     # p = 1 applies everything, up to the largest fp32 below 1
    assert A.gate_mask(row, 0.5) == D.COLOR                   # ug == p does not apply
    # (float)p == 0.25 == ug, but p > 0.25 in fp64: the transform applies, which an fp32 comparison would deny
    assert np.float32(A.EDGE_P) == np.float32(0.25) and A.EDGE_P > 0.25
    assert A.gate_mask(np.asarray([0.25, 0.25, 0.25, 0.9], dtype=np.float32), A.EDGE_P) == D.ALL
    assert A.gate_mask(np.asarray([0.25, 0.25, 0.25, 0.9], dtype=np.float32), 0.25) == 0
    # the spare column is never read
    assert A.gate_mask(np.asarray([0.9, 0.9, 0.9, 0.0], dtype=np.float32), 0.5) == 0


@pytest.mark.parametrize("shape", D.SHAPES + D.POW2_SHAPES, ids=IDS)
def test_the_gate_tables_cover_every_mask_and_both_states(shape):
    N, H, W = shape
    seen = set()
    for names, u, masks, ug in A.paired_batches(H, W, N):
        assert tuple(u.shape) == (N, 8) and tuple(ug.shape) == (N, 4)
        assert masks == [A.gate_mask(ug[n].numpy(), A.GATE_P) for n in range(N)]
        seen.update(masks)
    assert seen == set(range(8))
    # the random table at p = 0.5, over the batches the GPU test draws: every transform on for a sample and off for another
    on, off = 0, 0
    for i in range(len(D.batches(D.forced_rows(H, W), N))):
        for n in range(N):
            m = A.gate_mask(A.random_gates(N, H + i)[n].numpy(), 0.5)
            on, off = on | m, off | (D.ALL & ~m)
    assert on == D.ALL and off == D.ALL


def test_the_gated_reference_is_the_ungated_one_under_the_effective_flags():
    N, H, W = 2, 17, 13
    parse, fake, _ = D.gauss_inputs(N, H, W, 3)
    g = torch.randn(N, H, W, 12, generator=torch.Generator().manual_seed(1))
    u = torch.rand(N, 8, generator=torch.Generator().manual_seed(2))
    ug = torch.tensor([[A.ON, A.OFF, A.ON, 0.0], [A.OFF, A.ON, A.OFF, 0.0]])
    M = D.mean_ref(fake)
    got = A.forward_ref(parse, 7, fake, u, ug, A.GATE_P, D.ALL, mean=M)
    assert torch.equal(got[0:1], D.forward_ref(parse[0:1], 7, fake[0:1], u[0:1], D.COLOR | D.CUTOUT, mean=M[0:1]))
    assert torch.equal(got[1:2], D.forward_ref(parse[1:2], 7, fake[1:2], u[1:2], D.TRANSLATION, mean=M[1:2]))
    # p = 0: the plain assembly; p = 1: the ungated transform; a policy without a transform never gains it
    plain = A.forward_ref(parse, 7, fake, u, ug, 0.0, D.ALL, mean=M)
    assert torch.equal(plain[..., :7], parse[..., :7].double()) and torch.equal(plain[..., 7:10], fake.permute(0, 2, 3, 1).double())
    assert torch.equal(A.forward_ref(parse, 7, fake, u, ug, 1.0, D.ALL, mean=M), D.forward_ref(parse, 7, fake, u, D.ALL, mean=M))
    assert torch.equal(A.forward_ref(parse, 7, fake, u, ug, 1.0, D.CUTOUT), D.forward_ref(parse, 7, fake, u, D.CUTOUT))
    assert torch.equal(A.backward_ref(g, 7, u, ug, 1.0, D.ALL), D.backward_ref(g, 7, u, D.ALL))
    assert torch.equal(A.backward_ref(g, 7, u, ug, 0.0, D.ALL), g[..., 7:10].permute(0, 3, 1, 2).double())
    assert torch.equal(A.gsum_ref(g, 7, u, ug, 1.0, D.ALL), D.gsum_ref(g, 7, u, D.ALL))


# ------------------------------------------------------------------ the library, the class and the script
def test_symbols_constants_and_flags():
    import hr_viton_amd  # noqa: F401
    from hr_viton_amd import _lib
    from hr_viton_amd.diffaug import AdaptiveAugment, DiffAugment, diffaug_from_opt
    with open(os.path.join(ROOT, "include", "hrviton_hip.h"), encoding="utf-8") as f:
        hdr = f.read()
    declared = set(re.findall(r"\b(hrv_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SYMBOLS, name
    for name, val in (("WORDS", A.WORDS), ("P", A.P), ("ACC", A.ACC), ("SEEN", A.SEEN), ("UPDATES", A.UPDATES), ("RT_WINDOW", A.RT_WINDOW),
                      ("STEPS", A.STEPS), ("RT_LAST", A.RT_LAST)):
        assert re.search(r"#define\s+HRV_ADA_%s\s+%d\b" % (name, val), hdr), name
        assert getattr(_lib, "ADA_" + name) == val
    assert (_lib.DHEAD_WORDS, _lib.DHEAD_NONFINITE, _lib.DHEAD_STATE, _lib.DHEAD_SCALE_WORDS, _lib.DHEAD_RT) == \
        (A.DHEAD_WORDS, A.DHEAD_NONFINITE, A.DHEAD_STATE, A.DHEAD_SCALE_WORDS, A.DHEAD_RT)
    # the gated entry points: the ungated signature plus (ug, p) in front of the stream
    for base in ("concat", "gsum", "bwd"):
        plain, gated = _lib.SYMBOLS["hrv_diffaug_%s_f32" % base], _lib.SYMBOLS["hrv_diffaug_%s_gated_f32" % base]
        assert gated[0] == plain[0] and list(gated[1][:len(plain[1]) - 1]) == list(plain[1][:-1]) and len(gated[1]) == len(plain[1]) + 2
    import train_generator as tg
    base = ["--name", "t", "--synthetic"]
    opt = tg.get_opt(base)
    assert not [k for k in vars(opt) if k.startswith("ada_")]          # the option line of a plain run is the one it was
    assert diffaug_from_opt(opt) is None
    plain = diffaug_from_opt(tg.get_opt(base + ["--diffaug", "color,cutout"]))
    assert type(plain) is DiffAugment
    ada = diffaug_from_opt(tg.get_opt(base + ["--diffaug", "color,cutout", "--ada_target", "0.6", "--ada_interval", "2", "--ada_kimg", "100",
                                              "--ada_p_init", "0.125", "--ada_p_max", "0.75"]))
    assert isinstance(ada, AdaptiveAugment) and ada.adaptive and ada.flags == D.COLOR | D.CUTOUT
    assert (ada.target, ada.interval, ada.kimg, ada.p_max, ada.scalars()["p"]) == (0.6, 2, 100.0, 0.75, 0.125)
    fixed = diffaug_from_opt(tg.get_opt(base + ["--diffaug", "cutout", "--ada_fixed_p", "0.25"]))
    assert isinstance(fixed, AdaptiveAugment) and not fixed.adaptive and fixed.scalars()["p"] == 0.25
    for bad in (["--ada_target", "0.6"], ["--ada_fixed_p", "0.5"], ["--ada_kimg", "100"], ["--diffaug", "", "--ada_target", "0.6"],
                ["--diffaug", "color", "--ada_target", "0.6", "--ada_fixed_p", "0.5"], ["--diffaug", "color", "--ada_interval", "2"]):
        with pytest.raises(SystemExit) as e:
            diffaug_from_opt(tg.get_opt(base + bad))
        assert isinstance(e.value.code, str) and "--" in e.value.code, bad


def test_the_class_checks_its_arguments_and_round_trips_its_state_on_the_host():
    import hr_viton_amd  # noqa: F401
    from hr_viton_amd import ops
    from hr_viton_amd.diffaug import AdaptiveAugment
    for kw in ({}, dict(target=0.6, fixed_p=0.5), dict(target=2.0), dict(fixed_p=1.5), dict(target=0.6, interval=0),
               dict(target=0.6, kimg=0.0), dict(target=0.6, p_init=0.9, p_max=0.5), dict(fixed_p=0.5, p_max=2.0)):
        with pytest.raises(ops.HrvError):
            AdaptiveAugment("color", **kw)
    a = AdaptiveAugment("color,cutout", target=0.5, interval=2, p_init=0.25)
    sd = a.state_dict()
    assert sd["state"].tolist() == A.initial_state(0.25) and sd["policy"] == D.COLOR | D.CUTOUT
    sd["state"] = torch.tensor(A.run_sequence(A.HAND, A.HAND_SEQ)[3], dtype=torch.float64)
    b = AdaptiveAugment("color,cutout", target=0.5, interval=2)
    b.load_state_dict(sd)
    assert b.scalars() == {"p": 0.25, "acc": 1.0, "seen": 1.0, "updates": 1.0, "r_t_window": 0.5, "steps": 4.0, "r_t": 1.0}
    for other in (AdaptiveAugment("color", target=0.5, interval=2), AdaptiveAugment("color,cutout", target=0.5, interval=4),
                  AdaptiveAugment("color,cutout", fixed_p=0.5)):
        with pytest.raises(ops.HrvError, match="written with"):
            other.load_state_dict(sd)
    with pytest.raises(ops.HrvError, match="keys"):
        b.load_state_dict({k: v for k, v in sd.items() if k != "kimg"})
    with pytest.raises(ops.HrvError, match="fixed p"):
        AdaptiveAugment("color", fixed_p=0.5).update(None, 2)


def test_the_step_rejects_an_adaptive_aug_without_the_head():
    from argparse import Namespace
    import hr_viton_amd  # noqa: F401
    from hr_viton_amd import ops, pipeline
    from hr_viton_amd.diffaug import AdaptiveAugment

    class Pair:
        def forward_pair(self, *a, **k):
            raise AssertionError("not reached")
    with pytest.raises(ops.HrvError, match="lecam"):
        pipeline.generator_train_step(Namespace(), None, Pair(), None, None, None, None, None, None, None, None,
                                      aug=AdaptiveAugment("color", target=0.6))
