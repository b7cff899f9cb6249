"""CPU: the float64 restatement of the discriminator step's loss head (tests/lecam_cases.py) against torch autograd, the case
table, and the host side of hr_viton_amd.lecam (state_dict round trip, flags)."""
import argparse

import pytest
import torch

import lecam_cases as L


def test_the_table_covers_every_required_size_and_keeps_odd_ones():
    have = set(L.covered_n())
    assert set(L.REQUIRED_N) <= have, sorted(set(L.REQUIRED_N) - have)
    assert sum(1 for n in have if n % 2) >= 5                       # odd n: the real half is 4-byte aligned only
    assert {len(s) for s in L.CASES.values()} == {1, 2, 3}
    for shapes in L.CASES.values():
        assert all(len(s) == 4 and s[1] == 1 for s in shapes)
        assert len({L.numel(s) for s in shapes}) == len(shapes)    # a different n per scale
    assert L.SWEEP == 4 * L.BLOCK * L.SLOTS


@pytest.mark.parametrize("form", ["paper", "relu"])
@pytest.mark.parametrize("n", L.EXACT["n"])
def test_restatement_equals_autograd_and_stays_exact_in_fp32_on_the_integer_family(form, n):
    """6 chained steps, start = 2 (the first two steps move the anchors without a regulariser), two scales: the restated losses and
    gradients are torch.equal to float64 autograd of the loss written with torch ops and detached anchors, and every anchor, hinge
    loss and gradient is exactly representable in fp32 -- the condition the exact GPU tests rest on."""
    E = L.EXACT
    ns = [n, max(1, n // 2)] if n > 1 else [1, 1]
    ns = ns[:E["num_D"]]
    data = L.exact_logits(ns, E["steps"], seed=7 + n)
    ref = L.Restated(E["weight"], E["decay"], E["start"], form)
    fp32 = lambda v: torch.equal(torch.as_tensor(v, dtype=torch.float64).float().double(), torch.as_tensor(v, dtype=torch.float64))  # noqa: E731
    for step, pairs in enumerate(data):
        out = ref.step(pairs)
        assert out["lambda"] == (E["weight"] if step >= E["start"] else 0.0)
        assert ref.count == step + 1
        leaves = [(f.clone().requires_grad_(), r.clone().requires_grad_()) for f, r in pairs]
        anchors = list(zip(ref.anchor_real, ref.anchor_fake))
        d_fake, d_real, lecam = L.torch_loss(leaves, anchors, out["lambda"], form)
        (d_fake + d_real + lecam).backward()
        assert (d_fake.item(), d_real.item(), float(torch.as_tensor(lecam).detach())) == out["losses"]
        for (lf, lr), (gf, gr) in zip(leaves, out["grads"]):
            # (autograd's relu has gradient 0 AT the kink, as the hinge of the kernels has: x > -1, x < 1)
            assert torch.equal(lf.grad, gf) and torch.equal(lr.grad, gr)
            assert fp32(gf) and fp32(gr)
        # (the regulariser's VALUE needs more bits: the GPU tests compare it to the restated value rounded once to fp32)
        assert fp32(out["losses"][:2]) and fp32(ref.anchor_real) and fp32(ref.anchor_fake) and fp32(ref.rt_avg)
        if step < E["start"]:
            assert all(not bool(r.any()) for pair in out["reg"] for r in pair) and out["losses"][2] == 0.0
    assert any(bool(r.any()) for pair in out["reg"] for r in pair)


@pytest.mark.parametrize("form", ["paper", "relu"])
def test_restatement_equals_autograd_on_gaussian_logits(form):
    pairs = [(f.double(), r.double()) for f, r in L.gaussian_logits(L.CASES["n5_255_256"], seed=3)]
    ref = L.Restated(0.3, 0.9, 0, form)
    for _ in range(2):
        out = ref.step(pairs, g=(0.5, 2.0, 1.5))
    leaves = [(f.clone().requires_grad_(), r.clone().requires_grad_()) for f, r in pairs]
    d_fake, d_real, lecam = L.torch_loss(leaves, list(zip(ref.anchor_real, ref.anchor_fake)), 0.3, form)
    (0.5 * d_fake + 2.0 * d_real + 1.5 * lecam).backward()
    for got, want in zip(out["losses"], (d_fake, d_real, lecam)):
        assert abs(got - want.item()) <= 1e-14 * max(1.0, abs(got))
    for (lf, lr), (gf, gr) in zip(leaves, out["grads"]):
        assert torch.allclose(lf.grad, gf, rtol=1e-13, atol=1e-18) and torch.allclose(lr.grad, gr, rtol=1e-13, atol=1e-18)


def test_a_poisoned_step_leaves_the_restated_state_alone():
    ref = L.Restated(0.25, 0.5, 0, "paper")
    clean = L.exact_logits([64, 16], 1, seed=1)[0]
    ref.step(clean)
    before = (list(ref.anchor_real), list(ref.anchor_fake), list(ref.rt_avg), ref.count)
    bad = [(clean[0][0].clone(), clean[0][1].clone()), clean[1]]
    bad[0][1][5] = float("nan")
    out = ref.step(bad)
    assert out["poisoned"] and out["losses"][2] != out["losses"][2] and out["losses"][1] != out["losses"][1]
    assert (ref.anchor_real, ref.anchor_fake, ref.rt_avg, ref.count) == before


def test_state_dict_round_trip_is_strict():
    from hr_viton_amd.lecam import LeCam
    from hr_viton_amd.ops import HrvError
    a = LeCam(0.3, decay=0.9, start=4, form="relu")
    sd = {"weight": 0.3, "decay": 0.9, "start": 4, "form": "relu", "count": 17,
          "anchor_real": torch.tensor([0.25, -1.5], dtype=torch.float64), "anchor_fake": torch.tensor([-0.75, 0.125], dtype=torch.float64),
          "r_t_avg": torch.tensor([0.5, 0.625], dtype=torch.float64)}
    a.load_state_dict(sd)
    back = a.state_dict()
    assert set(back) == set(sd) and back["count"] == 17 and back["form"] == "relu"
    for k in ("anchor_real", "anchor_fake", "r_t_avg"):
        assert torch.equal(back[k], sd[k]) and back[k].dtype == torch.float64
    with pytest.raises(HrvError):
        a.load_state_dict({k: v for k, v in sd.items() if k != "r_t_avg"})
    with pytest.raises(HrvError):
        a.load_state_dict(dict(sd, extra=1))
    with pytest.raises(HrvError):
        LeCam(0.3, decay=0.9, start=4, form="paper").load_state_dict(sd)
    with pytest.raises(HrvError):
        a.load_state_dict(dict(sd, anchor_fake=torch.zeros(3, dtype=torch.float64)))
    for bad in (dict(weight=-1.0), dict(weight=0.1, decay=1.0), dict(weight=0.1, form="hinge"), dict(weight=0.1, start=-1)):
        with pytest.raises(HrvError):
            LeCam(**bad)


def test_flags():
    from hr_viton_amd.lecam import LeCam, add_lecam_args, lecam_from_opt, lecam_line, lecam_scalars
    from hr_viton_amd.ops import HrvError
    p = argparse.ArgumentParser()
    add_lecam_args(p)
    off = p.parse_args([])
    assert vars(off) == {} and lecam_from_opt(off) is None            # nothing in the option line, nothing built
    assert lecam_from_opt(p.parse_args(["--lecam", "0"])) is None
    assert lecam_line(None) == "" and lecam_scalars(None) == []
    h = lecam_from_opt(p.parse_args(["--lecam", "0.3", "--lecam_decay", "0.9", "--lecam_start", "5", "--lecam_form", "relu"]))
    assert isinstance(h, LeCam) and (h.weight, h.decay, h.start, h.form) == (0.3, 0.9, 5, "relu")
    h = lecam_from_opt(p.parse_args(["--lecam", "0.3"]))
    assert (h.weight, h.decay, h.start, h.form) == (0.3, 0.99, 0, "paper")
    s = lecam_from_opt(p.parse_args(["--d_stats"]))
    assert isinstance(s, LeCam) and s.weight == 0.0
    with pytest.raises(SystemExit):
        p.parse_args(["--lecam_form", "other"])
    with pytest.raises(HrvError):
        lecam_from_opt(p.parse_args(["--lecam_checkpoint", "x.pth"]))


def test_the_script_knows_the_flags_and_the_step_refuses_a_non_hinge_criterion():
    import train_generator as tg
    from hr_viton_amd.lecam import LeCam
    from hr_viton_amd.ops import HrvError
    from hr_viton_amd.pipeline import generator_train_step
    opt = tg.get_opt(["--name", "t", "--lecam", "0.3", "--lecam_start", "1", "--d_stats"])
    assert opt.lecam == 0.3 and opt.lecam_start == 1 and opt.d_stats
    assert not hasattr(tg.get_opt(["--name", "t"]), "lecam")

    class Crit:
        gan_mode = "w"
    with pytest.raises(HrvError, match="hinge"):
        generator_train_step(None, None, object(), Crit(), None, None, None, None, None, None, None, lecam=LeCam(0.1))
