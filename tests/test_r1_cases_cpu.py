"""CPU: the mathematics the R1 phase rests on, pinned in float64 -- the InstanceNorm closed form of include/hrviton_hip.h against
torch.autograd, the identity that turns the penalty's gradient into a tangent pass, and the condition on the end-to-end seeds."""
import pytest
import torch

import r1_cases as R


def _rel(a, b):
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)


@pytest.mark.parametrize("case", sorted(R.KERNEL_CASES))
def test_closed_form_equals_float64_autograd(case):
    c, t, df, _ = R.kernel_inputs(case)
    got, want = R.closed_form(c, t, df, torch.float64), R.autograd_form(c, t, df)
    for k in ("fdot", "tbar", "cbar"):
        scale = max(float(want[k].abs().max()), 1e-300)
        if c.shape[1] * c.shape[2] == 1:      # one pixel: y == 0 whatever c is, every derivative is exactly 0
            assert float(want[k].abs().max()) == 0.0 and float(got[k].abs().max()) == 0.0, (case, k)
        else:
            assert float((got[k] - want[k]).abs().max()) <= 1e-12 * scale, (case, k, _rel(got[k], want[k]))


def test_closed_form_with_an_incoming_adjoint_adds_it():
    c, t, df, cin = R.kernel_inputs("c5_3x5_off0")
    a, b = R.closed_form(c, t, df, torch.float64), R.closed_form(c, t, df, torch.float64, cin=cin)
    assert torch.equal(b["cbar"], a["cbar"] + cin.double()) and torch.equal(a["tbar"], b["tbar"])


@pytest.mark.parametrize("case", sorted(R.PHASE_CASES))
def test_penalty_gradient_is_gamma_times_the_tangent_pass(case):
    cs = R.PHASE_CASES[case]
    D = R.build_d(cs["num_D"], cs["seed"])
    parse, real = R.phase_inputs(cs)
    a = R.penalty_autograd(D, parse, real, R.GAMMA, R.INTERVAL, cs["num_D"])
    b = R.penalty_tangent(D, parse, real, R.GAMMA, R.INTERVAL, cs["num_D"])
    assert abs(a["r1_penalty"] - b["r1_penalty"]) <= 1e-12 * a["r1_penalty"] and a["r1_penalty"] > 0
    assert abs(a["D_R1"] - 0.5 * R.GAMMA * a["r1_penalty"]) <= 1e-15 * a["D_R1"]
    gmax = max(float(g.abs().max()) for g in a["grads"].values())
    assert gmax > 0
    for n, g in a["grads"].items():
        assert float((g - b["grads"][n]).abs().max()) <= 1e-10 * max(float(g.abs().max()), 1e-6 * gmax), n
    # a bias behind which no InstanceNorm sits gets nothing at all: the last layer's bias does not reach g
    last = [n for n in a["grads"] if n.endswith("model3.0.bias")]
    assert last and all(float(a["grads"][n].abs().max()) == 0.0 and float(b["grads"][n].abs().max()) == 0.0 for n in last)
    assert any(float(a["grads"][n].abs().max()) > 0 for n in a["grads"] if n.endswith("model0.0.bias"))


@pytest.mark.parametrize("case", sorted(R.PHASE_CASES))
def test_no_end_to_end_case_sits_on_a_leaky_relu_decision(case):
    cs = R.PHASE_CASES[case]
    D = R.build_d(cs["num_D"], cs["seed"])
    parse, real = R.phase_inputs(cs)
    closest = R.penalty_tangent(D, parse, real, R.GAMMA, R.INTERVAL, cs["num_D"])["closest"]
    assert closest >= R.MIN_PREACT, (case, closest)


def test_seed_restatement_on_integers():
    g = torch.Generator().manual_seed(3)
    d = torch.randint(-8, 9, (3, 3, 5, R.SEED_CP), generator=g).float()
    v, sums, pen, loss = R.seed_restated(d, R.SEED_CA, R.SEED_CB, 10.0)
    assert float(v[..., :R.SEED_CA].abs().max()) == 0 and float(v[..., R.SEED_CA + R.SEED_CB:].abs().max()) == 0
    assert torch.equal(sums, (d[..., 7:10].double() ** 2).sum(dim=(1, 2, 3))) and float(loss) == float((5.0 * sums.sum() / 3).float())
