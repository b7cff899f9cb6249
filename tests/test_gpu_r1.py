"""GPU: the R1 phase (hr_viton_amd.r1, csrc/r1.hip) -- the seed and the two InstanceNorm launches against the float64 restatements of
tests/r1_cases.py, the whole phase against the penalty's definition on the oracle's discriminator, its structure (linearity in
gamma, what it leaves alone, reproducibility), the train step and the script."""
import re

import pytest
import torch

import r1_cases as R

pytestmark = pytest.mark.gpu


def _mods():
    import hr_viton_amd  # noqa: F401
    from hr_viton_amd import ops, r1
    return r1, ops


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


# ---------------------------------------------------------------------------------------------------------------
# 1. the seed
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(R.SEED_CASES))
def test_seed_is_exact_on_integers_keeps_other_channels_out_and_is_reproducible(case):
    r1, ops = _mods()
    N, H, W = R.SEED_CASES[case]
    Ca, Cb = R.SEED_CA, R.SEED_CB
    g = torch.Generator().manual_seed(R.case_seed(case))
    d = torch.randint(-8, 9, (N, H, W, R.SEED_CP), generator=g).float()
    want_v, want_sums, want_pen, want_loss = R.seed_restated(d, Ca, Cb, R.GAMMA)
    runs = []
    for poison in (False, False, True):
        x = d.clone()
        if poison:      # a NaN in a parse channel and an Inf in a pad channel of d_in reach neither v nor the sums
            x[0, 0, 0, 2] = float("nan")
            x[-1, -1, -1, Ca + Cb] = float("inf")
        v, sums, out = r1.r1_seed(ops.Act(x.cuda(), Ca + Cb), Ca, Cb, R.GAMMA)
        torch.cuda.synchronize()
        runs.append((v.t.cpu(), sums.cpu(), out.cpu()))
    for v, sums, out in runs:
        assert torch.equal(v, want_v)
        assert float(v[..., :Ca].abs().max()) == 0.0 and float(v[..., Ca + Cb:].abs().max()) == 0.0
        assert torch.equal(sums, want_sums)
        assert torch.equal(out, torch.stack([want_pen, want_loss]))
    assert torch.equal(_bits(runs[0][0]), _bits(runs[1][0])) and torch.equal(_bits(runs[0][2]), _bits(runs[1][2]))


def test_seed_refuses_what_it_does_not_serve():
    r1, ops = _mods()
    d = torch.zeros(1, 2, 2, 12, device="cuda")
    with pytest.raises(ops.HrvError):
        r1.r1_seed(ops.Act(d, 9), 7, 3, 1.0)                     # Ca + Cb is not the activation's channel count
    with pytest.raises(ops.HrvError):
        r1.r1_seed(ops.Act(torch.zeros(1, 2, 2, 16, device="cuda"), 10, 4), 7, 3, 1.0)      # a channel slice


# ---------------------------------------------------------------------------------------------------------------
# 2. the two InstanceNorm launches
# ---------------------------------------------------------------------------------------------------------------
def _place(x, off, ops):
    """NHWC [N,H,W,C] (CPU) -> an Act over channels [off, off + C) of a wider zeroed device tensor"""
    N, H, W, C = x.shape
    cs = off + (C + 3) // 4 * 4 + (4 if off else 0)
    t = torch.zeros(N, H, W, cs)
    t[..., off:off + C] = x
    return ops.Act(t.cuda(), C, off)


def _take(a):
    return a.t[..., a.coff:a.coff + a.C].cpu()


def _stats(case, c, ops):
    """(mean, rstd) [N, C] fp32 of the forward's statistics pass, on the host: operands of the launches and of the restatements"""
    mean, rstd = ops.instnorm_stats(_place(c, R.KERNEL_CASES[case][3], ops))
    return mean[:, :c.shape[3]].cpu(), rstd[:, :c.shape[3]].cpu()


def _launch(case, c, t, df, cin, f, r1, ops):
    _, _, _, off = R.KERNEL_CASES[case]
    ca, ta, da, fa = (_place(x, off, ops) for x in (c, t, df, f))
    cia = None if cin is None else _place(cin, off, ops)
    mean, rstd = ops.instnorm_stats(ca)
    rec = r1.instnorm_jvp_stats(ca, mean, rstd, fa, ta, da, R.KSLOPE)
    tbar, cbar = r1.instnorm_jvp_bwd(ca, mean, rstd, fa, ta, da, rec, cia, R.KSLOPE)
    torch.cuda.synchronize()
    return rec[:, :c.shape[3]].cpu(), _take(tbar), _take(cbar)


@pytest.mark.parametrize("case", sorted(R.KERNEL_CASES))
def test_instnorm_jvp_launches_against_float64(case, capsys):
    """Limit per output (the record of five sums, tbar, cbar): twice the error torch's own fp32 evaluation of the same closed form makes
    on the same operands -- c, t, df, cin, the fp32 (mean, rstd) of the forward's statistics pass and the LeakyReLU decision, which
    the kernel receives through ``f``.  (That the closed form is the derivative, with exact statistics, is pinned in float64 by
    tests/test_r1_cases_cpu.py; the phase test below holds the whole chain to the float64 definition.)"""
    r1, ops = _mods()
    c, t, df, cin = R.kernel_inputs(case)
    stats = _stats(case, c, ops)
    R.check_stats(c, *stats)           # ... which are the float64 statistics of c up to what their fp32 accumulation allows
    want = R.closed_form(c, t, df, torch.float64, cin=cin, stats=stats)
    own = R.closed_form(c, t, df, torch.float32, cin=cin, mask=want["mask"], stats=stats)
    f = torch.nn.functional.leaky_relu(want["y"], R.KSLOPE).float()
    assert bool(((f > 0) == (want["y"] > 0)).all())
    rec, tbar, cbar = _launch(case, c, t, df, cin, f, r1, ops)
    worst = {}
    for k, got in (("sums", rec), ("tbar", tbar), ("cbar", cbar)):
        limit = 2.0 * float((own[k].double() - want[k]).abs().max())
        err = float((got.double() - want[k]).abs().max())
        worst[k] = err / limit if limit > 0 else (0.0 if err == 0 else float("inf"))
    with capsys.disabled():
        print("\n[instnorm_jvp %s] share of the limit: sums %.3f tbar %.3f cbar %.3f" % (case, worst["sums"], worst["tbar"], worst["cbar"]))
    assert all(v <= 1.0 for v in worst.values()), (case, worst)
    assert bool(torch.isfinite(tbar).all()) and bool(torch.isfinite(cbar).all())
    again = _launch(case, c, t, df, cin, f, r1, ops)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip((rec, tbar, cbar), again))


@pytest.mark.parametrize("case", ["c5_1x1_off0", "c5_3x5_off4", "c64_33x37_off0"])
def test_instnorm_jvp_zeros_and_scaling(case):
    r1, ops = _mods()
    c, t, df, _ = R.kernel_inputs(case)
    want = R.closed_form(c, t, df, torch.float64, stats=_stats(case, c, ops))
    f = torch.nn.functional.leaky_relu(want["y"], R.KSLOPE).float()
    zero = torch.zeros_like(t)
    _, _, cbar = _launch(case, c, zero, df, None, f, r1, ops)
    assert float(cbar.abs().max()) == 0.0                         # t = 0: the tangent path adds nothing to the adjoint of c
    rec, tbar, cbar = _launch(case, c, t, zero, None, f, r1, ops)
    assert float(tbar.abs().max()) == 0.0 and float(cbar.abs().max()) == 0.0      # q = 0
    _, tb1, cb1 = _launch(case, c, t, df, None, f, r1, ops)
    _, tb2, cb2 = _launch(case, c, t, 2.0 * df, None, f, r1, ops)
    assert torch.equal(_bits(2.0 * tb1), _bits(tb2)) and torch.equal(_bits(2.0 * cb1), _bits(cb2))


# ---------------------------------------------------------------------------------------------------------------
# 3. the phase against the definition
# ---------------------------------------------------------------------------------------------------------------
_REF = {}


def _reference(case):
    """float64 definition, the oracle's own fp32 run, and the tangent-pass restatement -- computed once per case, never changed"""
    if case not in _REF:
        cs = R.PHASE_CASES[case]
        D = R.build_d(cs["num_D"], cs["seed"])
        parse, real = R.phase_inputs(cs)
        _REF[case] = dict(D=D, parse=parse, real=real,
                          f64=R.penalty_autograd(D, parse, real, R.GAMMA, R.INTERVAL, cs["num_D"]),
                          f32=R.penalty_autograd(D, parse, real, R.GAMMA, R.INTERVAL, cs["num_D"], dtype=torch.float32),
                          tan=R.penalty_tangent(D, parse, real, R.GAMMA, R.INTERVAL, cs["num_D"]))
    return _REF[case]


def _device_d(case):
    import copy
    ref = _reference(case)
    _, ops = _mods()
    D = copy.deepcopy(ref["D"]).cuda().train()
    parse = torch.cat((ref["parse"].permute(0, 2, 3, 1), torch.zeros_like(ref["parse"][:, :1].permute(0, 2, 3, 1))), dim=3).contiguous().cuda()
    return D, ops.Act(parse, 7), ref["real"].cuda()


def _phase(case, gamma=R.GAMMA, interval=R.INTERVAL):
    r1, ops = _mods()
    D, parse7, real = _device_d(case)
    out = r1.R1(gamma, interval).phase(D, parse7, real)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}, {n: p.grad.detach().cpu().clone() for n, p in D.named_parameters()}


@pytest.mark.parametrize("case", sorted(R.PHASE_CASES))
def test_phase_against_the_float64_definition(case, capsys):
    """Per parameter: four times the error of the oracle's own fp32 autograd run against float64.  The two scalars: the penalty is
    sum_n ||g_n||^2 / N, so an error dg in the input gradient moves it by at most 2 sum|g| max|dg| / N; with max|dg| that of the
    oracle's fp32 run and the same factor four, plus one fp32 rounding of the result."""
    ref = _reference(case)
    out, grads = _phase(case)
    f64, f32, tan = ref["f64"], ref["f32"], ref["tan"]
    N = ref["real"].shape[0]
    dg = float((f32["g"].double() - f64["g"]).abs().max())
    pen_limit = 4.0 * 2.0 * float(f64["g"].abs().sum()) * dg / N + 2.0 ** -23 * f64["r1_penalty"]
    e_pen = abs(float(out["r1_penalty"].double()) - f64["r1_penalty"])
    e_loss = abs(float(out["D_R1"].double()) - f64["D_R1"])
    worst, worst_name = 0.0, ""
    rows = []
    gmax = max(float(g.abs().max()) for g in f64["grads"].values())
    for n, want in f64["grads"].items():
        limit = 4.0 * float((f32["grads"][n].double() - want).abs().max())
        err = float((grads[n].double() - want).abs().max())
        ratio = err / limit if limit > 0 else (0.0 if err == 0 else float("inf"))
        rows.append((n, ratio))
        if ratio > worst:
            worst, worst_name = ratio, n
        if n.endswith("bias"):
            # the restatement whose tangent convolutions carry no bias matches no worse: by no more than that restatement differs from
            # the definition in float64 (1e-10 of the parameter's scale, tests/test_r1_cases_cpu.py), with a margin of ten
            err_t = float((grads[n].double() - tan["grads"][n]).abs().max())
            assert err_t <= err + 1e-9 * max(float(want.abs().max()), 1e-6 * gmax), (case, n, err_t, err)
    with capsys.disabled():
        print("\n[r1 phase %s] penalty %.6g (share of its limit %.3f), worst parameter share %.3f (%s)"
              % (case, f64["r1_penalty"], e_pen / pen_limit, worst, worst_name))
    assert e_pen <= pen_limit and e_loss <= 0.5 * R.GAMMA * pen_limit, (case, e_pen, e_loss, pen_limit)
    assert worst <= 1.0, (case, sorted(rows, key=lambda r: -r[1])[:5])


# ---------------------------------------------------------------------------------------------------------------
# 4. structure
# ---------------------------------------------------------------------------------------------------------------
def test_gamma_doubled_doubles_every_gradient_bitwise_and_two_runs_agree():
    case = "d2_2x64x48"
    out1, g1 = _phase(case)
    out1b, g1b = _phase(case)
    out2, g2 = _phase(case, gamma=2 * R.GAMMA)
    for n in g1:
        assert torch.equal(_bits(g1[n]), _bits(g1b[n])), n
        assert torch.equal(_bits(2.0 * g1[n]), _bits(g2[n])), n
    assert torch.equal(_bits(out1["r1_penalty"]), _bits(out2["r1_penalty"])) and torch.equal(_bits(out1["D_R1"]), _bits(out1b["D_R1"]))
    assert torch.equal(_bits(2.0 * out1["D_R1"]), _bits(out2["D_R1"]))


def test_phase_leaves_weights_moments_and_power_iteration_vectors_alone_and_writes_the_flat_buffer():
    r1, ops = _mods()
    from hr_viton_amd.optim import Adam
    D, parse7, real = _device_d("d2_2x64x48")
    od = Adam(D.parameters(), lr=1e-3, betas=(0.0, 0.9))
    od.prepare_layer_stats()           # the flat buffers exist, the parameters live in them
    st = od._flat[0]
    st["m"].normal_()
    st["v"].uniform_()
    before = {k: v.detach().clone() for k, v in D.state_dict().items()}
    wmv = [st[k].clone() for k in ("w", "m", "v")]
    od.zero_grad()
    r1.R1(R.GAMMA, R.INTERVAL).phase(D, parse7, real)
    torch.cuda.synchronize()
    for k, v in D.state_dict().items():
        assert torch.equal(_bits(v), _bits(before[k])), k
    assert any(k.endswith("weight_u") for k in before)
    for a, k in zip(wmv, ("w", "m", "v")):
        assert torch.equal(_bits(a), _bits(st[k])), k
    base = st["g"].data_ptr()
    for p, off, _ in st["spans"]:
        assert p.grad is not None and p.grad.data_ptr() == base + 4 * off
    _, want = _phase("d2_2x64x48")
    for n, p in D.named_parameters():
        assert torch.equal(_bits(p.grad.cpu()), _bits(want[n])), n


def test_phase_keeps_fp32_operands_in_a_mixed_precision_step():
    from hr_viton_amd import train_ops as T
    _, want = _phase("d1_2x64x48")
    old = T.MMA_BF16[0]
    T.MMA_BF16[0] = True
    try:
        out, got = _phase("d1_2x64x48")
        assert T.MMA_BF16[0] is True
    finally:
        T.MMA_BF16[0] = old
    for n in want:
        assert torch.equal(_bits(want[n]), _bits(got[n])), n


def test_r1_arguments_schedule_and_state():
    r1, ops = _mods()
    with pytest.raises(ops.HrvError):
        r1.R1(0.0)
    with pytest.raises(ops.HrvError):
        r1.R1(1.0, 0)
    assert [s for s in range(7) if r1.R1(1.0, 3).due(s)] == [0, 3, 6]
    assert r1.R1(2.0, 8).state_dict() == {"gamma": 2.0, "interval": 8, "phases": 0}


# ---------------------------------------------------------------------------------------------------------------
# 5. the train step
# ---------------------------------------------------------------------------------------------------------------
def _steps(steps, r1_each=None, manual=None):
    from test_gpu_lecam import _build, _snapshot
    r1, ops = _mods()
    from hr_viton_amd import pipeline
    from hr_viton_amd.losses import GANLoss, L1Loss
    opt, gen, Dn, og, od, inputs, nz = _build()
    parse7 = ops.Act(inputs["parse7"], 7)
    for _ in range(steps):
        kw = {} if r1_each is None else {"r1": r1_each()}
        losses, _ = pipeline.generator_train_step(opt, gen, Dn, GANLoss("hinge"), L1Loss(), None, og, od, inputs["x"], parse7,
                                                  inputs["im"], noise=nz[0], noise_d=nz[1], **kw)
        if manual is not None:
            od.zero_grad()
            manual.phase(Dn, parse7, inputs["im"])
            od.step()
    return _snapshot(gen, Dn), losses


def test_r1_none_is_the_call_without_the_argument_for_three_steps():
    plain, lp = _steps(3)
    none, ln = _steps(3, r1_each=lambda: None)
    assert set(lp) == set(ln) and "D_R1" not in ln
    for k in plain:
        assert torch.equal(plain[k], none[k]), k


def test_step_with_r1_is_the_plain_step_then_zero_grad_phase_step():
    r1, ops = _mods()
    head = r1.R1(R.GAMMA, R.INTERVAL)
    got, losses = _steps(1, r1_each=lambda: head)
    want, _ = _steps(1, manual=r1.R1(R.GAMMA, R.INTERVAL))
    plain, _ = _steps(1)
    assert "D_R1" in losses and float(losses["D_R1"]) > 0 and head.phases == 1
    for k in want:
        assert torch.equal(got[k], want[k]), k
    assert any(not torch.equal(got[k], plain[k]) for k in got if k.startswith("D.") and got[k].is_floating_point())
    assert all(torch.equal(got[k], plain[k]) for k in got if k.startswith("G."))


# ---------------------------------------------------------------------------------------------------------------
# 6. the script
# ---------------------------------------------------------------------------------------------------------------
GEN_ARGV = ["--synthetic", "-b", "2", "--fine_height", "256", "--fine_width", "192", "--num_upsampling_layers", "more", "--ngf", "8",
            "--ndf", "8", "--tocg_ngf", "8", "--max_steps", "4", "--num_test_visualize", "0", "--no_vgg_loss", "--display_count", "1",
            "--lpips_count", "1000", "--save_count", "1000", "--board", "--tensorboard_count", "1"]


def test_train_generator_with_and_without_r1(tmp_path, capsys):
    import train_generator as tg
    r1, ops = _mods()
    from hr_viton_amd import validate as V

    def run(name, extra):
        torch.manual_seed(0)
        ops.profile_begin()
        try:
            tg.main(["--name", name, "--checkpoint_dir", str(tmp_path / "ck"), "--tensorboard_dir", str(tmp_path / "tb")] + GEN_ARGV + extra)
        finally:
            names = [r[1] for r in ops.profile_end()]
        sd = torch.load(str(tmp_path / "ck" / name / "dis_model_final.pth"), map_location="cpu")
        return names, sd, V.read_scalars(str(tmp_path / "tb" / name)), capsys.readouterr().out

    names_p, sd_p, recs_p, out_p = run("p", ["--max_steps", "2"])
    names_q, sd_q, _, out_q = run("q", ["--max_steps", "2"])
    assert not [n for n in names_p + names_q if n.startswith("r1_") or ".r1" in n or "jvp" in n]
    assert "D_r1" not in out_p and "r1_pen" not in out_p and "r1_gamma" not in out_p and not any("r1" in r["tag"] for r in recs_p)
    assert list(sd_p) == list(sd_q)
    for k, v in sd_p.items():
        assert torch.equal(v, sd_q[k]), k
    names_a, sd_a, recs_a, out_a = run("a", ["--r1_gamma", "10", "--r1_interval", "2"])
    lines = [ln for ln in out_a.splitlines() if ln.startswith("step:")]
    assert len(lines) == 4 and ["D_r1:" in ln and "r1_pen:" in ln for ln in lines] == [True, False, True, False], out_a
    vals = [float(v) for v in re.findall(r"(?:D_r1|r1_pen): (\S+?),?(?:\s|$)", out_a)]
    assert len(vals) == 4 and all(v == v and 0 < v < 1e9 for v in vals), out_a
    for tag in ("Loss/dis/r1", "Reg/r1_penalty"):
        got = [r["step"] for r in recs_a if r["tag"] == tag]
        assert got == [1, 3], (tag, got)
    assert names_a.count("r1_seed") == 2 and names_a.count("instnorm_jvp_stats") == names_a.count("instnorm_jvp_bwd") == 2 * 2 * 2
    _, sd_b, _, _ = run("b", ["--max_steps", "4"])
    assert any(not torch.equal(sd_a[k], sd_b[k]) for k in sd_b if sd_b[k].is_floating_point())
    assert all(bool(torch.isfinite(v).all()) for v in sd_a.values() if v.is_floating_point())
