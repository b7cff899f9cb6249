"""GPU: Inception-v3 on the HIP path (hr_viton_amd/inception.py, csrc/inception.hip, ConvLayer's horizontal padding) and
evaluate.py's Inception Score against the float64 restatement of tests/inception_cases.py.

Yardstick of the network tests: the SAME restatement run by torch in fp32 on the CPU, on the same weights and inputs, compared with
float64 in the same test.  Both are fp32 computations of one unit roundoff that differ in summation order (MFMA accumulation,
split-K), so each error is one draw of the same size; the HIP path has to stay within 4 x the CPU's error.  4 x covers the draw, not
a different precision.  Both sides are written to test_diagnostics/inception_parity.txt.

Measured on an MI355X (the calibrated weights and 12 images of inception_cases.reference_run(0), IS 2.27): max |log p - log p64|
2.7e-4 at batch 12 and 2.2e-4 at batch 1 against 2.9e-4 for torch fp32 on the CPU; score relative error 8.1e-6 / 2.9e-7 against
3.7e-6; batch of 12 against 12 singles 3.1e-4.  The test prints every figure before it asserts.
"""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from PIL import Image

import inception_cases as K
from conftest import diag_path
from conv_dispatch_cases import excess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
FACTOR = 4.0


@pytest.fixture(scope="module")
def I():
    import hr_viton_amd  # noqa: F401
    from hr_viton_amd import inception
    return inception


@pytest.fixture(scope="module")
def ref():
    r = K.reference_run(0)
    p64 = torch.softmax(r["logits64"], 1).numpy()
    # the condition on the test inputs, on the float64 restatement alone: a score that tells images apart, no zero probability
    is64 = K.score64(p64)[0]
    print(f"reference: IS {is64:.4f}, probabilities in [{p64.min():.3e}, {p64.max():.3f}]")
    assert is64 >= 1.5 and p64.min() > 0.0, (is64, p64.min())
    return r


@pytest.fixture(scope="module")
def net(I, ref):
    m = I.Inception3()
    m.load_state_dict(ref["sd"])
    return m.eval()


def _nhwc(x, cstride=None, coff=0, fill=0.0):
    """fp32 NCHW CPU -> (Act over a CUDA NHWC tensor of ``cstride`` channels filled with ``fill``, holding x at ``coff``)"""
    from hr_viton_amd.ops import Act
    N, C, H, W = x.shape
    cs = C if cstride is None else cstride
    t = torch.full((N, H, W, cs), fill, dtype=torch.float32)
    t[..., coff:coff + C] = x.permute(0, 2, 3, 1)
    return Act(t.cuda(), C, coff)


def _nchw(a, c0=0, c=None):
    c = a.C - c0 if c is None else c
    return a.t[..., a.coff + c0:a.coff + c0 + c].permute(0, 3, 1, 2).cpu()


# ---------------------------------------------------------------------------------------------------------- pools
SENTINEL = -7168.0


@pytest.mark.parametrize("mode", [0, 1], ids=["max_s2", "avg_s1p1"])
@pytest.mark.parametrize("N,H,W,C", [(2, 35, 35, 288), (2, 17, 17, 768), (1, 73, 73, 64), (3, 23, 38, 20), (1, 3, 3, 4), (1, 8, 8, 2048)])
def test_pool3x3_slices(I, mode, N, H, W, C):
    from hr_viton_amd.ops import Act
    g = torch.Generator().manual_seed(H * 100 + W + mode)
    x = torch.randn(N, C, H, W, generator=g) * (1.0 + 3.0 * torch.rand(1, C, 1, 1, generator=g))
    want = F.max_pool2d(x.double(), 3, 2) if mode == 0 else F.avg_pool2d(x.double(), 3, 1, 1)
    src = _nhwc(x, cstride=C + 12, coff=4, fill=3.0e3)           # finite junk around the source slice
    Ho, Wo = want.shape[2:]
    out = Act(torch.full((N, Ho, Wo, C + 20), SENTINEL, dtype=torch.float32, device="cuda"), C, 8)
    I.pool3x3(src, mode, out)
    torch.cuda.synchronize()
    got = _nchw(out)
    if mode == 0:
        assert torch.equal(got.double(), want)
    else:
        # nine additions and one division: at most 2 fp32 ulps of the float64 result
        ulp = torch.from_numpy(np.spacing(np.abs(want.float().numpy()))).double()
        worst = ((got.double() - want).abs() / ulp).max().item()
        print(f"avg-pool {N}x{H}x{W}x{C}: worst error {worst:.3f} ulp")
        assert worst <= 2.0, worst
    full = out.t.cpu()
    assert (full[..., :8] == SENTINEL).all() and (full[..., 8 + C:] == SENTINEL).all()
    # dense, allocated by the wrapper
    dense = I.pool3x3(_nhwc(x), mode)
    assert dense.t.shape == (N, Ho, Wo, C) and torch.equal(_nchw(dense), got)


def test_pool3x3_bad_arguments_raise(I):
    from hr_viton_amd._lib import HrvError
    from hr_viton_amd.ops import Act
    with pytest.raises(ValueError):
        I.pool3x3(_nhwc(torch.zeros(1, 4, 2, 9)), 0)
    a = _nhwc(torch.zeros(1, 4, 9, 9))
    with pytest.raises(HrvError):       # a destination slice off the 4-channel granule
        I.pool3x3(a, 1, Act(torch.zeros((1, 9, 9, 10), device="cuda"), 4, 2))


# ---------------------------------------------------------------------------------------------------------- ConvLayer(pad_w=...)
PADW_CASES = [  # (cin, cout, (kh, kw), (ph, pw), H, W): the table's shapes and channel counts
    (128, 128, (1, 7), (0, 3), 17, 17), (128, 192, (7, 1), (3, 0), 17, 17), (160, 160, (7, 1), (3, 0), 17, 17),
    (160, 192, (1, 7), (0, 3), 17, 17), (192, 192, (1, 7), (0, 3), 17, 17), (192, 192, (7, 1), (3, 0), 17, 17),
    (384, 384, (1, 3), (0, 1), 8, 8), (384, 384, (3, 1), (1, 0), 8, 8)]


@pytest.mark.parametrize("N", [1, 16])
@pytest.mark.parametrize("case", PADW_CASES, ids=lambda c: f"{c[0]}-{c[1]}-{c[2][0]}x{c[2][1]}")
def test_convlayer_pad_w(I, N, case):
    from hr_viton_amd import ops
    cin, cout, (kh, kw), (ph, pw), H, W = case
    g = torch.Generator().manual_seed(cin + 7 * kh + N)
    x = torch.relu(torch.randn(N, cin, H, W, generator=g))          # post-ReLU activations, zero-mean weights
    w = torch.randn(cout, cin, kh, kw, generator=g) * math.sqrt(2.0 / (cin * kh * kw))
    ref64 = F.conv2d(x.double(), w.double(), padding=(ph, pw))
    A = F.conv2d(x.double().abs(), w.double().abs(), padding=(ph, pw))
    layer = ops.ConvLayer(w, [cin], "cuda", pad=ph, pad_w=pw, name=f"padw{kh}x{kw}")
    # written into a slice of a wider tensor, as the blocks do
    out = ops.Act(torch.full((N, H, W, cout + 8), SENTINEL, dtype=torch.float32, device="cuda"), cout, 4)
    layer([_nhwc(x)], out=out)
    torch.cuda.synchronize()
    got = _nchw(out)
    assert got.shape == ref64.shape
    e, i = excess(got, ref64, A, cin * kh * kw)
    print(f"pad_w {case} N={N}: error / allowance {e:.3f}")
    assert e <= 1.0, (e, i)
    full = out.t.cpu()
    assert (full[..., :4] == SENTINEL).all() and (full[..., 4 + cout:] == SENTINEL).all()


@pytest.mark.parametrize("N", [1, 16])
def test_convlayer_pad_w_none_is_bit_identical(I, N):
    from hr_viton_amd import ops
    g = torch.Generator().manual_seed(3)
    x = torch.randn(N, 96, 35, 35, generator=g)
    w = torch.randn(96, 96, 3, 3, generator=g) * 0.05
    a = ops.ConvLayer(w, [96], "cuda", pad=1, act=ops.ACT_RELU)([_nhwc(x)])
    b = ops.ConvLayer(w, [96], "cuda", pad=1, pad_w=1, act=ops.ACT_RELU)([_nhwc(x)])
    torch.cuda.synchronize()
    assert torch.equal(a.t, b.t)


# ---------------------------------------------------------------------------------------------------------- blocks
@pytest.mark.parametrize("name", ["Mixed_5b", "Mixed_6a", "Mixed_6b", "Mixed_7a", "Mixed_7b"])
def test_block_branches(I, net, ref, name):
    """One block of each type on the restatement's own input for it (4 images): every branch slice against float64, bounded by
    4 x the error of the fp32 CPU run of the same block; a swapped cat order or a swapped (1,7)/(7,1) fails here by name."""
    x32 = ref["io"][name][0][:4].float()
    with torch.no_grad():
        want = K.BLOCK_FN[name](K._Run(ref["sd"], torch.float64), name, x32.double())
        cpu = K.BLOCK_FN[name](K._Run(ref["sd"], torch.float32), name, x32)
    out = net.run_block(name, _nhwc(x32))
    torch.cuda.synchronize()
    assert out.C == sum(b.shape[1] for b in want) and (out.H, out.W) == tuple(want[0].shape[2:])
    off = 0
    for k, (w64, c32) in enumerate(zip(want, cpu)):
        got = _nchw(out, off, w64.shape[1])
        off += w64.shape[1]
        err = (got.double() - w64).abs().max().item()
        err_cpu = (c32.double() - w64).abs().max().item()
        print(f"{name} branch {k} [{w64.shape[1]} ch]: HIP {err:.3e}, torch fp32 CPU {err_cpu:.3e}, |ref| max {w64.abs().max().item():.3f}")
        assert err <= FACTOR * err_cpu, (name, k, err, err_cpu)


# ---------------------------------------------------------------------------------------------------------- whole network
def _errors(logp, ref64):
    """(max |log p - log p64|, relative error of the score) of log-probabilities [n, 1000] in float64"""
    lp64 = K.log_probs(ref64)
    s64 = K.score64(torch.exp(lp64).numpy())[0]
    s = K.score64(torch.exp(logp).numpy())[0]
    return (logp - lp64).abs().max().item(), abs(s / s64 - 1.0)


def test_network_parity(I, net, ref):
    img = torch.from_numpy(ref["img"]).cuda()
    x = ref["x"].cuda()
    l64 = ref["logits64"]
    cpu_lp, cpu_sc = _errors(K.log_probs(ref["logits32"]).double(), l64)
    rows = [("torch fp32 CPU", cpu_lp, cpu_sc)]
    # batch 12
    p_u8 = net.forward_u8(img)
    logits = net(x)
    # 12 batches of 1
    p_single = torch.cat([net.forward_u8(img[i:i + 1]) for i in range(img.shape[0])])
    l_single = torch.cat([net(x[i:i + 1]) for i in range(img.shape[0])])
    torch.cuda.synchronize()
    assert p_u8.shape == (12, 1000) and p_u8.dtype == torch.float32 and logits.shape == (12, 1000)
    assert (p_u8 > 0).all() and abs(p_u8.double().sum(1) - 1).max().item() < 1e-5
    rows.append(("HIP forward_u8, batch 12", *_errors(torch.log(p_u8.double().cpu()), l64)))
    rows.append(("HIP forward, batch 12", *_errors(K.log_probs(logits.double().cpu()), l64)))
    rows.append(("HIP forward_u8, batch 1 x 12", *_errors(torch.log(p_single.double().cpu()), l64)))
    rows.append(("HIP forward, batch 1 x 12", *_errors(K.log_probs(l_single.double().cpu()), l64)))
    batch_vs_single = (torch.log(p_u8.double()) - torch.log(p_single.double())).abs().max().item()
    lines = ["Inception-v3 parity against the float64 restatement (calibrated random weights, 12 images, IS %.4f)"
             % K.score64(torch.softmax(l64, 1).numpy())[0],
             "%-32s %-24s %s" % ("", "max |log p - log p64|", "score relative error")]
    lines += ["%-32s %-24.3e %.3e" % r for r in rows]
    lines.append("batch of 12 against 12 singles, max |log p - log p|: %.3e" % batch_vs_single)
    lines.append("bound: %.0f x the torch fp32 CPU row" % FACTOR)
    text = "\n".join(lines)
    print(text)
    with open(diag_path("inception_parity.txt"), "w") as f:
        f.write(text + "\n")
    for what, lp, sc in rows[1:]:
        assert lp <= FACTOR * cpu_lp, (what, lp, cpu_lp)
        assert sc <= FACTOR * cpu_sc, (what, sc, cpu_sc)
    assert batch_vs_single <= FACTOR * cpu_lp, (batch_vs_single, cpu_lp)
    # repeat runs: the same bits
    assert torch.equal(net.forward_u8(img), p_u8) and torch.equal(net(x), logits)
    assert torch.equal(net.forward_u8(img[3:4]), p_single[3:4])


def test_network_taps_and_input_kernel(I, net, ref):
    """the input kernel is ToTensor + Normalize(0.5, 0.5) in that fp32 order (bit-exact), and the tap extents are the table's"""
    from hr_viton_amd.ops import Act
    img = torch.from_numpy(ref["img"][:2]).cuda()
    taps = {}
    x = torch.empty((2, 299, 299, 4), dtype=torch.float32, device="cuda")
    from hr_viton_amd import _lib, ops
    _lib.check(_lib.load().hrv_lpips_prep_u8(img.data_ptr(), 2, 299, 299, I._ZERO3, I._ONE3, x.data_ptr(), ops._stream()), "prep")
    assert torch.equal(x[..., :3].permute(0, 3, 1, 2).cpu(), ref["x"][:2]) and (x[..., 3] == 0).all()
    net.features(Act(x, 3), taps)
    for name, (c, hw) in K.TAPS_299.items():
        assert (taps[name].C, taps[name].H, taps[name].W) == (c, hw, hw), name


def test_no_aten_kernels_on_the_forward_path(I, net, ref):
    """no cat / copy / fill launches: everything between the input and the probabilities is the library's"""
    from torch.profiler import ProfilerActivity, profile
    img = torch.from_numpy(ref["img"][:2]).cuda()
    net.forward_u8(img)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU]) as prof:
        net.forward_u8(img)
        torch.cuda.synchronize()
    names = {e.key for e in prof.key_averages()}
    bad = {n for n in names if n in ("aten::cat", "aten::copy_", "aten::fill_", "aten::zeros", "aten::zero_", "aten::clone",
                                     "aten::_to_copy")}
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------- evaluate.py
def _smooth(rng, H, W, i):
    c = [3, 6, 12, 24, 40, 9][i % 6]
    coarse = (rng.random((c, c, 3)) * 255).astype(np.uint8)
    base = np.asarray(Image.fromarray(coarse).resize((W, H), Image.BILINEAR), np.float64)
    return np.clip(base + rng.normal(0, 3.0 + 3 * (i % 3), base.shape), 0, 255).astype(np.uint8)


def _is_line(path, k):
    ln = path.read_text().splitlines()[k]
    a, b = ln.split(" / ")
    assert a.startswith("IS_mean : ") and b.startswith("IS_std : "), ln
    return float(a[10:]), float(b[9:])


def test_evaluate_inception_score_end_to_end(tmp_path):
    gt_dir, pr_dir = tmp_path / "gt", tmp_path / "pred"
    gt_dir.mkdir()
    pr_dir.mkdir()
    rng = np.random.default_rng(11)
    names = []
    for i in range(6):
        Image.fromarray(_smooth(rng, 256, 192, i)).save(gt_dir / f"{i:05d}_00.jpg", quality=95)
        nm = f"{i:05d}_00_{(i + 2) % 6:05d}_00.png"
        Image.fromarray(_smooth(rng, 256, 192, i + 1)).save(pr_dir / nm, format="JPEG")
        names.append(nm)
    base = [sys.executable, os.path.join(ROOT, "evaluate.py"), "--predict_dir", str(pr_dir), "--ground_truth_dir", str(gt_dir),
            "--lpips_random_init", "--seed", "5", "-j", "2", "-b", "4", "--lpips_weights", str(tmp_path / "no.pth"),
            "--alexnet_weights", str(tmp_path / "no2.pth"), "--inception_weights", str(tmp_path / "no3.pth")]

    def run(extra):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=900, cwd=str(tmp_path))
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        return r

    r1 = run(["--inception_random_init"])
    r2 = run(["--inception_random_init", "--is_splits", "2"])
    r3 = run([])
    lines = (pr_dir / "eval.txt").read_text().splitlines()
    assert len(lines) == 4 + 4 + 3, lines
    assert lines[2] == "LPIPS weights : random init (plumbing only)" and lines[3] == "Inception weights : random init (plumbing only)"
    assert lines[7] == lines[3] and lines[9] == "IS_mean : nan / IS_std : nan" and lines[10] == lines[2]
    assert "RANDOMLY initialised Inception-v3" in r1.stderr and "Inception" in r3.stderr and "plumbing only" in r1.stdout
    # the restatement on the weights the script builds: torch.manual_seed(seed), then Inception3()
    import hr_viton_amd  # noqa: F401
    from hr_viton_amd.inception import Inception3
    torch.manual_seed(5)
    sd = {k: v.detach().clone() for k, v in Inception3().state_dict().items()}
    x = K.normalize_u8(np.stack([np.asarray(Image.open(pr_dir / nm).convert("RGB").resize((299, 299), Image.BILINEAR))
                                 for nm in sorted(names)]))
    with torch.no_grad():
        p64 = torch.softmax(K.forward(sd, x, torch.float64), 1).numpy()
        p32 = torch.softmax(K.forward(sd, x, torch.float32), 1).double().numpy()
    for k, splits in ((1, 1), (5, 2)):
        m64, s64 = K.score64(p64, splits)
        m32, s32 = K.score64(p32, splits)
        got_m, got_s = _is_line(pr_dir / "eval.txt", k)
        assert math.isfinite(got_m) and got_m >= 1.0
        cpu_rel = abs(math.log(m32) / math.log(m64) - 1.0)
        rel = abs(math.log(got_m) / math.log(m64) - 1.0)
        print(f"splits {splits}: IS {got_m} (float64 {m64}), log-score relative error {rel:.3e}, torch fp32 CPU {cpu_rel:.3e}; "
              f"std {got_s} (float64 {s64}, fp32 CPU {s32})")
        assert rel <= max(FACTOR * cpu_rel, 1e-6), (rel, cpu_rel)
        if splits == 1:
            assert got_s == 0.0
        else:
            assert abs(got_s - s64) <= max(FACTOR * abs(s32 - s64), 1e-6 * m64), (got_s, s64, s32)
