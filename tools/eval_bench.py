"""Evaluation micro-benchmark (evaluate.py's GPU work, csrc/metrics.hip + AlexNet on the fp32 conv engine).

  python tools/eval_bench.py [--pairs B] [--reps R] [--e2e N] [--out DIR] [--only viz|prdc]

1. pair statistics (gray + SSIM + SSE) on B synthetic device-resident 1024x768 RGB pairs: event time per pair and the fraction
   of the larger of two floors -- bytes (both uint8 images read once, at the measured 6.29 TB/s copy rate) and VALU FLOPs (the
   kernel's separable-filter arithmetic at the 157.3 TFLOP/s fp32 vector peak);
2. LPIPS (input conversion, five convolutions, two pools, fused head) per pair at 128x128, batch B;
3. Inception-v3 (input conversion, 94 convolutions, the pools, the head) per image at 299x299, batch 1 and B, on seeded random
   weights: event time per image, and the conv engine's TFLOP/s over the 94 convolutions from a per-launch profile (their
   algorithmic FLOPs, 11.4 GFLOP = 5.7 G multiply-adds per image, over the sum of their event times);
4. a full evaluate.py run over N synthetic 1024x768 JPEG pairs in a child process: wall time split into time blocked on the
   DataLoader (CPU decode / resize) and time in the GPU scorer.
5. the validation passes' kernels (csrc/validate.hip): LPIPS of two 1024x768 fp32 images resized to 128x128, fused front end
   (``forward_resized``: one launch for both resizes and ScalingLayers) against the unfused one (``forward`` of two
   ``glue.resize_nchw`` results: four launches and a round trip), batch 1 and B, whole call and front end alone; and the IoU count
   kernel at 8 x 256 x 192 and 4 x 1024 x 768 as bytes (108 per pixel) over event time.
6. FID / KID (``evaluate.py --fid``): the FID Inception-v3's pooled features per image from decoded 1024x768 uint8 images (input
   kernel with the 299x299 resize, 94 convolutions, pools, mean), batch 1 and B, on seeded random weights; and the statistics over
   feature banks of 2032 x 2048 (the size of a VITON-HD test set): ``moments`` (mean, centre-and-transpose, the symmetric fp64
   covariance GEMM: 2 x 2048^2 x 2032 / 2 FLOPs computed), one ``poly_gram`` of 2032 x 2032 x 2048, both as TFLOP/s of fp64 over
   event time, KID's subset sums for 100 subsets of 1000, and the host's Frechet distance (two 2048 x 2048 ``eigh``) in wall time.
7. the image grids (csrc/viz.hip, ``--only viz`` runs this section alone): ``viz.grid_u8`` over the 12 panels of the try-on grid at
   1024x768, N = 1 and 4 -- event time of the launch, the GB/s of its algorithmic bytes (every source element once, every output
   byte once) against the copy rate, and the wall time including the uint8 copy to the host -- next to the host path measured in
   the same process: the fp32 panels copied to the host and composed there as the reference does (argmax + PIL palette, make_grid,
   mul(255).add(0.5).clamp).  The same for ``save_images``' quantise-and-copy at 1024x768, batch 16, against the host expression.
8. precision / recall / density / coverage (``evaluate.py --prdc``, csrc/manifold.hip; ``--only prdc`` runs this section alone and,
   with ``--out DIR``, writes DIR/prdc_bench.txt): two Gaussian banks of 2032 x 2048 -- each of the four launches (row norms, one
   2032 x 2032 block of squared distances next to ``poly_gram`` on the same banks, the k-th smallest of its rows, ball counts and
   minima), the whole of ``manifold.prdc``, and in the same run the same computation written in torch (``torch.cdist`` on fp64
   copies, ``kthvalue``, compare and sum).
Event times include launch gaps; for kernel-only times run this under ``rocprofv3 --kernel-trace --stats`` in a run of its own.
Prints one JSON line.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import hr_viton_amd  # noqa: E402,F401
from hr_viton_amd import metrics  # noqa: E402
from hr_viton_amd import ops  # noqa: E402
from hr_viton_amd.eval_models import PerceptualLoss  # noqa: E402
from hr_viton_amd.inception import Inception3  # noqa: E402

HBM_BPS = 6.29e12          # measured float4 copy rate (MI355X_MICROARCH: 79 % of the 8 TB/s spec)
VALU_FLOPS = 157.3e12      # fp32 vector peak


def pair_floor_s(B, H, W):
    """max(byte floor, VALU floor) of one hrv_pair_stats_u8 launch (FMA = 2 FLOPs)."""
    tw, th, r = 64, 16, 5
    tiles = -(-W // tw) * -(-H // th)
    halo = (tw + 2 * r) * (th + 2 * r)
    # per block: gray of both staged images (3 mul-add + shift each), the vertical pass (5 sums x 11 taps + 3 products per
    # row-column), the horizontal pass (5 x 11 FMAs + ~16 FLOPs of the SSIM formula per output)
    flops = tiles * (halo * 2 * 7 + th * (tw + 2 * r) * (5 * 11 * 2 + 3) + th * tw * (5 * 11 * 2 + 16))
    return max(2.0 * B * H * W * 3 / HBM_BPS, B * flops / VALU_FLOPS), 2.0 * B * H * W * 3 / HBM_BPS, B * flops / VALU_FLOPS


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / 1e3 / reps


def inception_bench(B, reps):
    """Per batch size: event time per image of forward_u8, and from one profiled pass the convolutions' FLOPs, their summed event
    times and the launch count."""
    torch.manual_seed(0)
    net = Inception3().eval()
    g = torch.Generator(device="cuda").manual_seed(1)
    out = {}
    for b in sorted({1, B}):
        img = torch.randint(0, 256, (b, 299, 299, 3), dtype=torch.uint8, device="cuda", generator=g)
        t = timed(lambda: net.forward_u8(img), reps)
        net.forward_u8(img)
        ops.profile_begin()
        net.forward_u8(img)
        rec = ops.profile_end()
        conv = [r for r in rec if r[0] == "conv"]
        flops, ms = sum(r[2] for r in conv), sum(r[4] for r in conv)
        out[f"batch_{b}"] = {"us_per_image": 1e6 * t / b, "launches_profiled": len(rec), "convs": len(conv),
                             "conv_gflop_per_image": flops / b / 1e9, "conv_event_ms": ms,
                             "conv_tflops_over_event_time": flops / (ms * 1e-3) / 1e12 if ms > 0 else None,
                             "tflops_over_wall": flops / t / 1e12}
    return out


def fid_bench(B, reps, n=2032, D=2048):
    from hr_viton_amd import feat_stats
    from hr_viton_amd.inception import FIDInceptionV3
    torch.manual_seed(0)
    net = FIDInceptionV3().eval()
    g = torch.Generator(device="cuda").manual_seed(3)
    out = {"features_1024x768": {}}
    for b in sorted({1, B}):
        img = torch.randint(0, 256, (b, 1024, 768, 3), dtype=torch.uint8, device="cuda", generator=g)
        out["features_1024x768"][f"batch_{b}"] = {"us_per_image": 1e6 * timed(lambda: net.features_u8(img), reps) / b}
    del net
    fp = torch.randn(n, D, device="cuda", generator=g).abs_()
    fg = torch.randn(n, D, device="cuda", generator=g).abs_() * 1.1
    r = max(2, reps // 4)
    t_m = timed(lambda: feat_stats.moments(fp), r)
    t_g = timed(lambda: feat_stats.poly_gram(fp, fg), r)
    t_gs = timed(lambda: feat_stats.poly_gram(fp, fp), r)
    ix, iy = feat_stats.kid_subsets(n, n, 1000, 100)
    kxx, kyy, kxy = feat_stats.poly_gram(fp, fp), feat_stats.poly_gram(fg, fg), feat_stats.poly_gram(fp, fg)
    ixd, iyd = torch.from_numpy(ix).cuda(), torch.from_numpy(iy).cuda()
    t_k = timed(lambda: feat_stats.kid_subset_sums(kxx, kyy, kxy, ixd, iyd), r)
    (mu1, s1), (mu2, s2) = feat_stats.moments(fp), feat_stats.moments(fg)
    t0 = time.perf_counter()
    fid = feat_stats.frechet_distance(mu1, s1, mu2, s2)
    t_f = time.perf_counter() - t0
    tri = (D // 64) * (D // 64 + 1) // 2 * 64 * 64          # elements of the computed triangle of 64 x 64 tiles
    out["stats_%dx%d" % (n, D)] = {
        "moments_ms": 1e3 * t_m, "moments_tflops_f64": 2.0 * tri * n / t_m / 1e12,
        "poly_gram_ms": 1e3 * t_g, "poly_gram_tflops_f64": 2.0 * n * n * D / t_g / 1e12,
        "poly_gram_symmetric_ms": 1e3 * t_gs, "kid_subset_sums_100x1000_ms": 1e3 * t_k,
        "frechet_distance_host_s": t_f, "fid_of_the_synthetic_banks": fid}
    return out


def validation_bench(B, reps):
    from hr_viton_amd import _lib, glue
    torch.manual_seed(0)
    net = PerceptualLoss().net
    _, _, (sh, sc) = net.plan(torch.device("cuda"))
    lib = _lib.load()
    g = torch.Generator(device="cuda").manual_seed(2)
    out = {"lpips_resized_1024x768": {}, "seg_iou": {}}
    for b in sorted({1, B}):
        x = torch.rand(b, 3, 1024, 768, device="cuda", generator=g) * 2 - 1
        y = torch.rand(b, 3, 1024, 768, device="cuda", generator=g) * 2 - 1
        both = torch.empty(2 * b, 128, 128, 4, device="cuda")

        def front_fused():
            lib.hrv_lpips_prep_resize_nchw_f32(x.data_ptr(), y.data_ptr(), b, 1024, 768, 128, 128, 0, sh, sc, both.data_ptr(),
                                               ops._stream())

        def front_unfused():
            for i, t in enumerate((x, y)):
                r = glue.resize_nchw(t, (128, 128))
                lib.hrv_lpips_prep_nchw_f32(r.data_ptr(), b, 128, 128, 0, sh, sc, both[i * b:].data_ptr(), ops._stream())

        out["lpips_resized_1024x768"][f"batch_{b}"] = {
            "fused_us_per_pair": 1e6 * timed(lambda: net.forward_resized(x, y), reps) / b,
            "unfused_us_per_pair": 1e6 * timed(lambda: net.forward(glue.resize_nchw(x, (128, 128)), glue.resize_nchw(y, (128, 128))),
                                               reps) / b,
            "front_end_fused_us": 1e6 * timed(front_fused, reps), "front_end_unfused_us": 1e6 * timed(front_unfused, reps)}
    for n, h, w in ((8, 256, 192), (4, 1024, 768)):
        seg = torch.randn(n, 13, h, w, device="cuda", generator=g) * 4
        cm = torch.rand(n, 1, h, w, device="cuda", generator=g)
        lab = torch.zeros(n, 13, h, w, device="cuda").scatter_(1, torch.randint(0, 13, (n, 1, h, w), device="cuda", generator=g), 1.0)
        cnt = torch.empty(n, 3, dtype=torch.int64, device="cuda")
        t = timed(lambda: metrics.seg_iou_counts(seg, cm, lab, "warp_grad", out=cnt), reps)
        out["seg_iou"][f"{n}x{h}x{w}"] = {"us": 1e6 * t, "gb_per_s": 108.0 * n * h * w / t / 1e9,
                                          "fraction_of_copy_rate": 108.0 * n * h * w / t / HBM_BPS}
    return out


def _wall(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def _host_visualize_segmap(x, batch, palette):
    from PIL import Image
    im = Image.fromarray(np.argmax(x[batch].float().numpy(), axis=0).astype(np.uint8), "P")
    im.putpalette(palette)
    return torch.from_numpy(np.array(im.convert("RGB"))).permute(2, 0, 1).float().div(255)


def _host_make_grid(ts, nrow, pad=2):
    t = torch.stack(ts)
    n, _, H, W = t.shape
    xm = min(nrow, n)
    ym = -(-n // xm)
    g = t.new_zeros((3, ym * (H + pad) + pad, xm * (W + pad) + pad))
    for k in range(n):
        y0, x0 = (k // xm) * (H + pad) + pad, (k % xm) * (W + pad) + pad
        g[:, y0:y0 + H, x0:x0 + W].copy_(t[k])
    return g


def viz_bench(reps, H=1024, W=768):
    """Section 7.  The comparator is the reference's own path (test_generator.py:223-229, utils.py:93-109) on CPU tensors, never
    the code under test."""
    from hr_viton_amd import viz
    g = torch.Generator(device="cuda").manual_seed(4)
    out = {"tryon_grid_1024x768": {}}
    for N in (1, 4):
        u = lambda c: torch.rand(N, c, H, W, device="cuda", generator=g) * 2 - 1  # noqa: E731
        inputs = {"cloth": u(3), "parse_agnostic": u(13), "densepose": u(3), "pose": u(3), "agnostic": u(3), "image": u(3)}
        gauss = ops.alloc(N, H, W, 13, "cuda")
        gauss.t.copy_(torch.rand(N, H, W, 16, device="cuda", generator=g))
        res = {"pre_clothes_mask": (u(1) > 0).float(), "warped_cloth": u(3), "warped_clothmask": u(1) * 0.5 + 0.5,
               "fake_parse_gauss": gauss, "output": u(3)}
        src_bytes = 4.0 * N * H * W * (3 * 8 + 1 * 2 + 13 + 16)       # 8 colour panels, 2 masks, 13 planes, 4 float4 per NHWC pixel
        res_ref = dict(res, fake_parse_gauss=ops.to_nchw(gauss))    # the reference holds it NCHW on the device: not timed
        grid = viz.tryon_grid(inputs, res)
        nbytes = src_bytes + grid.numel()
        t_k = timed(lambda: viz.tryon_grid(inputs, res), reps)
        t_e2e = _wall(lambda: viz.to_host(viz.tryon_grid(inputs, res)), reps)

        def host_path():
            cpu = {k: v.cpu() for k, v in inputs.items()}
            r = {k: v.cpu() for k, v in res_ref.items()}
            grids = []
            for i in range(N):
                seg = lambda t: _host_visualize_segmap(t, i, viz.PALETTE)  # noqa: E731
                grids.append(_host_make_grid(
                    [cpu["cloth"][i] / 2 + 0.5, r["pre_clothes_mask"][i].expand(3, -1, -1), seg(cpu["parse_agnostic"]),
                     (cpu["densepose"][i] + 1) / 2, r["warped_cloth"][i] / 2 + 0.5, r["warped_clothmask"][i].expand(3, -1, -1),
                     seg(r["fake_parse_gauss"]), cpu["pose"][i] / 2 + 0.5, r["warped_cloth"][i] / 2 + 0.5, cpu["agnostic"][i] / 2 + 0.5,
                     cpu["image"][i] / 2 + 0.5, r["output"][i] / 2 + 0.5], 4).mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0)
                    .to(torch.uint8))
            return grids

        t_host = _wall(host_path, max(1, reps // 10))
        same = all(torch.equal(a, b) for a, b in zip(host_path(), viz.tryon_grid(inputs, res).cpu()))
        out["tryon_grid_1024x768"][f"N_{N}"] = {
            "kernel_us": 1e6 * t_k, "gb_per_s": nbytes / t_k / 1e9, "fraction_of_copy_rate": nbytes / t_k / HBM_BPS,
            "device_path_with_u8_copy_ms": 1e3 * t_e2e, "host_path_ms": 1e3 * t_host, "host_over_device": t_host / t_e2e,
            "bytes_equal": bool(same)}
    B = 16
    img = torch.rand(B, 3, H, W, device="cuda", generator=g) * 2.4 - 1.2
    t_k = timed(lambda: viz.quantize_images(img), reps)
    t_e2e = _wall(lambda: viz.to_host(viz.quantize_images(img)), reps)
    host = lambda: [((t.clone() + 1) * 0.5 * 255).cpu().clamp(0, 255).numpy().astype("uint8") for t in img]  # noqa: E731
    t_host = _wall(host, max(1, reps // 10))
    nbytes = 5.0 * B * H * W * 3                                   # 4 bytes in + 1 byte out per element
    out["save_images_1024x768_b16"] = {
        "kernel_us": 1e6 * t_k, "gb_per_s": nbytes / t_k / 1e9, "fraction_of_copy_rate": nbytes / t_k / HBM_BPS,
        "quantise_and_copy_ms": 1e3 * t_e2e, "host_path_ms": 1e3 * t_host, "host_over_device": t_host / t_e2e}
    return out


def _torch_prdc(real, fake, k):
    """Naeem et al.'s ``prdc`` written in torch on the device: fp64 copies, ``torch.cdist``, ``kthvalue`` (the k + 1-th of a row
    that holds its own zero), compare and sum."""
    R, F = real.double(), fake.double()
    dRR, dFF, dRF = torch.cdist(R, R), torch.cdist(F, F), torch.cdist(R, F)
    rR, rF = dRR.kthvalue(k + 1, dim=1).values, dFF.kthvalue(k + 1, dim=1).values
    inside = dRF < rR[:, None]
    return {"precision": inside.any(dim=0).double().mean().item(), "recall": (dRF < rF[None, :]).any(dim=1).double().mean().item(),
            "density": inside.sum(dim=0).double().mean().item() / k, "coverage": (dRF.min(dim=1).values < rR).double().mean().item()}


def prdc_bench(reps, n=2032, D=2048, k=5):
    """Section 8.  Returns (dict, text): the four launches of csrc/manifold.hip one by one (event time), the whole of
    ``manifold.prdc`` and the same computation in torch (host clock around calls that end in a read-back), same run, same GPU."""
    from hr_viton_amd import feat_stats, manifold
    g = torch.Generator(device="cuda").manual_seed(5)
    real = torch.randn(n, D, device="cuda", generator=g)
    fake = torch.randn(n, D, device="cuda", generator=g) * 1.05 + 0.02
    r = max(5, reps)
    nR, nF = manifold.row_sqnorm(real), manifold.row_sqnorm(fake)
    d_self = manifold.sqdist(real, real, nR, nR, self_offset=0)
    rR = manifold.row_kth(d_self, k)
    d = manifold.sqdist(real, fake, nR, nF)
    t = {"row_sqnorm": timed(lambda: manifold.row_sqnorm(real), r),
         "sqdist": timed(lambda: manifold.sqdist(real, fake, nR, nF), r),
         "row_kth": timed(lambda: manifold.row_kth(d_self, k), r),
         "row_ball": timed(lambda: manifold.row_ball(d, rR), r),
         "poly_gram": timed(lambda: feat_stats.poly_gram(real, fake), r)}
    t_hip = _wall(lambda: manifold.prdc(real, fake, k), r)
    t_torch = _wall(lambda: _torch_prdc(real, fake, k), r)
    got, ref = manifold.prdc(real, fake, k), _torch_prdc(real, fake, k)
    flop = 2.0 * n * n * D
    blk = 8.0 * n * n
    out = {"n": n, "D": D, "k": k, "reps": r,
           "row_sqnorm_us": 1e6 * t["row_sqnorm"], "row_sqnorm_gb_per_s": 4.0 * n * D / t["row_sqnorm"] / 1e9,
           "sqdist_ms": 1e3 * t["sqdist"], "sqdist_tflops_f64": flop / t["sqdist"] / 1e12,
           "poly_gram_ms": 1e3 * t["poly_gram"], "sqdist_over_poly_gram": t["sqdist"] / t["poly_gram"],
           "row_kth_us": 1e6 * t["row_kth"], "row_kth_gb_per_s": blk / t["row_kth"] / 1e9,
           "row_ball_us": 1e6 * t["row_ball"], "row_ball_gb_per_s": blk / t["row_ball"] / 1e9,
           "prdc_ms": 1e3 * t_hip, "torch_prdc_ms": 1e3 * t_torch, "torch_over_hip": t_torch / t_hip,
           "prdc": {m: got[m] for m in ("precision", "recall", "density", "coverage")}, "torch_prdc": ref}
    text = "\n".join([
        "prdc_bench: %s" % torch.cuda.get_device_name(0),
        "two Gaussian banks of %d x %d fp32, k = %d; %d repetitions after one warm-up call; event times include launch gaps" % (n, D, k, r),
        "  row_sqnorm   %9.1f us   (%.0f GB/s of the bank read once)" % (out["row_sqnorm_us"], out["row_sqnorm_gb_per_s"]),
        "  sqdist       %9.3f ms   (%.1f TFLOP/s fp64 over 2 n^2 D; poly_gram, the same skeleton, same run: %.3f ms, ratio %.2f)"
        % (out["sqdist_ms"], out["sqdist_tflops_f64"], out["poly_gram_ms"], out["sqdist_over_poly_gram"]),
        "  row_kth      %9.1f us   (%.0f GB/s of the %d x %d fp64 block read once)" % (out["row_kth_us"], out["row_kth_gb_per_s"], n, n),
        "  row_ball     %9.1f us   (%.0f GB/s of the block read once)" % (out["row_ball_us"], out["row_ball_gb_per_s"]),
        "  prdc() whole %9.3f ms   host clock, ends in the read-back of counts and radii (2 norms, 4 distance blocks, 2 row_kth, 2 row_ball)"
        % out["prdc_ms"],
        "  torch route  %9.3f ms   host clock: fp64 copies, 3 torch.cdist, 2 kthvalue, compare and sum, 4 .item()" % out["torch_prdc_ms"],
        "  torch route / prdc(): %.2f" % out["torch_over_hip"],
        "  prdc()      : " + " / ".join("%s %.6f" % (m, got[m]) for m in ("precision", "recall", "density", "coverage")),
        "  torch route : " + " / ".join("%s %.6f" % (m, ref[m]) for m in ("precision", "recall", "density", "coverage")),
    ]) + "\n"
    return out, text


def e2e(n, workers, batch):
    from PIL import Image
    rng = np.random.default_rng(0)
    with tempfile.TemporaryDirectory() as d:
        gt, pr = os.path.join(d, "gt"), os.path.join(d, "pred")
        os.makedirs(gt)
        os.makedirs(pr)
        base = rng.integers(0, 256, (1024, 768, 3), dtype=np.uint8)
        for i in range(n):
            img = np.roll(base, i, axis=1)
            Image.fromarray(img).save(os.path.join(gt, f"{i:05d}_00.jpg"), quality=95)
            Image.fromarray(np.roll(img, 1, axis=0)).save(os.path.join(pr, f"{i:05d}_00_{i:05d}_00.png"), format="JPEG")
        code = ("import sys, json; sys.argv=['evaluate.py']; import evaluate; "
                f"r = evaluate.main(['--predict_dir', {pr!r}, '--ground_truth_dir', {gt!r}, '--lpips_random_init', "
                f"'-j', '{workers}', '-b', '{batch}']); print('E2E ' + json.dumps(r['timings']))")
        t0 = time.perf_counter()
        r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=900)
        wall = time.perf_counter() - t0
        if r.returncode != 0:
            raise RuntimeError(r.stderr[-3000:])
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("E2E ")][-1]
        t = json.loads(line[4:])
        t["process_wall_s"] = wall
        t["pairs"] = n
        return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=16)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--e2e", type=int, default=64, help="pairs of the evaluate.py run (0: skip)")
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--out", default="")
    ap.add_argument("--only", default="", choices=["", "viz", "prdc"], help="run one section alone")
    a = ap.parse_args()
    if a.only == "prdc":
        res, text = prdc_bench(a.reps)
        print(text, end="")
        print(json.dumps({"prdc": res}))
        if a.out:
            os.makedirs(a.out, exist_ok=True)
            with open(os.path.join(a.out, "prdc_bench.txt"), "w") as f:
                f.write(text)
        return
    if a.only == "viz":
        res = {"viz": viz_bench(a.reps)}
        print(json.dumps(res))
        if a.out:
            os.makedirs(a.out, exist_ok=True)
            with open(os.path.join(a.out, "eval_bench_viz.json"), "w") as f:
                json.dump(res, f, indent=1)
        return
    B, H, W = a.pairs, 1024, 768
    g = torch.Generator(device="cuda").manual_seed(0)
    gt = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, device="cuda", generator=g)
    pred = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, device="cuda", generator=g)
    t_ps = timed(lambda: metrics.pair_stats(gt, pred), a.reps)
    floor, fb, ff = pair_floor_s(B, H, W)
    torch.manual_seed(0)
    model = PerceptualLoss()
    g128 = gt[:, :128, :128].contiguous()
    p128 = pred[:, :128, :128].contiguous()
    t_lp = timed(lambda: model.forward_u8(g128, p128), a.reps)
    res = {"pair_stats": {"B": B, "H": H, "W": W, "ms_per_pair": 1e3 * t_ps / B, "floor_ms_per_pair": 1e3 * floor / B,
                          "byte_floor_ms_per_pair": 1e3 * fb / B, "valu_floor_ms_per_pair": 1e3 * ff / B,
                          "fraction_of_floor": floor / t_ps},
           "lpips_128": {"B": B, "ms_per_pair": 1e3 * t_lp / B},
           "inception_299": inception_bench(B, a.reps), "validation": validation_bench(B, a.reps), "fid": fid_bench(B, a.reps),
           "viz": viz_bench(a.reps), "prdc": prdc_bench(a.reps)[0]}
    if a.e2e:
        res["evaluate_py"] = e2e(a.e2e, a.workers, B)
    print(json.dumps(res))
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "eval_bench.json"), "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
