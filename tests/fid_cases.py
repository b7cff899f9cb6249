"""Shared by tests/test_fid_cpu.py and tests/test_gpu_fid.py: FID / KID stated a second time in float64, independently of
hr_viton_amd/inception.py, hr_viton_amd/feat_stats.py and evaluate.py, and the case tables of the GPU tests.

  * ``prep64``: the FID input (x / 255, bilinear with align_corners=False and no antialiasing, 2v - 1) in float64 numpy;
  * ``forward``: pytorch-fid's Inception-v3 in ``torch.nn.functional`` on the CPU -- the units and the stem of tests/inception_cases.py,
    the pooled branches of FIDInceptionA / C / E_1 / E_2 -- up to the pooled 2048-wide vector;
  * ``frechet_sqrtm``: the Frechet distance through ``scipy.linalg.sqrtm(S1 @ S2).real`` (the formulation of pytorch-fid);
  * ``poly64`` / ``kid64``: KID's kernel and the unbiased MMD^2 over subsets by direct indexing of the Gram matrices;
  * ``fid_kid64``: the whole metric from two feature arrays (``np.cov``, the eigen formula, direct subset indexing).
"""
import numpy as np
import torch
import torch.nn.functional as F

import inception_cases as K

FID_SIZE = 299
# the torch-fidelity draw for (n_pred, n_gt, m, S) = (9, 11, 5, 3): np.random.RandomState(2020), per subset choice(9, 5, False) then
# choice(11, 5, False).  Stated in full; tests/test_fid_cpu.py holds the product's generator and ``draw_subsets`` below against it.
SUBSETS_9_11_5_3 = ([[2, 4, 7, 1, 5], [1, 2, 8, 7, 4], [1, 0, 3, 2, 4]],           # rows of the predictions, per subset
                    [[6, 9, 7, 4, 5], [0, 3, 10, 6, 8], [5, 0, 9, 10, 6]])        # rows of the ground truths


# ------------------------------------------------------------------------------------------------------------------ the input
def _axis(n_in, n_out):
    o = np.arange(n_out, dtype=np.float64)
    src = np.maximum(0.0, (o + 0.5) * n_in / n_out - 0.5)
    i0 = np.minimum(np.floor(src).astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    return i0, i1, src - i0


def prep64(img_u8, size=FID_SIZE):
    """uint8 [N,H,W,3] -> float64 [N,size,size,3]: 2 * interp(x / 255) - 1, source coordinate max(0, (o + 0.5) * in / out - 0.5), the
    upper neighbour clamped to the last row / column"""
    x = np.asarray(img_u8, np.float64) / 255.0
    y0, y1, ty = _axis(x.shape[1], size)
    x0, x1, tx = _axis(x.shape[2], size)
    tx = tx[None, None, :, None]
    ty = ty[None, :, None, None]
    top = x[:, y0][:, :, x0] * (1 - tx) + x[:, y0][:, :, x1] * tx
    bot = x[:, y1][:, :, x0] * (1 - tx) + x[:, y1][:, :, x1] * tx
    return 2.0 * (top * (1 - ty) + bot * ty) - 1.0


def prep_torch32(img_u8, size=FID_SIZE):
    """the same through torch's own fp32 CPU path, as pytorch-fid runs it: float32 [N,size,size,3]"""
    x = torch.from_numpy(np.ascontiguousarray(img_u8)).permute(0, 3, 1, 2).float() / 255
    y = F.interpolate(x, size=(size, size), mode="bilinear", align_corners=False)
    return (2 * y - 1).permute(0, 2, 3, 1).numpy()


# ------------------------------------------------------------------------------------------------------------------ the network
def _avg_inside(x):
    return F.avg_pool2d(x, kernel_size=3, stride=1, padding=1, count_include_pad=False)


def block_a(r, n, x):
    b1 = r.unit(f"{n}.branch1x1", x)
    b5 = r.unit(f"{n}.branch5x5_2", r.unit(f"{n}.branch5x5_1", x))
    b3 = r.unit(f"{n}.branch3x3dbl_3", r.unit(f"{n}.branch3x3dbl_2", r.unit(f"{n}.branch3x3dbl_1", x)))
    return [b1, b5, b3, r.unit(f"{n}.branch_pool", _avg_inside(x))]


def block_c(r, n, x):
    b1 = r.unit(f"{n}.branch1x1", x)
    b7 = r.unit(f"{n}.branch7x7_3", r.unit(f"{n}.branch7x7_2", r.unit(f"{n}.branch7x7_1", x)))
    bd = x
    for k in range(1, 6):
        bd = r.unit(f"{n}.branch7x7dbl_{k}", bd)
    return [b1, b7, bd, r.unit(f"{n}.branch_pool", _avg_inside(x))]


def _block_e(r, n, x, pooled):
    b1 = r.unit(f"{n}.branch1x1", x)
    b3 = r.unit(f"{n}.branch3x3_1", x)
    b3 = torch.cat([r.unit(f"{n}.branch3x3_2a", b3), r.unit(f"{n}.branch3x3_2b", b3)], 1)
    bd = r.unit(f"{n}.branch3x3dbl_2", r.unit(f"{n}.branch3x3dbl_1", x))
    bd = torch.cat([r.unit(f"{n}.branch3x3dbl_3a", bd), r.unit(f"{n}.branch3x3dbl_3b", bd)], 1)
    return [b1, b3, bd, r.unit(f"{n}.branch_pool", pooled)]


def block_e1(r, n, x):
    return _block_e(r, n, x, _avg_inside(x))


def block_e2(r, n, x):
    return _block_e(r, n, x, F.max_pool2d(x, kernel_size=3, stride=1, padding=1))


BLOCK_FN = dict(K.BLOCK_FN)
BLOCK_FN.update({"Mixed_5b": block_a, "Mixed_5c": block_a, "Mixed_5d": block_a, "Mixed_6b": block_c, "Mixed_6c": block_c,
                 "Mixed_6d": block_c, "Mixed_6e": block_c, "Mixed_7b": block_e1, "Mixed_7c": block_e2})
CHANGED_BLOCKS = ["Mixed_5b", "Mixed_6b", "Mixed_7b", "Mixed_7c"]      # one per changed type


def forward(sd, x, dtype=torch.float64):
    """x: [N,3,H,W] already normalised -> the pooled features [N,2048] in ``dtype`` (no fc: the metric never runs it)"""
    r = K._Run(sd, dtype)
    x = x.to(dtype)
    x = r.unit("Conv2d_2b_3x3", r.unit("Conv2d_2a_3x3", r.unit("Conv2d_1a_3x3", x)))
    x = F.max_pool2d(x, kernel_size=3, stride=2)
    x = r.unit("Conv2d_4a_3x3", r.unit("Conv2d_3b_1x1", x))
    x = F.max_pool2d(x, kernel_size=3, stride=2)
    for n in K.BLOCKS:
        x = torch.cat(BLOCK_FN[n](r, n, x), 1)
    return x.mean(dim=(2, 3))


def fid_state_dict(sd):
    """a torchvision-layout state dict of tests/inception_cases.py as the FID file lays it out: ``fc`` [1008, 2048]"""
    out = dict(sd)
    g = torch.Generator().manual_seed(1008)
    out["fc.weight"] = torch.randn(1008, 2048, generator=g) * 0.05
    out["fc.bias"] = torch.zeros(1008)
    return out


def state_keys():
    return K.state_keys(aux=False)


# ------------------------------------------------------------------------------------------------------------------ the statistics
def frechet_sqrtm(mu1, s1, mu2, s2):
    from scipy import linalg
    covmean = linalg.sqrtm(s1 @ s2)
    d = np.asarray(mu1, np.float64) - np.asarray(mu2, np.float64)
    return float(d @ d + np.trace(s1) + np.trace(s2) - 2.0 * np.trace(np.real(covmean)))


def frechet_eig(mu1, s1, mu2, s2, resolve=True):
    """the issue's formula, restated: eigenvalues of S1^(1/2) S2 S1^(1/2) from two eigh calls.  ``resolve``: eigenvalues below what
    a symmetric eigen-decomposition resolves (width x eps x the largest) are taken as the zeros they stand for; without it every null
    direction of a singular covariance adds sqrt(noise) ~ 1e-8 (measured on D = 32 from n = 8: asymmetry 1e-9, self-distance
    4e-8 tr S; 0 and 8e-16 with it)"""
    D = len(s1)
    w, V = np.linalg.eigh(s1)
    if resolve:
        w = np.where(w > D * np.finfo(np.float64).eps * w.max(), w, 0.0)
    root = (V * np.sqrt(np.maximum(w, 0.0))) @ V.T
    lam = np.linalg.eigvalsh(root @ s2 @ root)
    if resolve:
        lam = np.where(lam > D * np.finfo(np.float64).eps * lam.max(), lam, 0.0)
    d = np.asarray(mu1, np.float64) - np.asarray(mu2, np.float64)
    return float(d @ d + np.trace(s1) + np.trace(s2) - 2.0 * np.sqrt(np.maximum(lam, 0.0)).sum())


def frechet_svd(fp, fg):
    """the same distance from the feature rows themselves: with A = (X - mean)^T / sqrt(n - 1), S = A A^T, and the non-zero spectrum of
    S1 S2 is that of (A1^T A2)(A1^T A2)^T, so tr sqrtm(S1 S2) is the sum of the singular values of the n1 x n2 matrix A1^T A2 -- no
    square root of a noisy zero anywhere"""
    fp, fg = np.asarray(fp, np.float64), np.asarray(fg, np.float64)
    a1 = (fp - fp.mean(axis=0)) / np.sqrt(len(fp) - 1)
    a2 = (fg - fg.mean(axis=0)) / np.sqrt(len(fg) - 1)
    d = fp.mean(axis=0) - fg.mean(axis=0)
    return float(d @ d + (a1 * a1).sum() + (a2 * a2).sum() - 2.0 * np.linalg.svd(a1 @ a2.T, compute_uv=False).sum())


def gaussian_moments(n, D, seed, shift, scale):
    """(mean, cov) of n Gaussian rows of width D with a random mixing matrix: np.mean / np.cov in float64"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, D)) @ (rng.standard_normal((D, D)) * scale / np.sqrt(D)) + shift * rng.standard_normal(D)
    return x.mean(axis=0), np.cov(x, rowvar=False)


def poly64(X, Y):
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    return (X @ Y.T / X.shape[1] + 1.0) ** 3


def subset_sums64(Kxx, Kyy, Kxy, ix, iy):
    out = np.empty((len(ix), 3), np.float64)
    for s, (a, b) in enumerate(zip(ix, iy)):
        kxx, kyy, kxy = Kxx[np.ix_(a, a)], Kyy[np.ix_(b, b)], Kxy[np.ix_(a, b)]
        out[s] = (kxx.sum() - np.trace(kxx), kyy.sum() - np.trace(kyy), kxy.sum())
    return out


def kid64(Kxx, Kyy, Kxy, ix, iy):
    """(mean, std) over the subsets of the unbiased MMD^2, by direct indexing"""
    m = len(ix[0])
    vals = []
    for a, b in zip(ix, iy):
        kxx, kyy, kxy = Kxx[np.ix_(a, a)], Kyy[np.ix_(b, b)], Kxy[np.ix_(a, b)]
        vals.append((kxx.sum() - np.trace(kxx)) / (m * (m - 1)) + (kyy.sum() - np.trace(kyy)) / (m * (m - 1)) - 2.0 * kxy.mean())
    return float(np.mean(vals)), float(np.std(vals))


def draw_subsets(n_pred, n_gt, m, S):
    rng = np.random.RandomState(2020)
    ix, iy = [], []
    for _ in range(S):
        ix.append(rng.choice(n_pred, m, replace=False))
        iy.append(rng.choice(n_gt, m, replace=False))
    return np.asarray(ix), np.asarray(iy)


def fid_kid64(fp, fg, S, m):
    """(FID, KID mean, KID std) of two feature arrays on the host in float64"""
    fp, fg = np.asarray(fp, np.float64), np.asarray(fg, np.float64)
    fid = frechet_eig(fp.mean(axis=0), np.cov(fp, rowvar=False), fg.mean(axis=0), np.cov(fg, rowvar=False))
    ix, iy = draw_subsets(len(fp), len(fg), m, S)
    return (fid, *kid64(poly64(fp, fp), poly64(fg, fg), poly64(fp, fg), ix, iy))


# ------------------------------------------------------------------------------------------------------------------ GPU case tables
PREP_SIZES = [(5, 7), (11, 13), (64, 48), (300, 301), (1024, 768)]          # (H, W)
POOL_SHAPES = [(1, 3, 3, 4), (3, 23, 38, 20), (2, 8, 8, 2048), (2, 35, 35, 288)]      # (N, H, W, C)
GEMM_SHAPES = [(1, 1, 4), (16, 16, 4), (17, 33, 20), (48, 48, 100), (130, 70, 2048)]   # (rows, cols, k)
MOMENT_SHAPES = [(2, 16), (37, 20), (70, 2048)]                             # (n, D)


def write_pngs(folder, n, seed, H=64, W=48):
    """n smooth random RGB images H x W as PNG files NAME_00.png in ``folder``; returns the sorted names"""
    from PIL import Image
    rng = np.random.default_rng(seed)
    names = []
    for i in range(n):
        c = [2, 3, 5, 8][i % 4]
        coarse = (rng.random((c, c, 3)) * 255).astype(np.uint8)
        base = np.asarray(Image.fromarray(coarse).resize((W, H), Image.BILINEAR), np.float64)
        img = np.clip(base + rng.normal(0, 4.0 + 3 * (i % 3), base.shape), 0, 255).astype(np.uint8)
        nm = f"{i:05d}_00.png"
        Image.fromarray(img).save(folder / nm)
        names.append(nm)
    return sorted(names)


def read_images(folder, names):
    from PIL import Image
    return np.stack([np.asarray(Image.open(folder / nm).convert("RGB")) for nm in names])
