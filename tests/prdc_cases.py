"""Pure numpy float64 restatement of precision / recall / density / coverage as hr_viton_amd/manifold.py defines them (Naeem et
al.'s ``prdc`` on squared distances, own index excluded), the margins that let the GPU tests demand equality, and the case tables.

Nothing here imports the code under test."""
import numpy as np

U = 2.0 ** -53


def sqdist64(a, b):
    """[na, nb] squared distances by brute force on float64 copies: the differences squared and added over the last axis"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return ((a[:, None, :] - b[None, :, :]) ** 2).sum(-1)


def radii64(x, k):
    """the k-th smallest squared distance of every row to the OTHER rows: np.sort of the row with its own index removed"""
    d = sqdist64(x, x)
    n = d.shape[0]
    return np.array([np.sort(np.delete(d[i], i))[k - 1] for i in range(n)])


def parts64(real, fake, k):
    """dict(rR, rF, cntF, cntR, minR, dRF [nr, nf]) by direct comparison"""
    rR, rF = radii64(real, k), radii64(fake, k)
    dRF = sqdist64(real, fake)
    cntF = (dRF < rR[:, None]).sum(axis=0).astype(np.int64)          # cntF[j] = #{i : d2(F_j, R_i) < rR[i]}
    cntR = (dRF < rF[None, :]).sum(axis=1).astype(np.int64)          # cntR[i] = #{j : d2(R_i, F_j) < rF[j]}
    return {"rR": rR, "rF": rF, "cntF": cntF, "cntR": cntR, "minR": dRF.min(axis=1), "dRF": dRF}


def prdc64(real, fake, k):
    p = parts64(real, fake, k)
    nr, nf = p["cntR"].shape[0], p["cntF"].shape[0]
    return {"precision": float(np.count_nonzero(p["cntF"] > 0)) / nf, "recall": float(np.count_nonzero(p["cntR"] > 0)) / nr,
            "density": float(int(p["cntF"].sum())) / (k * nf), "coverage": float(np.count_nonzero(p["minR"] < p["rR"])) / nr,
            "k": k, "n_real": nr, "n_fake": nf}


def sqdist_bound(a, b):
    """[na, nb]: (D + 4) 2^-52 (|a_i|^2 + |b_j|^2) -- the dot-product bound gamma_D ~ D 2^-53 on the two norms and the product with
    (|x| + |y|)^2 <= 2 (|x|^2 + |y|^2), plus three roundings"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return (a.shape[1] + 4) * 2.0 ** -52 * ((a * a).sum(-1)[:, None] + (b * b).sum(-1)[None, :])


def margin64(real, fake, k):
    """(the smallest |d2 - r| over every comparison the metric makes, the smallest gap between the k-th and (k + 1)-th neighbour
    value of a row; inf where a bank has only k + 1 rows and no (k + 1)-th neighbour).  The comparisons: d2(R_i, F_j) against rR[i]
    and against rF[j], and min_j d2(R_i, F_j) against rR[i] (which is among the first)."""
    p = parts64(real, fake, k)
    m = min(np.abs(p["dRF"] - p["rR"][:, None]).min(), np.abs(p["dRF"] - p["rF"][None, :]).min())
    gap = np.inf
    for x in (real, fake):
        d = sqdist64(x, x)
        for i in range(d.shape[0]):
            s = np.sort(np.delete(d[i], i))
            if s.shape[0] > k:
                gap = min(gap, s[k] - s[k - 1])
    return float(m), float(gap)


def max_bound(real, fake):
    """the largest error bound of any squared distance the metric looks at (inside either bank, or across)"""
    return float(max(sqdist_bound(real, real).max(), sqdist_bound(fake, fake).max(), sqdist_bound(real, fake).max()))


def integer_bank(n, D, seed, dup=True):
    """values in -3 .. 3 as float32: many exact ties, and (``dup``) rows duplicated elsewhere in the bank"""
    rng = np.random.default_rng(seed)
    x = rng.integers(-3, 4, (n, D)).astype(np.float32)
    if dup and n >= 4:
        x[n - 1] = x[0]
        x[n // 2] = x[1]
    return x


def gaussian_bank(n, D, seed, shift=0.0, scale=1.0):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, D)) * scale + shift).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------ case tables
# (nr, nf, D, k): nr, nf from {k + 1, 17, 63, 64, 65, 129} in mixed pairs, D from {1, 3, 4, 5, 17, 64}, k from {1, 3, 5, 16}; every
# case runs with slab_rows 64 (129 crosses a slab, 64 | 65 sit at its edge) and 4096
SLAB_ROWS = [64, 4096]
CASES = [
    (2, 17, 3, 1), (17, 2, 1, 1), (64, 65, 4, 1),
    (4, 63, 5, 3), (65, 64, 17, 3), (129, 17, 1, 3),
    (6, 129, 64, 5), (63, 65, 3, 5), (129, 64, 17, 5), (17, 6, 4, 5),
    (17, 129, 5, 16), (129, 65, 64, 16), (64, 17, 1, 16),
]
# the Gaussian banks of a case: seeds and the fake bank's offset and spread (so that none of the four numbers is trivially 0 or 1
# everywhere)
GAUSS_SEEDS = {c: (100 + 2 * i, 101 + 2 * i) for i, c in enumerate(CASES)}


def case_id(c):
    return "nr%d-nf%d-D%d-k%d" % c


def gaussian_case(c):
    nr, nf, D, k = c
    sr, sf = GAUSS_SEEDS[c]
    return gaussian_bank(nr, D, sr), gaussian_bank(nf, D, sf, shift=0.3, scale=1.2)


def integer_case(c):
    nr, nf, D, k = c
    return integer_bank(nr, D, 7 * nr + D), integer_bank(nf, D, 11 * nf + D + 1)
