"""Cases and float64 restatement of the per-parameter statistics (csrc/span_stats.hip, train_ops.span_stats, optim.Adam.layer_stats).
Pure CPU torch and numpy: tests/test_span_stats_cases_cpu.py holds the restatement against torch.linalg.vector_norm, isfinite
counts and the float64 Adam of tests/guard_cases.py; tests/test_gpu_span_stats.py holds the kernels against the restatement.

The restatement follows the kernels' contract, per span and with x standing for g, w and u:
  non-finite = the exponent field is all ones (tested on the bit pattern); such elements are counted and left out
  sumsq = sum of (double)x^2 over the finite ones            maxabs = max |x| over the finite ones (0 if none)
  g_zeros = elements of g equal to +-0
  u = m / (sqrt(v) / bc2_sqrt + eps), every operation in fp32; an element whose m, v or u is non-finite counts in u_nonfinite"""
import numpy as np
import torch

PIECE = 16384               # elements per piece (hrv_span_stats_piece(); SPAN_PIECE in csrc/span_stats.hip)
BAND = 64                   # NaNs on either side of every buffer
WORDS = 16
EDGE_LENGTHS = [1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, PIECE - 1, PIECE, PIECE + 1, 2 * PIECE + 3]
POISONS = {"nan": float("nan"), "pinf": float("inf"), "ninf": float("-inf")}
TABLES = ("edges", "packed", "many", "one")
GAUSS_EPS = 1e-8
GAUSS_BC2_SQRT = float(np.sqrt(np.float32(1.0) - np.float32(0.999) ** np.float32(3)))


def setup_spans(lengths):
    """(offset, length) by optim.Adam._setup's rule: every span starts on a multiple of 4 elements"""
    spans, off = [], 0
    for k in lengths:
        spans.append((off, k))
        off += (k + 3) // 4 * 4
    return spans


def packed_spans(lengths):
    spans, off = [], 0
    for k in lengths:
        spans.append((off, k))
        off += k
    return spans


def table(name):
    """(spans, shift): ``shift`` = 1 views the storage through buf[1:] -- a base that is 4-byte aligned only"""
    if name == "edges":
        return setup_spans(EDGE_LENGTHS), 0
    if name == "packed":
        return packed_spans(EDGE_LENGTHS), 1
    if name == "many":
        return setup_spans([1 + i % 7 for i in range(300)]), 0
    if name == "one":
        return setup_spans([3 * PIECE + 5]), 0
    raise KeyError(name)


def extent(spans):
    return max(off + k for off, k in spans)


def int_data(spans, seed):
    """Per span (g, w, m, v): g, w in {0, +-1, +-2}; v in {1, 4, 16, 64}; m = k sqrt(v) with integer |k| <= 8.  With eps = 0 and
    bc2_sqrt = 1, u = k exactly; every sum of squares is an integer far below 2^53 in any order.  Every g holds a zero."""
    gen = torch.Generator().manual_seed(seed)
    out = []
    for _, k in spans:
        g = torch.randint(-2, 3, (k,), generator=gen).float()
        g[int(torch.randint(0, k, (1,), generator=gen))] = 0.0
        w = torch.randint(-2, 3, (k,), generator=gen).float()
        rv = 2.0 ** torch.randint(0, 4, (k,), generator=gen).float()            # sqrt(v) in {1, 2, 4, 8}
        kk = torch.randint(-8, 9, (k,), generator=gen).float()
        out.append((g, w, kk * rv, rv * rv))
    return out


def gauss_data(spans, seed):
    gen = torch.Generator().manual_seed(seed)
    out = []
    for _, k in spans:
        g, w, m = (torch.randn(k, generator=gen) for _ in range(3))
        out.append((g, w, m, torch.randn(k, generator=gen) ** 2 + 1e-12))
    return out


def lay_out(spans, shift, data):
    """Four storages [g, w, m, v], NaN everywhere except the spans' elements (the bands on both sides AND every gap between
    spans), and the offset of the view's element 0 inside them.  Storages are 16-byte aligned (torch allocations are at least
    64-byte aligned), so the view starts ``shift`` elements past a 16-byte boundary."""
    n = extent(spans)
    bufs = [torch.full((BAND + shift + n + BAND,), float("nan"), dtype=torch.float32) for _ in range(4)]
    for (off, k), arrs in zip(spans, data):
        for buf, a in zip(bufs, arrs):
            buf[BAND + shift + off:BAND + shift + off + k] = a
    return bufs, BAND + shift


def nonfinite(x: torch.Tensor) -> torch.Tensor:
    return (x.contiguous().view(torch.int32) & 0x7f800000) == 0x7f800000


def update_dir(m: torch.Tensor, v: torch.Tensor, bc2_sqrt: float, eps: float) -> torch.Tensor:
    """u in fp32, every operation rounded on its own (tensor operands throughout: no scalar is folded into a reciprocal)"""
    with np.errstate(all="ignore"):
        return m / (v.sqrt() / torch.full_like(v, float(np.float32(bc2_sqrt))) + torch.full_like(v, float(np.float32(eps))))


def _stat(x, bad):
    keep = x[~bad]
    return float((keep.double() ** 2).sum()), float(keep.abs().max()) if keep.numel() else 0.0, int(bad.sum())


def record_ref(g, w, m=None, v=None, bc2_sqrt=1.0, eps=0.0):
    gs, gm, gn = _stat(g, nonfinite(g))
    ws, wm, wn = _stat(w, nonfinite(w))
    us, um, un = 0.0, 0.0, 0
    if m is not None:
        u = update_dir(m, v, bc2_sqrt, eps)
        us, um, un = _stat(u, nonfinite(m) | nonfinite(v) | nonfinite(u))
    return {"g_sumsq": gs, "w_sumsq": ws, "u_sumsq": us, "g_maxabs": gm, "w_maxabs": wm, "u_maxabs": um, "g_nonfinite": gn,
            "w_nonfinite": wn, "u_nonfinite": un, "g_zeros": int((g == 0).sum())}


def records_ref(data, with_mv=True, bc2_sqrt=1.0, eps=0.0):
    return [record_ref(g, w, m if with_mv else None, v if with_mv else None, bc2_sqrt, eps) for g, w, m, v in data]


def pack_records(refs) -> torch.Tensor:
    """the restatement's records as the int32 [n][16] words the library writes (include/hrviton_hip.h)"""
    a = np.zeros((len(refs), WORDS), dtype=np.int32)
    d, f = a.view(np.float64), a.view(np.float32)
    for i, r in enumerate(refs):
        d[i, 0], d[i, 1], d[i, 2] = r["g_sumsq"], r["w_sumsq"], r["u_sumsq"]
        f[i, 6], f[i, 7], f[i, 8] = r["g_maxabs"], r["w_maxabs"], r["u_maxabs"]
        a[i, 9], a[i, 10], a[i, 11], a[i, 12] = r["g_nonfinite"], r["w_nonfinite"], r["u_nonfinite"], r["g_zeros"]
    return torch.from_numpy(a)


def poison_positions(k):
    """first element, last element, last element of a piece, first element of the next piece"""
    pos = {0, k - 1}
    if k > PIECE:
        pos |= {PIECE - 1, PIECE}
    return sorted(pos)


def check_pieces(spans, pieces, span_first, piece=PIECE):
    """train_ops.span_pieces' contract: the pieces tile every span exactly and in order, none crosses a span, none is longer than
    ``piece`` or empty, a span's pieces are consecutive, span_first is consistent"""
    assert len(span_first) == len(spans) + 1 and span_first[0] == 0 and span_first[-1] == len(pieces)
    for s, (off, k) in enumerate(spans):
        a, b = span_first[s], span_first[s + 1]
        assert b > a, (s, "a span without a piece")
        assert b - a == -(-k // piece), (s, "more pieces than needed")
        at = off
        for first, ln in pieces[a:b]:
            assert first == at and 1 <= ln <= piece, (s, first, ln)
            at += ln
        assert at == off + k, (s, "the pieces do not end where the span ends")
