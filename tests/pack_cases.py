"""Bit-exact cases for the device weight packers of csrc/conv_bwd.hip: pack_weight_kernel (hrv_conv2d_pack_weight_dev_f32 / _bf16 /
_pair_dev) and pack_weight_multi_kernel (hrv_conv2d_pack_weight_record + hrv_conv2d_pack_weight_multi: the LDS transpose, the nine-
float4 fast path of pack_col4 and its generic loop).  Shared by tests/test_pack_cases_cpu.py (the reference and the tables, proved
without a GPU) and tests/test_gpu_pack_exact.py (the kernels against this reference).  Needs no GPU and imports nothing of the project.

A pack is data movement, one fp32 multiply and an optional rounding to bf16, so every comparison is on raw bits: no tolerance.

THE LAYOUT (`ref_pack`, written from this description and not from the kernels' index arithmetic)
  packed [KHp * KWp][chunks_total][rows_pad][bke]; bke = 16 (fp32) or tile_row_bytes(cfg) / 2 (bf16); rows_pad = rows rounded up to
  tile_bn(cfg).
  * mode 0 (forward): rows are couts, k runs over the sources; every source is padded to whole chunks of bke and only its real
    channels are filled; the weight's Cin axis is the concatenation of the REAL channel counts.  Taps keep their order.
  * data gradient: rows are cins, k runs over ceil4(Cout) couts in chunks of bke.
      mode 1 flips both tap axes, its pads are K - 1 - pad;
      mode 2 (one phase (a, b) of stride 2) keeps, per axis, the taps k = a + pad - 2 j with 0 <= k < K in increasing j; its pad is
      -jmin; an axis without a valid tap has ONE all-zero tap plane and pad 0.
  * pair mode 1 (forward): virtual cout 64 g + l is gamma[32 g + l] for l < 32 and beta[32 g + l - 32] otherwise; virtual couts whose
    real index is >= rows_each are padding.  pair mode 2 (mode 1): the virtual cout axis is [gamma | beta], each half Cout / 2 wide.
  * an unfilled position holds +0.0 bits; a filled one the fp32 product w * mul with mul = float32(wscale) or the correctly rounded
    fp32 quotient float32(wscale) / sigma (the library is built without fast-math: the device division is IEEE); bf16 is round-to-
    nearest-even on the fp32 bit pattern.
  geom = (KHp, KWp, pad_h, pad_w, rows, rows_pad, chunks_total, elems).

WEIGHTS: a seeded standard normal (full mantissas) with `PLANTED` written to fixed (cout, cin) pairs AT EVERY TAP, so that every
phase that keeps a tap keeps all of them: bf16 ties with an even and with an odd kept mantissa, their negatives, -0.0, and
0x3F7FFFFF, whose rounding carries into the exponent.  No denormals: the project relies on nothing about them.

A stride-2 phase WITHOUT a tap (1x1, pad 0: three of its four phases) has no filled position at all; its whole pack is +0.0 and the
tie assertions of the CPU file state that instead of a tie."""
import zlib
from collections import namedtuple
from functools import lru_cache

import numpy as np

MAX_SRC = 4
MULTI_ELEMS = 1024                  # packed columns per block of the batched kernel
# tile config -> (output-channel tile, bytes per packed row of the bf16 engine); test_pack_cases_cpu.py holds it to the library's
TILE_BN = (128, 96, 96, 32, 64, 32, 64, 128, 128, 64, 128, 256, 128, 128, 128, 128, 128, 128, 64, 64)
TILE_RB = (64,) * 8 + (128,) * 12
SENTINEL32, SENTINEL16 = 0x7FC12345, 0x7FC1
# fp32 bit patterns planted into every weight (see the module docstring)
TIE_EVEN, TIE_ODD, NEG_ZERO, CARRY = 0x3F808000, 0x3F818000, 0x80000000, 0x3F7FFFFF
PLANTED = (TIE_EVEN, TIE_ODD, TIE_EVEN | 0x80000000, TIE_ODD | 0x80000000, NEG_ZERO, CARRY)

DEFECTS = ("noflip", "chunk0_real", "cbase_padded", "interleave0", "split4", "truncate", "negzero_pad", "phase_reversed")

Case = namedtuple("Case", "name table src_pad src_real cout k cfg bf16 mode stride pad phase wscale sigma pair_mode")


def ceil4(c):
    return (c + 3) // 4 * 4


def tile_bke(cfg, bf16):
    return TILE_RB[cfg] // 2 if bf16 else 16


def rne_bf16(bits32):
    """fp32 bit patterns (uint32) -> bf16 bit patterns (uint16), round to nearest, ties to even"""
    b = bits32.astype(np.uint64)
    return (((b + 0x7FFF + ((b >> 16) & 1)) >> 16) & 0xFFFF).astype(np.uint16)


def mul_of(wscale, sigma):
    m = np.float32(wscale)
    return m if sigma is None else np.float32(m / np.float32(sigma))


def is_dyadic(c):
    m = float(mul_of(c.wscale, c.sigma))
    return m > 0 and (np.log2(m) % 1.0) == 0.0


def phase_taps(a, K, pad):
    """one axis of a stride-2 phase -> (weight tap of each packed tap, pad): dX[2 h' + a] = sum_j dY[h' + j] W[a + pad - 2 j]"""
    js = [j for j in range(-8, 9) if 0 <= a + pad - 2 * j < K]
    if not js:
        return [-1], 0
    return [a + pad - 2 * j for j in js], -js[0]


def _virtual_couts(pair_mode, n_w, defect):
    """the cout axis the pack sees -> (which weight: 0 gamma / 1 beta, its cout, is it real), one entry per virtual cout"""
    if pair_mode == 0:
        c = np.arange(n_w)
        return np.zeros(n_w, np.int64), c, np.ones(n_w, bool)
    if pair_mode == 1:
        c = np.arange((n_w + 31) // 32 * 64)
        g, l = c // 64, c % 64
        which = (l >= 32).astype(np.int64)
        idx = 32 * g + np.where(which == 1, l - (0 if defect == "interleave0" else 32), l)
        return which, idx, idx < n_w
    c = np.arange(2 * n_w)
    split = n_w + (4 if defect == "split4" else 0)
    which = (c >= split).astype(np.int64)
    idx = np.where(which == 1, c - split, c)
    return which, idx, idx < n_w


def geometry(src_pad, src_real, cout, KH, KW, cfg, bf16, mode, stride, pad, phase, pair_mode=0, defect=None):
    """everything of the layout that does not depend on the weight values"""
    bke, bn = tile_bke(cfg, bf16), TILE_BN[cfg]
    which, idx, real = _virtual_couts(pair_mode, cout, defect)
    CoutV, cin = len(which), int(sum(src_real))
    g = dict(bke=bke, CoutV=CoutV, cin=cin, which=which, idx=idx, real=real)
    if mode == 0:
        assert 1 <= len(src_pad) <= MAX_SRC and all(p % 4 == 0 and 0 < r <= p for p, r in zip(src_pad, src_real))
        nch = [(p + bke - 1) // bke for p in src_pad]
        chunk0 = [sum(nch[:s]) for s in range(len(nch))]
        base = [sum(src_real[:s]) for s in range(len(nch))]
        if defect == "chunk0_real":         # sources laid down densely: the next one starts where the REAL channels end
            chunk0 = [(b + bke - 1) // bke for b in base]
        if defect == "cbase_padded":
            base = [sum(src_pad[:s]) for s in range(len(nch))]
        g.update(rows=CoutV, chunks=sum(nch), nch=nch, chunk0=chunk0, base=base, kh=list(range(KH)), kw=list(range(KW)),
                 pad_h=pad, pad_w=pad)
    else:
        g.update(rows=cin, chunks=(ceil4(CoutV) + bke - 1) // bke)
        if mode == 1:
            assert stride == 1
            kh, kw = list(range(KH))[::-1], list(range(KW))[::-1]
            if defect == "noflip":
                kh, kw = kh[::-1], kw[::-1]
            g.update(kh=kh, kw=kw, pad_h=KH - 1 - pad, pad_w=KW - 1 - pad)
        else:
            assert stride == 2 and mode == 2
            (kh, ph), (kw, pw) = phase_taps(phase[0], KH, pad), phase_taps(phase[1], KW, pad)
            if defect == "phase_reversed":
                kh, kw = kh[::-1], kw[::-1]
            g.update(kh=kh, kw=kw, pad_h=ph, pad_w=pw)
    g["rows_pad"] = (g["rows"] + bn - 1) // bn * bn
    g["KHp"], g["KWp"] = len(g["kh"]), len(g["kw"])
    g["geom"] = (g["KHp"], g["KWp"], g["pad_h"], g["pad_w"], g["rows"], g["rows_pad"], g["chunks"],
                 g["KHp"] * g["KWp"] * g["chunks"] * g["rows_pad"] * bke)
    return g


def _pack(w, src_pad, src_real, cfg, mode, stride, pad, phase, wscale, sigma, bf16, w2=None, pair_mode=0, defect=None):
    """-> dict(bits: what the buffer holds, flat; geom; filled: the positions a weight lands on; raw32: fp32 products before any
    rounding, same positions)"""
    w = np.ascontiguousarray(np.asarray(w, dtype=np.float32))
    cout, cin_w, KH, KW = w.shape
    g = geometry(src_pad, src_real, cout, KH, KW, cfg, bf16, mode, stride, pad, phase, pair_mode, defect)
    assert cin_w == g["cin"], "the weight's Cin axis is the concatenation of the real channel counts"
    prod = [(w * mul_of(wscale, sigma)).view(np.uint32)]
    if pair_mode:
        w2 = np.ascontiguousarray(np.asarray(w2, dtype=np.float32))
        assert w2.shape == w.shape
        prod.append((w2 * mul_of(wscale, sigma)).view(np.uint32))
    # the virtual weight [CoutV][Cin][KH][KW] as fp32 bit patterns, padding couts zero
    which, idx, real = g["which"], g["idx"], g["real"]
    V = np.zeros((g["CoutV"], cin_w, KH, KW), np.uint32)
    for h, p in enumerate(prod):
        sel = real & (which == h)
        V[sel] = p[idx[sel]]
    bke, rows_pad, chunks, CoutV = g["bke"], g["rows_pad"], g["chunks"], g["CoutV"]
    T = g["KHp"] * g["KWp"]
    out = np.zeros((T, chunks, rows_pad, bke), np.uint32)
    filled = np.zeros((T, chunks, rows_pad, bke), bool)
    if mode == 0:
        for s, r in enumerate(src_real):
            ci = (g["base"][s] + np.arange(r)) % cin_w
            A = np.zeros((T, g["nch"][s] * bke, rows_pad), np.uint32)
            M = np.zeros(A.shape, bool)
            A[:, :r, :CoutV] = V[:, ci].transpose(2, 3, 1, 0).reshape(T, r, CoutV)
            M[:, :r, :CoutV] = real[None, None, :]
            sl = slice(g["chunk0"][s], g["chunk0"][s] + g["nch"][s])
            out[:, sl] = A.reshape(T, g["nch"][s], bke, rows_pad).transpose(0, 1, 3, 2)
            filled[:, sl] = M.reshape(T, g["nch"][s], bke, rows_pad).transpose(0, 1, 3, 2)
    else:
        A = np.zeros((g["KHp"], g["KWp"], chunks * bke, rows_pad), np.uint32)
        M = np.zeros(A.shape, bool)
        for jh, kh in enumerate(g["kh"]):
            for jw, kw in enumerate(g["kw"]):
                if kh >= 0 and kw >= 0:
                    A[jh, jw, :CoutV, :cin_w] = V[:, :, kh, kw]
                    M[jh, jw, :CoutV, :cin_w] = real[:, None]
        out = A.reshape(T, chunks, bke, rows_pad).transpose(0, 1, 3, 2).copy()
        filled = M.reshape(T, chunks, bke, rows_pad).transpose(0, 1, 3, 2).copy()
    raw32 = out.copy()
    if bf16:
        out = (out >> 16).astype(np.uint16) if defect == "truncate" else rne_bf16(out)
    if defect == "negzero_pad":
        out[~filled] = 0x8000 if bf16 else 0x80000000
    return dict(bits=out.reshape(-1), geom=g["geom"], filled=filled.reshape(-1), raw32=raw32.reshape(-1), shape=filled.shape)


def ref_pack(w, src_pad, src_real, cfg, mode, stride, pad, phase, wscale, sigma, bf16, w2=None, pair_mode=0):
    """-> (packed, geom): `packed` flat, geom[7] bit patterns (uint32 of fp32 / uint16 of bf16) in the layout of the docstring"""
    r = _pack(w, src_pad, src_real, cfg, mode, stride, pad, phase, wscale, sigma, bf16, w2, pair_mode)
    return r["bits"], r["geom"]


# ---------------------------------------------------------------------------------------------------------------
# case tables
# ---------------------------------------------------------------------------------------------------------------
def _tname(cfg, bf16):
    return ("bf16" if bf16 else "f32") + f"c{cfg}"


def _fwd(src, cout, k, cfg, bf16, table="forward", wscale=1.0, sigma=None, tag=""):
    name = f"fwd-{'_'.join(map(str, src))}-co{cout}-k{k}-{_tname(cfg, bf16)}{tag}"
    return Case(name, table, tuple(ceil4(c) for c in src), tuple(src), cout, k, cfg, bf16, 0, 1, k // 2, (0, 0), wscale, sigma, 0)


def _dg(cin, cout, k, pad, cfg, bf16, mode=1, phase=(0, 0), table="mode1", wscale=1.0, sigma=None, tag=""):
    ph = f"-ph{phase[0]}{phase[1]}" if mode == 2 else ""
    name = f"dg{mode}-ci{cin}-co{cout}-k{k}p{pad}{ph}-{_tname(cfg, bf16)}{tag}"
    return Case(name, table, (ceil4(cin),), (cin,), cout, k, cfg, bf16, mode, 1 if mode == 1 else 2, pad, tuple(phase), wscale, sigma, 0)


FORWARD_SHAPES = [([96, 16, 4], 40, 3), ([9], 20, 3), ([10, 6, 3], 35, 3), ([80], 13, 1), ([10], 64, 4), ([144], 64, 3),
                  ([4, 4, 4, 4], 8, 3)]
FORWARD_TYPES = [(0, False), (1, False), (5, False), (1, True), (9, True), (11, True)]
MODE1_SHAPES = [(116, 40, 3, 1), (20, 24, 3, 1), (80, 24, 3, 1), (32, 3, 3, 1), (10, 70, 4, 2), (80, 13, 1, 0), (24, 130, 3, 1)]
MODE1_TYPES = [(0, False), (1, False), (5, False), (6, False), (1, True), (9, True)]
MODE2_SHAPES = [(10, 64, 4, 2), (12, 16, 3, 1), (12, 16, 4, 1), (8, 8, 1, 0)]
MODE2_TYPES = [(5, False), (6, False), (9, True)]
PAIR_ROWS = [32, 48, 80]
PAIR_TYPES = [(6, False), (9, True)]
SCALES = [(0.5, 4.0), (0.7, None), (1.0, 1.7)]
SCALE_TYPES = [(0, False), (9, True)]

FORWARD = [_fwd(s, co, k, cfg, b) for s, co, k in FORWARD_SHAPES for cfg, b in FORWARD_TYPES]
MODE1 = [_dg(ci, co, k, p, cfg, b) for ci, co, k, p in MODE1_SHAPES for cfg, b in MODE1_TYPES]
MODE2 = [_dg(ci, co, k, p, cfg, b, 2, (a, bb), "mode2") for ci, co, k, p in MODE2_SHAPES for cfg, b in MODE2_TYPES
         for a in (0, 1) for bb in (0, 1)]
PAIRS = ([Case(f"pair1-re{r}-ci32-k3-{_tname(cfg, b)}", "pairs", (32,), (32,), r, 3, cfg, b, 0, 1, 1, (0, 0), 1.0, None, 1)
          for r in PAIR_ROWS for cfg, b in PAIR_TYPES] +
         [Case(f"pair2-re{r}-ci32-k3p1-{_tname(cfg, b)}", "pairs", (32,), (32,), r, 3, cfg, b, 1, 1, 1, (0, 0), 1.0, None, 2)
          for r in PAIR_ROWS for cfg, b in PAIR_TYPES])
SCALE = ([_fwd([96, 16, 4], 40, 3, cfg, b, "scale", ws, sg, f"-ws{ws}-sg{sg}") for ws, sg in SCALES for cfg, b in SCALE_TYPES] +
         [_dg(116, 40, 3, 1, cfg, b, 1, (0, 0), "scale", ws, sg, f"-ws{ws}-sg{sg}") for ws, sg in SCALES for cfg, b in SCALE_TYPES])
TABLES = dict(forward=FORWARD, mode1=MODE1, mode2=MODE2, pairs=PAIRS, scale=SCALE)
ALL = FORWARD + MODE1 + MODE2 + PAIRS + SCALE
BY_NAME = {c.name: c for c in ALL}
assert len(BY_NAME) == len(ALL) == 42 + 42 + 48 + 12 + 12
# the two record tables of a batched launch, as PackBatch keeps them: forward packs / data-gradient packs
LAUNCH_TABLES = dict(forward=[c for c in ALL if c.mode == 0], dgrad=[c for c in ALL if c.mode != 0])


def shuffled(cases, seed=5):
    """a fixed order that mixes the types and puts one-block records between many-block ones"""
    order = np.random.RandomState(seed).permutation(len(cases))
    return [cases[i] for i in order]


def two_records(table):
    """a launch of n = 2: the largest bf16 record of a launch table and a one-block fp32 record"""
    cases = LAUNCH_TABLES[table]
    big = max((c for c in cases if c.bf16), key=blocks_of)
    one = next(c for c in cases if not c.bf16 and blocks_of(c) == 1)
    return big, one


def _plant(w):
    cout, cin = w.shape[:2]
    assert cout * cin > 7 * len(PLANTED)
    bits = w.view(np.uint32)
    for i, v in enumerate(PLANTED):
        p = 7 * i + 1
        bits[p // cin, p % cin] = v        # every tap of the (cout, cin) pair
    return w


@lru_cache(maxsize=None)
def _weights(cout, cin, k, pair, salt):
    rs = np.random.RandomState(zlib.crc32(f"{cout}/{cin}/{k}/{salt}".encode()) & 0x7FFFFFFF)
    ws = tuple(_plant(rs.standard_normal((cout, cin, k, k)).astype(np.float32)) for _ in range(2 if pair else 1))
    for w in ws:
        w.setflags(write=False)
    return ws


def case_weights(c, salt=0):
    """-> (w, w2 or None): read-only fp32 OIHW arrays; `salt` picks other random values (the planted ones stay)"""
    ws = _weights(c.cout, sum(c.src_real), c.k, c.pair_mode != 0, salt)
    return ws[0], (ws[1] if c.pair_mode else None)


def case_int_weights(c):
    """small integers instead: every product with an integer image and every partial sum is exact in float64"""
    rs = np.random.RandomState(zlib.crc32(c.name.encode()) & 0x7FFFFFFF)
    shape = (c.cout, sum(c.src_real), c.k, c.k)
    ws = [rs.randint(-8, 9, shape).astype(np.float32) for _ in range(2 if c.pair_mode else 1)]
    return ws[0], (ws[1] if c.pair_mode else None)


def case_pack(c, w=None, w2=None, defect=None, wscale=None, sigma="case"):
    if w is None:
        w, w2 = case_weights(c)
    return _pack(w, c.src_pad, c.src_real, c.cfg, c.mode, c.stride, c.pad, c.phase, c.wscale if wscale is None else wscale,
                 c.sigma if sigma == "case" else sigma, c.bf16, w2, c.pair_mode, defect)


@lru_cache(maxsize=None)
def case_ref(name, salt=0):
    """the reference of a case, computed once: (bits, geom); read-only"""
    c = BY_NAME[name]
    w, w2 = case_weights(c, salt)
    bits, geom = ref_pack(w, c.src_pad, c.src_real, c.cfg, c.mode, c.stride, c.pad, c.phase, c.wscale, c.sigma, c.bf16, w2, c.pair_mode)
    bits.setflags(write=False)
    return bits, geom


def case_geometry(c, defect=None):
    return geometry(c.src_pad, c.src_real, c.cout, c.k, c.k, c.cfg, c.bf16, c.mode, c.stride, c.pad, c.phase, c.pair_mode, defect)


def virtual_cout(c):
    """the Cout argument of the C entry points: the virtual cout count of a pair"""
    return case_geometry(c)["CoutV"]


def upper_bound_elems(c):
    """KH * KW * chunks * rows_pad * bke: what the Python wrappers allocate (a stride-2 phase uses fewer taps)"""
    g = case_geometry(c)
    return c.k * c.k * g["chunks"] * g["rows_pad"] * g["bke"]


def blocks_of(c):
    g = case_geometry(c)
    return (g["chunks"] * g["rows_pad"] * g["bke"] + MULTI_ELEMS - 1) // MULTI_ELEMS


def same_bits(got, want):
    """THE comparison: same dtype, same length, every bit pattern equal"""
    got, want = np.asarray(got), np.asarray(want)
    return got.dtype == want.dtype and got.shape == want.shape and bool(np.array_equal(got, want))


def defect_applies(c, defect):
    """does the seeded defect describe another layout for this case?  Decided from the case alone, never from packed bits."""
    g = case_geometry(c)
    if defect == "noflip":
        return c.mode == 1 and c.k > 1
    if defect == "chunk0_real":
        return c.mode == 0 and case_geometry(c, defect)["chunk0"] != g["chunk0"]
    if defect == "cbase_padded":
        return c.mode == 0 and case_geometry(c, defect)["base"] != g["base"]
    if defect == "interleave0":
        return c.pair_mode == 1
    if defect == "split4":
        return c.pair_mode == 2
    if defect == "truncate":
        return c.bf16 and has_tap(c)
    if defect == "negzero_pad":         # any position no weight lands on: padding rows, channels, couts or an absent tap
        return filled_count(c) < g["geom"][7]
    if defect == "phase_reversed":
        return c.mode == 2 and (g["KHp"] > 1 or g["KWp"] > 1)
    raise KeyError(defect)


def has_tap(c):
    g = case_geometry(c)
    return all(k >= 0 for k in g["kh"]) and all(k >= 0 for k in g["kw"])


def filled_count(c):
    """positions a weight lands on: (real couts) x (real cins) x (taps kept)"""
    g = case_geometry(c)
    return int(g["real"].sum()) * sum(c.src_real) * g["KHp"] * g["KWp"] if has_tap(c) else 0


# ---------------------------------------------------------------------------------------------------------------
# which path of pack_weight_multi_kernel a block takes -- used only to prove that the tables reach all three
# ---------------------------------------------------------------------------------------------------------------
def fast_groups(c, offset=0):
    """-> one bool per 4-column group of the case's tap plane: does it take the nine-float4 path (see `multi_path`)"""
    g = case_geometry(c)
    bke, rows_pad = g["bke"], g["rows_pad"]
    i0 = np.arange(0, g["chunks"] * rows_pad * bke, 4)
    if c.mode != 0 or c.k != 3:
        return np.zeros(len(i0), bool)
    k, t = i0 % bke, i0 // bke
    row, chunk = t % rows_pad, t // rows_pad
    src = np.zeros(len(i0), np.int64)
    for s in range(1, len(c.src_real)):
        src[chunk >= g["chunk0"][s]] = s
    chunk0, base, creal = (np.asarray(x)[src] for x in (g["chunk0"], g["base"], c.src_real))
    ch = (chunk - chunk0) * bke + k                          # first of the four channels, within its source
    rowc = np.minimum(row, g["CoutV"] - 1)
    ok = (row < g["rows"]) & g["real"][rowc] & (ch + 3 < creal)
    addr = offset + 4 * 9 * (g["idx"][rowc] * g["cin"] + base + ch)
    return ok & (addr % 16 == 0)


def multi_path(c, offset=0):
    """-> one tuple of path names per block of the case's record: ("lds",), or the sorted subset of ("col4", "col4_fast") that the
    block's 4-column groups take.  ``offset``: assumed byte offset of the weight's base address from a 16-byte boundary (both
    weights of a pair).  The kernel's gates, restated: the LDS transpose serves data-gradient packs of at most nine taps whose
    rows_pad is a multiple of 1024 / bke; a 4-column group takes the nine-float4 path when the pack is a forward 3x3, its four
    channels are real channels of one source and of a real cout, and the address of the first one is a multiple of 16."""
    g = case_geometry(c)
    nblk = blocks_of(c)
    if c.mode != 0 and c.k * c.k <= 9 and g["rows_pad"] % (MULTI_ELEMS // g["bke"]) == 0:
        return [("lds",)] * nblk
    fast = fast_groups(c, offset)
    out = []
    for b in range(nblk):
        f = fast[b * (MULTI_ELEMS // 4):(b + 1) * (MULTI_ELEMS // 4)]
        out.append(tuple(n for n, hit in (("col4", bool((~f).any())), ("col4_fast", bool(f.any()))) if hit))
    return out


# ---------------------------------------------------------------------------------------------------------------
# the convolution a pack stands for (float64), for integer weights
# ---------------------------------------------------------------------------------------------------------------
def engine(values, g, X, Ho, Wo, stride=1):
    """What the convolution engine computes from a pack: `values` the packed numbers (flat), ``g`` its geometry, X [N][H][W][chunks *
    bke] the source with its channels where the pack's k axis expects them.  out[n][ho][wo][row] = sum over taps (jh, jw) and k of
    X[n][ho * stride - pad_h + jh][wo * stride - pad_w + jw][k] * packed[jh * KWp + jw][k / bke][row][k % bke]; float64."""
    KHp, KWp, bke, chunks, rows_pad = g["KHp"], g["KWp"], g["bke"], g["chunks"], g["rows_pad"]
    P = np.asarray(values, np.float64).reshape(KHp * KWp, chunks, rows_pad, bke).transpose(0, 1, 3, 2).reshape(KHp * KWp, chunks * bke,
                                                                                                             rows_pad)
    N, H, W, _ = X.shape
    B = 16                                                   # a zero border wide enough for every pad of the tables
    Xp = np.zeros((N, H + 2 * B, W + 2 * B, X.shape[3]), np.float64)
    Xp[:, B:B + H, B:B + W] = X
    out = np.zeros((N, Ho, Wo, rows_pad), np.float64)
    for jh in range(KHp):
        for jw in range(KWp):
            h0, w0 = B - g["pad_h"] + jh, B - g["pad_w"] + jw
            win = Xp[:, h0:h0 + (Ho - 1) * stride + 1:stride, w0:w0 + (Wo - 1) * stride + 1:stride]
            out += win @ P[jh * KWp + jw]
    return out[..., :g["rows"]]
