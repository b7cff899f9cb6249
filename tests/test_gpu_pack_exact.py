"""The device weight packers of csrc/conv_bwd.hip against the layout reference of tests/pack_cases.py (the layout, the case tables and
why every comparison is on raw bits: that module's docstring; tests/test_pack_cases_cpu.py proves the reference against the host
packers, the record geometry and float64 convolutions, that the tables reach the LDS transpose, the nine-float4 path and the generic
loop of the batched kernel, and that the comparison rejects each seeded layout defect).

  pack_weight_kernel        hrv_conv2d_pack_weight_dev_f32 / _bf16 / _pair_dev          every case
  pack_weight_multi_kernel  hrv_conv2d_pack_weight_record + hrv_conv2d_pack_weight_multi  every case alone; every forward and every
                                                                                        data-gradient record in ONE launch each (fixed
                                                                                        shuffled order, fp32 and bf16 mixed); n = 2;
                                                                                        weights at +4 / +8 bytes; T.PackBatch

Every buffer is the test's own, as long as the Python wrappers' bound KH * KW * chunks * rows_pad * bke and pre-filled with a sentinel
(fp32 bits 0x7FC12345, bf16 bits 0x7FC1): the first geom[7] elements must equal the reference (torch.equal on int32 / int16 views),
everything after them -- the unused taps of a stride-2 phase -- and every gap between the buffers of a launch must keep the sentinel.
No tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest
import torch

import pack_cases as P

pytestmark = pytest.mark.gpu
IDS = dict(ids=lambda c: c.name)
GAP = 128                                # int16 elements between two buffers of a launch (and the alignment of each)


def _mods():
    import hr_viton_amd  # noqa: F401
    from hr_viton_amd import _lib, ops
    from hr_viton_amd import train_ops as T
    return _lib, _lib.load(), ops, T


def _stream():
    return torch.cuda.current_stream().cuda_stream


_DEV = {}


def _dev_weights(c, salt=0, shift=0):
    """the case's weights on the device (uploaded once per shape); ``shift``: a contiguous view that many bytes into a larger
    allocation"""
    key = (c.cout, sum(c.src_real), c.k, c.pair_mode != 0, salt, shift)
    if key not in _DEV:
        out = []
        for a in P.case_weights(c, salt):
            if a is None:
                out.append(None)
                continue
            big = torch.zeros(a.size + 4, dtype=torch.float32, device="cuda")
            v = big[shift // 4:shift // 4 + a.size].view(a.shape)
            v.copy_(torch.from_numpy(a.copy()))
            assert v.is_contiguous() and v.data_ptr() % 16 == shift
            out.append(v)
        _DEV[key] = tuple(out)
    return _DEV[key]


def _sigma(c):
    return None if c.sigma is None else torch.tensor([c.sigma], dtype=torch.float32, device="cuda")


def _blank(c):
    """the wrappers' upper bound of elements, every one the sentinel; an int32 / int16 tensor"""
    if c.bf16:
        return torch.full((P.upper_bound_elems(c),), P.SENTINEL16, dtype=torch.int16, device="cuda")
    return torch.full((P.upper_bound_elems(c),), P.SENTINEL32, dtype=torch.int32, device="cuda")


def _want(c, salt=0):
    bits, geom = P.case_ref(c.name, salt)
    return torch.from_numpy(bits.view(np.int16 if c.bf16 else np.int32).copy()), geom


def _check(got, c, what, salt=0):
    """``got``: the whole buffer as integers on the CPU"""
    want, geom = _want(c, salt)
    assert got.dtype == want.dtype and got.numel() == P.upper_bound_elems(c) >= geom[7]
    assert torch.equal(got[:geom[7]], want), f"{what} {c.name}: {int((got[:geom[7]] != want).sum())} of {geom[7]} elements differ"
    tail = got[geom[7]:]
    assert torch.equal(tail, torch.full_like(tail, P.SENTINEL16 if c.bf16 else P.SENTINEL32)), f"{what} {c.name}: written past geom[7]"


def _args(c):
    n = len(c.src_pad)
    return n, (C.c_int32 * n)(*c.src_pad), (C.c_int32 * n)(*c.src_real)


def _single(_lib, lib, c, w, w2, sigma, out_ptr):
    n, srcC, srcR = _args(c)
    geom = (C.c_int32 * 8)()
    if c.pair_mode:
        _lib.check(lib.hrv_conv2d_pack_weight_pair_dev(w.data_ptr(), w2.data_ptr(), c.cout, c.pair_mode, P.virtual_cout(c), c.k, c.k, n,
                                                       srcC, srcR, c.cfg, c.mode, c.pad, 1 if c.bf16 else 0, out_ptr, geom, _stream()),
                   "hrv_conv2d_pack_weight_pair_dev")
    else:
        fn = lib.hrv_conv2d_pack_weight_dev_bf16 if c.bf16 else lib.hrv_conv2d_pack_weight_dev_f32
        _lib.check(fn(w.data_ptr(), c.cout, c.k, c.k, n, srcC, srcR, c.cfg, c.mode, c.stride, c.pad, c.phase[0], c.phase[1], c.wscale,
                      None if sigma is None else sigma.data_ptr(), out_ptr, geom, _stream()), "hrv_conv2d_pack_weight_dev")
    return tuple(geom)


def _record(_lib, lib, c, w, w2, sigma, out_ptr):
    n, srcC, srcR = _args(c)
    rec = C.create_string_buffer(lib.hrv_conv2d_pack_record_bytes())
    geom, blocks = (C.c_int32 * 8)(), C.c_int32(0)
    _lib.check(lib.hrv_conv2d_pack_weight_record(w.data_ptr(), P.virtual_cout(c), c.k, c.k, n, srcC, srcR, c.cfg, c.mode, c.stride, c.pad,
                                                 c.phase[0], c.phase[1], c.wscale, None if sigma is None else sigma.data_ptr(),
                                                 1 if c.bf16 else 0, None if w2 is None else w2.data_ptr(), c.pair_mode,
                                                 c.cout if c.pair_mode else 0, out_ptr, geom, rec, C.byref(blocks)),
               "hrv_conv2d_pack_weight_record")
    assert blocks.value == P.blocks_of(c) and tuple(geom) == P.case_ref(c.name)[1]
    return rec.raw, blocks.value


def _launch(_lib, lib, recs):
    """one hrv_conv2d_pack_weight_multi over ``recs``: [(record, blocks)] in order"""
    tbl = torch.from_numpy(np.frombuffer(b"".join(r for r, _ in recs), dtype=np.uint8).copy()).cuda()
    first = np.zeros(len(recs) + 1, dtype=np.int32)
    first[1:] = np.cumsum([b for _, b in recs])
    first_d = torch.from_numpy(first).cuda()
    _lib.check(lib.hrv_conv2d_pack_weight_multi(tbl.data_ptr(), first_d.data_ptr(), len(recs), int(first[-1]), _stream()),
               "hrv_conv2d_pack_weight_multi")
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------
# 1, 2: every case, the single kernel and the batched kernel with one record
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", P.ALL, **IDS)
def test_single_pack_is_the_reference(c):
    _lib, lib, _, _ = _mods()
    w, w2 = _dev_weights(c)
    buf = _blank(c)
    geom = _single(_lib, lib, c, w, w2, _sigma(c), buf.data_ptr())
    torch.cuda.synchronize()
    assert geom == P.case_ref(c.name)[1]
    _check(buf.cpu(), c, "single")


@pytest.mark.parametrize("c", P.ALL, **IDS)
def test_batched_pack_of_one_record_is_the_reference(c):
    _lib, lib, _, _ = _mods()
    w, w2 = _dev_weights(c)
    buf, sg = _blank(c), _sigma(c)
    _launch(_lib, lib, [_record(_lib, lib, c, w, w2, sg, buf.data_ptr())])
    _check(buf.cpu(), c, "multi")


# ---------------------------------------------------------------------------------------------------------------
# 3: all records of a table in one launch
# ---------------------------------------------------------------------------------------------------------------
def _arena_launch(cases):
    """Every case a slot of one int16 arena, GAP elements apart, all packed by ONE launch in the order given; then every slot is the
    reference, and every tail and every gap still holds the sentinel it was filled with."""
    _lib, lib, _, _ = _mods()
    offs, total = [], GAP
    for c in cases:
        offs.append(total)
        n16 = P.upper_bound_elems(c) * (1 if c.bf16 else 2)
        total += (n16 + GAP + GAP - 1) // GAP * GAP
    host = np.full(total, P.SENTINEL16, dtype=np.uint16)
    for c, o in zip(cases, offs):
        if not c.bf16:
            host[o:o + 2 * P.upper_bound_elems(c)].view(np.uint32)[:] = P.SENTINEL32
    before = host.copy()
    arena = torch.from_numpy(host.view(np.int16)).cuda()
    keep, recs = [], []
    for c, o in zip(cases, offs):
        w, w2 = _dev_weights(c)
        sg = _sigma(c)
        keep.append(sg)
        recs.append(_record(_lib, lib, c, w, w2, sg, arena.data_ptr() + 2 * o))
    _launch(_lib, lib, recs)
    got = arena.cpu()
    untouched = torch.ones(total, dtype=torch.bool)
    for c, o in zip(cases, offs):
        n16 = P.upper_bound_elems(c) * (1 if c.bf16 else 2)
        slot = got[o:o + n16]
        _check(slot if c.bf16 else slot.view(torch.int32), c, f"{len(cases)} records in one launch:")
        untouched[o:o + n16] = False
    assert torch.equal(got[untouched], torch.from_numpy(before.view(np.int16))[untouched]), "a gap between two buffers was written"
    return [b for _, b in recs]


@pytest.mark.parametrize("table", sorted(P.LAUNCH_TABLES))
def test_one_launch_packs_every_record_of_a_table(table):
    blocks = _arena_launch(P.shuffled(P.LAUNCH_TABLES[table]))
    assert blocks == [P.blocks_of(c) for c in P.shuffled(P.LAUNCH_TABLES[table])] and 1 in blocks and max(blocks) >= 16


@pytest.mark.parametrize("table", sorted(P.LAUNCH_TABLES))
def test_one_launch_of_two_records(table):
    big, one = P.two_records(table)
    assert _arena_launch([big, one]) == [P.blocks_of(big), 1]
    assert _arena_launch([one, big]) == [1, P.blocks_of(big)]


# ---------------------------------------------------------------------------------------------------------------
# 4: the address of the weight decides the nine-float4 path
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [c for c in P.FORWARD if c.k == 3], **IDS)
def test_a_shifted_weight_packs_the_same(c):
    _lib, lib, _, _ = _mods()
    for shift in (4, 8):
        w, _ = _dev_weights(c, shift=shift)
        buf = _blank(c)
        _launch(_lib, lib, [_record(_lib, lib, c, w, None, None, buf.data_ptr())])
        _check(buf.cpu(), c, f"multi, weight at +{shift} bytes")
        buf = _blank(c)
        _single(_lib, lib, c, w, None, None, buf.data_ptr())
        torch.cuda.synchronize()
        _check(buf.cpu(), c, f"single, weight at +{shift} bytes")


# ---------------------------------------------------------------------------------------------------------------
# 5: T.PackBatch
# ---------------------------------------------------------------------------------------------------------------
BATCH_CASES = ["fwd-10_6_3-co35-k3-f32c5", "fwd-144-co64-k3-bf16c9", "fwd-96_16_4-co40-k3-f32c0-ws1.0-sg1.7", "pair1-re48-ci32-k3-bf16c9",
               "dg1-ci20-co24-k3p1-f32c5", "dg1-ci116-co40-k3p1-bf16c9", "dg2-ci12-co16-k4p1-ph01-f32c6", "dg2-ci8-co8-k1p0-ph11-bf16c9",
               "pair2-re48-ci32-k3p1-f32c6"]


def _ints(buf):
    return buf.view(torch.int16 if buf.dtype == torch.bfloat16 else torch.int32)


def test_pack_batch_repacks_from_the_current_weights():
    _lib, lib, _, T = _mods()
    cases = [P.BY_NAME[n] for n in BATCH_CASES]
    old = T.PACK_BATCHING[0]
    T.PACK_BATCHING[0] = True
    try:
        batch = T.PackBatch(torch.device("cuda"))
        batch.run()                                              # nothing recorded: this only makes the batch fresh
        assert batch.fresh() and batch.launches == 0
        held = []
        for c in cases:
            w, w2 = (None if a is None else torch.from_numpy(a.copy()).cuda() for a in P.case_weights(c))
            sg = _sigma(c)
            if c.pair_mode:
                buf, geom, cout = T.pack_weight_pair_dev(w, w2, c.pair_mode, list(c.src_pad), list(c.src_real), c.cfg, c.mode, c.pad, c.bf16,
                                                         batch=batch)
                assert cout == P.virtual_cout(c)
            else:
                buf, geom = T.pack_weight_dev(w, list(c.src_pad), list(c.src_real), c.cfg, c.mode, c.stride, c.pad, c.phase, c.wscale, sg,
                                              bf16=c.bf16, batch=batch)
            assert geom == P.case_ref(c.name)[1] and buf is batch.bufs[-1] and buf.numel() == P.upper_bound_elems(c)
            torch.cuda.synchronize()
            want, _ = _want(c)
            assert torch.equal(_ints(buf)[:geom[7]].cpu(), want), c.name     # the recording pack: a batch of this one record
            held.append((w, w2, sg))
        assert len(batch.bufs) == len(cases) and batch.group == [0 if c.mode == 0 else 1 for c in cases] and batch.launches == 0

        def refill():
            for b, c in zip(batch.bufs, cases):
                _ints(b).fill_(P.SENTINEL16 if c.bf16 else P.SENTINEL32)

        for c, (w, w2, _) in zip(cases, held):                  # an optimizer step: new values at the same addresses
            for t, a in zip((w, w2), P.case_weights(c, 1)):
                if t is not None:
                    t.copy_(torch.from_numpy(a.copy()))
        refill()
        batch.run()
        torch.cuda.synchronize()
        assert batch.launches == 2                               # one per group
        for b, c in zip(batch.bufs, cases):
            _check(_ints(b).cpu(), c, "PackBatch.run()", salt=1)
        refill()
        batch.run(backward=False)
        torch.cuda.synchronize()
        assert batch.launches == 3
        for b, c in zip(batch.bufs, cases):
            got = _ints(b).cpu()
            if c.mode == 0:
                _check(got, c, "PackBatch.run(backward=False)", salt=1)
            else:
                assert torch.equal(got, torch.full_like(got, P.SENTINEL16 if c.bf16 else P.SENTINEL32)), c.name
    finally:
        T.PACK_BATCHING[0] = old
