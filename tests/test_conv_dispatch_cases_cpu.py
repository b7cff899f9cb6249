"""The dispatcher sweep's case table and error limit, checked without a GPU (tests/conv_dispatch_cases.py): LIMIT_U is pinned to the
float64 reference from both sides, mutations of the reference exceed it, and the table leaves nothing out."""
import pytest
import torch

import conv_dispatch_cases as T


@pytest.fixture(scope="module")
def measured():
    """per case: E / 2^-24 of a strictly sequential fp32 chain (>= 256 sampled elements) and of torch's fp32 CPU convolution (all)"""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    rows = []
    for c in T.CASES:
        d = T.make_inputs(c)
        a, b = T.operands(c, d)
        lin, A = T._lin(c, a, b), T._lin(c, a.abs(), b.abs())
        idx, vals = T.chain_sample(c, d, 256)
        assert len(idx) >= min(256, lin.numel())
        e_chain = float(((torch.from_numpy(vals).double() - lin.flatten()[idx]).abs() / A.flatten()[idx].clamp_min(1e-300)).max()) / T.U
        a32, b32 = T.operands(c, d, dtype=torch.float32)
        e_t32, _ = T.e_units(T._lin(c, a32, b32), lin, A)
        rows.append((c.id, T.k_terms(c), e_chain, e_t32))
    return rows


def test_limit_is_pinned_to_the_reference(measured):
    worst = max(measured, key=lambda r: max(r[2], r[3]))
    w = max(worst[2], worst[3])
    print(f"\nworst reference E = {w:.2f} * 2^-24 ({worst[0]}, K = {worst[1]}; chain {worst[2]:.2f}, torch fp32 {worst[3]:.2f}); "
          f"LIMIT_U = {T.LIMIT_U}")
    for r in sorted(measured, key=lambda r: -max(r[2], r[3]))[:5]:
        print("  %-28s K %7d  chain %.2f  torch-fp32 %.2f" % r)
    assert 4 * w <= T.LIMIT_U <= 16 * w, (w, T.LIMIT_U)
    # the reference's own fp32 evaluations stay inside the limit, the short-K bound included
    for cid, K, e1, e2 in measured:
        assert max(e1, e2) <= min(T.LIMIT_U, 2.0 * K), (cid, K, e1, e2)


# (the bias gradient belongs to conv_wgrad alone: that mutation runs on the weight-gradient case only)
_MUTATION_PAIRS = [(m, cid) for m in T.MUTATIONS for cid in T.MUTATION_CASES
                   if m != "dbias_last_column_missing" or T.BY_ID[cid].entry == "wgrad"]


@pytest.mark.parametrize("mutation,cid", _MUTATION_PAIRS)
def test_mutation_of_the_reference_is_caught(cid, mutation):
    c = T.BY_ID[cid]
    d = T.make_inputs(c)
    K = T.k_terms(c)
    if mutation == "dbias_last_column_missing":
        _, _, ref, A = T.reference(c, d)
        K = c.p["N"] * T.wgrad_out_hw(c.p)[0] * T.wgrad_out_hw(c.p)[1]
    else:
        ref, A = T.reference(c, d)[:2]
    ok, _ = T.excess(ref, ref, A, K)
    x, _ = T.excess(T.mutate(c, d, mutation), ref, A, K)
    print(f"\n{cid}: {mutation}: error / limit = {x:.3g} (caught)" if x > 1 else f"\n{cid}: {mutation}: {x:.3g} NOT caught")
    assert ok == 0.0 and x > 1.0, (cid, mutation, x)


def test_table_hygiene():
    ids = [c.id for c in T.CASES]
    assert len(set(ids)) == len(ids)
    for g in T.GATES:
        sides = {c.side for c in T.CASES if c.gate == g}
        assert {"in", "out"} <= sides, f"gate {g}: inside and outside case needed, has {sides}"
    assert {c.gate for c in T.CASES if c.gate} <= set(T.GATES)
    served = {c.family for c in T.CASES}
    assert len(set(T.FAMILIES)) == len(T.FAMILIES)
    assert set(T.FAMILIES) - served == set(), f"families no case expects: {set(T.FAMILIES) - served}"
    assert served - set(T.FAMILIES) == set(), f"cases expect families that FAMILIES does not list: {served - set(T.FAMILIES)}"
    assert set(T.LAUNCHES) <= set(ids)
    assert {m for m, _ in _MUTATION_PAIRS} == set(T.MUTATIONS) and {T.BY_ID[i].entry for i in T.MUTATION_CASES} == {"fwd", "dgrad", "wgrad"}
    # no two cases alike
    keys = [(c.entry, c.mode, repr(sorted(c.p.items())), repr(sorted(c.env.items()))) for c in T.CASES]
    assert len(set(keys)) == len(keys), [k for k in keys if keys.count(k) > 1]
    # an in / out pair differs in what the gate reads, not in entry point
    for c in T.CASES:
        assert c.side in ("in", "out", "-") and c.mode in ("f32", "mb", "st") and c.entry in ("fwd", "dgrad", "wgrad")
        assert (c.side == "-") == (c.gate == "")
    # zero cases left out: the table has no skip / xfail vocabulary, and every case is in CASES
    assert len(T.CASES) == len(T._FWD) + len(T._DGRAD) + len(T._WGRAD)
    assert not any("skip" in repr(c).lower() or "xfail" in repr(c).lower() for c in T.CASES)
    assert set(T.ACCEPT_THEN_DECLINE) <= set(ids) and set(T.MUTATION_CASES) <= set(ids)
    for name in {e for c in T.CASES for e in c.env}:
        assert name.startswith("HRV_")
