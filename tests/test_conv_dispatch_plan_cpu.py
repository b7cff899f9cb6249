"""The kernel every case of tests/conv_dispatch_cases.py lands on, asked of hr_viton_amd/conv_dispatch.py without a GPU: the plan
functions read only metadata, so ``Act`` views over ``meta`` tensors (the case's shapes, storage types and slice layouts; ``data_ptr()``
answers 0 there, which satisfies the ``% 16`` gates as every real torch allocation does) get the answer the entry points act on.
tests/test_gpu_conv_dispatch.py asserts on the GPU that the plan names the kernel the launch record reports.

The library's host predicates size their tile thresholds by the CU count, which falls back to 256 without a device
(csrc/sample.hip, device_cus): the MI355X's count, and what the table's thresholds were written for.  No device compute is launched."""
import os

import pytest

import conv_dispatch_cases as T


@pytest.fixture(scope="module")
def lib():
    import hr_viton_amd  # noqa: F401
    from hr_viton_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from hr_viton_amd import build
        build.build(verbose=False)
    return _lib.load()


@pytest.mark.parametrize("cid", [c.id for c in T.CASES])
def test_conv_dispatch_plan(cid, lib, monkeypatch):
    from hr_viton_amd import _lib
    c = T.BY_ID[cid]
    for k, v in c.env.items():
        monkeypatch.setenv(k, v)
    _lib.reload_env()
    try:
        kw = T.entry_kwargs(c, T.make_inputs(c), device="meta")
        p = T.plan(c, kw, mb=c.mode != "f32")
    finally:
        monkeypatch.undo()          # (the library caches its switches: the next case starts from the process's own)
        _lib.reload_env()
    assert p.family == c.family, f"{cid}: planned {p.family}, the table expects {c.family}"
    planned = T.planned_launches(c, p, kw)
    for kind, name, count in T.LAUNCHES.get(cid, ()):
        assert planned[(kind, name)] == count, f"{cid}: the plan gives {planned[(kind, name)]} launches of {kind!r} {name!r}, the table {count}"
    if c.entry != "wgrad":
        assert p.out_bf16 == T.output_is_bf16(c), (cid, p.out_bf16)

