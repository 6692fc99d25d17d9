"""GPU: the shared gradient coalesce (csrc/mf_coalesce.h, mf_coalesce.hip: radix sort, run heads, fan-out-32 tree of run
sums) on its own, over its whole domain, driven through ``mf_pool_backward`` by the C ABI so that the test owns every buffer.

Every call gets ``out_ids`` prefilled with a sentinel, ``out_grad`` with NaN, the workspace with 0xFF bytes (a read of
something the call never wrote shows up as NaN or -1), gradient rows of invalid explicit ids filled with NaN, and VALID ids
in the gaps between the owners' lists.  Reference: ``tests/_coalesce_cases.reference`` (plain torch, fp64, written from the
header comment of include/mf_hip.h).  Checked on every case: ids (exact, ascending, then -1, no sentinel left); rows of -1
slots still NaN, no NaN in the others.  Exact cases (small integers times 1, 1/2, 1/4; every fp32 partial sum exact in any
order): ``torch.equal``.  Float cases (standard normal): ``|got - want| <= gamma_L * sum|g|`` per element with
``gamma_L = (L-1)u / (1 - (L-1)u)``, u = 2^-24, L the run's length -- the bound of an fp32 sum in any order, derived, no
margin -- and two calls bit-identical.  Host bound: the same case with n_entries exact, +1, +4095, x3 is bit-identical.

Which family of ``_coalesce_cases.specs()`` covers which row of the plan (p1 / p2 / p3 = tables of 255 / 257 / 65,537
rows: one, two, three radix passes):

  d                 every family at d = 32, 64, 128, 256; giant at d = 32 (p3) and d = 256 (p2)
  n_rows -> passes  tables: n_rows = 2, 255 | 256, 257, 65,535 | 65,536, 65,537, 2^20 at every d, with runs on ids 0
                    (extras only), 1, 2 (bottom digit only), 1 + 256^(passes-1) (top digit only), n_rows - 1
  entry count n     counts: n = 1, 2, 255, 256, 257, 4095, 4096, 4097, 8192, 3*4096+1, 64*4096-1, 64*4096, 64*4096+1
                    (padding included), each under p1, p2, p3 and at d = 32 and 256; the last is the scan's second sweep
  run length L      boundaries (exact) and float: L = 1, 2, 3, 4, 5, 31, 32, 33, 1023, 1024, 1025 (float-long and
  head position     boundaries: ... 32,767, 32,768, 32,769), each with head = 0, 1, 31 (mod 32) and 1023 (mod 1024); runs
                    ending exactly on a 32 / 1024 / 32,768 boundary; runs whose head is a block start (one block exactly,
                    one block + 1); runs across a 4096 tile edge; first run at position 0; the last run ending at n - 1
                    (no padding) or followed directly by padding keys -- under p1, p2, p3 x every d
  top level         giant: one run of 2^20 + 4097 + p entries between short runs (the level with unit 2^20 has work)
  saturation        saturated: every id of a 255- and a 257-row table, n >= n_rows: U == capacity, no -1
  nothing valid     nothing: padding only -- extras only, pooled only (extra_* null, n_extra = 0), both
  owners, mode      owners: B = 1 / one entry per owner / 0, 1, many with empty owners at the front, middle and end, each
                    under mode 0 (count in {1, 2, 4}) and mode 1 (hand-made arg, -1 for owners without a valid entry);
                    the other families alternate modes and owner shapes
"""
from __future__ import annotations

import pytest
import torch

from tests import _coalesce_cases as cc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -7
EXACT = [s for s in cc.specs() if s.values == "exact"]
FLOAT = [s for s in cc.specs() if s.values == "float"]


def _call(mf, t, slack=0):
    """One mf_pool_backward with the host bound n_entries = exact count + slack; returns (out_ids, out_grad)."""
    lib = mf._lib.lib()
    n_rows, d, n_extra = t["n_rows"], t["d"], t["n_extra"]
    n_entries = t["n_entries"] + slack
    cap = min(n_rows, n_extra + n_entries)
    out_ids = torch.full((cap,), SENTINEL, dtype=torch.int64, device=DEV)
    out_grad = torch.full((cap, d), float("nan"), dtype=torch.float32, device=DEV)
    ws = torch.full((max(int(lib.mf_pool_backward_ws_bytes(n_extra, n_entries, d)), 256),), 0xFF, dtype=torch.uint8, device=DEV)
    ptr = mf._lib.ptr
    mf._lib.check(lib.mf_pool_backward(n_rows, d, t["mode"], t["items"].data_ptr(), t["B"], t["lo"].data_ptr(), t["ent_off"].data_ptr(),
                                       t["count"].data_ptr(), ptr(t["arg"]), t["grad_p"].data_ptr(), n_entries, ptr(t["extra_ids"]),
                                       ptr(t["extra_grad"]), n_extra, cap, out_ids.data_ptr(), out_grad.data_ptr(), ws.data_ptr(),
                                       ws.numel(), mf._lib.stream_ptr()))
    torch.cuda.synchronize()
    return out_ids, out_grad


def _where(spec, slot):
    """The run of output slot `slot`: what to look at when a case fails."""
    if slot >= len(spec.layout):
        return f"slot {slot} (past the {len(spec.layout)} runs)"
    return f"slot {slot}: id {spec.layout[slot][0]}, head at sorted position {int(spec.heads[slot])}, length {spec.layout[slot][1]}"


def _check_ids_and_untouched(spec, out_ids, out_grad, uniq):
    n_u = len(uniq)
    assert [i for i, _ in spec.layout] == uniq.tolist()                      # the builder and the reference agree on the case
    got = out_ids[:n_u]
    if not torch.equal(got, uniq):
        bad = int(torch.nonzero(got != uniq)[0])
        raise AssertionError(f"{spec.name}: out_ids differ first at {_where(spec, bad)}: got {int(got[bad])}")
    assert bool((out_ids[n_u:] == -1).all()), (spec.name, "slots past the unique ids must hold -1", out_ids[n_u:][:8].tolist())
    assert not bool((out_ids == SENTINEL).any())
    assert bool(torch.isnan(out_grad[n_u:]).all()), (spec.name, "a row of a -1 slot was written")
    nan_rows = torch.isnan(out_grad[:n_u]).any(1)
    assert not bool(nan_rows.any()), (spec.name, "NaN in", _where(spec, int(torch.nonzero(nan_rows)[0])) if bool(nan_rows.any()) else "")


def _run(mf, spec, slack=0):
    t = cc.torch_inputs(cc.build(spec), DEV)
    assert t["n_extra"] + t["n_entries"] == spec.n
    return t, _call(mf, t, slack)


@pytest.mark.parametrize("spec", EXACT, ids=lambda s: s.name)
def test_exact_sums(mf, spec):
    t, (out_ids, out_grad) = _run(mf, spec)
    uniq, want, _, counts = cc.reference(t)
    assert counts.tolist() == [c for _, c in spec.layout]
    assert 4 * spec.magnitude * spec.longest < cc.EXACT_LIMIT                # every fp32 partial sum is exact
    _check_ids_and_untouched(spec, out_ids, out_grad, uniq)
    got = out_grad[: len(uniq)]
    want32 = want.float()
    assert torch.equal(want32.double(), want)                                # ... and so is the expected row
    if not torch.equal(got, want32):
        bad = int(torch.nonzero((got != want32).any(1))[0])
        ch = int(torch.nonzero(got[bad] != want32[bad])[0])
        raise AssertionError(f"{spec.name}: wrong sum at {_where(spec, bad)}, channel {ch}: got {float(got[bad, ch])}, "
                             f"want {float(want32[bad, ch])}; {int((got != want32).any(1).sum())} rows differ")


@pytest.mark.parametrize("spec", FLOAT, ids=lambda s: s.name)
def test_float_sums_within_the_summation_bound(mf, spec):
    t, (out_ids, out_grad) = _run(mf, spec)
    uniq, want, mass, counts = cc.reference(t)
    _check_ids_and_untouched(spec, out_ids, out_grad, uniq)
    err = (out_grad[: len(uniq)].double() - want).abs()
    bound = cc.gamma(counts)[:, None] * mass
    ratio = float((err / bound.clamp_min(1e-300)).max()) if len(uniq) else 0.0
    print(f"{spec.name}: max |err| {float(err.max()):.3e}, max err / bound {ratio:.3f}")
    over = (err > bound).any(1)
    assert not bool(over.any()), (spec.name, _where(spec, int(torch.nonzero(over)[0])) if bool(over.any()) else "")
    again_ids, again_grad = _call(mf, t)
    assert torch.equal(again_ids, out_ids)
    assert torch.equal(again_grad[: len(uniq)], out_grad[: len(uniq)])        # deterministic (the rest is NaN: never equal)


@pytest.mark.parametrize("name", cc.HOST_BOUND_CASES)
def test_result_does_not_depend_on_the_host_bound(mf, name):
    spec = cc.spec_named(name)
    t = cc.torch_inputs(cc.build(spec), DEV)
    uniq = cc.reference(t)[0]
    n_u = len(uniq)
    base_ids, base_grad = _call(mf, t)
    _check_ids_and_untouched(spec, base_ids, base_grad, uniq)
    for slack in (1, 4095, 2 * t["n_entries"]):                              # the bound: exact + 1, + 4095, x 3
        out_ids, out_grad = _call(mf, t, slack)
        assert len(out_ids) == min(spec.n_rows, spec.n + slack)
        _check_ids_and_untouched(spec, out_ids, out_grad, uniq)
        assert torch.equal(out_ids[:n_u], base_ids[:n_u]), slack
        assert torch.equal(out_grad[:n_u], base_grad[:n_u]), slack
