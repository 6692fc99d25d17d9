"""CPU: the plan of tests/test_gpu_coalesce.py holds what it says (tests/_coalesce_cases.py): the reference is pinned to a
brute-force dict, every exact case meets the precondition of exactness, every layout contains the boundary it is named
for, the planned tables give one, two and three radix passes, and the largest case fits a stated memory cap."""
from __future__ import annotations

import collections

import numpy as np
import pytest
import torch

from tests import _coalesce_cases as cc

# The largest allocation of a direct coalesce case (workspace + inputs + outputs + the fp64 reference).  From what the
# C3-size history test (test_backward_zipf_c3_size) already holds on the device at once: ~0.8 M entries x 128 channels in
# fp64 three times over (the gathered rows, the per-entry gradients, one temporary) = 2.5 GB, plus its tables.
MEMORY_CAP = 3 << 30


def _brute(t):
    """The header comment of mf_pool_backward, entry by entry, in Python floats."""
    n_rows, d, n_own = t["n_rows"], t["d"], t["B"]
    sums = collections.defaultdict(lambda: [0.0] * d)
    for q in range(t["n_extra"]):
        i = int(t["extra_ids"][q])
        if 0 <= i < n_rows:
            for ch in range(d):
                sums[i][ch] += float(t["extra_grad"][q, ch])
    for b in range(n_own):
        for j in range(int(t["ent_off"][b + 1] - t["ent_off"][b])):
            i = int(t["items"][int(t["lo"][b]) + j])
            if not 1 <= i < n_rows:
                continue
            for ch in range(d):
                g = float(t["grad_p"][b, ch])
                if t["mode"] == 0:
                    sums[i][ch] += g / int(t["count"][b])
                elif int(t["arg"][b, ch]) == j:
                    sums[i][ch] += g
                else:
                    sums[i][ch] += 0.0
    return dict(sums)


def _hand_case(mode):
    """Three owners (one empty, one behind a gap), padding in both lists, id 0 as an extra and as a pooled padding id."""
    d = 4
    t = {"n_rows": 6, "d": d, "mode": mode, "B": 4, "n_extra": 4,
         "items": torch.tensor([3, 0, 5, 9, 1, 1, 3, -3, 5, 2]),          # owner 0: [3, 0, 5]; gap (9, 1); owner 2: [1, 3, -3, 5]; 2 unused
         "lo": torch.tensor([0, 3, 5, 9]), "ent_off": torch.tensor([0, 3, 3, 7, 7]),
         "count": torch.tensor([2, 1, 4, 1], dtype=torch.int32),
         "grad_p": torch.tensor([[1., 2., 3., 4.], [50., 50., 50., 50.], [8., -4., 12., 16.], [70., 70., 70., 70.]]),
         "arg": torch.tensor([[0, 2, 2, 0], [-1] * 4, [1, 1, 3, 0], [-1] * 4], dtype=torch.int32) if mode else None,
         "extra_ids": torch.tensor([0, 6, 3, -1]),
         "extra_grad": torch.tensor([[.5, .5, .5, .5], [float("nan")] * 4, [1., 1., 1., 1.], [float("nan")] * 4])}
    t["n_entries"] = 7
    return t


def test_reference_on_a_hand_worked_case():
    uniq, want, mass, counts = cc.reference(_hand_case(0))
    assert uniq.tolist() == [0, 1, 3, 5] and counts.tolist() == [1, 1, 3, 2]
    assert want.tolist() == [[.5] * 4, [2., -1., 3., 4.], [3.5, 1., 5.5, 7.], [2.5, 0., 4.5, 6.]]
    assert mass.tolist() == [[.5] * 4, [2., 1., 3., 4.], [3.5, 3., 5.5, 7.], [2.5, 2., 4.5, 6.]]
    uniq, want, _, _ = cc.reference(_hand_case(1))
    assert uniq.tolist() == [0, 1, 3, 5]
    assert want.tolist() == [[.5] * 4, [0., 0., 0., 16.], [10., -3., 1., 5.], [0., 2., 15., 0.]]


@pytest.mark.parametrize("name", ["two-rows-d32", "owners-mixed-m1-p3-d128", "owners-each-m0-p2-d32", "count-257-p2-d32",
                                  "saturated-257-d64", "nothing-both-257-d64", "table-65536-d32"])
def test_reference_matches_a_brute_force_dict(name):
    spec = cc.spec_named(name)
    t = cc.torch_inputs(cc.build(spec), "cpu")
    uniq, want, _, counts = cc.reference(t, chunk=97)                     # (chunk edges inside the extras and the owners)
    brute = _brute(t)
    assert uniq.tolist() == sorted(brute) == [i for i, _ in spec.layout]
    assert counts.tolist() == [c for _, c in spec.layout]
    for k, i in enumerate(uniq.tolist()):
        assert want[k].tolist() == brute[i], (name, i)                    # exact cases: both are exact


def test_hand_cases_agree_with_the_brute_force_dict():
    for mode in (0, 1):
        t = _hand_case(mode)
        uniq, want, _, _ = cc.reference(t)
        brute = _brute(t)
        assert {i: want[k].tolist() for k, i in enumerate(uniq.tolist())} == brute


def test_planned_tables_give_one_two_and_three_passes():
    assert [cc.radix_passes(n) for n in cc.TABLES] == [1, 1, 2, 2, 2, 3, 3, 3]
    assert [cc.radix_passes(n) for n in (1, 127, 128, (1 << 16) - 1, 1 << 16, (1 << 20) - 1)] == [1, 1, 1, 2, 3, 3]
    assert {ps: cc.radix_passes(n) for ps, n in cc.PASS_TABLE.items()} == {1: 1, 2: 2, 3: 3}
    specs = cc.specs()
    for n_rows in cc.TABLES:                                              # every table at every width
        assert {s.d for s in specs if s.n_rows == n_rows and s.family == "tables"} == set(cc.WIDTHS), n_rows
    for family in ("boundaries", "float", "counts", "owners", "giant"):
        assert {s.passes for s in specs if s.family == family} == ({2, 3} if family == "giant" else {1, 2, 3}), family
        assert {32, 256} <= {s.d for s in specs if s.family == family}, family
    for family in ("boundaries", "float", "saturated"):
        for d in cc.WIDTHS:
            assert {s.passes for s in specs if s.family == family and s.d == d} >= ({1, 2} if family == "saturated" else {1, 2, 3})
    for n in cc.ENTRY_COUNTS:                                             # every entry count: three pass counts, d = 32 and 256
        mine = [s for s in specs if s.family == "counts" and s.n == n]
        assert {s.passes for s in mine} == {1, 2, 3} and {32, 256} <= {s.d for s in mine}, n
    for length in cc.LENGTHS:                                             # every run length x head residue: three pass counts, d = 32 and 256
        for r, m in cc.HEADS:
            mine = [s for s in specs if s.values == "exact" and ("head", length, r, m) in s.claims]
            assert {s.passes for s in mine} == {1, 2, 3} and {32, 256} <= {s.d for s in mine}, (length, r, m)
    assert {(s.mode, s.owners) for s in specs if s.family == "owners"} == {(m, o) for m in (0, 1) for o in ("one", "each", "mixed")}
    assert {s.source for s in specs if s.family == "nothing"} == {"extras", "pooled", "both"}
    assert {s.passes for s in specs if ("scan_sweeps", 2) in s.claims} == {1, 2, 3}


@pytest.mark.parametrize("spec", cc.specs(), ids=lambda s: s.name)
def test_layout_holds_what_it_is_named_for(spec):
    ids = [i for i, _ in spec.layout]
    assert ids == sorted(set(ids)) and all(0 <= i < spec.n_rows for i in ids)
    assert all(c > 0 for _, c in spec.layout)
    assert spec.claims, "a case without a stated purpose"
    for claim in spec.claims:
        assert cc.claim_holds(spec, claim), (spec.name, claim)
    assert spec.passes == cc.radix_passes(spec.n_rows)
    if spec.values == "exact":                                            # the precondition of torch.equal on fp32 sums
        assert 4 * spec.magnitude * spec.longest < cc.EXACT_LIMIT and spec.magnitude >= 1
    if spec.n <= 20000:  # noqa: PLR2004  (the built inputs agree with the plan; the large ones are built on the GPU run)
        inp = cc.build(spec)
        assert inp["n_extra"] + inp["n_entries"] == spec.n
        assert (inp["extra_ids"] is None) == (spec.source == "pooled")
        if spec.values == "exact":
            scaled = np.concatenate([inp["grad_p"].ravel() * 4, np.nan_to_num(inp["extra_grad"]).ravel() * 4
                                     if inp["extra_grad"] is not None else np.zeros(0, np.float32)])
            assert np.array_equal(scaled, np.round(scaled)) and float(np.abs(scaled).max(initial=0)) <= 4 * spec.magnitude
        assert set(np.unique(inp["count"]).tolist()) <= {1, 2, 4}
        if spec.owners == "mixed" and inp["n_entries"] > 100:  # noqa: PLR2004
            lengths = np.diff(inp["ent_off"])
            assert (lengths[:3] == 0).all() and (lengths[-3:] == 0).all() and (lengths[3:-3] == 0).any() and (lengths > 1).any()
            assert (inp["lo"][1:] - inp["lo"][:-1] - lengths[:-1]).max() > 0      # gaps between the owners' lists


def test_the_largest_case_fits_the_memory_cap(mf):
    lib = mf._lib.lib()                                                   # (sizes only: no GPU call)
    worst = 0
    for spec in sorted(cc.specs(), key=lambda s: -s.n * s.d)[:3]:           # the workspace and the rows grow with n * d
        inp = cc.build(spec)
        cap = min(spec.n_rows, spec.n)
        ws = lib.mf_pool_backward_ws_bytes(inp["n_extra"], 3 * inp["n_entries"] if spec.name in cc.HOST_BOUND_CASES else inp["n_entries"], spec.d)
        out = cap * (8 + 4 * spec.d)
        ref = 2 * len(spec.layout) * spec.d * 8 + (1 << 16) * spec.d * (4 + 4 + 8 + 8) + spec.n * (8 + 8 + 1 + 8)
        worst = max(worst, int(ws) + cc.input_bytes(inp) + 2 * out + ref)
    assert 0 < worst < MEMORY_CAP, worst
