"""CPU: the plan of tests/test_gpu_update.py holds what it says (tests/_update_cases.py).

The sort regime, the bucket and the sort of the multi-launch path that a case reaches are PLANNED through a Python mirror
of ``fused_bucket_bits`` / ``fused_bucket`` / ``sort_packed_posbits``; nothing observes them on the device.  What ties the
cases to the kernel is checked here: the mirror's constants are read out of csrc/mf_update.h (a retuned kernel fails here
instead of silently missing its edge on the GPU), every case's target bucket holds exactly the planned keys and nothing
else, every named boundary is present in the sorted layout, the bound of exactness holds on the built lists, and the
reference is pinned on a hand-worked case."""
from __future__ import annotations

import pathlib
import re

import numpy as np
import pytest
import torch

from tests import _update_cases as uc

CSRC = pathlib.Path(__file__).resolve().parents[1] / "matrix-factorization-torch_amd" / "csrc"


def _header_int(text: str, pattern: str) -> int:
    found = re.findall(pattern, text)
    assert len(found) == 1, (pattern, found)
    return int(found[0], 0)


def test_the_mirror_has_the_kernels_constants():
    h = (CSRC / "mf_update.h").read_text()
    assert _header_int(h, r"static constexpr int FUSED_MAX_N = (\d+);") == uc.FUSED_MAX_N
    assert _header_int(h, r"static constexpr int FUSED_CAP = (\d+);") == uc.FUSED_CAP
    assert _header_int(h, r"static constexpr int RUN_CHUNK = (\d+);") == uc.RUN_CHUNK
    assert _header_int(h, r"\(unsigned\)id \* (0x[0-9A-Fa-f]+)u\) >> \(32 - bucket_bits\)") == uc.HASH_MULT
    assert _header_int(h, r"#define MF_FUSED_RANK_MAX (\d+)") == uc.FUSED_RANK_MAX
    assert _header_int(h, r"#define MF_FUSED_MAX_BITS (\d+)") == uc.FUSED_MAX_BITS
    assert _header_int(h, r"#define FUSED_NF_ADAM (\d+)") == uc.NF_ADAM
    assert _header_int(h, r"OPT == RowOpt::ADAM \? FUSED_NF_ADAM : (\d+);") == uc.NF_SGD
    # The rules the mirror restates, as literal source lines: a tripwire.  If one of these fails after a mere reformatting,
    # update the string.  If the rule itself changed, re-derive in tests/_update_cases.py: `fused_bucket_bits` (buckets per n),
    # `regime` (rank / bitonic with its padded size / overflow per bucket size), the n at which the multi-launch path starts,
    # and `sort_packed_posbits` (packed or generic sort per (n, n_rows)) -- then PLANNED_REGIME and the cases' sizes.
    assert "while (bits < FUSED_MAX_BITS && (32ll << bits) < n) ++bits;" in h
    assert "if (m <= FUSED_RANK_MAX) {" in h and "} else if (m <= FUSED_CAP) {" in h and "int P = 1024;" in h
    e = (CSRC / "mf_embed.hip").read_text()
    assert "if (n <= FUSED_MAX_N) {" in e
    assert "(((unsigned long long)(id_limit + 1)) << posbits) <= (1ull << 32) ? posbits : -1" in e
    assert "while ((1ll << posbits) < n) ++posbits;" in e


def test_the_mirror_on_known_values():
    assert [uc.fused_bucket_bits(n) for n in (1, 32, 33, 64, 65, 4096, 4097, 8192, 8193, 65536)] == [0, 0, 1, 1, 2, 7, 8, 8, 8, 8]
    assert [uc.regime(m) for m in (1, 512, 513, 1024, 1025, 2048, 2049, 8192, 8193)] == [
        ("rank",), ("rank",), ("bitonic", 1024), ("bitonic", 1024), ("bitonic", 2048), ("bitonic", 2048), ("bitonic", 4096),
        ("bitonic", 8192), ("overflow",)]
    # (unsigned)id * 0x9E3779B1 >> (32 - bits), by hand: id 1 -> 0x9E3779B1 -> top 8 bits 0x9E; id 2 -> 0x3C6EF362 -> 0x3C
    assert uc.fused_bucket([1, 2, 0], 8).tolist() == [0x9E, 0x3C, 0] and uc.fused_bucket([1, 2], 1).tolist() == [1, 0]
    assert uc.fused_bucket([12345, 7], 0).tolist() == [0, 0]
    # the first table for which (n_rows + 1) << 17 > 2^32 is 32,768
    assert (uc.sort_packed_posbits(65537, 32767), uc.sort_packed_posbits(65537, 32768)) == (17, -1)
    assert (uc.sort_packed_posbits(131072, 16383), uc.sort_packed_posbits(131072, 40000)) == (17, -1)
    assert uc.sort_packed_posbits(65536, 65535) == 16 and uc.sort_packed_posbits((1 << 20) + 1, 5) == -1


def test_reference_on_a_hand_worked_case():
    """Three ids (4 repeated three times), -1 and n_rows among them."""
    n_rows = 6
    idx = np.array([4, -1, 0, 4, 6, 5, 4])
    grad = np.array([[1., 10.], [np.nan, np.nan], [2., -20.], [3., 30.], [np.nan, np.nan], [-4., 40.], [5., -50.]], dtype=np.float32)
    uniq, sums = uc.reference(idx, grad, n_rows)
    assert uniq.tolist() == [0, 4, 5] and sums.dtype == torch.int64
    assert sums.tolist() == [[2, -20], [9, -10], [-4, 40]]
    ids, g = uc.presummed(uniq, sums, n_rows)
    assert ids.tolist() == [0, 4, 5] and g.tolist() == [[2., -20.], [9., -10.], [-4., 40.]]
    ids, g = uc.presummed(uniq, sums, n_rows, pad_to=8)
    assert ids.tolist() == [0, 4, 5, -1, -7, 6, 15, -1] and torch.equal(g[:3].to(torch.int64), sums) and bool(torch.isnan(g[3:]).all())


def test_the_plan_covers_every_row_of_the_table():
    specs = uc.specs()
    by = lambda fam: [s for s in specs if s.family == fam]                               # noqa: E731
    for m in uc.BUCKET_SIZES:                                                            # every bucket size at every width
        assert {s.d for s in by("bucket") if ("m", m) in s.claims and len(s.targets) == 1} == set(uc.WIDTHS), m
    assert {s.d for s in by("bucket") if ("m", 9000) in s.claims and ("one_run",) in s.claims} == set(uc.WIDTHS)
    assert {s.d for s in by("bucket") if ("two_overflow",) in s.claims} == set(uc.WIDTHS)
    for n in uc.N_EDGES:
        assert {s.d for s in by("n") if s.n == n} == set(uc.WIDTHS), n
    claims_of = lambda fam, d: {c for s in by(fam) if s.d == d for c in s.claims}         # noqa: E731
    for d in uc.WIDTHS:
        have = claims_of("placement", d)
        want = {("head", length, 0) for length in uc.ROW_LENGTHS} | {("head", length, r) for length in uc.TABLE_LENGTHS for r in uc.TABLE_RESIDUES}
        want |= {("head_at", 1023), ("head_at", 1024), ("across", 1024), ("across", 2048), ("ends_last",), ("chunk_end_is_m",), ("first",)}
        assert want <= have, (d, want - have)
        have = claims_of("ladder", d)
        assert {("ladder", x, extra, r) for x in uc.LADDER_X for extra in (0, 1) for r in (0, 5)} <= have, d
    assert sorted(uc.LADDER_X) == [11, 12, 13, 15, 16, 17, 24, 25, 32, 33]
    for n, n_rows, sort in uc.MULTI:
        mine = [s for s in by("multi") if (s.n, s.n_rows) == (n, n_rows)]
        assert {s.d for s in mine} == set(uc.MULTI_WIDTHS) and all(("sort", sort) in s.claims for s in mine), (n, n_rows)
        for s in mine:
            assert {("head", length, r) for length in uc.TABLE_LENGTHS for r in uc.TABLE_RESIDUES} <= set(s.claims)
            assert {("longest", 9000), ("block",), ("long_ends_last",)} <= set(s.claims)
    assert any(("bad_behind",) in s.claims for s in by("multi")) and any(("no_bad",) in s.claims for s in by("multi"))
    assert {a.d for a, _ in uc.pair_specs()} == set(uc.MULTI_WIDTHS)


@pytest.mark.parametrize("spec", uc.specs() + tuple(s for pair in uc.pair_specs() for s in pair), ids=lambda s: s.name)
def test_case_holds_what_it_is_named_for(spec):
    assert spec.claims, "a case without a stated purpose"
    for claim in spec.claims:
        assert uc.claim_holds(spec, claim), (spec.name, claim)
    assert spec.multi == (spec.n > uc.FUSED_MAX_N) and spec.n_fill >= 0 and spec.d in uc.WIDTHS
    idx = uc.indices(spec)
    assert idx.shape == (spec.n,) and idx.dtype == np.int64
    valid = (idx >= 0) & (idx < spec.n_rows)
    assert int((~valid).sum()) == spec.n_bad
    if spec.n_bad >= 4:                                                      # noqa: PLR2004
        assert {-1, -7, spec.n_rows, spec.n_rows + 9} == set(idx[~valid].tolist())
    # the exactness bound, on the list as built
    mag = uc.magnitude(idx, spec.n_rows)
    longest = int(np.bincount(idx[valid]).max())
    assert mag >= 1 and mag * longest + uc.W0_MAX < uc.EXACT_LIMIT
    for t, (bucket, counts) in enumerate(spec.targets):
        ids = uc.target_ids(spec, t)
        assert len(ids) == len(counts) and (np.diff(ids) > 0).all() and ids[0] >= 0 and ids[-1] < spec.n_rows
        assert all(c > 0 for c in counts)
        if spec.multi:
            # the global sorted order: the valid ids ascending (both sorts put every out-of-range id behind them), run for run
            assert bucket is None and spec.n_fill == 0
            uniq, cnt = np.unique(idx[valid], return_counts=True)
            assert np.array_equal(uniq, ids) and cnt.tolist() == list(counts)
            assert uc.multi_sort(spec.n, spec.n_rows) in ("packed", "generic")
            continue
        # the bucket of the mirror: the target's keys and only they; the runs in the planned order; the regime of its size
        assert 0 <= bucket < (1 << spec.bits)
        occupancy = np.bincount(uc.fused_bucket(idx[valid], spec.bits), minlength=1 << spec.bits)
        m = int(sum(counts))
        assert int(occupancy[bucket]) == m
        mine = idx[valid][uc.fused_bucket(idx[valid], spec.bits) == bucket]
        uniq, cnt = np.unique(mine, return_counts=True)
        assert np.array_equal(uniq, ids) and cnt.tolist() == list(counts)        # no filler id among them
        named = [c for c in spec.claims if c[0] == "regime"]                  # the regime the case names, for the occupancy found
        assert len(named) == 1 and uc.regime(int(occupancy[bucket])) == tuple(named[0][1:]), (spec.name, named, m)
        if spec.n_fill:                                                       # the others are filled: keys below and above the target
            others = np.delete(occupancy, [b for b, _ in spec.targets])
            assert int(others.sum()) == spec.n_fill
            if spec.n_fill >= 100 and 0 < bucket < (1 << spec.bits) - 1:         # noqa: PLR2004
                assert occupancy[:bucket].sum() > 0 and occupancy[bucket + 1:].sum() > 0
    if len(spec.targets) == 2:                                                # noqa: PLR2004  (both overflow; different buckets)
        assert spec.targets[0][0] != spec.targets[1][0]


def test_pair_tables_share_their_ids():
    for a, b in uc.pair_specs():
        assert (a.n, b.n) == (uc.PAIR_N_A, uc.PAIR_N_B) and a.bits == 0 and b.bits == 8 and a.d == b.d          # noqa: PLR2004
        assert uc.regime(sum(b.targets[0][1])) == ("overflow",)
        assert set(uc.target_ids(a).tolist()) <= set(uc.target_ids(b).tolist())


@pytest.mark.parametrize("name", ["n-65-d32", "bucket-33-d256", "bucket-9000-one-run-d32", "placement-B-d64"])
def test_built_values_are_the_exact_integers_of_the_plan(name):
    spec = uc.spec_named(name)
    inp = uc.build(spec)
    bad = (inp["idx"] < 0) | (inp["idx"] >= spec.n_rows)
    assert len(inp["grads"]) == 2 and not np.array_equal(inp["grads"][0][~bad], inp["grads"][1][~bad])
    for g in inp["grads"]:
        assert g.shape == (spec.n, spec.d) and g.dtype == np.float32
        assert np.isnan(g[bad]).all() and np.array_equal(g[~bad], np.round(g[~bad])) and float(np.abs(g[~bad]).max()) <= inp["M"]
        assert len(np.unique(g[~bad][0])) > 1 and (len(g[~bad]) == 1 or not np.array_equal(g[~bad][0], g[~bad][1]))
    w0 = inp["w0"]
    assert w0.shape == (spec.n_rows, spec.d) and np.array_equal(w0, np.round(w0)) and float(np.abs(w0).max()) <= uc.W0_MAX
    assert (np.abs(w0).sum(1) > 0).all()
    uniq, sums = uc.reference(inp["idx"], inp["grads"][0], spec.n_rows)
    assert int(sums.abs().max()) + uc.W0_MAX < uc.EXACT_LIMIT
    # ... and the reference against a loop over the entries
    brute: dict = {}
    for q in np.nonzero(~bad)[0]:
        brute.setdefault(int(inp["idx"][q]), []).append(q)
    assert sorted(brute) == uniq.tolist()
    for i, qs in list(brute.items())[:50]:
        want = [sum(int(inp["grads"][0][q, ch]) for q in qs) for ch in (0, spec.d - 1)]
        k = int(torch.nonzero(uniq == i)[0])
        assert [int(sums[k, 0]), int(sums[k, spec.d - 1])] == want
