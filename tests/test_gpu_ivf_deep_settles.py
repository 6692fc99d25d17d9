"""GPU: the keeping of the deep cell scan (``mf_ivf_scan_deep`` / ``mf_ivf_scan_deep_allow``, csrc/mf_ivf_deep_scan.inc) -- the
workgroup's buffer, the bound, the count exchange, the settle in its four sort lengths, the capacity rule in its four kept
classes -- where tests/test_gpu_ivf_deep.py drives it in one setting only (one plain kernel, scores ``s * e0``, the row its own
position, no list, two kept classes).  Here: a cell of 13,288 rows of real dot products that starts at block 3 of the mask, its
rows dealt by a permutation, ``idx_base = 30``, three queries in one launch (scores ascending, descending, shuffled along the
cell), a depth per kept class, slicings whose slices are no multiples of four blocks; the allow twin under masks that leave
one, two or all four waves of a pass without a word; exclusion lists that name the best rows, so that a listed key which moved
the bound would cost entries; and a cell of identical rows behind a shuffled ``row_of``, where later passes hold better tied keys.
Every comparison is an equality, rows as integers and scores as int32 views: list by list against numpy's selection over the
chain oracle's scores, merged against the oracle's own top-k (``_ivf_deep_spec.settle_expected``, ``_ivf_spec.expected``).
tests/test_ivf_deep_cpu.py asserts from the walk of the buffer that these inputs settle inside the loop under a live bound, run
every sort length, and tell a mask by row, ties by position, listed keys in the bound and a word past the slice's end from the
right kernel."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from oracle import chain
from tests import _cell_mask_spec as cell_mask_spec
from tests import _filter_spec
from tests import _ivf_deep_spec as deep
from tests import _ivf_spec as spec
from tests.test_gpu_ivf_deep import _poison, _same

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PATH = "cells_deep"
BASE = deep.SETTLE_BASE
N_LONG = deep.settle_rows()
BLOCKS = -(-N_LONG // 64)
NQ = 3
ALLOW_CASES = [(64, m) for m in deep.SETTLE_MASKS] + [(256, "half"), (256, "every other block")]


def _dev(x):
    return torch.from_numpy(np.array(x)).to(DEV)            # (a copy first: the shared inputs are read-only)


# ------------------------------------------------------------------------------------- the references, each once ----
@functools.lru_cache(maxsize=None)
def _wanted(d, k, mask="all", family=None):
    """The oracle's top-k of the long cell alone.  Shared and never written."""
    return deep.settle_expected(d, k, mask, deep.settle_lists(family, d, k, mask) if family else None)


@functools.lru_cache(maxsize=None)
def _wanted_search(d, k, nprobe, mask, family):
    """The spec of the partitioned index: the probes are the oracle's (query 1 probes a short cell at ``nprobe = 1``)."""
    c = deep.settle_catalog(d)
    every = _filter_spec.extended_lists(deep.settle_lists(family, d, k, mask), NQ, deep.settle_ok(mask, d), BASE)
    return spec.expected(c.q, c.items, c.centroids, c.assign, k, nprobe, every, BASE)


def _bounds(s, slices):
    """The positions ``[lo, hi)`` of the cell that slice ``s`` of ``slices`` scans."""
    return min(N_LONG, 64 * (BLOCKS * s // slices)), min(N_LONG, 64 * (BLOCKS * (s + 1) // slices))


# ------------------------------------------------------------------------------------------------- the indexes ----
@pytest.fixture(scope="module")
def indexes(mf):
    made = {}

    def get(d):
        if d not in made:
            c = deep.settle_catalog(d)
            index = mf.retrieval.PartitionedIndex.from_assignment(_dev(c.items), _dev(c.centroids), _dev(c.assign), idx_base=BASE, num_probes=1)
            first = 64 * deep.SETTLE_FIRST_BLOCK
            assert index.cell_blk.cpu().tolist() == [0, 3, 3 + BLOCKS, 5 + BLOCKS] and index.max_cell_blocks == BLOCKS
            assert np.array_equal(index.row_of[first: first + N_LONG].cpu().numpy(), deep.long_rows(d))
            made[d] = index
        return made[d]

    return get


@pytest.fixture(scope="module")
def twins(mf):
    """One cell of identical rows; ``row_of`` is the identity until a test hands the export another."""
    c = deep.tie_catalog()
    index = mf.retrieval.PartitionedIndex.from_assignment(_dev(c.items), _dev(c.centroids), _dev(c.assign), idx_base=BASE, num_probes=1)
    assert torch.equal(index.row_of[:N_LONG].cpu(), torch.arange(N_LONG)) and index.max_cell_blocks == BLOCKS
    return index


def _scan(mf, index, q, k, slices, *, cell=deep.SETTLE_CELL, row_of=None, lists=None, words=None, allow_of=None):
    """One launch of the export with every query's probe set to ``cell``: the workspace ``int64 [slices, Q, k]``, filled with
    -2 before the launch -- every entry has to be written."""
    lib = mf._lib.lib()
    nq, d = q.shape
    row_of = index.row_of if row_of is None else row_of
    assert row_of.numel() == index.row_of.numel() and 1 <= slices <= index.max_cell_blocks and slices * k <= deep.MERGE_KEYS
    probes = torch.full((nq, 1), cell, dtype=torch.int64, device=DEV)
    off, ids = mf.retrieval._csr(None if lists is None else [list(e) for e in lists], nq, DEV)
    ws = torch.full((slices, nq, k), -2, dtype=torch.int64, device=DEV)
    head = (q.data_ptr(), nq, index.cell_blocked().data_ptr(), index.cell_blk.data_ptr(), row_of.data_ptr(), row_of.numel(), index.num_items,
            index.num_partitions, d, index.max_cell_blocks, probes.data_ptr(), 1, k, slices, mf._lib.ptr(off), mf._lib.ptr(ids), BASE)
    if words is None:
        mf._lib.check(lib.mf_ivf_scan_deep(*head, ws.data_ptr(), ws.numel() * 8, None))
    else:
        assert words.dtype == torch.int64 and words.shape[1] == row_of.numel() // 64 and words.is_contiguous()
        of = None if allow_of is None else torch.tensor(allow_of, dtype=torch.int64, device=DEV)
        mf._lib.check(lib.mf_ivf_scan_deep_allow(*head, words.data_ptr(), words.shape[0], mf._lib.ptr(of), ws.data_ptr(), ws.numel() * 8, None))
    torch.cuda.synchronize()
    return ws


def _merge(mf, ws):
    slices, nq, k = ws.shape
    out_s = torch.empty(nq, k, dtype=torch.float32, device=DEV)
    out_r = torch.empty(nq, k, dtype=torch.int64, device=DEV)
    mf._lib.check(mf._lib.lib().mf_topk_merge_packed_deep(ws.data_ptr(), slices, nq, k, out_s.data_ptr(), out_r.data_ptr(), None))
    return out_s, out_r


def _lists_are(ws, scores, rows, admitted, what, queries=None):
    """Every list ``[slice][q]`` is numpy's top-k of the slice's admitted positions (score descending, row ascending) as packed
    entries -- score bits above, GLOBAL row below -- and -1 from there on.  ``scores``, ``admitted``: ``[Q, positions]``;
    ``rows``: the local row per position."""
    slices, nq, k = ws.shape
    got = ws.cpu().numpy()
    assert not (got == -2).any(), (what, "an entry that was never written")
    for s in range(slices):
        lo, hi = _bounds(s, slices)
        for i in range(nq) if queries is None else queries:
            at = deep.best_first(scores[i], rows, admitted[i], lo, hi)[:k]
            mine = got[s, i]
            assert (mine[at.size:] == -1).all(), (what, slices, s, i, "the tail")
            assert np.array_equal(mine[: at.size] & 0xFFFFFFFF, rows[at] + BASE), (what, slices, s, i, "rows")
            assert np.array_equal((mine[: at.size] >> 32).astype(np.uint32), scores[i][at].view(np.uint32)), (what, slices, s, i, "scores")


def _slicings(index, k):
    """One slice, the planned number, three (69, 69 and 70 blocks) and a list per block as far as the merge's keys go."""
    planned = index.plan(NQ, k, 1, PATH)["slices"]
    most = min(BLOCKS, deep.MERGE_KEYS // k)
    assert 3 < planned <= most
    return sorted({1, planned, 3, most})


def _mask_of(index, d, name):
    ok = deep.settle_ok(name, d)
    mask = index.cell_mask(_dev(ok))
    assert np.array_equal(mask.words[0].cpu().numpy(), cell_mask_spec.words(ok, index.row_of.cpu().numpy())), name
    return mask


# ------------------------------------------------------- 1: every kept class, list by list, real dot products ----
@pytest.mark.parametrize("k", deep.SETTLE_DEPTHS)
@pytest.mark.parametrize("d", [64, 256])
def test_every_kept_class_list_by_list(mf, indexes, d, k):
    index, c = indexes(d), deep.settle_catalog(d)
    q = _dev(c.q)
    admitted = deep.settle_admitted(d, "all")
    for slices in _slicings(index, k):
        ws = _scan(mf, index, q, k, slices)
        _lists_are(ws, deep.long_scores(d), deep.long_rows(d), admitted, (d, k))
        _same(_merge(mf, ws), _wanted(d, k), (d, k, slices, "merged"))
    found = index.search(q[[0, 2]], k, nprobe=1, path=PATH)                        # (the two queries that probe the long cell themselves)
    want = _wanted(d, k)
    _same(found, (want[0][[0, 2]], want[1][[0, 2]]), (d, k, "the search"))


# ------------------------------------------------------------------------------ 2: the allow twin, list by list ----
@pytest.mark.parametrize("k", deep.SETTLE_DEPTHS)
@pytest.mark.parametrize("d,mask", ALLOW_CASES)
def test_the_allow_twin_list_by_list(mf, indexes, d, mask, k):
    index, c = indexes(d), deep.settle_catalog(d)
    q = _dev(c.q)
    words = _mask_of(index, d, mask).words
    admitted = deep.settle_admitted(d, mask)
    scores, rows = deep.long_scores(d), deep.long_rows(d)
    for slices in _slicings(index, k):
        ws = _scan(mf, index, q, k, slices, words=words)
        _lists_are(ws, scores, rows, admitted, (d, mask, k))
        _same(_merge(mf, ws), _wanted(d, k, mask), (d, mask, k, slices, "merged"))
        if mask == "all":
            assert torch.equal(ws, _scan(mf, index, q, k, slices)), (k, slices, "all ones against the plain kernel")
        if mask == "none":
            assert bool((ws == -1).all()), (k, slices)
    if mask == "last block only":                                                 # exactly the rows of that block, then the tail
        got = _scan(mf, index, q, k, 1, words=words).cpu().numpy()[0]
        last = np.sort(rows[N_LONG - 40:] + BASE)
        for i in range(NQ):
            assert np.array_equal(np.sort(got[i, :40] & 0xFFFFFFFF), last) and (got[i, 40:] == -1).all(), (k, i)
    found = index.search(q[[0, 2]], k, nprobe=1, path=PATH, allow=_dev(deep.settle_ok(mask, d)))
    want = _wanted(d, k, mask)
    _same(found, (want[0][[0, 2]], want[1][[0, 2]]), (d, mask, k, "the search"))


@pytest.mark.parametrize("k", [100, 1000])
def test_three_masks_in_one_launch(mf, indexes, k):
    """Query 0 reads mask 2, query 1 mask 0, query 2 names mask 7 of three: nothing is admitted for it -- its workgroups still
    take every barrier of every pass, and the launch returns."""
    d = 64
    index, c = indexes(d), deep.settle_catalog(d)
    q = _dev(c.q)
    names = ["half", "late", "one block in five"]
    of = [2, 0, 7]
    three = index.cell_mask([_dev(deep.settle_ok(name, d)) for name in names])
    assert three.num_masks == 3 and three.words.shape == (3, index.row_of.numel() // 64)
    scores, rows = deep.long_scores(d), deep.long_rows(d)
    for slices in (1, index.plan(NQ, k, 1, PATH)["slices"]):
        ws = _scan(mf, index, q, k, slices, words=three.words, allow_of=of)
        assert bool((ws[:, 2] == -1).all()), (k, slices, "a mask number out of range")
        for i in (0, 1):
            name = names[of[i]]
            single = _scan(mf, index, q, k, slices, words=_mask_of(index, d, name).words)
            assert torch.equal(ws[:, i], single[:, i]), (k, slices, i, "against the single-mask launch")
            admitted = deep.settle_admitted(d, name)
            _lists_are(ws, scores, rows, admitted, (k, name), queries=[i])
            merged = _merge(mf, ws)
            want = _wanted(d, k, name)
            _same((merged[0][i], merged[1][i]), (want[0][i], want[1][i]), (k, slices, i, "merged"))


# ------------------------------------------------------------------------- 3: exclusion lists under a live bound ----
@pytest.mark.parametrize("k", [100, 1000])
@pytest.mark.parametrize("mask", ["all", "half"])
@pytest.mark.parametrize("family", deep.SETTLE_LISTS)
def test_exclusion_lists_under_a_live_bound(mf, indexes, family, mask, k):
    """``mask == "all"``: the plain kernel; ``"half"``: the allow kernel.  A listed key beats the bound like any other and is
    looked up only then (``mf_cells_admit``): it must neither wait nor move the bound."""
    d = 64
    index, c = indexes(d), deep.settle_catalog(d)
    q = _dev(c.q)
    lists = [list(e) for e in deep.settle_lists(family, d, k, mask)]
    allow = None if mask == "all" else _mask_of(index, d, mask)
    ws = _scan(mf, index, q, k, 1, lists=lists, words=None if allow is None else allow.words)
    _lists_are(ws, deep.long_scores(d), deep.long_rows(d), deep.settle_admitted(d, mask, lists), (family, mask, k))
    want = _wanted(d, k, mask, family)
    _same(_merge(mf, ws), want, (family, mask, k, "merged"))
    filled = (want[1] >= 0).sum(axis=1).tolist()
    assert filled == ([3] * NQ if family == "all but three" else [k] * NQ)
    csr = mf.retrieval._csr(lists, NQ, DEV)
    for nprobe in (1, 3):                                                         # at 3 the two short cells contribute
        assert index.plan(NQ, k, nprobe, PATH)["slices"] > 1
        want = _wanted_search(d, k, nprobe, mask, family)
        _same(index.search(q, k, exclude=lists, nprobe=nprobe, path=PATH, allow=allow), want, (family, mask, k, nprobe, "exclude="))
        _same(index.search(q, k, exclude_csr=csr, nprobe=nprobe, path=PATH, allow=allow), want, (family, mask, k, nprobe, "exclude_csr="))


# --------------------------------------------------------------------------------- 4: ties under a live bound ----
@pytest.mark.parametrize("k", deep.TIE_DEPTHS)
@pytest.mark.parametrize("mask", ["all", "half"])
def test_ties_under_a_live_bound_break_by_the_global_row(mf, twins, mask, k):
    """Every score is the same; ``row_of`` is shuffled over the positions, so pass after pass brings lower rows -- better keys --
    and the bound moves (through the index a cell is in ascending row order, and it never does).  Each list: the k lowest
    global rows of its slice, ascending.  The mask goes by position: the admitted rows are those AT the admitted positions."""
    c = deep.tie_catalog()
    q = _dev(c.q)
    row_of = deep.tie_row_of()
    admitted = deep.settle_mask(mask)
    words = None if mask == "all" else twins.cell_mask(_dev(admitted)).words     # (the index's row_of is the identity: rows are positions)
    bits = chain.scores(c.q, c.items[:1]).view(np.uint32)[0, 0]
    for slices in (1, 3):
        ws = _scan(mf, twins, q, k, slices, cell=0, row_of=_dev(row_of), words=words)
        got = ws.cpu().numpy()
        for s in range(slices):
            lo, hi = _bounds(s, slices)
            want = np.sort(row_of[lo:hi][admitted[lo:hi]])[:k] + BASE
            assert want.size == k
            assert np.array_equal(got[s, 0] & 0xFFFFFFFF, want), (mask, k, slices, s)
            assert ((got[s, 0] >> 32).astype(np.uint32) == bits).all(), (mask, k, slices, s)
        out_s, out_r = _merge(mf, ws)
        lowest = np.sort(row_of[:N_LONG][admitted])[:k] + BASE
        assert np.array_equal(out_r.cpu().numpy()[0], lowest) and (out_s.cpu().numpy().view(np.uint32) == bits).all(), (mask, k, slices)


# ------------------------------------------------------------------------------------------ 5: poison and replay ----
def test_a_masked_and_listed_search_after_poison_and_from_a_graph(mf, indexes):
    d, k, nprobe = 64, 1000, 3
    index, c = indexes(d), deep.settle_catalog(d)
    q = _dev(c.q)
    lists = [list(e) for e in deep.settle_lists("long and scattered", d, k, "half")]
    want = _wanted_search(d, k, nprobe, "half", "long and scattered")
    allow = _mask_of(index, d, "half")
    csr = mf.retrieval._csr(lists, NQ, DEV)
    eager = index.search(q, k, exclude_csr=csr, nprobe=nprobe, path=PATH, allow=allow)   # (also builds the copies and workspaces)
    _same(eager, want, "eager")
    _poison(index)
    _same(index.search(q, k, exclude_csr=csr, nprobe=nprobe, path=PATH, allow=allow), want, "after poisoning")
    _same(index.search(q, k, exclude=lists, nprobe=nprobe, path=PATH, allow=allow), eager, "a repeat call")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = index.search(q, k, exclude_csr=csr, nprobe=nprobe, path=PATH, allow=allow)
    for _ in range(2):
        out[0].fill_(7.0)
        out[1].fill_(7)
        _poison(index)
        graph.replay()
        torch.cuda.synchronize()
        _same(out, eager, "replay")
        _same(out, want, "replay against the spec")
