"""GPU: the quantised allow scan (``mf_pq_scan_allow``, csrc/mf_pq_scan.inc) on slices longer than one strip of mask words.  The
kernel holds the words of 64 blocks in a strip (lane = block), asks for the next strip ahead and rotates once ``blk0 - strip0 >=
64``; tests/test_gpu_cell_mask.py never gets there (its longest filtered slice has 33 blocks).  Here: a cell of 129 blocks that
starts at block 1 of the mask (``_cell_mask_spec.long_cell_case``), scanned as one slice (two rotations), as two (64 blocks: none;
65: one) and finer, under masks that tell a strip from its neighbours and masks that leave some waves of a pass without a word
(``MASK_FAMILIES``; tests/test_cell_mask_cpu.py asserts from ``strip_walk`` that they reach what they are chosen for, and that a
kernel which keeps its first strip would see other bits).  Every comparison is an equality, rows as integers and scores as int32
views: against the numpy restatement (tests/_ivf_pq_spec.py, tests/_ivf_spec.py) with every inadmissible row appended to every
query's exclusion list, and against another slicing of the same lists."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from tests import _cell_mask_spec as spec
from tests import _ivf_pq_spec as pq
from tests import _ivf_spec as ivf
from tests.test_gpu_cell_mask import _dev, _ok_of, _same

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K = 20
N, NQ, BASE = sum(spec.LONG_CELL_SIZES), spec.LONG_NQ, spec.LONG_IDX_BASE
GEOMETRIES = [(64, 8), (32, 16), (256, 4)]          # M = 8 in four-byte units, M = 2 on the two-byte path, M = 64
FAMILIES = list(spec.MASK_FAMILIES)
DEPTHS = (1, 80, 256)


# ------------------------------------------------------------------------------------- the references, each once ----
@functools.lru_cache(maxsize=None)
def _user(d):
    """Short seeded lists: rows of the catalog (three of the long cell's last block among them), two entries outside it; the
    last query has none."""
    rng = np.random.default_rng(d)
    _, row_of = spec.long_cell_layout(d)
    last = row_of[129 * 64: 129 * 64 + 38]
    return [[] if i == NQ - 1 else [*(rng.integers(0, N, 12) + BASE).tolist(), *(rng.choice(last, 3, replace=False) + BASE).tolist(), BASE - 1, BASE + N]
            for i in range(NQ)]


def _every(d, family, with_user, nq=NQ):
    return spec.extended_lists(_user(d) if with_user else None, nq, spec.family_ok(family, d), BASE)


def _pair(s, rows):
    return torch.from_numpy(np.ascontiguousarray(s)).to(DEV), torch.from_numpy(np.ascontiguousarray(rows)).to(DEV)


@functools.lru_cache(maxsize=None)
def _wanted(d, dsub, family, r, with_user):
    """The spec's candidates under the family's mask.  Shared and never written."""
    c = spec.long_cell_case(d, dsub)
    return _pair(*pq.candidates(*c._args(), r, 1, _every(d, family, with_user), BASE))


@functools.lru_cache(maxsize=None)
def _wanted_search(d, dsub, family, path, with_user):
    """``path="pq"``: the 80 best candidates refined; ``"cells"``: every admissible probed row scored exactly; ``"ivf"``: the same
    from the exact engines' oracle, for the partitioned index."""
    c = spec.long_cell_case(d, dsub)
    every = _every(d, family, with_user)
    if path == "ivf":
        b = c.base
        return _pair(*ivf.expected(b.q, b.items, b.centroids, b.assign, K, 1, every, BASE))
    return _pair(*pq.search(*c._args(), K, 4 if path == "pq" else None, 1, every, BASE))


@pytest.fixture(scope="module")
def indexes(mf):
    made = {}

    def get(d, dsub):
        if (d, dsub) not in made:
            c = spec.long_cell_case(d, dsub)
            b = c.base
            index = mf.retrieval.QuantizedIndex.from_codebooks(_dev(b.items, torch.float32), _dev(b.centroids, torch.float32), _dev(b.assign),
                                                               _dev(c.books, torch.float32), idx_base=BASE, num_probes=1)
            assert index.max_cell_blocks == 129 and int(index.cell_blk[1]) == 1 and index.num_sub_vectors == d // dsub
            tags = sum(spec.family_ok(f, d).astype(np.int64) << i for i, f in enumerate(FAMILIES))      # bit i: family i admits the row
            index.set_tags(torch.from_numpy(tags))
            made[d, dsub] = index
        return made[d, dsub]

    return get


@pytest.fixture(scope="module")
def partitioned(mf):
    made = {}

    def get(d):
        if d not in made:
            b = spec.long_cell_case(d, 8 if d < 256 else 4).base
            made[d] = mf.retrieval.PartitionedIndex.from_assignment(_dev(b.items, torch.float32), _dev(b.centroids, torch.float32), _dev(b.assign),
                                                                    idx_base=BASE, num_probes=1)
        return made[d]

    return get


def _queries(d, dsub):
    return _dev(spec.long_cell_case(d, dsub).base.q, torch.float32)


def _bool(family, d):
    return _dev(spec.family_ok(family, d).copy(), torch.bool)          # (the shared mask is read-only: a tensor wants its own)


def _poison(index):
    """Whatever the search keeps between calls holds garbage (tests/test_gpu_ivf_pq.py)."""
    for part in (index, index.coarse):
        for ws in part._ws.values():
            ws.fill_(0xA5)


def _largest(mf, r):
    return min(129, mf.retrieval.MERGE_DEEP_MAX_KEYS // r)


# ------------------------------------------------------------------------------- a. candidates against numpy ----
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("d,dsub", GEOMETRIES)
def test_candidates_on_slices_of_more_than_one_strip(mf, indexes, d, dsub, family):
    index, q = indexes(d, dsub), _queries(d, dsub)
    where = _bool(family, d)
    ok = _ok_of(where, None)
    assert np.array_equal(ok, spec.family_ok(family, d)) and 1 <= int(ok.sum()) <= N - 1
    mask = index.cell_mask(where)
    assert torch.equal(mask.words[0].cpu(), torch.from_numpy(spec.words(ok, index.row_of.cpu().numpy())))
    for with_user in (False, True):
        user = _user(d) if with_user else None
        for r in DEPTHS:
            want = _wanted(d, dsub, family, r, with_user)
            for slices in (1, 2, 3, None, _largest(mf, r)):
                got = index.candidates(q, r, exclude=user, slices=slices, allow=mask)
                _same(got, want, (family, r, slices, with_user))
            if d == 64:
                _same(index.candidates(q, r, exclude=_every(d, family, with_user)), want, (family, r, with_user, "the device's unfiltered scan"))
                _same(index.candidates(q, r, exclude=user, allow=mask), index.candidates(q, r, exclude=user, slices=1, allow=mask),
                      (family, r, with_user, "planned against one slice"))
    assert not torch.equal(index.candidates(q, 80, allow=mask)[1], index.candidates(q, 80)[1]), "a mask that is ignored"
    if family == "third_strip":                       # 38 admitted rows in the probed cell: all of them, then the tail
        _, row_of = spec.long_cell_layout(d)
        admitted = torch.from_numpy(np.sort(row_of[129 * 64: 129 * 64 + 38]) + BASE).to(DEV)
        for r in (80, 256):
            scores, rows = index.candidates(q, r, slices=1, allow=mask)
            assert bool((rows[:, 38:] == -1).all()) and bool(torch.isinf(scores[:, 38:]).all()) and bool(torch.isfinite(scores[:, :38]).all())
            assert torch.equal(rows[:, :38].sort(dim=1).values, admitted.expand(NQ, 38))
        assert bool(torch.isin(index.candidates(q, 1, slices=1, allow=mask)[1], admitted).all())


@pytest.mark.parametrize("d,dsub", GEOMETRIES)
def test_candidates_do_not_rely_on_a_cleared_workspace(mf, indexes, d, dsub):
    index, q = indexes(d, dsub), _queries(d, dsub)
    for family in ("alternate_blocks", "third_strip"):
        mask = index.cell_mask(_bool(family, d))
        for r in DEPTHS:
            for slices in (1, 2, None, _largest(mf, r)):
                index.candidates(q, r, exclude=_user(d), slices=slices, allow=mask)          # (the workspace of this call exists)
                _poison(index)
                _same(index.candidates(q, r, exclude=_user(d), slices=slices, allow=mask), _wanted(d, dsub, family, r, True), (family, r, slices))


# ---------------------------------------------------------------------------------------- b. search, both paths ----
@pytest.mark.parametrize("d,dsub", GEOMETRIES)
def test_search_on_both_paths_and_the_partitioned_control(mf, indexes, partitioned, d, dsub):
    """The quantised search (``mf_pq_scan_allow`` + refine), the parent's ``path="cells"`` on the same index, and a
    ``PartitionedIndex`` over the same rows: ``mf_ivf_scan_allow`` reads its words block by block, so it is the control."""
    index, plain, q = indexes(d, dsub), partitioned(d), _queries(d, dsub)
    for i, family in enumerate(FAMILIES):
        where = mf.retrieval.TagFilter(all_of=1 << i) if i % 2 == 0 else _bool(family, d)        # both ways to a mask
        for with_user in (False, True):
            user = _user(d) if with_user else None
            for path in ("pq", "cells"):
                got = index.search(q, K, exclude=user, path=path, allow=where)
                _same(got, _wanted_search(d, dsub, family, path, with_user), (family, path, with_user))
            got = plain.search(q, K, exclude=user, nprobe=1, allow=_bool(family, d))
            _same(got, _wanted_search(d, dsub, family, "ivf", with_user), (family, "partitioned", with_user))


# ------------------------------------------------------------------------------------------ c. per-query masks ----
@pytest.mark.parametrize("d,dsub", GEOMETRIES)
def test_per_query_masks_on_long_slices(mf, indexes, partitioned, d, dsub):
    """Query i reads mask ``allow_of[i]`` at ``m * stride`` words; -1 and 3 name no mask of three: those queries admit nothing."""
    index, plain, q = indexes(d, dsub), partitioned(d), _queries(d, dsub)
    families = ["third_strip", "alternate_blocks", "half"]
    of = [2, 0, 1, -1, 3]
    bools = [_bool(f, d) for f in families]
    masks = index.cell_mask(bools)
    assert masks.num_masks == 3 and masks.words.shape == (3, 134)

    def check(got, want_of, what):
        assert got[0].dtype == torch.float32 and got[1].dtype == torch.int64
        for i in range(3):
            want = want_of(families[of[i]])
            assert got[0].shape == want[0].shape, what
            assert torch.equal(got[0][i].view(torch.int32), want[0][i].view(torch.int32)) and torch.equal(got[1][i], want[1][i]), (what, i)
        for i in (3, 4):
            assert bool((got[1][i] == -1).all()) and bool(torch.isinf(got[0][i]).all()) and bool((got[0][i] < 0).all()), (what, i)

    for allow_of in (_dev(of), torch.tensor(of, dtype=torch.int64)):
        for with_user in (False, True):
            user = _user(d) if with_user else None
            for slices in (1, 2, None):
                got = index.candidates(q, 80, exclude=user, slices=slices, allow=masks, allow_of=allow_of)
                check(got, lambda f: _wanted(d, dsub, f, 80, with_user), ("candidates", slices, with_user))  # noqa: B023
            for path in ("pq", "cells"):
                got = index.search(q, K, exclude=user, path=path, allow=masks, allow_of=allow_of)
                check(got, lambda f: _wanted_search(d, dsub, f, path, with_user), (path, with_user))  # noqa: B023
            got = plain.search(q, K, exclude=user, nprobe=1, allow=plain.cell_mask(bools), allow_of=allow_of)
            check(got, lambda f: _wanted_search(d, dsub, f, "ivf", with_user), ("partitioned", with_user))  # noqa: B023


# ------------------------------------------------------------------- d. the shape that rotates without being told ----
@pytest.mark.parametrize("family", ["not_first_strip", "alternate_blocks"])
def test_a_thousand_queries_scan_the_long_cell_as_one_slice(mf, indexes, family):
    """Q * nprobe = 1024: the plan leaves every probed cell in one slice, and a cell of 129 blocks rotates twice -- nothing is
    forced.  Every 32nd query against numpy; all of them against the same call in four groups of 256, which the plan cuts into
    four slices each (33, 32, 32, 32 blocks: no rotation)."""
    d, dsub = 64, 8
    index, c = indexes(d, dsub), spec.long_cell_case(d, dsub)
    q_np = spec.long_cell_queries(d, 1024)
    q = _dev(q_np, torch.float32)
    assert index.plan(1024, K, 1)["slices"] == 1 and index.plan(256, K, 1)["slices"] == 4
    mask = index.cell_mask(_bool(family, d))
    cand = index.candidates(q, 80, allow=mask)
    found = index.search(q, K, allow=mask)
    b = c.base
    every = _every(d, family, False, 32)
    some = np.ascontiguousarray(q_np[::32])
    _same((cand[0][::32].contiguous(), cand[1][::32].contiguous()), _pair(*pq.candidates(some, b.items, b.centroids, b.assign, c.books, c.codes, 80, 1, every, BASE)),
          "candidates against numpy")
    _same((found[0][::32].contiguous(), found[1][::32].contiguous()), _pair(*pq.search(some, b.items, b.centroids, b.assign, c.books, c.codes, K, 4, 1, every, BASE)),
          "search against numpy")
    groups = [index.candidates(q[a: a + 256], 80, allow=mask) for a in range(0, 1024, 256)]
    _same(cand, (torch.cat([g[0] for g in groups]), torch.cat([g[1] for g in groups])), "candidates in four groups")
    groups = [index.search(q[a: a + 256], K, allow=mask) for a in range(0, 1024, 256)]
    _same(found, (torch.cat([g[0] for g in groups]), torch.cat([g[1] for g in groups])), "search in four groups")
    assert not torch.equal(cand[1], index.candidates(q, 80)[1])


# ------------------------------------------------------------------------------------------------- e. replay ----
def test_mask_build_and_a_rotating_scan_replay_from_one_graph(mf, indexes):
    """As ``test_mask_build_and_search_replay_from_one_graph`` of tests/test_gpu_cell_mask.py for the exact index: the words are
    written and read on the device, so another mask in the same buffer gives the other result on replay -- at one slice, where
    the scan loads strips inside its loop."""
    d, dsub = 64, 8
    index, q = indexes(d, dsub), _queries(d, dsub)
    allow = _bool("half", d).clone()
    second = _bool("not_first_strip", d)
    eager_first = index.candidates(q, 80, slices=1, allow=index.cell_mask(allow, cache=False))       # (also builds the codes and workspaces)
    eager_second = index.candidates(q, 80, slices=1, allow=index.cell_mask(second, cache=False))
    _same(eager_first, _wanted(d, dsub, "half", 80, False))
    _same(eager_second, _wanted(d, dsub, "not_first_strip", 80, False))
    assert not torch.equal(eager_first[1], eager_second[1])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = index.candidates(q, 80, slices=1, allow=index.cell_mask(allow, cache=False))
    allow.copy_(second)
    for t in out:
        t.fill_(0)
    _poison(index)
    graph.replay()
    torch.cuda.synchronize()
    _same(out, eager_second)
