"""GPU: the cell scans filtered in place by an allow bitmap (``mf_filter_cell_bits``, ``mf_ivf_scan_allow``, ``mf_pq_scan_allow``;
``PartitionedIndex.cell_mask``, ``search(allow=...)``, ``QuantizedIndex.candidates(allow=...)``).  The words against the numpy
spec (tests/_cell_mask_spec.py); then the sentence that defines the feature, the one the views are held to: a search with
``allow=`` is ``torch.equal``, scores and rows, to the same search on the same index with every inadmissible global row appended
to every query's exclusion list -- for exact scores and for the quantiser's approximate ones."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from tests import _cell_mask_spec as spec

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K = 20
POISON = 0x5A5A5A5A5A5A5A5A


def _dev(a, dtype=torch.int64):
    return torch.as_tensor(np.asarray(a), dtype=dtype).to(DEV)


def _same(got, want, what=None):
    assert got[0].shape == want[0].shape and got[1].dtype == torch.int64
    assert torch.equal(got[0].view(torch.int32), want[0].view(torch.int32)) and torch.equal(got[1], want[1]), what


def _ok_of(where, tags):
    return where.cpu().numpy() if isinstance(where, torch.Tensor) else spec.admits(tags, where.any_of, where.all_of, where.none_of)


# ------------------------------------------------------------------------------------------- mf_filter_cell_bits ----
def _cell_bits(mf, tags, f, row_of):
    lib = mf._lib.lib()
    out = torch.full((row_of.numel() // 64,), POISON, dtype=torch.int64, device=DEV)
    mf._lib.check(lib.mf_filter_cell_bits(tags.data_ptr(), tags.numel(), f[0], f[1], f[2], row_of.data_ptr(), row_of.numel(), out.data_ptr(),
                                          mf._lib.stream_ptr()))
    return out


@pytest.mark.parametrize("n,cells", [(1, 1), (33, 4), (1000, 16), (2500, 16)])
def test_cell_bits_equal_the_spec(mf, n, cells):
    rng = np.random.default_rng(n)
    assign = rng.integers(0, cells, n)
    if n == 1000:
        assign[assign == 3] = 4                                                  # an empty cell
    _, cell_blk, row_of = mf.retrieval.partition_layout(_dev(assign), cells)
    want_blk, want_row_of = spec.layout(assign, cells)
    assert torch.equal(cell_blk.cpu(), torch.from_numpy(want_blk)) and torch.equal(row_of.cpu(), torch.from_numpy(want_row_of))
    assert n != 1000 or int(cell_blk[3]) == int(cell_blk[4])
    pad = torch.from_numpy(spec.words(np.ones(n, bool), want_row_of)).to(DEV)     # the bits of the places that hold a row
    tags = rng.integers(0, 1 << 6, n, dtype=np.int64) | (rng.integers(0, 2, n, dtype=np.int64) << 63)        # bit 63: the sign bit

    def check(words, f):
        got = _cell_bits(mf, _dev(words), f, row_of)
        want = spec.words(spec.admits(words, *f), want_row_of)
        assert torch.equal(got.cpu(), torch.from_numpy(want)), f
        assert bool(((got & ~pad) == 0).all()), "a padding position is never set"
        assert torch.equal(_cell_bits(mf, _dev(words), f, row_of), got)
        return got

    three = (0b000110, 0b000001, 0b100000)
    for f in (three, (0, 0b11, 0), (0b1, 0, 0), (0, 0, 0b1), (0, 1 << 63, 0), (1 << 63, 0, 0b1), (0, 0, 1 << 63)):
        check(tags, f)
    assert torch.equal(check(tags, (0, 0, 0)), pad)                                                     # all rows
    assert torch.equal(check(np.full(n, -1, dtype=np.int64), (2**64 - 1, 2**64 - 1, 0)), pad)           # all rows, every bit asked for
    assert bool((check(tags, (0, 1 << 40, 0)) == 0).all())                                              # no row
    for one in {0, n // 2, n - 1}:                                                                      # exactly one row, as a bool mask
        mask = np.zeros(n, dtype=bool)
        mask[one] = True
        got = check(mask.astype(np.int64), (0, 1, 0))
        at = int(np.flatnonzero(want_row_of == one)[0])
        assert int((got != 0).sum()) == 1 and int(got[at // 64]) == np.uint64(1 << (at % 64)).astype(np.int64)


# ---------------------------------------------------------------------------------------------------- the worlds ----
@functools.lru_cache(maxsize=None)
def _world(d, n, nq, base):
    """Catalog (300 identical rows from row 100 on when it is large enough: ties are decided by the row), queries (query 0 is
    that row), user exclusion lists with rows outside the catalog, and tags."""
    gen = torch.Generator().manual_seed(1000 * d + n + nq)
    items = torch.nn.functional.normalize(torch.randn(n, d, generator=gen), dim=-1)
    if n >= 1000:
        items[100:400] = items[100]
    q = torch.nn.functional.normalize(torch.randn(nq, d, generator=gen), dim=-1)
    q[0] = items[min(100, n - 1)]
    rng = np.random.default_rng(n + nq)
    lists = [[] if i % 5 == 4 else [*(rng.integers(0, n, 12) + base).tolist(), base - 1, base + n] for i in range(nq)]
    tags = rng.integers(0, 1 << 6, n, dtype=np.int64)
    return items.to(DEV), q.to(DEV), lists, tags


def _filters(mf, index, tags, n):
    """(name, filter): tag filters, a mask that empties the cell of row 0 (and keeps half of the rest, so the identical rows lie
    on both sides), a mask of fewer than ``K`` rows."""
    F = mf.retrieval.TagFilter
    rng = np.random.default_rng(n)
    assign = index.assign.cpu().numpy()
    emptied = (assign != assign[0]) & (rng.random(n) < 0.5)
    if not emptied.any():
        emptied[np.flatnonzero(assign != assign[0])[:1]] = True
    few = np.zeros(n, dtype=bool)
    few[rng.choice(n, min(K - 1, n - 1), replace=False)] = True
    return [("half", F(any_of=0b1)), ("three masks", F(any_of=0b000110, all_of=0b000001, none_of=0b100000)),
            ("a cell emptied", torch.from_numpy(emptied).to(DEV)), ("fewer than k", torch.from_numpy(few).to(DEV))]


WORLDS = [(32, 33, 1, 0, 4), (48, 1000, 33, 0, 16), (64, 2500, 70, 40, 16), (128, 1000, 33, 5000, 16), (256, 2500, 1, 0, 16),
          (128, 2500, 33, 0, 16), (48, 33, 70, 7, 4)]


# --------------------------------------------------------------------------------------------- the partitioned index ----
@pytest.mark.parametrize("d,n,nq,base,cells", WORLDS)
def test_partitioned_search_with_a_mask_equals_the_search_with_the_other_rows_excluded(mf, d, n, nq, base, cells):
    items, q, lists, tags = _world(d, n, nq, base)
    index = mf.retrieval.PartitionedIndex.build(items, cells, iters=2, idx_base=base, num_probes=min(8, cells))
    index.set_tags(torch.from_numpy(tags))
    plain = {nprobe: index.search(q, K, nprobe=nprobe) for nprobe in (1, min(8, cells), cells)}
    for what, where in _filters(mf, index, tags, n):
        ok = _ok_of(where, tags)
        assert 1 <= int(ok.sum()) <= n - 1, what
        mask = index.cell_mask(where)
        assert mask.words.shape == (1, index.row_of.numel() // 64) and mask.words.dtype == torch.int64 and mask.row_of is index.row_of
        assert torch.equal(mask.words[0].cpu(), torch.from_numpy(spec.words(ok, index.row_of.cpu().numpy())))
        differs = False
        for nprobe, unfiltered in plain.items():
            for user in (None, lists):
                want = index.search(q, K, exclude=spec.extended_lists(user, nq, ok, base), nprobe=nprobe)
                got = index.search(q, K, exclude=user, nprobe=nprobe, allow=mask)
                _same(got, want, (what, nprobe, user is not None))
                _same(index.search(q, K, exclude=user, nprobe=nprobe, where=where), want, (what, nprobe, "the view"))
                if user is None:
                    differs |= not torch.equal(got[1], unfiltered[1])
        assert differs, "a mask that is ignored gives the unfiltered result"
        _same(index.search(q, K, exclude=lists, nprobe=cells, allow=where), index.search(q, K, exclude=lists, path="exact", where=where), what)
        if what == "fewer than k":
            rows = index.search(q, K, nprobe=cells, allow=where)[1]
            assert bool((rows[:, int(ok.sum()):] == -1).all()) and bool((rows[:, : int(ok.sum())] >= 0).all())
        if what == "a cell emptied":
            assert not ok[index.assign.cpu().numpy() == int(index.assign[0])].any()
    nothing = index.search(q, K, exclude=lists, allow=torch.zeros(n, dtype=torch.bool, device=DEV))
    assert bool((nothing[1] == -1).all()) and bool(torch.isinf(nothing[0]).all()) and bool((nothing[0] < 0).all())
    everything = index.search(q, K, exclude=lists, allow=torch.ones(n, dtype=torch.bool, device=DEV))
    _same(everything, index.search(q, K, exclude=lists))
    # the identical rows were decided by the row: query 0's list starts with the admitted ones, in ascending row order
    if n >= 1000:
        ok = spec.admits(tags, 0b1)
        rows = index.search(q[:1], K, nprobe=cells, allow=mf.retrieval.TagFilter(any_of=0b1))[1][0].cpu().numpy() - base
        same = np.flatnonzero(ok[100:400])[:K] + 100
        assert 0 < int(ok[100:400].sum()) < 300 and np.array_equal(rows[: same.size], same)


def test_the_python_refusals(mf):
    items, q, lists, tags = _world(64, 1000, 33, 0)
    index = mf.retrieval.PartitionedIndex.build(items, 8, iters=1)
    F = mf.retrieval.TagFilter
    with pytest.raises(ValueError, match="set_tags"):
        index.cell_mask(F(any_of=1))
    index.set_tags(torch.from_numpy(tags))
    mask = index.cell_mask(F(any_of=1))
    with pytest.raises(ValueError, match="give one of them"):
        index.search(q, K, allow=mask, where=F(any_of=1))
    for path in ("exact", "auto", "scan", "tiles", "bf16", "deep"):
        with pytest.raises(ValueError, match="no bitmap route"):
            index.search(q, K, allow=mask, path=path)
    three = index.cell_mask([F(any_of=1), F(any_of=2), F(any_of=4)])
    assert three.num_masks == 3
    with pytest.raises(ValueError, match="need allow_of"):
        index.search(q, K, allow=three)
    with pytest.raises(ValueError, match="need allow_of"):
        index.search(q, K, allow=[F(any_of=1), F(any_of=2)])
    for bad in (torch.zeros(32, dtype=torch.int64), torch.zeros(34, dtype=torch.int64), torch.zeros(33, dtype=torch.int32), torch.zeros(33, 1, dtype=torch.int64)):
        with pytest.raises(ValueError, match="allow_of should be"):
            index.search(q, K, allow=three, allow_of=bad)
    with pytest.raises(ValueError, match="it needs one"):
        index.search(q, K, allow_of=torch.zeros(33, dtype=torch.int64))
    for bad in (torch.zeros(999, dtype=torch.bool, device=DEV), torch.zeros(1000, dtype=torch.int64, device=DEV), "comedy", []):
        with pytest.raises(ValueError):
            index.cell_mask(bad)
    other = mf.retrieval.PartitionedIndex.build(items, 8, iters=1)
    with pytest.raises(ValueError, match="another cell layout"):
        other.search(q, K, allow=mask)
    exact = mf.retrieval.ItemIndex(items)
    with pytest.raises(TypeError):
        exact.search(q, K, allow=mask)


# ---------------------------------------------------------------------------------------- the C export, slice by slice ----
def test_the_scan_export_on_one_large_cell(mf):
    """One cell of 1,100 rows (18 blocks) and a filter that admits about half: at S = 1 every wave selects more than once within
    its slice (more than 64 admitted keys waiting); at S = max_cell_blocks every workgroup holds one block."""
    d, n, nq, base = 64, 1100, 5, 30
    gen = torch.Generator().manual_seed(5)
    items = torch.nn.functional.normalize(torch.randn(n, d, generator=gen), dim=-1).to(DEV)
    q = torch.nn.functional.normalize(torch.randn(nq, d, generator=gen), dim=-1).to(DEV)
    index = mf.retrieval.PartitionedIndex.from_assignment(items, items[:1].clone(), torch.zeros(n, dtype=torch.int64, device=DEV), idx_base=base,
                                                          num_probes=1)
    assert index.max_cell_blocks == 18
    rng = np.random.default_rng(0)
    ok = rng.random(n) < 0.5
    assert int(ok.sum()) > 4 * 2 * 64
    mask = index.cell_mask(torch.from_numpy(ok).to(DEV))
    user = [[*(rng.integers(0, n, 9) + base).tolist()] for _ in range(nq)]
    lib = mf._lib.lib()
    probes = torch.zeros(nq, 1, dtype=torch.int64, device=DEV)
    cells, npad = index.cell_blocked(), index.row_of.numel()

    def run(slices, lists, allow):
        off, ids = mf.retrieval._csr(lists, nq, DEV)
        ws = torch.full((slices * nq * K,), -2, dtype=torch.int64, device=DEV)
        head = (q.data_ptr(), nq, cells.data_ptr(), index.cell_blk.data_ptr(), index.row_of.data_ptr(), npad, n, 1, d, index.max_cell_blocks,
                probes.data_ptr(), 1, K, slices, off.data_ptr(), ids.data_ptr(), base)
        if allow:
            mf._lib.check(lib.mf_ivf_scan_allow(*head, mask.words.data_ptr(), 1, None, ws.data_ptr(), ws.numel() * 8, None))
        else:
            mf._lib.check(lib.mf_ivf_scan(*head, ws.data_ptr(), ws.numel() * 8, None))
        scores = torch.empty(nq, K, dtype=torch.float32, device=DEV)
        rows = torch.empty(nq, K, dtype=torch.int64, device=DEV)
        mf._lib.check(lib.mf_topk_merge_packed(ws.data_ptr(), slices, nq, K, scores.data_ptr(), rows.data_ptr(), None))
        return ws, scores, rows

    for slices in (1, index.max_cell_blocks):
        want = run(slices, spec.extended_lists(user, nq, ok, base), False)
        got = run(slices, user, True)
        assert torch.equal(got[0], want[0]), "the partial lists themselves"
        _same(got[1:], want[1:], slices)
        assert not torch.equal(got[2], run(slices, user, False)[2])
    _same(run(1, user, True)[1:], index.search(q, K, exclude=user, allow=mask))


# ------------------------------------------------------------------------------------------------ the quantised index ----
def _quantized(mf, d, m, n, nq, base=0):
    """Seeded random codebooks; at n = 2500 cell 0 holds 2,100 rows (33 blocks: one strip of mask words -- slices of 64, 65 and 129
    blocks are in tests/test_gpu_cell_mask_strips.py) and three small cells follow, else 8 random cells."""
    items, q, lists, tags = _world(d, n, nq, base)
    gen = torch.Generator().manual_seed(d + m)
    if n >= 2500:
        cells = 4
        assign = torch.cat([torch.zeros(2100, dtype=torch.int64), torch.randint(1, 4, (n - 2100,), generator=gen)])
    else:
        cells = 8
        assign = torch.randint(0, cells, (n,), generator=gen)
    index = mf.retrieval.QuantizedIndex.from_codebooks(items, items[:cells].clone(), assign.to(DEV), torch.randn(m, 256, d // m, generator=gen).to(DEV),
                                                       idx_base=base, num_probes=min(cells, 4))
    index.set_tags(torch.from_numpy(tags))
    return index, q, lists, tags


@pytest.mark.parametrize("d,m,n,nq", [(32, 2, 2500, 33), (32, 8, 1000, 1), (64, 8, 2500, 1), (128, 16, 1000, 33), (256, 64, 2500, 33)])
def test_quantised_candidates_and_search_with_a_mask(mf, d, m, n, nq):
    base = 17
    index, q, lists, tags = _quantized(mf, d, m, n, nq, base)
    assert index.num_sub_vectors == m and index.dsub == d // m
    F = mf.retrieval.TagFilter
    rng = np.random.default_rng(d)
    wheres = [("half", F(any_of=0b1)), ("a quarter", torch.from_numpy(rng.random(n) < 0.25).to(DEV)), ("three masks", F(any_of=0b000110, all_of=0b000001, none_of=0b100000))]
    nprobe = index.num_probes
    for what, where in wheres:
        ok = _ok_of(where, tags)
        assert 1 <= int(ok.sum()) <= n - 1
        if n >= 2500 and what == "half":
            # cell 0 at slices=1: the workgroup sorts mid-slice.  Its 33 blocks stay inside the first strip of mask words (64 blocks,
            # from block 0 of the mask): the second strip and the rotation are tests/test_gpu_cell_mask_strips.py's
            assert int(ok[:2100].sum()) > 512
        mask = index.cell_mask(where)
        for user in (None, lists):
            every = spec.extended_lists(user, nq, ok, base)
            for r in (1, 80, 256):
                largest = min(index.max_cell_blocks, mf.retrieval.MERGE_DEEP_MAX_KEYS // (nprobe * r))
                for slices in (1, largest, None):
                    want = index.candidates(q, r, exclude=every, slices=slices)
                    got = index.candidates(q, r, exclude=user, slices=slices, allow=mask)
                    _same(got, want, (what, r, slices, user is not None))
            for path in ("pq", "cells"):
                want = index.search(q, K, exclude=every, path=path)
                got = index.search(q, K, exclude=user, path=path, allow=where)
                _same(got, want, (what, path))
        assert not torch.equal(index.candidates(q, 80, allow=mask)[1], index.candidates(q, 80)[1]), "a mask that is ignored"
    nothing = index.search(q, K, allow=torch.zeros(n, dtype=torch.bool, device=DEV))
    assert bool((nothing[1] == -1).all()) and bool(torch.isinf(nothing[0]).all())
    for path in ("pq", "cells", "exact"):
        with pytest.raises(NotImplementedError, match="QuantizedIndex"):
            index.search(q, K, path=path, where=F(any_of=1))
    with pytest.raises(ValueError, match="no bitmap route"):
        index.search(q, K, path="exact", allow=F(any_of=1))
    with pytest.raises(ValueError, match="give one of them"):
        index.search(q, K, allow=F(any_of=1), where=F(any_of=1))


# ------------------------------------------------------------------------------------------------- per-query masks ----
@pytest.mark.parametrize("kind", ["partitioned", "quantized"])
def test_per_query_masks_equal_the_groups_searched_one_by_one(mf, kind):
    d, n, nq, base = 64, 1000, 33, 11
    F = mf.retrieval.TagFilter
    if kind == "partitioned":
        items, q, lists, tags = _world(d, n, nq, base)
        index = mf.retrieval.PartitionedIndex.build(items, 8, iters=2, idx_base=base, num_probes=3)
        index.set_tags(torch.from_numpy(tags))
        searches = [lambda qs, **kw: index.search(qs, K, **kw)]
    else:
        index, q, lists, tags = _quantized(mf, d, 8, n, nq, base)
        searches = [lambda qs, **kw: index.search(qs, K, **kw), lambda qs, **kw: index.search(qs, K, path="cells", **kw),
                    lambda qs, **kw: index.candidates(qs, 80, **kw)]
    kinds = [F(any_of=0b1), F(all_of=1 << 50), torch.from_numpy(tags % 4 == 2).to(DEV)]          # the second admits nothing
    masks = index.cell_mask(kinds)
    assert masks.num_masks == 3 and bool((masks.words[1] == 0).all())
    of = np.array([(i + i // 5) % 3 for i in range(nq)], dtype=np.int64)
    for search in searches:
        for allow_of in (torch.from_numpy(of), _dev(of)):
            got = search(q, exclude=lists, allow=masks, allow_of=allow_of)
            for f in range(3):
                qs = np.flatnonzero(of == f).tolist()
                want = search(q[qs], exclude=[lists[i] for i in qs], allow=kinds[f])
                _same((got[0][qs], got[1][qs]), want, f)
        _same(search(q, exclude=lists, allow=kinds, allow_of=_dev(of)), got, "a sequence of filters as allow=")
        out = of.copy()
        out[3], out[7] = -1, 3                                                  # outside [0, F): nothing is admitted
        edge = search(q, exclude=lists, allow=masks, allow_of=_dev(out))
        for i in (3, 7):
            assert bool((edge[1][i] == -1).all()) and bool(torch.isinf(edge[0][i]).all())
        keep = [i for i in range(nq) if i not in (3, 7)]
        _same((edge[0][keep], edge[1][keep]), (got[0][keep], got[1][keep]))
        one = search(q, exclude=lists, allow=kinds[0], allow_of=_dev(np.where(np.arange(nq) % 2, 0, -1)))      # F = 1: allow_of is optional
        whole = search(q, exclude=lists, allow=kinds[0])
        assert bool((one[1][0::2] == -1).all()) and torch.equal(one[1][1::2], whole[1][1::2])


# ------------------------------------------------------------------------------------------------------ no host read ----
def test_mask_build_and_search_replay_from_one_graph(mf):
    d, n, nq, base = 128, 2500, 33, 9
    items, q, lists, tags = _world(d, n, nq, base)
    index = mf.retrieval.PartitionedIndex.build(items, 16, iters=2, idx_base=base)
    csr = mf.retrieval._csr(lists, nq, DEV)
    allow = torch.from_numpy(tags % 2 == 1).to(DEV)
    second = torch.from_numpy(tags % 3 == 1).to(DEV)
    eager_first = index.search(q, K, exclude_csr=csr, allow=index.cell_mask(allow, cache=False))       # (also builds the copies and workspaces)
    eager_second = index.search(q, K, exclude_csr=csr, allow=index.cell_mask(second, cache=False))
    assert not torch.equal(eager_first[1], eager_second[1])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                 # nothing is read back: the mask is built and used on the device
        out = index.search(q, K, exclude_csr=csr, allow=index.cell_mask(allow, cache=False))
    allow.copy_(second)
    for t in out:
        t.fill_(0)
    graph.replay()
    torch.cuda.synchronize()
    _same(out, eager_second)


# ------------------------------------------------------------------------------------------- the cache and snapshots ----
def test_the_cache_of_masks_and_a_mask_from_before_a_rebuild(mf):
    items, q, _, tags = _world(64, 1000, 33, 0)
    index = mf.retrieval.PartitionedIndex.build(items, 8, iters=1)
    index.set_tags(torch.from_numpy(tags))
    F = mf.retrieval.TagFilter
    first = index.cell_mask(F(any_of=1))
    assert index.cell_mask(F(any_of=1)) is first and index.cell_mask(F(any_of=1), cache=False) is not first
    assert index.cell_mask(first) is first
    bits = torch.from_numpy(tags % 2 == 1).to(DEV)
    assert index.cell_mask(bits) is not index.cell_mask(bits) and len(index._masks) == 1              # a bool mask is never cached
    assert torch.equal(index.cell_mask(bits).words, first.words)
    index.cell_mask([F(any_of=2), F(any_of=4)])
    assert len(index._masks) == 1                                                                    # nor is a sequence
    view = index.filtered(F(any_of=1))
    before = index.search(q, K, allow=first)
    index.refresh()                                # a view is a copy of rows and goes; a mask depends on tags and cells, and stays
    assert index.cell_mask(F(any_of=1)) is first and index.filtered(F(any_of=1)) is not view
    _same(index.search(q, K, allow=first), before)
    index.set_tags(torch.from_numpy(tags ^ 1))
    assert len(index._masks) == 0 and index.cell_mask(F(any_of=1)) is not first
    assert torch.equal(index.cell_mask(F(any_of=1)).words[0].cpu(), torch.from_numpy(spec.words(tags % 2 == 0, index.row_of.cpu().numpy())))
    stale = index.cell_mask(F(any_of=1))
    index.rebuild()
    assert len(index._masks) == 0 and index.cell_mask(F(any_of=1)) is not stale
    with pytest.raises(ValueError, match="another cell layout"):
        index.search(q, K, allow=stale)
    _same(index.search(q, K, allow=F(any_of=1)), index.search(q, K, where=F(any_of=1)))
