"""GPU: filtered retrieval (csrc/mf_filter.hip, ``retrieval.TagFilter`` / ``FilteredView``, ``search(where=...)``).  The four
exports against the numpy spec (tests/_filter_spec.py), integers compared with ``torch.equal``; then the sentence that defines
the feature -- a search with ``where=F`` returns, bit for bit, what the same search returns when every row ``F`` does not admit
is added to every query's exclusion list -- on every engine, and what hangs on it: positions, the partitioned index, per-query
filters, the cache of views, a captured search."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from tests import _filter_spec as spec

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROWS_PER_WG = 2048            # FILTER_ROWS of csrc/mf_filter.hip
POISON = -7777


def _dev(a, dtype=torch.int64):
    return torch.as_tensor(np.asarray(a), dtype=dtype).to(DEV)


# ---------------------------------------------------------------------------------------------------- mf_filter_rows ----
def _filter_rows(mf, tags, f, *, offset_words=0):
    """``mf_filter_rows`` on poisoned buffers: ``(rows [N] with its tail, rank [N], count)``.  ``offset_words=1``: the tag words
    start 8 bytes past a 16-byte boundary (the kernel's other load path)."""
    lib = mf._lib.lib()
    n = len(tags)
    buf = torch.zeros(n + 2, dtype=torch.int64, device=DEV)
    assert buf.data_ptr() % 16 == 0
    t = buf[offset_words: offset_words + n]
    t.copy_(_dev(tags))
    rows = torch.full((n,), POISON, dtype=torch.int64, device=DEV)
    rank = torch.full((n,), POISON, dtype=torch.int32, device=DEV)
    count = torch.full((1,), POISON, dtype=torch.int64, device=DEV)
    ws = torch.full((lib.mf_filter_ws_bytes(n),), 0xA5, dtype=torch.uint8, device=DEV)
    mf._lib.check(lib.mf_filter_rows(t.data_ptr(), n, f[0], f[1], f[2], ws.data_ptr(), ws.numel(), rows.data_ptr(), rank.data_ptr(),
                                     count.data_ptr(), mf._lib.stream_ptr()))
    return rows, rank, count


def _check_rows(mf, tags, f, **kw):
    rows, rank, count = _filter_rows(mf, tags, f, **kw)
    want_rows, want_rank = spec.compact(spec.admits(tags, *f))
    m = want_rows.size
    assert int(count) == m
    assert torch.equal(rows[:m].cpu(), torch.from_numpy(want_rows))
    assert bool((rows[m:] == POISON).all()), "entries from M on must not be written"
    assert torch.equal(rank.cpu(), torch.from_numpy(want_rank)), "rank is written in full"
    again = _filter_rows(mf, tags, f, **kw)
    assert all(torch.equal(a, b) for a, b in zip((rows, rank, count), again))


SIZES = (1, 33, ROWS_PER_WG - 1, ROWS_PER_WG, ROWS_PER_WG + 1, 2 * ROWS_PER_WG + 1, 5000)


@pytest.mark.parametrize("n", SIZES)
def test_filter_rows_equals_the_spec(mf, n):
    rng = np.random.default_rng(n)
    tags = rng.integers(0, 1 << 6, n, dtype=np.int64) | (rng.integers(0, 2, n, dtype=np.int64) << 63)        # bit 63: the sign bit
    three = (0b000110, 0b000001, 0b100000)
    for f in (three, (0, 0b11, 0), (0b1, 0, 0), (0, 0, 0b1), (0, 1 << 63, 0), (1 << 63, 0, 0b1), (0, 0, 1 << 63), (0, 0, 0)):
        _check_rows(mf, tags, f)
    _check_rows(mf, tags, three, offset_words=1)
    _check_rows(mf, tags, (0, 1 << 40, 0))                                     # no row
    _check_rows(mf, np.full(n, -1, dtype=np.int64), (2**64 - 1, 2**64 - 1, 0))     # all rows, every bit asked for
    for one in {0, n // 2, n - 1}:                                              # one row
        mask = np.zeros(n, dtype=np.int64)
        mask[one] = 1
        _check_rows(mf, mask, (0, 1, 0))
        _check_rows(mf, mask, (0, 1, 0), offset_words=1)


def test_filter_rows_at_the_first_and_last_place_of_a_block(mf):
    n = 3 * ROWS_PER_WG + 7
    edges = [0, 1, 63, 64, 127, 128, ROWS_PER_WG - 1, ROWS_PER_WG, 2 * ROWS_PER_WG - 1, 2 * ROWS_PER_WG, 3 * ROWS_PER_WG - 1,
             3 * ROWS_PER_WG, n - 1]
    mask = np.zeros(n, dtype=np.int64)
    mask[edges] = 1
    _check_rows(mf, mask, (0, 1, 0))
    _check_rows(mf, 1 - mask, (0, 1, 0))
    for e in edges:
        only = np.zeros(n, dtype=np.int64)
        only[e] = 1
        rows, rank, count = _filter_rows(mf, only, (0, 1, 0))
        assert int(count) == 1 and int(rows[0]) == e and int(rank[e]) == 0 and int((rank == -1).sum()) == n - 1


# --------------------------------------------------------------------------------------------- remap, unmap, lists ----
def _view_of(n, seed):
    rng = np.random.default_rng(seed)
    ok = rng.random(n) < 0.4
    rows, rank = spec.compact(ok)
    return ok, rows, rank


@pytest.mark.parametrize("n_ids", [1, 2, 511, 512, 513, 3001])
def test_remap_and_unmap_elementwise(mf, n_ids):
    lib = mf._lib.lib()
    n, base = 1000, 37
    _, rows, rank = _view_of(n, 1)
    rng = np.random.default_rng(n_ids)
    ids = rng.integers(base - 5, base + n + 5, n_ids)
    ids[0] = base - 1
    ids[-1] = base + n
    slots_want = spec.remap(ids, base, rank)
    d_rank, d_rows = _dev(rank, torch.int32), _dev(rows)
    for shift in (0, 1):                       # 1: both buffers start 8 bytes past a 16-byte boundary
        src = torch.zeros(n_ids + 2, dtype=torch.int64, device=DEV)[shift: shift + n_ids]
        src.copy_(_dev(ids))
        out = torch.full((n_ids + 2,), POISON, dtype=torch.int64, device=DEV)
        mf._lib.check(lib.mf_filter_remap(src.data_ptr(), n_ids, base, d_rank.data_ptr(), n, out[shift:].data_ptr(), None))
        assert torch.equal(out[shift: shift + n_ids].cpu(), torch.from_numpy(slots_want))
        assert int((out == POISON).sum()) == 2
        back = torch.full((n_ids + 2,), POISON, dtype=torch.int64, device=DEV)
        mf._lib.check(lib.mf_filter_unmap(out[shift:].data_ptr(), n_ids, d_rows.data_ptr(), rows.size, base, back[shift:].data_ptr(), None))
        want = spec.unmap(slots_want, rows, base)
        assert torch.equal(back[shift: shift + n_ids].cpu(), torch.from_numpy(want))
        assert np.array_equal(want[slots_want >= 0], ids[slots_want >= 0]) and (want[slots_want < 0] == -1).all()
        assert int((back == POISON).sum()) == 2
        inplace = out[shift: shift + n_ids]
        mf._lib.check(lib.mf_filter_unmap(inplace.data_ptr(), n_ids, d_rows.data_ptr(), rows.size, base, inplace.data_ptr(), None))
        assert torch.equal(inplace.cpu(), torch.from_numpy(want))


def _lists_case(nq, n, base, rng, ok):
    """Sorted per-query lists of GLOBAL rows: empty, all admissible, none admissible, mixed with out-of-range rows and
    duplicates, and one of 30,000 entries."""
    inside, outside = np.flatnonzero(ok) + base, np.flatnonzero(~ok) + base
    lists = []
    for i in range(nq):
        kind = i % 6
        if kind == 0:
            e = []
        elif kind == 1:
            e = rng.choice(inside, 40)
        elif kind == 2:
            e = rng.choice(outside, 40)
        elif kind == 3:
            e = np.concatenate([rng.integers(base - 20, base + n + 20, 200), [base - 1, base + n], rng.choice(inside, 5).repeat(3)])
        elif kind == 4:
            e = rng.integers(base, base + n, 30000 if i == 4 else 1025)
        else:
            e = rng.integers(base, base + n, 1 + i)
        lists.append(np.sort(np.asarray(e, dtype=np.int64)))
    return lists


@pytest.mark.parametrize("nq,base", [(1, 0), (33, 0), (70, 0), (33, 123456)])
def test_filter_lists_equals_the_spec(mf, nq, base):
    lib = mf._lib.lib()
    n = 2500
    ok, rows, rank = _view_of(n, 2)
    rng = np.random.default_rng(nq)
    lists = _lists_case(nq, n, base, rng, ok) if nq > 1 else [np.sort(rng.integers(base - 3, base + n + 3, 77))]
    off = np.concatenate([[0], np.cumsum([len(e) for e in lists])]).astype(np.int64)
    ids = np.concatenate(lists) if off[-1] else np.zeros(1, np.int64)
    want_off, want_ids = spec.map_lists(off, ids, base, rank)
    d_off, d_ids, d_rank = _dev(off), _dev(ids), _dev(rank, torch.int32)
    ws = torch.full((lib.mf_filter_lists_ws_bytes(nq),), 0xA5, dtype=torch.uint8, device=DEV)
    outs = []
    for _ in range(2):
        out_off = torch.full((nq + 1,), POISON, dtype=torch.int64, device=DEV)
        out_ids = torch.full((max(int(off[-1]), 1),), POISON, dtype=torch.int64, device=DEV)
        mf._lib.check(lib.mf_filter_lists(d_off.data_ptr(), d_ids.data_ptr(), int(off[-1]), nq, base, d_rank.data_ptr(), n, ws.data_ptr(),
                                          ws.numel(), out_off.data_ptr(), out_ids.data_ptr(), None))
        outs.append((out_off, out_ids))
    out_off, out_ids = outs[0]
    assert torch.equal(out_off.cpu(), torch.from_numpy(want_off))
    kept = int(want_off[-1])
    assert torch.equal(out_ids[:kept].cpu(), torch.from_numpy(want_ids)) and bool((out_ids[kept:] == POISON).all())
    assert all(torch.equal(a, b) for a, b in zip(*outs))
    for i in range(nq):                                     # sorted lists stay sorted
        mine = want_ids[want_off[i]: want_off[i + 1]]
        assert (np.diff(mine) >= 0).all()


def test_filter_lists_without_entries_still_writes_the_offsets(mf):
    lib = mf._lib.lib()
    nq, n = 5, 100
    _, _, rank = _view_of(n, 3)
    d_rank = _dev(rank, torch.int32)
    off, ids = torch.zeros(nq + 1, dtype=torch.int64, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV)
    out_off = torch.full((nq + 1,), POISON, dtype=torch.int64, device=DEV)
    out_ids = torch.full((1,), POISON, dtype=torch.int64, device=DEV)
    ws = torch.empty(lib.mf_filter_lists_ws_bytes(nq), dtype=torch.uint8, device=DEV)
    mf._lib.check(lib.mf_filter_lists(off.data_ptr(), ids.data_ptr(), 0, nq, 0, d_rank.data_ptr(), n, ws.data_ptr(), ws.numel(),
                                      out_off.data_ptr(), out_ids.data_ptr(), None))
    assert bool((out_off == 0).all()) and int(out_ids[0]) == POISON


# ---------------------------------------------------------------------------------------------- the oracle sentence ----
K = 20
K_DEEP = 100


@functools.lru_cache(maxsize=None)
def _world(d, n, nq, base):
    """Catalog (300 identical rows from row 100 on when it is large enough: ties are decided by the row), queries (query 0 is
    that row), user exclusion lists that mix rows the views hold, rows they do not and rows outside the catalog, and tags."""
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


def _mask_of(n, m, seed):
    """An allow-mask of exactly m rows: for a large catalog half of them (rounded up) inside the identical rows."""
    rng = np.random.default_rng(seed)
    ok = np.zeros(n, dtype=bool)
    if n >= 1000 and 0 < m <= 300:
        ok[rng.choice(np.arange(100, 400), (m + 1) // 2, replace=False)] = True
    rest = np.flatnonzero(~ok)
    ok[rng.choice(rest, m - int(ok.sum()), replace=False)] = True
    assert int(ok.sum()) == m
    return ok


def _paths(mf, d, nq):
    paths = [("tiles", K), ("deep", K_DEEP), ("auto", K)]
    if nq <= mf.retrieval.ItemIndex.SMALL_Q:
        paths.append(("scan", K))
    if d >= 64:
        paths.append(("bf16", K))
    return paths


WORLDS = [(32, 33, 1, 0), (64, 1000, 33, 0), (128, 2500, 70, 0), (256, 1000, 1, 0), (48, 1000, 33, 0), (128, 33, 70, 0),
          (64, 2500, 1, 0), (32, 2500, 33, 0), (128, 1000, 33, 5000), (48, 2500, 70, 77), (256, 2500, 33, 0)]


@pytest.mark.parametrize("d,n,nq,base", WORLDS)
def test_a_filtered_search_equals_the_search_with_the_other_rows_excluded(mf, d, n, nq, base):
    items, q, lists, tags = _world(d, n, nq, base)
    index = mf.retrieval.ItemIndex(items, idx_base=base)
    index.set_tags(torch.from_numpy(tags))
    genre = mf.retrieval.TagFilter(any_of=0b1)
    wheres = [(m, torch.from_numpy(_mask_of(n, m, m)).to(DEV)) for m in (0, 1, K - 1, K, K + 1, 65, K_DEEP - 1, K_DEEP, K_DEEP + 1) if m <= n]
    wheres += [("half", genre), ("three masks", mf.retrieval.TagFilter(any_of=0b000110, all_of=0b000001, none_of=0b100000))]
    for what, where in wheres:
        ok = where.cpu().numpy() if isinstance(where, torch.Tensor) else spec.admits(tags, where.any_of, where.all_of, where.none_of)
        view = index.filtered(where)
        assert view.num_items == int(ok.sum()) and torch.equal(view.rows.cpu(), torch.from_numpy(np.flatnonzero(ok)))
        assert (view.index is None) == (view.num_items == 0)
        for user in (None, lists):
            mine = None if user is None else mf.retrieval._csr(user, nq, DEV)
            every = mf.retrieval._csr(spec.extended_lists(user, nq, ok, base), nq, DEV)
            for path, k in _paths(mf, d, nq):
                want = index.search(q, k, exclude_csr=every, path=path)
                got = view.search(q, k, exclude_csr=mine, path=path)
                assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (what, path, user is not None)
                assert got[1].dtype == torch.int64 and got[0].shape == (nq, k)
        # ... and through the public argument, with host lists
        want = index.search(q, K, exclude=spec.extended_lists(lists, nq, ok, base))
        got = index.search(q, K, exclude=lists, where=where)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), what
        if view.num_items == 0:
            assert bool((got[1] == -1).all()) and bool(torch.isinf(got[0]).all())
    # the identical rows were decided by the row: query 0's list starts with them, in ascending row order
    if n >= 1000:
        ok = spec.admits(tags, 0b1)
        rows = index.search(q[:1], K, where=genre)[1][0].cpu().numpy() - base
        same = np.flatnonzero(ok[100:400])[:K] + 100
        assert np.array_equal(rows[: same.size], same)


@pytest.mark.parametrize("d,n,nq,base", [(64, 1000, 33, 0), (128, 2500, 70, 900), (48, 33, 1, 0)])
def test_positions_with_a_filter(mf, d, n, nq, base):
    items, q, lists, tags = _world(d, n, nq, base)
    index = mf.retrieval.ItemIndex(items, idx_base=base)
    index.set_tags(torch.from_numpy(tags))
    rng = np.random.default_rng(7)
    targets = [[*(rng.integers(0, n, 9) + base).tolist(), base - 1, base + n, *lists[i][:2]] if i % 4 else [] for i in range(nq)]
    t_off = _dev(np.concatenate([[0], np.cumsum([len(t) for t in targets])]))
    flat = [y for t in targets for y in t]
    t_ids = _dev(flat if flat else [0])[: len(flat)]
    for where in (mf.retrieval.TagFilter(any_of=0b1), torch.from_numpy(_mask_of(n, min(n, 21), 5)).to(DEV),
                  torch.zeros(n, dtype=torch.bool, device=DEV)):
        ok = where.cpu().numpy() if isinstance(where, torch.Tensor) else spec.admits(tags, where.any_of)
        for user in (None, lists):
            want = index.positions(q, (t_off, t_ids), exclude=spec.extended_lists(user, nq, ok, base))
            got = index.positions(q, (t_off, t_ids), exclude=user, where=where)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1].view(torch.int32), want[1].view(torch.int32))
            assert torch.equal(got[2], want[2])
            out = torch.from_numpy(~ok[np.clip(np.asarray(flat, dtype=np.int64) - base, 0, n - 1)]).to(DEV) if flat else None
            if out is not None:                 # an inadmissible target reads -1 / -inf
                assert bool((got[0][out] == -1).all()) and bool(torch.isinf(got[1][out]).all())


# ------------------------------------------------------------------------------------------- the partitioned index ----
def test_partitioned_index_with_a_filter(mf):
    d, n, nq, base, cells = 64, 2500, 33, 40, 16
    items, q, lists, tags = _world(d, n, nq, base)
    index = mf.retrieval.PartitionedIndex.build(items, cells, iters=3, idx_base=base)
    index.set_tags(torch.from_numpy(tags))
    assign = index.assign.cpu().numpy()
    emptied = (assign != assign[0]) & (np.random.default_rng(0).random(n) < 0.5)          # the filter empties row 0's cell
    for where in (torch.from_numpy(emptied).to(DEV), mf.retrieval.TagFilter(any_of=0b11, none_of=0b100)):
        ok = where.cpu().numpy() if isinstance(where, torch.Tensor) else spec.admits(tags, where.any_of, 0, where.none_of)
        view = index.filtered(where)
        assert type(view.index) is mf.retrieval.PartitionedIndex and view.index.num_partitions == cells and view.index.idx_base == 0
        assert torch.equal(view.index.assign, index.assign[view.rows])
        for nprobe in (1, 8, cells):
            for user in (None, lists):
                want = index.search(q, K, exclude=spec.extended_lists(user, nq, ok, base), nprobe=nprobe)
                got = index.search(q, K, exclude=user, nprobe=nprobe, where=where)
                assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), nprobe
        want = index.search(q, K, exclude=spec.extended_lists(None, nq, ok, base), path="exact")
        got = index.search(q, K, path="exact", where=where)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
        full = index.search(q, K, nprobe=cells, where=where)
        assert torch.equal(full[0], got[0]) and torch.equal(full[1], got[1])             # all cells: the exact answer
    index.filtered(mf.retrieval.TagFilter(any_of=1))
    assert len(index._views) == 2
    index.rebuild()
    assert len(index._views) == 0


def test_quantized_index_takes_no_filter(mf):
    n, d = 1000, 32
    items, q, _, tags = _world(d, n, 1, 0)
    gen = torch.Generator().manual_seed(0)
    index = mf.retrieval.QuantizedIndex.from_codebooks(items, items[:4].clone(), torch.randint(0, 4, (n,), generator=gen).to(DEV),
                                                       torch.randn(4, 256, 8, generator=gen).to(DEV))
    index.set_tags(torch.from_numpy(tags))
    with pytest.raises(NotImplementedError, match="QuantizedIndex"):
        index.filtered(mf.retrieval.TagFilter(any_of=1))
    for path in ("pq", "cells", "exact"):
        with pytest.raises(NotImplementedError, match="QuantizedIndex"):
            index.search(q, K, path=path, where=mf.retrieval.TagFilter(any_of=1))


# ------------------------------------------------------------------------- per-query filters, the cache, a capture ----
def test_a_sequence_of_filters_equals_the_searches_of_its_groups(mf):
    d, n, nq, base = 64, 1000, 33, 11
    items, q, lists, tags = _world(d, n, nq, base)
    index = mf.retrieval.ItemIndex(items, idx_base=base)
    index.set_tags(torch.from_numpy(tags))
    F = mf.retrieval.TagFilter
    kinds = [F(any_of=0b1), F(all_of=0b10), F(none_of=0b111), F(all_of=1 << 50)]              # the last admits nothing
    where = [kinds[(i + i // 5) % 4] for i in range(nq)]
    assert set(where) == set(kinds)
    csr = mf.retrieval._csr(lists, nq, DEV)
    t_off = torch.arange(nq + 1, dtype=torch.int64, device=DEV) * 2
    t_ids = torch.from_numpy(np.random.default_rng(1).integers(0, n, 2 * nq) + base).to(DEV)
    for kw in (dict(exclude=lists), dict(exclude_csr=csr), {}):
        s, r = index.search(q, K, where=where, **kw)
        p, ps, nc = index.positions(q, (t_off, t_ids), where=where, **kw)
        for f in kinds:
            qs = [i for i in range(nq) if where[i] == f]
            sub = {"exclude": [lists[i] for i in qs]} if kw else {}
            ws, wr = index.search(q[qs], K, where=f, **sub)
            assert torch.equal(s[qs], ws) and torch.equal(r[qs], wr)
            ent = [2 * i + j for i in qs for j in (0, 1)]
            wp, wps, wnc = index.positions(q[qs], (torch.arange(len(qs) + 1, device=DEV) * 2, t_ids[ent]), where=f, **sub)
            assert torch.equal(p[ent], wp) and torch.equal(ps[ent].view(torch.int32), wps.view(torch.int32)) and torch.equal(nc[qs], wnc)
    with pytest.raises(ValueError, match="one filter per query"):
        index.search(q, K, where=where[:-1])


def test_the_cache_of_views(mf):
    n, d = 1000, 32
    items, q, _, tags = _world(d, n, 1, 0)
    index = mf.retrieval.ItemIndex(items)
    F = mf.retrieval.TagFilter
    with pytest.raises(ValueError, match="set_tags"):
        index.filtered(F(any_of=1))
    for bad in (torch.zeros(n, dtype=torch.int32), torch.zeros(n + 1, dtype=torch.int64), torch.zeros(n, 1, dtype=torch.int64), [0] * n):
        with pytest.raises(ValueError, match="tags should be"):
            index.set_tags(bad)
    index.set_tags(torch.from_numpy(tags))
    assert index.tags.device.type == "cuda" and index.MAX_VIEWS == 8
    first = index.filtered(F(any_of=1))
    assert index.filtered(F(any_of=1)) is first and index.filtered(F(any_of=1), cache=False) is not first
    mask = torch.from_numpy(tags % 2 == 1).to(DEV)
    assert index.filtered(mask) is not index.filtered(mask) and len(index._views) == 1          # an allow-mask is never cached
    assert torch.equal(index.filtered(mask).rows, first.rows)
    second = index.filtered(F(any_of=2))
    for bit in range(2, 8):
        index.filtered(F(any_of=1 << bit))
    assert len(index._views) == 8 and index.filtered(F(any_of=1)) is first                      # (used again: now the newest)
    index.filtered(F(any_of=1 << 9))                                                          # the ninth: the oldest goes
    assert len(index._views) == 8 and F(any_of=2) not in index._views and index.filtered(F(any_of=1)) is first
    assert index.filtered(F(any_of=2)) is not second
    index.refresh()
    assert len(index._views) == 0 and index.filtered(F(any_of=1)) is not first
    index.set_tags(torch.from_numpy(tags ^ 1))
    assert len(index._views) == 0
    assert torch.equal(index.filtered(F(any_of=1)).rows.cpu(), torch.from_numpy(np.flatnonzero(tags % 2 == 0)))
    for bad in (torch.zeros(n - 1, dtype=torch.bool, device=DEV), torch.zeros(n, dtype=torch.int64, device=DEV), "comedy"):
        with pytest.raises(ValueError, match="where should be"):
            index.filtered(bad)


def test_a_search_on_a_cached_view_replays_from_a_graph(mf):
    d, n, nq, base = 128, 2500, 33, 9
    items, q, lists, tags = _world(d, n, nq, base)
    index = mf.retrieval.ItemIndex(items, idx_base=base)
    index.set_tags(torch.from_numpy(tags))
    where = mf.retrieval.TagFilter(any_of=0b11)
    csr = mf.retrieval._csr(lists, nq, DEV)
    t_off = torch.arange(nq + 1, dtype=torch.int64, device=DEV)
    t_ids = torch.from_numpy(np.random.default_rng(2).integers(0, n, nq) + base).to(DEV)
    paths = ("tiles", "bf16", "deep")
    eager = [index.search(q, K, exclude_csr=csr, where=where, path=p) for p in paths]     # (also builds the view, its copies, the workspaces)
    eager_pos = index.positions(q, (t_off, t_ids), exclude_csr=csr, where=where)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                 # the view is cached: nothing is read back, nothing is built
        out = [index.search(q, K, exclude_csr=csr, where=where, path=p) for p in paths]
        out_pos = index.positions(q, (t_off, t_ids), exclude_csr=csr, where=where)
    for t in (*[x for o in out for x in o], *out_pos):
        t.fill_(0)
    graph.replay()
    torch.cuda.synchronize()
    for got, want in zip(out, eager):
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert all(torch.equal(a, b) for a, b in zip(out_pos, eager_pos))
