"""GPU: deep lists from the cell scan (``PartitionedIndex.search(path="cells_deep")``, csrc/mf_ivf_deep.hip) against the spec of
the partitioned index (tests/_ivf_spec.py, which takes any k), against the exact deep engine, against ``path="cells"`` where both
serve the depth, and list by list on a cell long enough for several settles of the workgroup's buffer -- to the bit: rows as
integers, scores as int32 views, every query and every column.  tests/test_ivf_deep_cpu.py asserts what these comparisons lean
on (the tails, the settles with a live bound, the ties)."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from tests import _filter_spec
from tests import _ivf_deep_spec as deep
from tests import _ivf_spec as spec

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = deep.cases()
PATH = "cells_deep"


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _index(mf, c, **kw):
    return mf.retrieval.PartitionedIndex.from_assignment(_dev(c.items), _dev(c.centroids), _dev(c.assign), idx_base=c.idx_base, **kw)


def _same(got, want, what=None):
    gs, gi = (x if isinstance(x, torch.Tensor) else torch.from_numpy(x) for x in got)
    ws, wi = (x if isinstance(x, torch.Tensor) else torch.from_numpy(x) for x in want)
    gs, gi, ws, wi = gs.cpu(), gi.cpu(), ws.cpu(), wi.cpu()
    assert gi.dtype == torch.int64 and gs.dtype == torch.float32 and gi.shape == wi.shape == gs.shape == ws.shape, what
    assert torch.equal(gi, wi), what
    assert torch.equal(gs.view(torch.int32), ws.view(torch.int32)), what


def _poison(index):
    for part in (index, index.coarse):
        for ws in part._ws.values():
            ws.fill_(0xA5)


@pytest.fixture(scope="module")
def wanted():
    return {name: c.expected() for name, c in CASES.items()}


# ------------------------------------------------------------------------------------------------ 1: the spec ----
@pytest.mark.parametrize("name", sorted(CASES))
def test_search_matches_the_spec(mf, wanted, name):
    c = CASES[name]
    index = _index(mf, c)
    q = _dev(c.q)
    first = index.search(q, c.k, exclude=c.exclude, nprobe=c.nprobe, path=PATH)
    _same(first, wanted[name], name)
    _poison(index)
    again = index.search(q, c.k, exclude=c.exclude, nprobe=c.nprobe, path=PATH)
    _same(again, wanted[name], f"{name}: after poisoning")
    _same(index.search(q, c.k, exclude=c.exclude, nprobe=c.nprobe, path=PATH), first, f"{name}: a repeat call")
    if name == "deep_k1000_tail":
        filled = (first[1] >= 0).sum(dim=1).cpu().tolist()
        assert all(3 <= f < 1000 for f in filled), filled
    if name == "deep_ties_k1024":
        assert index.plan(2, 1024, 4, PATH)["slices"] >= 2
        assert first[1][0].cpu().tolist() == list(range(1024))                   # lowest global row first, across cells and slices


# ------------------------------------------------------------------------------------ 2: the exact deep engine ----
@pytest.mark.parametrize("name", ["deep_w48_k128", "deep_w64_k129", "deep_k513_all_cells", "deep_idx_base", "deep_cell_sizes_nprobe16",
                                  "deep_k1024"])
def test_against_the_exact_deep_engine(mf, name):
    c = CASES[name]
    index = _index(mf, c)
    exact = mf.retrieval.ItemIndex(_dev(c.items), idx_base=c.idx_base)
    q = _dev(c.q)
    ncell = c.centroids.shape[0]
    every = min(ncell, 64, deep.MERGE_KEYS // c.k)
    if every == ncell:
        _same(index.search(q, c.k, exclude=c.exclude, nprobe=ncell, path=PATH), exact.search(q, c.k, exclude=c.exclude, path="deep"),
              f"{name}: all cells")
    else:
        assert name == "deep_w64_k129"                                           # 37 cells of which 3 are probed: the second half only
    barred = spec.not_allowed(c.assign, spec.probes(c.q, c.centroids, c.nprobe))
    more = [sorted(set(c.exclude[i] if c.exclude else []) | set((b + c.idx_base).tolist())) for i, b in enumerate(barred)]
    _same(index.search(q, c.k, exclude=c.exclude, nprobe=c.nprobe, path=PATH), exact.search(q, c.k, exclude=more, path="deep"),
          f"{name}: probed cells")


# ------------------------------------------------------------------------------------------- 3: shallow depths ----
@pytest.mark.parametrize("name", sorted(spec.cases()))
def test_shallow_depths_equal_the_wavefront_scan(mf, name):
    c = spec.cases()[name]
    index = _index(mf, c)
    q = _dev(c.q)
    _same(index.search(q, c.k, exclude=c.exclude, nprobe=c.nprobe, path=PATH), index.search(q, c.k, exclude=c.exclude, nprobe=c.nprobe, path="cells"),
          name)


# ------------------------------------------------------------------------------------------- 4: several settles ----
# (the plain kernel on scores s * e0; masks, lists, ties and every kept class on real dot products: tests/test_gpu_ivf_deep_settles.py)
@pytest.fixture(scope="module")
def long_cell(mf):
    """One cell of ``settle_rows()`` rows, the row at cell position i = (its score) * e0; the query is e0."""
    n, d = deep.settle_rows(), deep.SETTLE_DIM
    worlds = {}
    for order in deep.SETTLE_ORDERS:
        scores = deep.settle_scores(order)
        items = np.zeros((n, d), dtype=np.float32)
        items[:, 0] = scores
        centroid = np.zeros((1, d), dtype=np.float32)
        centroid[0, 0] = 1.0
        index = mf.retrieval.PartitionedIndex.from_assignment(_dev(items), _dev(centroid), torch.zeros(n, dtype=torch.int64, device=DEV),
                                                              num_probes=1)
        assert torch.equal(index.row_of[:n].cpu(), torch.arange(n)) and index.max_cell_blocks == (n + 63) // 64
        worlds[order] = (index, scores)
    return worlds


@pytest.mark.parametrize("k", [100, 1000, 1024])
@pytest.mark.parametrize("order", deep.SETTLE_ORDERS)
def test_a_cell_of_several_settles_list_by_list(mf, long_cell, order, k):
    index, scores = long_cell[order]
    n, d, nb = deep.settle_rows(), deep.SETTLE_DIM, index.max_cell_blocks
    lib = mf._lib.lib()
    q = torch.zeros(1, d, device=DEV)
    q[0, 0] = 1.0
    probes = torch.zeros(1, 1, dtype=torch.int64, device=DEV)
    cells, npad = index.cell_blocked(), index.row_of.numel()
    planned = index.plan(1, k, 1, PATH)["slices"]
    # the most slices the export takes: a list per block, within the merge's keys (S * k <= 16,384)
    most = min(nb, deep.MERGE_KEYS // k)
    assert 1 < planned <= most
    for slices in (1, planned, most):
        ws = torch.full((slices * k,), -2, dtype=torch.int64, device=DEV)
        mf._lib.check(lib.mf_ivf_scan_deep(q.data_ptr(), 1, cells.data_ptr(), index.cell_blk.data_ptr(), index.row_of.data_ptr(), npad, n, 1, d,
                                           nb, probes.data_ptr(), 1, k, slices, None, None, 0, ws.data_ptr(), ws.numel() * 8, None))
        lists = ws.cpu().numpy().reshape(slices, k)
        for s in range(slices):
            lo, hi = min(n, 64 * (nb * s // slices)), min(n, 64 * (nb * (s + 1) // slices))
            want = deep.top_of(scores, lo, hi, k)
            got = lists[s]
            assert (got[want.size:] == -1).all(), (slices, s)
            assert np.array_equal(got[: want.size] & 0xFFFFFFFF, want), (slices, s)
            assert np.array_equal((got[: want.size] >> 32).astype(np.uint32), scores[want].view(np.uint32)), (slices, s)
        out_s = torch.empty(1, k, dtype=torch.float32, device=DEV)
        out_r = torch.empty(1, k, dtype=torch.int64, device=DEV)
        mf._lib.check(lib.mf_topk_merge_packed_deep(ws.data_ptr(), slices, 1, k, out_s.data_ptr(), out_r.data_ptr(), None))
        best = deep.top_of(scores, 0, n, k)
        _same((out_s, out_r), (scores[best][None], best[None].astype(np.int64)), (order, k, slices))
    _same(index.search(q, k, path=PATH), (out_s, out_r), "the search")


# ------------------------------------------------------------------------------------------------------ 5: ties ----
def test_ties_on_both_sides_of_a_mask_and_a_zero_query(mf, wanted):
    """(1,100 identical rows over four cells and two slices each at k = 1024, and the zero query: test_search_matches_the_spec.)
    Here 300 identical rows of which a mask admits about half: the admitted ones first, in ascending row order."""
    c = CASES["deep_ties_k1024"]
    index = _index(mf, c)
    rng = np.random.default_rng(3)
    ok = rng.random(c.items.shape[0]) < 0.5
    ok[300:1100] = False                                                         # 300 of the twins stay, on both sides of the mask
    assert 100 < int(ok[:300].sum()) < 200
    q = _dev(c.q)
    got = index.search(q, 1024, nprobe=4, path=PATH, allow=_dev(ok))
    want = index.search(q, 1024, nprobe=4, path=PATH, exclude=_filter_spec.extended_lists(None, 2, ok, 0))
    _same(got, want, "mask against lists")
    twins = np.flatnonzero(ok[:300])
    assert got[1][0, : twins.size].cpu().tolist() == twins.tolist()
    _same(got, spec.expected(c.q, c.items, c.centroids, c.assign, 1024, 4, _filter_spec.extended_lists(None, 2, ok, 0)), "the spec")
    z = CASES["deep_zero_query"]
    rows = wanted["deep_zero_query"][1][1]
    assert rows.tolist() == [r for r in range(z.items.shape[0]) if z.assign[r] < 3 and r not in z.exclude[1]][:100]


# ------------------------------------------------------------------------------------------------ 6: the allow twin ----
@pytest.fixture(scope="module")
def world(mf):
    d, n, nq, base, cells = 64, 2500, 33, 40, 16
    gen = torch.Generator().manual_seed(11)
    items = torch.nn.functional.normalize(torch.randn(n, d, generator=gen), dim=-1)
    items[100:400] = items[100]
    q = torch.nn.functional.normalize(torch.randn(nq, d, generator=gen), dim=-1)
    q[0] = items[100]
    rng = np.random.default_rng(n + nq)
    lists = [[] if i % 5 == 4 else [*(rng.integers(0, n, 12) + base).tolist(), base - 1, base + n] for i in range(nq)]
    tags = rng.integers(0, 1 << 6, n, dtype=np.int64)
    index = mf.retrieval.PartitionedIndex.build(items.to(DEV), cells, iters=2, idx_base=base, num_probes=8)
    index.set_tags(torch.from_numpy(tags))
    return index, q.to(DEV), lists, tags, n, nq, base


@pytest.mark.parametrize("k", [100, 1024])
def test_a_mask_equals_the_search_with_the_other_rows_excluded(mf, world, k):
    index, q, lists, tags, n, nq, base = world
    rng = np.random.default_rng(k)
    assign = index.assign.cpu().numpy()
    emptied = (assign != assign[0]) & (rng.random(n) < 0.5)                       # every word of the cell of row 0 is 0
    one = np.zeros(n, dtype=bool)
    one[777] = True
    masks = {"all": np.ones(n, dtype=bool), "none": np.zeros(n, dtype=bool), "one row": one, "half": _filter_spec.admits(tags, 0b1),
             "a cell emptied": emptied}
    plain = index.search(q, k, nprobe=8, path=PATH)
    for what, ok in masks.items():
        for nprobe in (3, 16):
            for user in (None, lists):
                want = index.search(q, k, exclude=_filter_spec.extended_lists(user, nq, ok, base), nprobe=nprobe, path=PATH)
                got = index.search(q, k, exclude=user, nprobe=nprobe, path=PATH, allow=_dev(ok))
                _same(got, want, (what, nprobe, user is not None))
                _same(index.search(q, k, exclude=user, nprobe=nprobe, path=PATH, where=_dev(ok)), want, (what, nprobe, "the view"))
        if what == "none":
            assert bool((got[1] == -1).all()) and bool(torch.isinf(got[0]).all())
        if what == "one row":
            assert bool((got[1][:, 1:] == -1).all()) and set(got[1][:, 0].cpu().tolist()) <= {-1, 777 + base}
        if what == "half":
            assert not torch.equal(index.search(q, k, nprobe=8, path=PATH, allow=_dev(ok))[1], plain[1])
    F = mf.retrieval.TagFilter
    _same(index.search(q, k, exclude=lists, path=PATH, allow=F(any_of=0b1)), index.search(q, k, exclude=lists, path=PATH, where=F(any_of=0b1)),
          "a tag filter: allow= and where=")
    # three masks, one per query through allow_of; a number outside [0, 3) admits nothing
    kinds = [F(any_of=0b1), F(all_of=1 << 50), torch.from_numpy(tags % 4 == 2).to(DEV)]
    three = index.cell_mask(kinds)
    of = np.array([(i + i // 5) % 3 for i in range(nq)], dtype=np.int64)
    of[3], of[7] = -1, 3
    got = index.search(q, k, exclude=lists, path=PATH, allow=three, allow_of=_dev(of))
    for f in range(3):
        qs = np.flatnonzero(of == f).tolist()
        want = index.search(q[qs], k, exclude=[lists[i] for i in qs], path=PATH, allow=kinds[f])
        _same((got[0][qs], got[1][qs]), want, f)
    for i in (3, 7):
        assert bool((got[1][i] == -1).all()) and bool(torch.isinf(got[0][i]).all())


# ------------------------------------------------------------------------------------------- 7: limits and plan ----
def test_limits_plan_and_the_quantised_index(mf):
    c = spec.make("deep_limits", 64, 1000, 3, 64, 8, 100)
    index = _index(mf, c)
    q = _dev(c.q)
    for top_k, nprobe in ((0, 8), (1025, 8), (1025, 1), (1024, 17), (257, 64)):
        with pytest.raises(ValueError):
            index.search(q, top_k, nprobe=nprobe, path=PATH)
    assert not index._ws and not index.coarse._ws and index._cells is None          # refused before any workspace or copy appeared
    with pytest.raises(ValueError):
        index.search(q, 65, path="cells")                                         # the wavefront scan keeps its limit
    for top_k, nprobe in ((1024, 16), (256, 64)):                                  # at the boundary: 16,384 keys
        _same(index.search(q, top_k, nprobe=nprobe, path=PATH), spec.expected(c.q, c.items, c.centroids, c.assign, top_k, nprobe), (top_k, nprobe))
    for nq, nprobe, k in ((1, 8, 100), (1, 1, 1000), (33, 3, 65), (1, 16, 1024), (1024, 8, 1000), (1, 64, 256)):
        got = index.plan(nq, k, nprobe, PATH)
        s = spec.plan_slices(nq, nprobe, k, index.max_cell_blocks, merge_keys=deep.MERGE_KEYS)
        assert got == {"slices": s, "lists": nprobe * s, "workgroups": nq * nprobe * s, "bytes": nprobe * s * nq * k * 8}, (nq, nprobe, k)
    assert [index.default_path(k) for k in (1, 64, 65, 1024)] == ["cells", "cells", PATH, PATH]
    gen = torch.Generator().manual_seed(2)
    quant = mf.retrieval.QuantizedIndex.from_codebooks(_dev(c.items), _dev(c.centroids), _dev(c.assign), torch.randn(8, 256, 8, generator=gen).to(DEV),
                                                       num_probes=8)
    _same(quant.search(q, 100, path=PATH), index.search(q, 100, path=PATH), "the quantised index's parent route")
    assert quant.plan(3, 100, 8, path=PATH) == index.plan(3, 100, 8, PATH) and quant.default_path(100) == "pq"
    with pytest.raises(ValueError):
        quant.search(q, 100, path="pq")


# ----------------------------------------------------------------------------------------------------- 8: graph ----
def test_a_captured_search_equals_the_eager_one(mf, wanted):
    c = CASES["deep_k1000_tail"]
    index = _index(mf, c)
    q = _dev(c.q)
    off, ids = mf.retrieval._csr(c.exclude, q.shape[0], DEV)
    eager = index.search(q, c.k, exclude_csr=(off, ids), nprobe=c.nprobe, path=PATH)  # (also builds the copies and workspaces)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = index.search(q, c.k, exclude_csr=(off, ids), nprobe=c.nprobe, path=PATH)
    for _ in range(2):
        out[0].fill_(7.0)
        out[1].fill_(7)
        _poison(index)
        graph.replay()
        torch.cuda.synchronize()
        _same(out, eager, "replay")
        _same(out, wanted["deep_k1000_tail"], "replay against the spec")


# -------------------------------------------------------------------------------------- 9: module and processor ----
def test_item_processor_and_module_at_top_k_100(mf):
    g = torch.Generator().manual_seed(5)
    rows = torch.nn.functional.normalize(torch.randn(2500, 64, generator=g), dim=-1).to(DEV)
    ids = torch.arange(2500) * 3 + 11
    proc = mf.retrieval.ItemProcessor(ids, index_type="partitioned", num_partitions=16, num_probes=4, index_seed=2)
    index = proc.set_index(rows)
    q = rows[7:8].cpu().numpy()
    frame = proc.search(q, exclude_item_ids=[int(ids[7]), int(ids[100]), 5], top_k=100)
    ws, wr = spec.expected(q, rows.cpu().numpy(), index.centroids.cpu().numpy(), index.assign.cpu().numpy(), 100, 4, [[7, 100]])
    assert len(frame) == 100 and frame[proc.idx_col].tolist() == wr[0].tolist() and frame[proc.id_col].tolist() == (wr[0] * 3 + 11).tolist()
    assert np.array_equal(frame["score"].to_numpy().view(np.uint32), ws[0].view(np.uint32))

    cfg = dict(num_users=50, num_items=600, hidden_size=64, index_type="partitioned", num_partitions=8, num_probes=8, index_seed=3, top_k=100)
    module = mf.lightning.MatrixFactorizationLitModule(cfg)
    module.configure_model(device=DEV)
    index = module.item_processor.get_index(module)
    assert isinstance(index, mf.retrieval.PartitionedIndex) and (index.num_partitions, index.num_probes) == (8, 8)
    exact = mf.lightning.MatrixFactorizationLitModule({**cfg, "index_type": "exact"})
    exact.towers = module.towers
    exact.configure_model(device=DEV)
    exact.item_processor.get_index(exact)
    assert type(exact.item_processor.index) is mf.retrieval.ItemIndex
    users = torch.arange(1, 9, device=DEV)
    hist = (torch.arange(9, device=DEV) * 2, torch.arange(16, device=DEV) + 20)
    target = (torch.arange(9, device=DEV) * 3, torch.arange(24, device=DEV) * 7 % 600, torch.ones(24, device=DEV))
    batch = {"user": {"idx": users}, "history": hist, "target": target}
    got = {k: float(v) for k, v in module.update_metrics(batch, "val").items()}
    want = {k: float(v) for k, v in exact.update_metrics(batch, "val").items()}
    assert got == want and got
    _same(module.predict_step(batch), exact.predict_step(batch), "predict_step: every cell probed")
    frame = module.recommend(4, top_k=100)
    assert len(frame) == 100 and frame.equals(exact.recommend(4, top_k=100))
