"""GPU: the partitioned index (``retrieval.PartitionedIndex``, csrc/mf_ivf.hip) against its spec (tests/_ivf_spec.py: the
oracle's exact top-k over the rows of the probed cells) and against the exact engines, to the bit: rows as integers, scores as
uint32 views.  tests/test_ivf_cpu.py asserts that the case set holds a tail, a probed empty cell, ties across cells and both
plan geometries, so none of the comparisons here is an empty one."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

from oracle import chain
from tests import _ivf_spec as spec

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = spec.cases()


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _index(mf, c, **kw):
    return mf.retrieval.PartitionedIndex.from_assignment(_dev(c.items), _dev(c.centroids), _dev(c.assign), idx_base=c.idx_base, **kw)


def _same(got, want, what):
    gs, gi = (x.cpu().numpy() for x in got)
    ws, wi = (x.cpu().numpy() if isinstance(x, torch.Tensor) else x for x in want)
    assert gi.dtype == np.int64 and gs.dtype == np.float32 and gi.shape == wi.shape, what
    assert np.array_equal(gi, wi), what
    assert np.array_equal(gs.view(np.uint32), ws.view(np.uint32)), what


def _poison(index):
    """Whatever the search keeps between calls holds garbage: nothing may rely on a cleared buffer."""
    for part in (index, index.coarse):
        for ws in part._ws.values():
            ws.fill_(0xA5)


@pytest.fixture(scope="module")
def wanted():
    return {name: c.expected() for name, c in CASES.items()}


@pytest.mark.parametrize("name", sorted(CASES))
def test_search_matches_the_spec(mf, wanted, name):
    c = CASES[name]
    index = _index(mf, c)
    q = _dev(c.q)
    assert index.max_cell_blocks == c.max_cell_blocks
    if name == "big_cell":
        assert index.plan(1, c.k, 1)["slices"] == 10
    if name == "width64":
        assert index.plan(33, c.k, 3)["slices"] == 1
    first = index.search(q, c.k, exclude=c.exclude, nprobe=c.nprobe)
    _same(first, wanted[name], name)
    _poison(index)
    again = index.search(q, c.k, exclude=c.exclude, nprobe=c.nprobe)
    _same(again, wanted[name], f"{name}: after poisoning")
    assert torch.equal(first[0].view(torch.int32), again[0].view(torch.int32)) and torch.equal(first[1], again[1])


@pytest.mark.parametrize("name", ["width128", "cell_sizes_nprobe16", "idx_base", "padded_width", "long_lists"])
def test_against_the_exact_engines(mf, name):
    """Every cell probed: ``ItemIndex.search`` on the same matrix.  Fewer: that search with the rows outside the probed cells
    added to the exclusions."""
    c = CASES[name]
    index = _index(mf, c)
    exact = mf.retrieval.ItemIndex(_dev(c.items), idx_base=c.idx_base)
    q = _dev(c.q)
    ncell = c.centroids.shape[0]
    _same(index.search(q, c.k, exclude=c.exclude, nprobe=min(ncell, 64)), exact.search(q, c.k, exclude=c.exclude), f"{name}: all cells")
    _same(index.search(q, c.k, exclude=c.exclude, path="exact"), exact.search(q, c.k, exclude=c.exclude), f"{name}: path exact")
    barred = spec.not_allowed(c.assign, spec.probes(c.q, c.centroids, c.nprobe))
    more = [sorted(set(c.exclude[i] if c.exclude else []) | set((b + c.idx_base).tolist())) for i, b in enumerate(barred)]
    _same(index.search(q, c.k, exclude=c.exclude, nprobe=c.nprobe), exact.search(q, c.k, exclude=more), f"{name}: probed cells")


def test_default_nprobe_and_the_python_refusals(mf):
    c = CASES["width64"]
    index = _index(mf, c, num_probes=3)
    q = _dev(c.q)
    _same(index.search(q, c.k, exclude=c.exclude), index.search(q, c.k, exclude=c.exclude, nprobe=3), "num_probes")
    # a prebuilt CSR in ANY order (the lists of the case are unsorted; ``exclude=`` sorts them on the way in)
    off = _dev(np.cumsum([0] + [len(e) for e in c.exclude]).astype(np.int64))
    ids = _dev(np.array([r for e in c.exclude for r in e], dtype=np.int64))
    assert any(list(e) != sorted(e) for e in c.exclude)
    _same(index.search(q, c.k, exclude_csr=(off, ids)), index.search(q, c.k, exclude=c.exclude), "unsorted lists")
    for kw in (dict(top_k=0), dict(top_k=65), dict(nprobe=0), dict(nprobe=17)):
        with pytest.raises(ValueError):
            index.search(q, **{"top_k": 20, **kw})


def test_a_captured_search_equals_the_eager_one(mf, wanted):
    c = CASES["cell_sizes_nprobe3"]
    index = _index(mf, c)
    q = _dev(c.q)
    off, ids = mf.retrieval._csr(c.exclude, q.shape[0], DEV)
    eager = index.search(q, c.k, exclude_csr=(off, ids), nprobe=c.nprobe)             # (also builds the copies and workspaces)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = index.search(q, c.k, exclude_csr=(off, ids), nprobe=c.nprobe)
    for _ in range(2):
        out[0].fill_(7.0)
        out[1].fill_(7)
        _poison(index)
        graph.replay()
        torch.cuda.synchronize()
        _same(out, eager, "replay")
        _same(out, wanted["cell_sizes_nprobe3"], "replay against the spec")


# ------------------------------------------------------------------------------------------------------- build ----
def _layout_holds(mf, index):
    assign = index.assign.cpu().numpy()
    sizes = np.bincount(assign, minlength=index.num_partitions)
    assert index.cell_blk.cpu().tolist() == [0] + np.cumsum((sizes + 63) // 64).tolist()
    row_of = index.row_of.cpu().numpy()
    assert sorted(row_of[row_of >= 0].tolist()) == list(range(index.num_items))
    for cell in range(index.num_partitions):
        lo = 64 * int(index.cell_blk[cell])
        assert row_of[lo : lo + sizes[cell]].tolist() == np.nonzero(assign == cell)[0].tolist(), cell
    assert index.max_cell_blocks == int(((sizes + 63) // 64).max())


@pytest.fixture(scope="module")
def rows_2500():
    g = torch.Generator().manual_seed(5)
    return torch.nn.functional.normalize(torch.randn(2500, 64, generator=g), dim=-1).to(DEV)


def test_build_is_deterministic_and_leaves_every_row_with_its_best_centroid(mf, rows_2500):
    one = mf.retrieval.PartitionedIndex.build(rows_2500, 16, iters=3, seed=4)
    two = mf.retrieval.PartitionedIndex.build(rows_2500, 16, iters=3, seed=4)
    assert torch.equal(one.centroids, two.centroids) and torch.equal(one.assign, two.assign) and torch.equal(one.row_of, two.row_of)
    assert one.num_partitions == 16 and one.centroids.shape == (16, 64)
    _layout_holds(mf, one)
    best = chain.topk(rows_2500.cpu().numpy(), one.centroids.cpu().numpy(), 1)[1][:, 0]
    assert np.array_equal(one.assign.cpu().numpy(), best)
    norms = one.centroids.norm(dim=1).cpu()
    assert torch.allclose(norms, torch.ones(16), atol=1e-5)                            # (no cell of 2,500 random rows in 16 is empty)
    other = mf.retrieval.PartitionedIndex.build(rows_2500, 16, iters=3, seed=5)
    assert not torch.equal(one.centroids, other.centroids)
    # searching it: the spec on the built cells
    q = rows_2500[:33] + 0.0
    want = spec.expected(q.cpu().numpy(), rows_2500.cpu().numpy(), one.centroids.cpu().numpy(), one.assign.cpu().numpy(), 20, 3)
    _same(one.search(q, 20, nprobe=3), want, "built index")
    one.rebuild()
    assert torch.equal(one.centroids, two.centroids) and torch.equal(one.assign, two.assign)
    _same(one.search(q, 20, nprobe=3), want, "rebuilt index")


def test_build_without_iterations_and_the_default_cell_count(mf, rows_2500):
    index = mf.retrieval.PartitionedIndex.build(rows_2500, iters=0, seed=1)
    assert index.num_partitions == 32 == mf.retrieval.default_num_partitions(2500)
    first = torch.randperm(2500, generator=torch.Generator().manual_seed(1))[:32]
    assert torch.equal(index.centroids, rows_2500[first.to(DEV)])                       # the seeded rows themselves
    best = chain.topk(rows_2500.cpu().numpy(), index.centroids.cpu().numpy(), 1)[1][:, 0]
    assert np.array_equal(index.assign.cpu().numpy(), best)
    _layout_holds(mf, index)
    with pytest.raises(ValueError):
        mf.retrieval.PartitionedIndex.build(rows_2500, 2501)


@pytest.mark.parametrize("d", [32, 256])
def test_cell_mean_is_exact_on_integer_rows(mf, d):
    """Sums of small integers are exact in fp32 in any order, so the kernel's are the int64 sums: the mean is one division."""
    lib, L = mf._lib.lib(), mf._lib
    rng = np.random.default_rng(d)
    n, ncell = 1500, 7
    rows = rng.integers(-8, 9, (n, d)).astype(np.float32)
    assign = rng.integers(0, ncell - 1, n)                                             # the last cell stays empty
    assign[:3] = [0, 0, 0]
    order = np.argsort(assign, kind="stable")
    cell_off = np.searchsorted(assign[order], np.arange(ncell + 1))
    out = torch.full((ncell, d), 123.0, device=DEV)
    d_rows, d_order, d_off = _dev(rows), _dev(order), _dev(cell_off)                     # (named: alive until the kernels have run)
    L.check(lib.mf_ivf_cell_mean(d_rows.data_ptr(), n, d, d_order.data_ptr(), d_off.data_ptr(), ncell, 0, out.data_ptr(), L.stream_ptr()))
    got = out.cpu().numpy()
    for cell in range(ncell - 1):
        inside = rows[assign == cell].astype(np.int64)
        want = inside.sum(axis=0).astype(np.float32) / np.float32(inside.shape[0])
        assert np.array_equal(got[cell].view(np.uint32), want.view(np.uint32)), cell
    assert (got[ncell - 1] == 123.0).all()                                              # an empty cell keeps what it held
    unit = torch.full((ncell, d), 123.0, device=DEV)
    L.check(lib.mf_ivf_cell_mean(d_rows.data_ptr(), n, d, d_order.data_ptr(), d_off.data_ptr(), ncell, 1, unit.data_ptr(), L.stream_ptr()))
    mean = torch.from_numpy(got[: ncell - 1])
    np.testing.assert_allclose(unit[: ncell - 1].cpu().numpy(), torch.nn.functional.normalize(mean, dim=1).numpy(), rtol=2e-6, atol=1e-7)
    zero = torch.full((1, d), 5.0, device=DEV)                                          # a mean of exactly zero stays zero
    pair, both, ends = _dev(np.stack([rows[0], -rows[0]])), _dev(np.arange(2)), _dev(np.array([0, 2]))
    L.check(lib.mf_ivf_cell_mean(pair.data_ptr(), 2, d, both.data_ptr(), ends.data_ptr(), 1, 1, zero.data_ptr(), L.stream_ptr()))
    assert not zero.cpu().numpy().any()


# ----------------------------------------------------------------------------------------------------- surface ----
def test_item_processor_end_to_end(mf, rows_2500):
    ids = torch.arange(2500) * 3 + 11
    proc = mf.retrieval.ItemProcessor(ids, index_type="partitioned", num_partitions=16, num_probes=4, index_seed=2)
    index = proc.set_index(rows_2500)
    assert isinstance(index, mf.retrieval.PartitionedIndex) and index.num_partitions == 16 and index.num_probes == 4
    same = mf.retrieval.PartitionedIndex.build(rows_2500, 16, seed=2, num_probes=4)
    assert torch.equal(index.centroids, same.centroids) and torch.equal(index.assign, same.assign)
    q = rows_2500[7:8].cpu().numpy()
    excluded = [int(ids[7]), int(ids[100]), 5]                                          # (5 is no item id: ignored)
    frame = proc.search(q, exclude_item_ids=excluded, top_k=20)
    ws, wr = spec.expected(q, rows_2500.cpu().numpy(), index.centroids.cpu().numpy(), index.assign.cpu().numpy(), 20, 4, [[7, 100]])
    assert frame[proc.idx_col].tolist() == wr[0].tolist() and frame[proc.id_col].tolist() == (wr[0] * 3 + 11).tolist()
    assert np.array_equal(frame["score"].to_numpy().view(np.uint32), ws[0].view(np.uint32))
    grown = proc.append([9_000_001, 9_000_002], rows_2500[:2] * 0.5)
    assert isinstance(grown, mf.retrieval.PartitionedIndex) and grown.num_items == 2502 and grown.num_partitions == 16


def test_module_with_a_partitioned_index(mf, tmp_path):
    cfg = dict(num_users=50, num_items=600, hidden_size=64, index_type="partitioned", num_partitions=8, num_probes=3, index_seed=3, top_k=20)
    module = mf.lightning.MatrixFactorizationLitModule(cfg)
    module.configure_model(device=DEV)
    index = module.item_processor.get_index(module)
    assert isinstance(index, mf.retrieval.PartitionedIndex) and (index.num_partitions, index.num_probes) == (8, 3)
    module.history = {4: [10, 11, 12]}
    frame = module.recommend(4, top_k=20, exclude_item_ids=[13])
    with torch.no_grad():
        q = module(torch.tensor([4], device=DEV)).cpu().numpy()
    items = index.embeddings[:, : index.dim].cpu().numpy()
    ws, wr = spec.expected(q, items, index.centroids.cpu().numpy(), index.assign.cpu().numpy(), 20, 3, [[10, 11, 12, 13]])
    assert frame["score"].size == 20 and frame[module.item_processor.idx_col].tolist() == wr[0].tolist()
    assert np.array_equal(frame["score"].to_numpy().view(np.uint32), ws[0].view(np.uint32))

    module.save(tmp_path / "m")
    exact = mf.lightning.MatrixFactorizationLitModule({**cfg, "index_type": "exact"})
    exact.configure_model(device=DEV)
    exact.item_processor.set_index(index.embeddings[:, : index.dim])
    exact.save(tmp_path / "e")
    assert sorted(p.name for p in (tmp_path / "m").iterdir()) == sorted(p.name for p in (tmp_path / "e").iterdir())      # the same files
    loaded = mf.lightning.MatrixFactorizationLitModule.load(tmp_path / "m", device=DEV)
    again = loaded.item_processor.index
    assert isinstance(again, mf.retrieval.PartitionedIndex) and again.num_probes == 3
    assert torch.equal(again.centroids, index.centroids) and torch.equal(again.assign, index.assign) and torch.equal(again.row_of, index.row_of)
    assert loaded.recommend(4, top_k=20, exclude_item_ids=[13]).equals(frame)

    # metrics_mode="positions" reads the whole catalog, whatever the index type
    users = torch.arange(1, 9, device=DEV)
    hist = (torch.arange(9, device=DEV) * 2, torch.arange(16, device=DEV) + 20)
    target = (torch.arange(9, device=DEV) * 3, torch.arange(24, device=DEV) * 7 % 600, torch.ones(24, device=DEV))
    batch = {"user": {"idx": users}, "history": hist, "target": target}
    got = {}
    for kind in ("partitioned", "exact"):
        m = mf.lightning.MatrixFactorizationLitModule({**cfg, "index_type": kind, "metrics_mode": "positions"})
        m.towers = module.towers
        m.configure_model(device=DEV)
        m.item_processor.get_index(m)
        got[kind] = {k: float(v) for k, v in m.update_metrics(batch, "val").items()}
    assert got["partitioned"] == got["exact"] and got["exact"]
    # and the list metrics run through the cells
    module.update_metrics(batch, "val")
    s, r = module.predict_step(batch)
    want = spec.expected(module(users).detach().cpu().numpy(), items, index.centroids.cpu().numpy(), index.assign.cpu().numpy(), 20, 3,
                         [list(range(20 + 2 * i, 22 + 2 * i)) for i in range(8)])
    _same((s, r), want, "predict_step")
