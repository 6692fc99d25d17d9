"""GPU: deep lists from the quantised index (``QuantizedIndex.search(path="pq_deep")``: ``mf_pq_scan_deep`` / ``_allow``,
``mf_topk_merge_packed_deep``, ``mf_pq_refine_deep``) against the numpy restatement of tests/_ivf_pq_spec.py at any depth, and
against the other paths of the library where they answer the same question -- to the bit: rows as integers, approximate and
exact scores as uint32 views, no tolerance anywhere.  tests/test_ivf_pq_deep_cpu.py asserts that the cases of
tests/_ivf_pq_deep_spec.py hold what the comparisons here lean on (widths, sub-vector lengths, depths, the merge's boundary,
the long cell's settles under a live bound)."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from tests import _filter_spec
from tests import _ivf_deep_spec as deep
from tests import _ivf_pq_deep_spec as pqd
from tests import _ivf_pq_spec as spec
from tests import _ivf_spec as ivf

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PATH = "pq_deep"
CASES = pqd.cases()
SHALLOW = spec.cases()


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


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


def _make(mf, c, **kw):
    b = c.base
    return mf.retrieval.QuantizedIndex.from_codebooks(_dev(b.items), _dev(b.centroids), _dev(b.assign), _dev(c.books),
                                                      refine_factor=c.refine_factor, idx_base=b.idx_base, **kw)


@pytest.fixture(scope="module")
def indexes(mf):
    made = {}

    def get(name):
        if name not in made:
            made[name] = _make(mf, CASES[name] if name in CASES else SHALLOW[name])
        return made[name]

    return get


@pytest.fixture(scope="module")
def wanted():
    made = {}

    def get(name):
        if name not in made:
            made[name] = CASES[name].expected()
        return made[name]

    return get


# ------------------------------------------------------------------------------------- 1: candidates against the spec ----
@pytest.mark.parametrize("name", sorted(SHALLOW))
def test_candidates_and_search_on_the_shared_cases_equal_the_spec_and_the_shallow_path(indexes, name):
    """k <= 64 and R <= 256: both paths take the shape -- the same candidates, approximate-score bits included, and the same result."""
    c = SHALLOW[name]
    index, q, b = indexes(name), _dev(c.base.q), c.base
    deep_c = index.candidates(q, c.r, exclude=b.exclude, nprobe=b.nprobe, path=PATH)
    _same(deep_c, c.candidates(), name)
    shallow_c = index.candidates(q, c.r, exclude=b.exclude, nprobe=b.nprobe)
    assert torch.equal(deep_c[1], shallow_c[1]) and torch.equal(deep_c[0].view(torch.int32), shallow_c[0].view(torch.int32)), name
    got = index.search(q, b.k, exclude=b.exclude, nprobe=b.nprobe, path=PATH)
    want = index.search(q, b.k, exclude=b.exclude, nprobe=b.nprobe, path="pq")
    assert torch.equal(got[1], want[1]) and torch.equal(got[0].view(torch.int32), want[0].view(torch.int32)), name
    assert index._cells is None


@pytest.mark.parametrize("r", pqd.DEPTHS)
def test_every_kept_class_boundary_on_one_case(indexes, r):
    """R over the class boundaries of ``ivfd_kept``, on cells of several blocks and with all cells probed."""
    c = SHALLOW["long_lists"]
    index, b = indexes("long_lists"), c.base
    for nprobe in (1, 3, 37) if r * 37 <= pqd.MERGE_KEYS else (1, 3, pqd.MERGE_KEYS // r):
        want = spec.candidates(b.q, b.items, b.centroids, b.assign, c.books, c.codes, r, nprobe, b.exclude)
        got = index.candidates(_dev(b.q), r, exclude=b.exclude, nprobe=nprobe, path=PATH)
        _same(got, want, (r, nprobe))
        if r <= 256:
            shallow = index.candidates(_dev(b.q), r, exclude=b.exclude, nprobe=nprobe)
            assert torch.equal(got[1], shallow[1]) and torch.equal(got[0].view(torch.int32), shallow[0].view(torch.int32)), (r, nprobe)


# ------------------------------------------------------------------------------------------ 2: search against the spec ----
@pytest.mark.parametrize("name", sorted(CASES))
def test_search_matches_the_spec(indexes, wanted, name):
    c = CASES[name]
    index, q, b = indexes(name), _dev(c.base.q), c.base
    first = index.search(q, b.k, exclude=b.exclude, nprobe=b.nprobe, path=PATH)
    _same(first, wanted(name), name)
    _poison(index)
    again = index.search(q, b.k, exclude=b.exclude, nprobe=b.nprobe, path=PATH)
    _same(again, wanted(name), f"{name}: after poisoning")
    assert index._cells is None                                          # no cell-ordered fp32 copy on this path
    _same(index.candidates(q, c.r, exclude=b.exclude, nprobe=b.nprobe, path=PATH), c.candidates(), f"{name}: candidates")


def test_ties_a_tail_and_a_zero_query(indexes, wanted):
    # 1,100 rows with identical codes and base across four cells and their slices at R = 1024: the lowest rows, in order
    c = CASES["pqd_ties_r1024"]
    approx, rows = indexes(c.name).candidates(_dev(c.base.q), 1024, nprobe=4, path=PATH)
    assert rows[0].cpu().tolist() == list(range(1024)) and len(set(approx[0].view(torch.int32).cpu().tolist())) == 1
    assert indexes(c.name).plan(2, 1024, 4, 1, path=PATH)["slices"] > 1
    # fewer probed rows than top_k: a tail in every list
    s, r = wanted("pqd_k1000_tail")
    filled = (r >= 0).sum(axis=1)
    assert (filled >= 500).all() and (filled < 1000).all() and np.isneginf(s[0, filled[0]:]).all()
    z = CASES["pqd_zero_query"].base
    assert wanted("pqd_zero_query")[1][1].tolist() == [r for r in range(1000) if z.assign[r] < 3 and r not in z.exclude[1]][:100]


# ------------------------------------------------------------------------------- 3: against other paths of the library ----
def test_a_refine_that_covers_the_cells_is_the_deep_partitioned_search(mf):
    """N = 1000 in 8 cells, nprobe = 3, top_k = 100, refine_factor = 10: R = 1000 covers every probed row, nothing is approximate."""
    base = ivf.make("pqd_covering", 64, 1000, 33, 8, 3, 100, lengths=(0, 1, 17))
    assert np.sort(base.sizes)[-3:].sum() <= 1000
    index = _make(mf, spec.PqCase(base, 8, 10, 0), num_probes=3)
    plain = mf.retrieval.PartitionedIndex.from_assignment(_dev(base.items), _dev(base.centroids), _dev(base.assign), num_probes=3)
    q = _dev(base.q)
    got = index.search(q, 100, exclude=base.exclude, path=PATH)
    _same(got, plain.search(q, 100, exclude=base.exclude, path="cells_deep"), "cells_deep")
    _same(got, ivf.expected(base.q, base.items, base.centroids, base.assign, 100, 3, base.exclude), "the partitioned spec")
    assert index._cells is None


# ------------------------------------------------------------------------------ 4: the buffer under a live bound ----
@pytest.fixture(scope="module")
def long_cells(mf):
    made = {}

    def get(order):
        if order not in made:
            c = pqd.long_cell(order)
            index = _make(mf, c, num_probes=1)
            n = deep.settle_rows()
            assert torch.equal(index.row_of[:n].cpu(), torch.arange(n)) and index.max_cell_blocks == pqd.LONG_BLOCKS
            made[order] = index
        return made[order]

    return get


def _scan_long(mf, index, q, r, slices, mask=None):
    """``mf_pq_scan_deep`` (``_allow`` with a mask) on the one-cell catalog: ``[slices, r]`` packed entries."""
    lib, n = mf._lib.lib(), deep.settle_rows()
    base, probes = index.coarse.search(q, 1)
    ws = torch.full((slices * r,), -2, dtype=torch.int64, device=DEV)
    head = (q.data_ptr(), 1, index.codes().data_ptr(), index.codebooks.data_ptr(), index.dsub, index.cell_blk.data_ptr(), index.row_of.data_ptr(),
            index.row_of.numel(), n, 1, 32, pqd.LONG_BLOCKS, probes.data_ptr(), base.data_ptr(), 1, r, slices, None, None, pqd.LONG_BASE)
    if mask is None:
        mf._lib.check(lib.mf_pq_scan_deep(*head, ws.data_ptr(), ws.numel() * 8, None))
    else:
        mf._lib.check(lib.mf_pq_scan_deep_allow(*head, mask.words.data_ptr(), 1, None, ws.data_ptr(), ws.numel() * 8, None))
    return ws


@pytest.mark.parametrize("r", pqd.LONG_DEPTHS)
@pytest.mark.parametrize("order", pqd.LONG_ORDERS)
def test_a_cell_of_several_settles_list_by_list(mf, long_cells, order, r):
    index = long_cells(order)
    q = _dev(pqd.long_cell(order).base.q)
    for slices in sorted(set(pqd.long_slices(r))):
        ws = _scan_long(mf, index, q, r, slices)
        assert np.array_equal(ws.cpu().numpy().reshape(slices, r), pqd.long_lists(order, r, slices)), (order, r, slices)
    assert index.plan(1, r, 1, 1, path=PATH)["slices"] == pqd.long_slices(r)[1]
    want = pqd.long_cell(order).candidates(r)
    _same(index.candidates(q, r, nprobe=1, path=PATH), want, "the planned slices")
    _same(index.candidates(q, r, nprobe=1, slices=1, path=PATH), want, "one slice")


def test_a_slice_longer_than_one_strip_of_mask_words(mf, long_cells):
    """208 blocks in one slice: the allow twin moves on to a fourth strip of 64 words, under a live bound."""
    order, r = "ascending", 1000
    index = long_cells(order)
    c = pqd.long_cell(order)
    q = _dev(c.base.q)
    n = deep.settle_rows()
    rng = np.random.default_rng(5)
    for what, ok in (("half", rng.random(n) < 0.5), ("every other block", np.repeat(np.arange(pqd.LONG_BLOCKS) % 2 == 0, 64)[:n]),
                     ("late", np.arange(n) >= 9000)):
        mask = index.cell_mask(_dev(ok))
        for slices in (1, 3):
            ws = _scan_long(mf, index, q, r, slices, mask)
            assert np.array_equal(ws.cpu().numpy().reshape(slices, r), pqd.long_lists(order, r, slices, ok)), (what, slices)
        want = spec.candidates(*c._args(), r, 1, _filter_spec.extended_lists(None, 1, ok, pqd.LONG_BASE), pqd.LONG_BASE)
        _same(index.candidates(q, r, nprobe=1, slices=1, allow=mask, path=PATH), want, what)


# ----------------------------------------------------------------------------------------------- 5: the allow twin ----
def test_a_mask_equals_the_search_with_the_other_rows_excluded(mf, indexes):
    c = CASES["pqd_w64_k256"]
    index, b = indexes(c.name), c.base
    q, n, nq = _dev(b.q), b.items.shape[0], b.q.shape[0]
    rng = np.random.default_rng(256)
    masks = {"1 %": rng.random(n) < 0.01, "50 %": rng.random(n) < 0.5, "all": np.ones(n, dtype=bool), "none": np.zeros(n, dtype=bool)}
    for what, ok in masks.items():
        for user in (None, b.exclude):
            every = _filter_spec.extended_lists(user, nq, ok, b.idx_base)
            got = index.search(q, b.k, exclude=user, nprobe=b.nprobe, path=PATH, allow=_dev(ok))
            _same(got, index.search(q, b.k, exclude=every, nprobe=b.nprobe, path=PATH), (what, user is not None))
        _same(got, spec.search(*c._args(), b.k, c.refine_factor, b.nprobe, every, b.idx_base), (what, "the spec"))
        if what == "none":
            assert bool((got[1] == -1).all()) and bool(torch.isinf(got[0]).all())
    # three masks, one per query through allow_of; a number outside [0, 3) admits nothing
    kinds = [_dev(masks["50 %"]), _dev(masks["1 %"]), _dev(np.arange(n) % 4 == 2)]
    three = index.cell_mask(kinds)
    of = np.array([(i + i // 5) % 3 for i in range(nq)], dtype=np.int64)
    of[3], of[7] = -1, 3
    got = index.search(q, b.k, exclude=b.exclude, nprobe=b.nprobe, path=PATH, allow=three, allow_of=_dev(of))
    for f in range(3):
        qs = np.flatnonzero(of == f).tolist()
        want = index.search(q[qs], b.k, exclude=[b.exclude[i] for i in qs], nprobe=b.nprobe, path=PATH, allow=kinds[f])
        _same((got[0][qs], got[1][qs]), want, f)
    for i in (3, 7):
        assert bool((got[1][i] == -1).all()) and bool(torch.isinf(got[0][i]).all())
    assert index._cells is None


def test_ties_on_both_sides_of_a_mask(indexes):
    """300 of the identical rows stay, about half of them admitted: the admitted ones first, in ascending row order."""
    c = CASES["pqd_ties_r1024"]
    index, b = indexes(c.name), c.base
    rng = np.random.default_rng(3)
    ok = rng.random(b.items.shape[0]) < 0.5
    ok[300:1100] = False
    twins = np.flatnonzero(ok[:300])
    assert 100 < twins.size < 200
    q = _dev(b.q)
    every = _filter_spec.extended_lists(None, 2, ok, 0)
    got = index.candidates(q, 1024, nprobe=4, path=PATH, allow=_dev(ok))
    _same(got, index.candidates(q, 1024, nprobe=4, path=PATH, exclude=every), "mask against lists")
    _same(got, spec.candidates(*c._args(), 1024, 4, every), "the spec")
    first = got[1][0, : twins.size].cpu().tolist()
    assert sorted(first) == twins.tolist() and first == twins.tolist()


# ------------------------------------------------------------------------------------------------ 6: the refine alone ----
@pytest.mark.parametrize("d", [32, 256])
def test_the_deep_refine_against_the_spec_and_the_shallow_refine(mf, d):
    lib, L = mf._lib.lib(), mf._lib
    n, nq, base = 3000, 5, 40
    rng = np.random.default_rng(d)
    items = ivf._unit(rng.standard_normal((n, d)))
    items[100:140] = items[100]                                             # equal exact scores: the row orders them
    q = ivf._unit(rng.standard_normal((nq, d)))
    q[0] = items[100]
    d_items, d_q = _dev(items), _dev(q)
    for r in (1, 255, 256, 257, 1024):
        cand = np.stack([rng.permutation(n)[:r] for _ in range(nq)]).astype(np.int64) + base
        if r >= 255:
            cand[0, :40] = np.arange(100, 140)[::-1] + base
            cand[0, 40:] = np.setdiff1d(rng.permutation(n), np.arange(100, 140), assume_unique=True)[: r - 40] + base
            cand[1, 5:9] = (-1, base - 1, base + n, 2**31 + 7)               # no candidates: -1 and rows outside [base, base + N)
            cand[2, :] = -1
            cand[3, 200:] = -1
        clean = [row[(row >= base) & (row < base + n)] for row in cand]
        d_cand = _dev(cand)
        for k in sorted({1, min(64, r), min(65, r), r}):
            want = spec.refine(q, items, clean, k, base)
            s = torch.full((nq, k), 7.0, dtype=torch.float32, device=DEV)
            rows = torch.full((nq, k), 7, dtype=torch.int64, device=DEV)
            L.check(lib.mf_pq_refine_deep(d_q.data_ptr(), nq, d_items.data_ptr(), n, d, d_cand.data_ptr(), r, k, base, s.data_ptr(), rows.data_ptr(),
                                          L.stream_ptr()))
            _same((s, rows), want, (d, r, k))
            if k <= 64 and r <= 256:
                s2, rows2 = torch.empty_like(s), torch.empty_like(rows)
                L.check(lib.mf_pq_refine(d_q.data_ptr(), nq, d_items.data_ptr(), n, d, d_cand.data_ptr(), r, k, base, s2.data_ptr(),
                                         rows2.data_ptr(), L.stream_ptr()))
                _same((s, rows), (s2, rows2), (d, r, k, "mf_pq_refine"))


# ---------------------------------------------------------------------------------------- 7: graph, limits, plan ----
def test_a_captured_search_equals_the_eager_one(mf, indexes, wanted):
    name = "pqd_cell_sizes"                                               # (top_k, refine_factor) = (100, 4)
    c = CASES[name]
    index = indexes(name)
    q = _dev(c.base.q)
    off, ids = mf.retrieval._csr(c.base.exclude, q.shape[0], DEV)
    eager = index.search(q, 100, exclude_csr=(off, ids), nprobe=3, path=PATH)      # (also builds the codes and workspaces)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = index.search(q, 100, exclude_csr=(off, ids), nprobe=3, path=PATH)
    for _ in range(2):
        out[0].fill_(7.0)
        out[1].fill_(7)
        _poison(index)
        graph.replay()
        torch.cuda.synchronize()
        _same(out, eager, "replay")
        _same(out, wanted(name), "replay against the spec")


def test_limits_the_boundary_and_the_plan(mf, indexes, wanted):
    c = CASES["pqd_nprobe64_k256"]
    index = _make(mf, c, num_probes=8)
    q = _dev(c.base.q)
    for kw in (dict(top_k=0), dict(top_k=1025, refine_factor=1), dict(top_k=257, refine_factor=4), dict(top_k=1024, refine_factor=1, nprobe=17),
               dict(top_k=257, refine_factor=1, nprobe=64), dict(top_k=100, refine_factor=4, nprobe=41), dict(nprobe=0), dict(nprobe=65),
               dict(refine_factor=0)):
        with pytest.raises(ValueError):
            index.search(q, **{"top_k": 100, "path": PATH, **kw})
    with pytest.raises(ValueError):
        index.candidates(q, 1025, path=PATH)
    with pytest.raises(NotImplementedError):
        index.search(q, 100, path=PATH, where=_dev(np.ones(2500, dtype=bool)))
    assert not index._ws and not index.coarse._ws and index._cells is None and index._codes is None      # refused before anything appeared
    for top_k, rf in ((100, 4), (65, 1), (64, 5)):                         # the shallow path keeps its limits
        with pytest.raises(ValueError):
            index.search(q, top_k, refine_factor=rf, path="pq")
    # at the boundary: 16,384 keys of a query in the merge
    _same(index.search(q, 256, exclude=c.base.exclude, refine_factor=1, nprobe=64, path=PATH), c.expected(), "(256, 1, 64)")
    m64 = CASES["pqd_w256_m64_k1024"]
    _same(indexes(m64.name).search(_dev(m64.base.q), 1024, exclude=m64.base.exclude, nprobe=16, path=PATH), wanted(m64.name), "(1024, 1, 16)")
    for nq, nprobe, top_k, rf in ((1, 8, 100, 4), (1, 1, 1000, 1), (33, 3, 65, 1), (1, 16, 1024, 1), (1024, 8, 256, 4), (1, 64, 256, 1)):
        got = index.plan(nq, top_k, nprobe, rf, path=PATH)
        s = ivf.plan_slices(nq, nprobe, rf * top_k, index.max_cell_blocks, merge_keys=16384)
        assert got == {"slices": s, "lists": nprobe * s, "workgroups": nq * nprobe * s, "bytes": nprobe * s * nq * rf * top_k * 8}, (nq, nprobe, top_k)
    assert [index.serving_path(k) for k in (1, 64, 65, 1024)] == ["pq", "pq", PATH, PATH] and index.default_path(100) == "pq"
    # R in 257..1024 at top_k <= 64 is reached by naming the path
    _same(index.search(q, 20, exclude=c.base.exclude, refine_factor=40, nprobe=8, path=PATH), spec.search(*c._args(), 20, 40, 8, c.base.exclude, c.base.idx_base), "(20, 40)")


# -------------------------------------------------------------------------------------- 8: module and processor ----
def _spec_of(index, q, k, nprobe, exclude, refine_factor):
    items = index.embeddings[:, : index.dim].cpu().numpy()
    cen, assign, books = index.centroids.cpu().numpy(), index.assign.cpu().numpy(), index.codebooks.cpu().numpy()
    codes = spec.encode(spec.residuals(items, cen, assign), books)
    return spec.search(q, items, cen, assign, books, codes, k, refine_factor, nprobe, exclude)


def test_item_processor_at_top_k_100(mf):
    g = torch.Generator().manual_seed(5)
    rows = torch.nn.functional.normalize(torch.randn(2500, 64, generator=g), dim=-1).to(DEV)
    ids = torch.arange(2500) * 3 + 11
    proc = mf.retrieval.ItemProcessor(ids, index_type="quantized", num_partitions=16, num_probes=4, index_seed=2, refine_factor=3)
    index = proc.set_index(rows)
    assert isinstance(index, mf.retrieval.QuantizedIndex)
    q = rows[7:8].cpu().numpy()
    frame = proc.search(q, exclude_item_ids=[int(ids[7]), int(ids[100]), 5], top_k=100)
    ws, wr = _spec_of(index, q, 100, 4, [[7, 100]], 3)
    assert len(frame) == 100 and frame[proc.idx_col].tolist() == wr[0].tolist() and frame[proc.id_col].tolist() == (wr[0] * 3 + 11).tolist()
    assert np.array_equal(frame["score"].to_numpy().view(np.uint32), ws[0].view(np.uint32))
    hand = index.search(rows[7:8], 100, exclude=[[7, 100]], path=PATH)
    assert frame[proc.idx_col].tolist() == hand[1][0].cpu().tolist() and index._cells is None


def test_module_with_a_quantized_index_at_top_k_100(mf, tmp_path):
    cfg = dict(num_users=50, num_items=600, hidden_size=64, index_type="quantized", num_partitions=8, num_probes=3, index_seed=3, top_k=100,
               num_sub_vectors=16, refine_factor=4)
    module = mf.lightning.MatrixFactorizationLitModule(cfg)
    module.configure_model(device=DEV)
    index = module.item_processor.get_index(module)
    assert isinstance(index, mf.retrieval.QuantizedIndex) and (index.num_probes, index.refine_factor, index.num_sub_vectors) == (3, 4, 16)
    module.history = {4: [10, 11, 12]}
    frame = module.recommend(4, top_k=100, exclude_item_ids=[13])
    with torch.no_grad():
        q = module(torch.tensor([4], device=DEV)).cpu().numpy()
    ws, wr = _spec_of(index, q, 100, 3, [[10, 11, 12, 13]], 4)
    filled = int((wr[0] >= 0).sum())
    assert filled > 64 and frame[module.item_processor.idx_col].tolist() == wr[0][:filled].tolist()
    assert np.array_equal(frame["score"].to_numpy().view(np.uint32), ws[0][:filled].view(np.uint32))

    users = torch.arange(1, 9, device=DEV)
    hist = (torch.arange(9, device=DEV) * 2, torch.arange(16, device=DEV) + 20)
    target = (torch.arange(9, device=DEV) * 3, torch.arange(24, device=DEV) * 7 % 600, torch.ones(24, device=DEV))
    batch = {"user": {"idx": users}, "history": hist, "target": target}
    lists = [list(range(20 + 2 * i, 22 + 2 * i)) for i in range(8)]
    want = _spec_of(index, module(users).detach().cpu().numpy(), 100, 3, lists, 4)
    _same(module.predict_step(batch), want, "predict_step")
    # the list metrics are those of the rows the deep search returns: a hand-built call on the same queries
    hand = index.search(module(users).detach(), 100, exclude=lists, path=PATH)
    assert torch.equal(hand[1].cpu(), torch.from_numpy(want[1]))
    got = {k: float(v) for k, v in module.update_metrics(batch, "val").items()}
    metrics = mf.retrieval.RetrievalMetrics(top_k=100, prefix="val/")
    metrics.update(hand[1], target[0], target[1], target[2])
    assert got and got == {k: float(v) for k, v in metrics.compute().items()}

    module.save(tmp_path / "m")
    loaded = mf.lightning.MatrixFactorizationLitModule.load(tmp_path / "m", device=DEV)
    again = loaded.item_processor.index
    assert isinstance(again, mf.retrieval.QuantizedIndex) and (again.num_probes, again.refine_factor) == (3, 4)
    assert torch.equal(again.codebooks, index.codebooks) and torch.equal(again.codes(), index.codes())
    assert loaded.recommend(4, top_k=100, exclude_item_ids=[13]).equals(frame)
