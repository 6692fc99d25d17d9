"""GPU: the quantised index (``retrieval.QuantizedIndex``, csrc/mf_pq.hip) against its numpy restatement
(tests/_ivf_pq_spec.py), to the bit: codes as bytes, rows as integers, approximate and exact scores as uint32 views.
tests/test_ivf_pq_cpu.py pins that restatement to the oracle of the exact engines and asserts that the case set holds what the
comparisons here lean on (R = 1 / 20 / 80 / 256, a sliced cell, tails, approximate ties, refined results that differ from the
exact ones)."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from tests import _ivf_pq_spec as spec
from tests import _ivf_spec as ivf

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = spec.cases()


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


def _make(mf, base, books, refine_factor=4, **kw):
    return mf.retrieval.QuantizedIndex.from_codebooks(_dev(base.items), _dev(base.centroids), _dev(base.assign), _dev(books),
                                                      refine_factor=refine_factor, idx_base=base.idx_base, **kw)


@pytest.fixture(scope="module")
def indexes(mf):
    made = {}

    def get(name):
        if name not in made:
            c = CASES[name]
            made[name] = _make(mf, c.base, c.books, c.refine_factor)
        return made[name]

    return get


def _codes_hold(index, res, books, what):
    """The index's codes are the spec's, byte for byte in the documented layout; padding positions hold 0."""
    want = spec.device_codes(spec.encode(res, books), index.row_of.cpu().numpy())
    got = index.codes()
    assert got.dtype == torch.uint8 and got.numel() == index.row_of.numel() * index.num_sub_vectors == want.size, what
    assert torch.equal(got.cpu(), torch.from_numpy(want)), what


# ------------------------------------------------------------------------------------------------------ encode ----
@pytest.mark.parametrize("dsub", spec.SUB_LENGTHS)
@pytest.mark.parametrize("d", ivf.WIDTHS)
def test_encode_at_every_width_and_sub_length(mf, d, dsub):
    base = ivf.make(f"encode_{d}_{dsub}", d, 1000, 1, 16, 1, 1, lengths=None)
    res = spec.residuals(base.items, base.centroids, base.assign)
    books = spec.build_codebooks(res, d // dsub, 0)
    index = _make(mf, base, books)
    assert (index.num_sub_vectors, index.dsub) == (d // dsub, dsub)
    _codes_hold(index, res, books, (d, dsub))
    # the plain form the codebook training reads: residuals in, [N][M] bytes out
    lib, L = mf._lib.lib(), mf._lib
    plain = torch.full((1000, d // dsub), 0xA5, dtype=torch.uint8, device=DEV)
    d_res, d_books = _dev(res), _dev(books)
    L.check(lib.mf_pq_encode(d_res.data_ptr(), 1000, d, None, None, d_books.data_ptr(), dsub, None, 1000, plain.data_ptr(), L.stream_ptr()))
    assert torch.equal(plain.cpu(), torch.from_numpy(spec.encode(res, books)))


@pytest.mark.parametrize("name", sorted(CASES))
def test_codes_on_every_shared_case(indexes, name):
    """Among them the padded width (48 stored as 64) and cells of 0 / 1 / 63 / 64 / 65 rows."""
    c = CASES[name]
    _codes_hold(indexes(name), c.residuals, c.books, name)


def test_twin_codewords_and_a_row_on_its_centroid(mf):
    c = CASES["width64"]
    base = ivf.Case(**{**c.base.__dict__, "items": c.base.items.copy()})
    base.items[7] = base.centroids[base.assign[7]]                        # residual 0: the codeword of least norm
    books = c.books.copy()
    books[:, 5] = books[:, 3]                                             # twins: the lower code is the one written
    books[2, 200] = 0.0                                                   # and a zero codeword: half norm 0
    res = spec.residuals(base.items, base.centroids, base.assign)
    assert not res[7].any()
    want = spec.encode(res, books)
    assert (want != 5).all() and (want == 3).any() and want[7, 2] == 200
    _codes_hold(_make(mf, base, books), res, books, "twins")


# ------------------------------------------------------------------------------------------------ scan + merge ----
@pytest.fixture(scope="module")
def wanted_candidates():
    return {name: c.candidates() for name, c in CASES.items()}


@pytest.mark.parametrize("name", sorted(CASES))
def test_candidates_match_the_spec(indexes, wanted_candidates, name):
    c = CASES[name]
    index = indexes(name)
    q = _dev(c.base.q)
    if name == "big_cell":
        assert index.plan(1, c.base.k, 1)["slices"] == 10
    first = index.candidates(q, c.r, exclude=c.base.exclude, nprobe=c.base.nprobe)
    _same(first, wanted_candidates[name], name)
    _poison(index)
    again = index.candidates(q, c.r, exclude=c.base.exclude, nprobe=c.base.nprobe)
    _same(again, wanted_candidates[name], f"{name}: after poisoning")
    assert index._cells is None


@pytest.mark.parametrize("r", [1, 20, 80, 256])
def test_every_depth_on_one_case(indexes, r):
    """R through the sort sizes of the scan's buffer, on cells of several blocks and with all cells probed."""
    c = CASES["long_lists"]
    index = indexes("long_lists")
    for nprobe in (1, 3, 37):
        want = spec.candidates(c.base.q, c.base.items, c.base.centroids, c.base.assign, c.books, c.codes, r, nprobe, c.base.exclude)
        _same(index.candidates(_dev(c.base.q), r, exclude=c.base.exclude, nprobe=nprobe), want, (r, nprobe))


@pytest.mark.parametrize("r", [1, 80, 256])
@pytest.mark.parametrize("name", ["steady", "steady_tail"])
def test_a_cell_of_forty_blocks_as_one_slice(mf, name, r):
    """Ten passes of one workgroup: the bound, the settles inside the loop and both ways out of it (tests/test_ivf_pq_cpu.py
    asserts that these cases take them), with exclusions among the best candidates."""
    c = spec.steady_cases()[name]
    index = _make(mf, c.base, c.books, c.refine_factor)
    q = _dev(c.base.q)
    want = c.candidates(r)
    _same(index.candidates(q, r, exclude=c.base.exclude, nprobe=1, slices=1), want, (name, r, "one slice"))
    _poison(index)
    _same(index.candidates(q, r, exclude=c.base.exclude, nprobe=1, slices=1), want, (name, r, "one slice, after poisoning"))
    for slices in (None, 3, 40):                                          # the lists do not depend on the slicing
        _same(index.candidates(q, r, exclude=c.base.exclude, nprobe=1, slices=slices), want, (name, r, slices))
    bare = spec.candidates(*c._args(), r, 1, None, c.base.idx_base)
    _same(index.candidates(q, r, nprobe=1, slices=1), bare, (name, r, "no exclusions"))
    for bad in (0, 41, 65 if r == 256 else 41):
        with pytest.raises(ValueError, match="slices"):
            index.candidates(q, r, nprobe=1, slices=bad)


def test_many_queries_each_scan_whole_cells(mf):
    """Q * nprobe >= 1024: the plan itself leaves every 40-block cell in one slice, the shape of a batched evaluation."""
    c = spec.steady_cases()["steady_many"]
    index = _make(mf, c.base, c.books, c.refine_factor)
    q = _dev(c.base.q)
    assert index.plan(1024, 20, 1) == {"slices": 1, "lists": 1, "workgroups": 1024, "bytes": 1024 * 80 * 8}
    _same(index.candidates(q, 80, exclude=c.base.exclude, nprobe=1), c.candidates(80), "candidates")
    _same(index.search(q, 20, exclude=c.base.exclude, nprobe=1), c.expected(), "search")
    assert index._cells is None


# ------------------------------------------------------------------------------------------------------ search ----
@pytest.fixture(scope="module")
def wanted():
    return {name: c.expected() for name, c in CASES.items()}


@pytest.mark.parametrize("name", sorted(CASES))
def test_search_matches_the_spec(indexes, wanted, name):
    c = CASES[name]
    index = indexes(name)
    q = _dev(c.base.q)
    first = index.search(q, c.base.k, exclude=c.base.exclude, nprobe=c.base.nprobe)
    _same(first, wanted[name], name)
    _poison(index)
    again = index.search(q, c.base.k, exclude=c.base.exclude, nprobe=c.base.nprobe)
    _same(again, wanted[name], f"{name}: after poisoning")
    assert torch.equal(first[0].view(torch.int32), again[0].view(torch.int32)) and torch.equal(first[1], again[1])
    assert index._cells is None                                          # no cell-ordered fp32 copy on this path
    # the scores returned are the exact chain scores of the rows returned
    exact = _exact_scores(c, first[1].cpu().numpy())
    assert np.array_equal(first[0].cpu().numpy().view(np.uint32), exact.view(np.uint32)), name


def _exact_scores(c, rows):
    from oracle import chain

    full = chain.scores(ivf.padded(c.base.q), ivf.padded(c.base.items))
    local = np.where(rows >= 0, rows - c.base.idx_base, 0)
    return np.where(rows >= 0, np.take_along_axis(full, local, axis=1), -np.inf).astype(np.float32)


def test_a_refine_that_covers_the_cells_is_the_partitioned_and_the_exact_search(mf):
    """N = 200 in 4 cells, k = 64, refine_factor = 4: R = 256 is every row of the probed cells, so nothing is approximate."""
    base = ivf.make("pq_covering", 64, 200, 5, 4, 1, 64, lengths=(0, 1, 17))
    books = spec.build_codebooks(spec.residuals(base.items, base.centroids, base.assign), 8, 0)
    index = _make(mf, base, books, 4)
    q = _dev(base.q)
    plain = mf.retrieval.PartitionedIndex.from_assignment(_dev(base.items), _dev(base.centroids), _dev(base.assign))
    exact = mf.retrieval.ItemIndex(_dev(base.items))
    for nprobe in (1, 3):
        got = index.search(q, 64, exclude=base.exclude, nprobe=nprobe)
        want = plain.search(q, 64, exclude=base.exclude, nprobe=nprobe)
        assert torch.equal(got[0].view(torch.int32), want[0].view(torch.int32)) and torch.equal(got[1], want[1]), nprobe
    assert index._cells is None
    got = index.search(q, 64, exclude=base.exclude, nprobe=4)
    want = exact.search(q, 64, exclude=base.exclude)
    assert torch.equal(got[0].view(torch.int32), want[0].view(torch.int32)) and torch.equal(got[1], want[1])
    # the parent's paths stay the parent's
    _same(index.search(q, 64, exclude=base.exclude, nprobe=1, path="cells"), plain.search(q, 64, exclude=base.exclude, nprobe=1), "cells")
    _same(index.search(q, 64, exclude=base.exclude, path="exact"), want, "exact")


def test_defaults_and_the_python_refusals(mf, indexes, wanted):
    c = CASES["width64"]
    index = _make(mf, c.base, c.books, c.refine_factor, num_probes=3)
    q = _dev(c.base.q)
    _same(index.search(q, 20, exclude=c.base.exclude), wanted["width64"], "num_probes and refine_factor of the index")
    _same(index.search(q, 20, exclude=c.base.exclude, refine_factor=1), c.expected(1), "refine_factor = 1")
    assert index.plan(33, 20, 3) == index.plan(33, 20, 3, refine_factor=4) and index.plan(33, 20, 3)["lists"] == 3
    kept_before = set(index._ws)
    for kw in (dict(top_k=0), dict(top_k=65), dict(refine_factor=0), dict(refine_factor=13), dict(top_k=64, refine_factor=5), dict(nprobe=0),
               dict(nprobe=17)):
        with pytest.raises(ValueError):
            index.search(q, **{"top_k": 20, **kw})
    with pytest.raises(ValueError):
        index.candidates(q, 257)
    for kw in (dict(nprobe=0), dict(nprobe=17), dict(top_k=65), dict(refine_factor=13), dict(num_queries=0)):      # the plan refuses like the search
        with pytest.raises(ValueError):
            index.plan(**{"num_queries": 33, "top_k": 20, **kw})
    assert set(index._ws) == kept_before                                 # refused before any launch or workspace
    rows = _dev(c.base.items)
    for m in (3, 64, 2, 0):                                               # 64 / m outside {4, 8, 16}
        with pytest.raises(ValueError, match="num_sub_vectors"):
            mf.retrieval.QuantizedIndex.build(rows, 4, num_sub_vectors=m)
    with pytest.raises(ValueError, match="refine_factor"):
        mf.retrieval.QuantizedIndex.build(rows, 4, refine_factor=0)
    with pytest.raises(ValueError, match="codebooks"):
        _make(mf, c.base, c.books[:, :255])


def test_a_captured_search_equals_the_eager_one(mf, indexes, wanted):
    name = "cell_sizes_nprobe3"
    c = CASES[name]
    index = indexes(name)
    q = _dev(c.base.q)
    off, ids = mf.retrieval._csr(c.base.exclude, q.shape[0], DEV)
    eager = index.search(q, c.base.k, exclude_csr=(off, ids), nprobe=c.base.nprobe)      # (also builds the codes and workspaces)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = index.search(q, c.base.k, exclude_csr=(off, ids), nprobe=c.base.nprobe)
    for _ in range(2):
        out[0].fill_(7.0)
        out[1].fill_(7)
        _poison(index)
        graph.replay()
        torch.cuda.synchronize()
        _same(out, eager, "replay")
        _same(out, wanted[name], "replay against the spec")


# ------------------------------------------------------------------------------------------------------- build ----
@pytest.fixture(scope="module")
def rows_600():
    g = torch.Generator().manual_seed(11)
    return torch.nn.functional.normalize(torch.randn(600, 32, generator=g), dim=-1).to(DEV)


def _plain_codes(index) -> np.ndarray:
    """``[N, M]`` codes out of the cell-ordered layout."""
    m = index.num_sub_vectors
    u = min(m, 4)
    at = index.codes().cpu().numpy().reshape(-1, m // u, 64, u).transpose(0, 2, 1, 3).reshape(-1, m)
    row_of = index.row_of.cpu().numpy()
    out = np.zeros((index.num_items, m), dtype=np.uint8)
    out[row_of[row_of >= 0]] = at[row_of >= 0]
    assert not at[row_of < 0].any()
    return out


def _mse(index) -> float:
    books = index.codebooks.cpu().numpy().astype(np.float64)
    codes = _plain_codes(index)
    recon = np.concatenate([books[j][codes[:, j]] for j in range(index.num_sub_vectors)], axis=1)
    recon += index.centroids.cpu().numpy().astype(np.float64)[index.assign.cpu().numpy()]
    return float(((index.embeddings.cpu().numpy().astype(np.float64) - recon) ** 2).mean())


def test_the_tiny_build_is_the_numpy_restatement(mf, rows_600):
    index = mf.retrieval.QuantizedIndex.build(rows_600, 4, num_sub_vectors=4, pq_iters=2, iters=2, seed=1)
    assert (index.num_sub_vectors, index.dsub, index.refine_factor) == (4, 8, 4) and index.codebooks.shape == (4, 256, 8)
    cells = mf.retrieval.PartitionedIndex.build(rows_600, 4, iters=2, seed=1)
    assert torch.equal(index.centroids, cells.centroids) and torch.equal(index.assign, cells.assign)      # the parent's cells
    res = spec.residuals(rows_600.cpu().numpy(), index.centroids.cpu().numpy(), index.assign.cpu().numpy())
    books = spec.build_codebooks(res, 4, 2)
    got = index.codebooks.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), books.view(np.uint32))
    _codes_hold(index, res, books, "tiny build")
    assert np.array_equal(_plain_codes(index), spec.encode(res, books))
    # searching it: the spec on the built cells and codebooks
    q = rows_600[:9] + 0.0
    want = spec.search(q.cpu().numpy(), rows_600.cpu().numpy(), index.centroids.cpu().numpy(), index.assign.cpu().numpy(), books,
                       spec.encode(res, books), 20, 4, 2)
    _same(index.search(q, 20, nprobe=2), want, "built index")


def test_build_is_deterministic_and_training_does_not_hurt(mf, rows_600):
    one = mf.retrieval.QuantizedIndex.build(rows_600, 4, pq_iters=10, iters=2, seed=4)
    two = mf.retrieval.QuantizedIndex.build(rows_600, 4, pq_iters=10, iters=2, seed=4)
    assert one.num_sub_vectors == 4                                       # the default: the stored width // 8
    assert torch.equal(one.codebooks, two.codebooks) and torch.equal(one.codes(), two.codes()) and torch.equal(one.assign, two.assign)
    other = mf.retrieval.QuantizedIndex.build(rows_600, 4, pq_iters=10, iters=2, seed=5)
    assert not torch.equal(one.codebooks, other.codebooks) and not torch.equal(one.codes(), other.codes())
    raw = mf.retrieval.QuantizedIndex.build(rows_600, 4, pq_iters=0, iters=2, seed=4)
    res = spec.residuals(rows_600.cpu().numpy(), raw.centroids.cpu().numpy(), raw.assign.cpu().numpy())
    assert np.array_equal(raw.codebooks.cpu().numpy(), spec.build_codebooks(res, 4, 0))          # the seeded rows themselves
    assert _mse(one) <= _mse(raw)
    before = one.codebooks.clone()
    one.rebuild()
    assert torch.equal(one.codebooks, before) and torch.equal(one.codes(), two.codes())
    one.refresh()
    assert one._codes is None and torch.equal(one.codes(), two.codes())


def test_codebooks_of_a_large_catalog_train_on_the_seeded_sample(mf, rows_600):
    """Above ``TRAIN_ROWS`` rows the training set is the rows at the first ``TRAIN_ROWS`` places of the seeded host permutation,
    in that order: here with the limit lowered to 300 of 600 rows, against numpy on those rows."""

    class Small(mf.retrieval.QuantizedIndex):
        TRAIN_ROWS = 300

    index = Small.build(rows_600, 4, num_sub_vectors=4, pq_iters=2, iters=2, seed=7)
    picked = torch.randperm(600, generator=torch.Generator().manual_seed(7))[:300].numpy()
    res = spec.residuals(rows_600.cpu().numpy(), index.centroids.cpu().numpy(), index.assign.cpu().numpy())
    books = spec.build_codebooks(res[picked], 4, 2)
    assert np.array_equal(index.codebooks.cpu().numpy().view(np.uint32), books.view(np.uint32))
    assert not np.array_equal(books, spec.build_codebooks(res, 4, 2)) and not np.array_equal(books, spec.build_codebooks(res[np.sort(picked)], 4, 2))
    _codes_hold(index, res, books, "sampled training")                   # all 600 rows are encoded
    whole = mf.retrieval.QuantizedIndex.build(rows_600, 4, num_sub_vectors=4, pq_iters=2, iters=2, seed=7)
    assert not torch.equal(whole.codebooks, index.codebooks)


# ----------------------------------------------------------------------------------------------------- surface ----
def _spec_of(index, q, k, nprobe, exclude, refine_factor=4):
    items = index.embeddings[:, : index.dim].cpu().numpy()
    cen, assign, books = index.centroids.cpu().numpy(), index.assign.cpu().numpy(), index.codebooks.cpu().numpy()
    codes = spec.encode(spec.residuals(items, cen, assign), books)
    return spec.search(q, items, cen, assign, books, codes, k, refine_factor, nprobe, exclude)


def test_item_processor_end_to_end(mf, rows_600):
    ids = torch.arange(600) * 3 + 11
    proc = mf.retrieval.ItemProcessor(ids, index_type="quantized", num_partitions=8, num_probes=4, index_seed=2, refine_factor=3)
    index = proc.set_index(rows_600)
    assert isinstance(index, mf.retrieval.QuantizedIndex) and (index.num_partitions, index.num_probes, index.refine_factor) == (8, 4, 3)
    same = mf.retrieval.QuantizedIndex.build(rows_600, 8, seed=2, num_probes=4, refine_factor=3)
    assert torch.equal(index.codebooks, same.codebooks) and torch.equal(index.codes(), same.codes())
    q = rows_600[7:8].cpu().numpy()
    frame = proc.search(q, exclude_item_ids=[int(ids[7]), int(ids[100]), 5], top_k=20)      # (5 is no item id: ignored)
    ws, wr = _spec_of(index, q, 20, 4, [[7, 100]], 3)
    assert frame[proc.idx_col].tolist() == wr[0].tolist() and frame[proc.id_col].tolist() == (wr[0] * 3 + 11).tolist()
    assert np.array_equal(frame["score"].to_numpy().view(np.uint32), ws[0].view(np.uint32))
    grown = proc.append([9_000_001, 9_000_002], rows_600[:2] * 0.5)
    assert isinstance(grown, mf.retrieval.QuantizedIndex) and grown.num_items == 602 and grown.refine_factor == 3
    assert grown.codes().numel() == grown.row_of.numel() * 4
    with pytest.raises(ValueError, match="index_type"):
        mf.retrieval.ItemProcessor(index_type="ivf")
    # "auto" on the exact engines never chooses the new index: the parent's search is the exact one
    exact = mf.retrieval.ItemIndex(rows_600)
    _same(mf.retrieval.ItemIndex.search(index, _dev(q), 20), exact.search(_dev(q), 20), "ItemIndex.search")


def test_module_with_a_quantized_index(mf, tmp_path):
    cfg = dict(num_users=50, num_items=600, hidden_size=64, index_type="quantized", num_partitions=8, num_probes=3, index_seed=3, top_k=20,
               num_sub_vectors=16, refine_factor=2)
    module = mf.lightning.MatrixFactorizationLitModule(cfg)
    module.configure_model(device=DEV)
    index = module.item_processor.get_index(module)
    assert isinstance(index, mf.retrieval.QuantizedIndex)
    assert (index.num_partitions, index.num_probes, index.num_sub_vectors, index.dsub, index.refine_factor) == (8, 3, 16, 4, 2)
    module.history = {4: [10, 11, 12]}
    frame = module.recommend(4, top_k=20, exclude_item_ids=[13])
    with torch.no_grad():
        q = module(torch.tensor([4], device=DEV)).cpu().numpy()
    ws, wr = _spec_of(index, q, 20, 3, [[10, 11, 12, 13]], 2)
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
    assert isinstance(again, mf.retrieval.QuantizedIndex) and (again.num_probes, again.refine_factor) == (3, 2)
    assert torch.equal(again.codebooks, index.codebooks) and torch.equal(again.codes(), index.codes()) and torch.equal(again.assign, index.assign)
    assert loaded.recommend(4, top_k=20, exclude_item_ids=[13]).equals(frame)

    # metrics_mode="positions" reads the whole catalog, whatever the index type
    users = torch.arange(1, 9, device=DEV)
    hist = (torch.arange(9, device=DEV) * 2, torch.arange(16, device=DEV) + 20)
    target = (torch.arange(9, device=DEV) * 3, torch.arange(24, device=DEV) * 7 % 600, torch.ones(24, device=DEV))
    batch = {"user": {"idx": users}, "history": hist, "target": target}
    got = {}
    for kind in ("quantized", "exact"):
        m = mf.lightning.MatrixFactorizationLitModule({**cfg, "index_type": kind, "metrics_mode": "positions"})
        m.towers = module.towers
        m.configure_model(device=DEV)
        m.item_processor.get_index(m)
        got[kind] = {k: float(v) for k, v in m.update_metrics(batch, "val").items()}
    assert got["quantized"] == got["exact"] and got["exact"]
    # and the list metrics run through the quantiser
    assert module.update_metrics(batch, "val")
    s, r = module.predict_step(batch)
    want = _spec_of(index, module(users).detach().cpu().numpy(), 20, 3, [list(range(20 + 2 * i, 22 + 2 * i)) for i in range(8)], 2)
    _same((s, r), want, "predict_step")
