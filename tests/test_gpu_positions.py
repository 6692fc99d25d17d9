"""GPU: exact catalog positions (``mf_target_positions``, ``ItemIndex.positions``) and the metrics read from them
(``mf_position_metrics``, ``PositionMetrics``, ``metrics_mode="positions"``) against the numpy spec (tests/_position_spec.py)
and against the engines they must agree with.  Positions and counts are compared as integers, scores as uint32 views."""
from __future__ import annotations

import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import _position_spec as spec

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 2.0 ** -22


def _unit(n, d, gen):
    return torch.nn.functional.normalize(torch.randn(n, d, generator=gen), dim=-1)


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _dev(a, dtype):
    return torch.as_tensor(np.asarray(a), dtype=dtype).to(DEV)


class Call:
    """``mf_target_positions`` through the C ABI on buffers that are kept (graph capture) and poisoned before every call."""

    def __init__(self, mf, q, items, t_off, t_ids, excl=None, idx_base=0, ws="preferred"):
        self.mf, self.lib = mf, mf._lib.lib()
        self.q, self.items = q.to(DEV).contiguous(), items.to(DEV).contiguous()
        (self.nq, self.d), self.n = self.q.shape, self.items.shape[0]
        self.off, self.ids = mf.retrieval._csr(excl, self.nq, DEV)
        self.t_off, self.nt = _dev(t_off, torch.int64), len(t_ids)
        self.t_ids = _dev(t_ids if self.nt else [0], torch.int64)
        size = self.lib.mf_target_positions_ws_bytes if ws == "preferred" else self.lib.mf_target_positions_min_ws_bytes
        self.nbytes = size(self.nq, self.n, self.d)
        self.ws = torch.empty(self.nbytes, dtype=torch.uint8, device=DEV)
        self.pos = torch.empty(max(self.nt, 1), dtype=torch.int64, device=DEV)
        self.score = torch.empty(max(self.nt, 1), dtype=torch.float32, device=DEV)
        self.ncand = torch.empty(self.nq, dtype=torch.int64, device=DEV)
        self.idx_base = idx_base

    def poison(self, word=0xA5):
        self.ws.fill_(word)
        self.pos.fill_(-7777)
        self.score.fill_(float("nan"))
        self.ncand.fill_(-7777)

    def launch(self):
        p = self.mf._lib.ptr
        self.mf._lib.check(self.lib.mf_target_positions(
            self.q.data_ptr(), self.nq, self.items.data_ptr(), self.n, self.d, self.t_off.data_ptr(), self.t_ids.data_ptr(), self.nt,
            p(self.off), p(self.ids), self.idx_base, self.ws.data_ptr(), self.nbytes, self.pos.data_ptr(), self.score.data_ptr(),
            self.ncand.data_ptr(), self.mf._lib.stream_ptr()))

    def result(self):
        return self.pos[: self.nt].cpu().numpy(), self.score[: self.nt].cpu().numpy(), self.ncand.cpu().numpy()

    def __call__(self, word=0xA5):
        self.poison(word)
        self.launch()
        return self.result()


def _same(got, want, what=""):
    assert np.array_equal(got[0], want[0]), (what, "positions")
    assert np.array_equal(_bits(got[1]), _bits(want[1])), (what, "scores")
    assert np.array_equal(got[2], want[2]), (what, "ncand")


# ------------------------------------------------------------------------------------------------------- the cases ----
KINDS = 10


def _target_list(kind, order, n, base, excl_r, rng):
    """Global target rows of one query, chosen through the spec's order so that the cases are certain."""
    glob = lambda rows: [int(y) + base for y in rows]       # noqa: E731
    top = order[:1024]

    def draw(m):                                            # half of them from the best 1024, so a deep list holds most
        if order.size == 0:
            return glob(rng.integers(0, n, m))
        return glob(np.where(rng.random(m) < 0.5, rng.choice(top, m), rng.integers(0, n, m)))

    special = [order[p] for p in (0, 1, 63, 64, 1023, 1024, order.size - 1) if 0 <= p < order.size]
    special = glob(special) + [base, base + n - 1]          # ... and column 0 and column N - 1
    special += [excl_r[0]] if len(excl_r) else []           # on the exclusion list: -1
    special += [base + n, base - 1, special[0]]             # out of range on both sides: -1; a duplicate
    if kind == 0:
        assert len(special) <= 16
        return special
    if kind == 1:
        return []
    if kind == 7:
        return glob(rng.choice(order[:5] if order.size else np.arange(min(n, 5)), 40))      # 40 entries, at most 5 different rows
    if kind == 8:
        return special + draw(30)
    return draw({2: 1024, 3: 1025, 4: 1, 5: 16, 6: 17, 9: 300}[kind])


@functools.lru_cache(maxsize=None)
def _world(nq, n, d, base=0, seed=0, first_kind=0):
    """Queries, catalog, exclusion lists (global rows, some outside the catalog) and one target list of every kind in turn;
    the spec's answer, computed once and shared."""
    g = torch.Generator().manual_seed(1000 * d + n + nq + seed)
    rng = np.random.default_rng(1000 * d + n + nq + seed)
    q, items = _unit(nq, d, g), _unit(n, d, g)
    items[10] = items[3]                                    # an exact score tie in every query
    excl = [sorted(set(rng.integers(base - 3, base + n + 3, int(rng.integers(0, 60))).tolist())) for _ in range(nq)]
    scores = spec.chain.scores(q.numpy(), items.numpy())
    orders = spec.orders(scores, excl, base)
    lists = [_target_list((first_kind + r) % KINDS, orders[r], n, base, [y for y in excl[r] if base <= y < base + n], rng) for r in range(nq)]
    t_off = np.cumsum([0] + [len(x) for x in lists])
    t_ids = np.array([y for x in lists for y in x], dtype=np.int64)
    want = spec.positions_from_scores(scores, t_off, t_ids, excl, base)
    return q, items, excl, t_off, t_ids, want, orders


@pytest.mark.parametrize("nq", [1, 33, 70])
@pytest.mark.parametrize("n", [33, 1000, 2500])
@pytest.mark.parametrize("d", [32, 64, 128, 256])
def test_positions_equal_the_spec(mf, d, n, nq):
    first = (d // 32 + n) % KINDS if nq == 1 else 0          # one query: another kind of list per shape
    q, items, excl, t_off, t_ids, want, _ = _world(nq, n, d, first_kind=first)
    _same(Call(mf, q, items, t_off, t_ids, excl)(), want)
    if nq > 1:
        mine = want[0][: t_off[1]].tolist()                  # query 0 holds the special places
        assert -1 in mine and 0 in mine and int(want[2][0]) - 1 in mine


@pytest.mark.parametrize("kind", range(KINDS))
def test_every_kind_of_list_alone(mf, kind):
    """One query, so a pass count, the few-entries path or an empty list cannot hide behind another query's."""
    q, items, excl, t_off, t_ids, want, _ = _world(1, 2500, 64, seed=kind, first_kind=kind)
    assert len(t_ids) == {1: 0, 2: 1024, 3: 1025, 4: 1, 5: 16, 6: 17, 7: 40, 9: 300}.get(kind, len(t_ids))
    if kind in (0, 8):
        assert {0, 1, 63, 64, 1023, 1024, int(want[2][0]) - 1, -1} <= set(want[0].tolist())
    _same(Call(mf, q, items, t_off, t_ids, excl)(), want, kind)


@pytest.mark.parametrize("base", [0, 7])
def test_three_query_blocks_on_the_minimum_workspace(mf, base):
    nq, n, d = 70, 1000, 64
    lib = mf._lib.lib()
    plan = (ctypes.c_int64 * 3)()
    assert lib.mf_topk_deep_plan(nq, n, d, 1, lib.mf_target_positions_min_ws_bytes(nq, n, d), plan) == 0 and (plan[0], plan[1]) == (32, 3)
    q, items, excl, t_off, t_ids, want, _ = _world(nq, n, d, base=base)
    if base:
        assert any(e and e[0] < base for e in excl) and any(e and e[-1] >= base + n for e in excl)
    small = Call(mf, q, items, t_off, t_ids, excl, idx_base=base, ws="minimum")()
    _same(small, want)
    _same(Call(mf, q, items, t_off, t_ids, excl, idx_base=base)(), small)


# ----------------------------------------------------------------------------------------------------------- ties ----
def test_a_run_of_identical_rows_is_ordered_by_row(mf):
    g = torch.Generator().manual_seed(5)
    n, d = 1500, 64
    q, items = _unit(3, d, g), 0.3 * _unit(n, d, g)
    run = torch.randperm(n, generator=g)[:300].sort().values
    items[run] = 0.5 * q[0]
    t_ids = run[[0, 1, 150, 298, 299]].tolist() + run.tolist() + [int(run[7])] * 3
    t_off = [0, 5, 5 + 300, len(t_ids)]
    want = spec.positions(q.numpy(), items.numpy(), t_off, t_ids)
    first = want[0][0]
    assert want[0][:5].tolist() == [first, first + 1, first + 150, first + 298, first + 299]      # consecutive places, ascending rows
    _same(Call(mf, q, items, t_off, t_ids)(), want)


def test_a_zero_query_places_every_row_at_its_own_number(mf):
    n, d = 1100, 32
    items = _unit(n, d, torch.Generator().manual_seed(6))
    excl = [[0, 2, 5], []]
    t_ids = [1, 3, 4, 6, n - 1, 2] + list(range(0, n, 3))
    t_off = [0, 6, len(t_ids)]
    pos, score, ncand = Call(mf, torch.zeros(2, d), items, t_off, t_ids, excl)()
    assert pos[:6].tolist() == [0, 1, 2, 3, n - 4, -1] and pos[6:].tolist() == list(range(0, n, 3)) and ncand.tolist() == [n - 3, n]
    assert (_bits(score[:5]) == 0).all() and np.isneginf(score[5]) and (_bits(score[6:]) == 0).all()      # +0.0


# ------------------------------------------------------------------------------------------------- exclusion lists ----
def test_everything_excluded_but_three_rows(mf):
    g = torch.Generator().manual_seed(7)
    n, d = 2000, 64
    q, items = _unit(3, d, g), _unit(n, d, g)
    left = [17, 1203, 1999]
    excl = [[y for y in range(n) if y not in left], list(range(n)), []]
    t_ids = left + [5] + left + list(range(20))
    t_off = [0, 4, 7, len(t_ids)]
    want = spec.positions(q.numpy(), items.numpy(), t_off, t_ids, excl)
    assert sorted(want[0][:3].tolist()) == [0, 1, 2] and want[0][3:7].tolist() == [-1] * 4 and want[2].tolist() == [3, 0, n]
    _same(Call(mf, q, items, t_off, t_ids, excl)(), want)


def test_no_exclusion_lists_at_all(mf):
    q, items, _, t_off, t_ids, _, _ = _world(33, 1000, 128)
    want = spec.positions(q.numpy(), items.numpy(), t_off, t_ids)
    assert (want[2] == 1000).all()
    _same(Call(mf, q, items, t_off, t_ids, None)(), want)


# --------------------------------------------------------------------------------------- the engine it must agree with ----
@pytest.mark.parametrize("shape", [(33, 1000, 64), (70, 2500, 128)], ids=lambda s: "x".join(map(str, s)))
def test_positions_agree_with_the_deep_search(mf, shape):
    nq, n, d = shape
    q, items, excl, t_off, t_ids, _, _ = _world(nq, n, d)
    index = mf.retrieval.ItemIndex(items.to(DEV))
    pos, score, ncand = index.positions(q.to(DEV), (_dev(t_off, torch.int64), _dev(t_ids, torch.int64)), exclude=excl)
    s, rows = index.search(q.to(DEV), 1024, exclude=excl, path="deep")
    pos, score, s, rows = pos.cpu().numpy(), score.cpu().numpy(), s.cpu().numpy(), rows.cpu().numpy()
    assert np.array_equal((rows >= 0).sum(axis=1), np.minimum(ncand.cpu().numpy(), 1024))
    inside = 0
    for r in range(nq):
        listed = set(rows[r][rows[r] >= 0].tolist())
        for e in range(t_off[r], t_off[r + 1]):
            if 0 <= pos[e] < 1024:
                inside += 1
                assert rows[r, pos[e]] == t_ids[e] and _bits(s[r, pos[e]]) == _bits(score[e]), (r, e)
            else:
                assert int(t_ids[e]) not in listed, (r, e)
    assert inside >= len(t_ids) / 2 and len(t_ids) > 1000, (inside, len(t_ids))       # most targets are checked by value
    assert ("positions", nq) in index._ws                    # the workspace is kept like the searches'


def test_positions_surface_takes_the_searches_checks_and_padding(mf):
    g = torch.Generator().manual_seed(3)
    q, items = _unit(6, 48, g), _unit(700, 48, g)             # dim 48: padded to 64 by ItemIndex
    index = mf.retrieval.ItemIndex(items.to(DEV))
    rng = np.random.default_rng(3)
    excl = [sorted(set(rng.integers(0, 700, 30).tolist())) for _ in range(6)]
    t_off, t_ids = np.arange(0, 6 * 25 + 1, 25), rng.integers(0, 700, 150)
    pad = lambda x: torch.nn.functional.pad(x, (0, 16)).numpy()   # noqa: E731
    want = spec.positions(pad(q), pad(items), t_off, t_ids, excl)
    csr = (_dev(t_off, torch.int64), _dev(t_ids, torch.int64))
    got = index.positions(q.to(DEV), csr, exclude=excl)
    _same(tuple(x.cpu().numpy() for x in got), want)
    as_csr = index.positions(q.to(DEV), csr, exclude_csr=mf.retrieval._csr(excl, 6, DEV))
    assert all(torch.equal(a, b) for a, b in zip(got, as_csr))
    empty = index.positions(q.to(DEV), (torch.zeros(7, dtype=torch.int64, device=DEV), torch.zeros(0, dtype=torch.int64, device=DEV)))
    assert empty[0].numel() == 0 and empty[1].numel() == 0 and empty[2].tolist() == [700] * 6
    with pytest.raises(ValueError, match="queries should be"):
        index.positions(torch.zeros(6, 64, device=DEV), csr)
    with pytest.raises(ValueError, match="one target list per query"):
        index.positions(q[:5].to(DEV), csr)
    with pytest.raises(mf.MfHipError, match="no CPU path"):
        index.positions(q, csr)


# -------------------------------------------------------------------------------------------------------- metrics ----
@functools.lru_cache(maxsize=None)
def _metric_world():
    """Positions of the (70, 2500, 128) world (every kind of list, -1 among them) with ratings 0 .. 5."""
    _, _, _, t_off, t_ids, want, _ = _world(70, 2500, 128)
    rel = np.random.default_rng(3).integers(0, 6, len(t_ids)).astype(np.float32)
    rel[t_off[8]: t_off[8] + 5] = 0.0
    rel[t_off[5]: t_off[6]] = 0.0                           # a list without a relevant target
    return want[0], t_off, rel, want[2]


def _check_metrics(got, want, t_off, nk):
    n = np.diff(t_off)[:, None]
    tol = (n + 4) * EPS
    cut = np.r_[0: 6 * nk, 6 * nk, 6 * nk + 2]              # every value in [0, 1]: the per-k ones, MRR and AUC
    err = np.abs(got[:, cut] - want[:, cut])
    assert (err <= tol).all(), (err.max(), np.unravel_index(np.argmax(err - tol), err.shape))
    mp = 6 * nk + 1
    assert (np.abs(got[:, mp] - want[:, mp]) <= EPS * np.abs(want[:, mp])).all()


@pytest.mark.parametrize("ks", [(20,), (1, 20, 100, 5000)], ids=str)
def test_position_metrics_equal_the_spec(mf, ks):
    pos, t_off, rel, ncand = _metric_world()
    want = spec.metrics(pos, t_off, rel, ncand, ks)
    assert (want[:, -3:] > 0).any() and (want[5] == 0).all() and want[1].sum() == 0 and (pos == -1).any()
    metric = mf.retrieval.PositionMetrics(ks, prefix="val/")
    args = (_dev(pos, torch.int64), _dev(t_off, torch.int64), _dev(rel, torch.float32), _dev(ncand, torch.int64))
    got = metric.update(*args).cpu().numpy().astype(np.float64)
    assert got.shape == (70, 6 * len(ks) + 3)
    _check_metrics(got, want, t_off, len(ks))
    again = metric.update(*args).cpu().numpy()
    assert np.array_equal(_bits(again), _bits(got.astype(np.float32)))
    means = metric.compute()
    assert list(means) == ["val/" + x for x in metric.names] and metric._n == 140
    np.testing.assert_allclose([float(v) for v in means.values()], got.mean(axis=0), rtol=1e-6, atol=1e-7)


@pytest.mark.parametrize("k", [20, 100])
def test_position_metrics_equal_the_list_metrics_where_both_are_defined(mf, k):
    """Every target admissible and distinct, at least k admissible rows: the six @k values of mf_retrieval_metrics on the
    deep search's rows."""
    nq, n, d = 33, 1000, 64
    q, items, excl, _, _, _, orders = _world(nq, n, d)
    rng = np.random.default_rng(k)
    lists = [np.unique(np.r_[rng.choice(o[:k], 3), rng.choice(o, int(rng.integers(1, 40)))]) for o in orders]      # some of the best k
    t_off = np.cumsum([0] + [len(x) for x in lists])
    t_ids, rel = np.concatenate(lists), rng.integers(0, 6, t_off[-1]).astype(np.float32)
    index = mf.retrieval.ItemIndex(items.to(DEV))
    csr = (_dev(t_off, torch.int64), _dev(t_ids, torch.int64))
    pos, _, ncand = index.positions(q.to(DEV), csr, exclude=excl)
    assert int(pos.min()) >= 0 and int(ncand.min()) >= k and int((pos < k).sum()) >= nq
    got = mf.retrieval.PositionMetrics(k).update(pos, csr[0], _dev(rel, torch.float32), ncand).cpu().numpy()
    _, rows = index.search(q.to(DEV), k, exclude=excl, path="deep")
    want = mf.retrieval.RetrievalMetrics(k).update(rows, csr[0], csr[1], _dev(rel, torch.float32)).cpu().numpy()
    assert (np.abs(got[:, :6].astype(np.float64) - want) <= (np.diff(t_off)[:, None] + 4) * EPS).all()


# ------------------------------------------------------------------------------------- determinism, capture, poison ----
def test_repeat_calls_capture_and_poisoned_buffers(mf):
    q, items, excl, t_off, t_ids, want, _ = _world(70, 2500, 128)
    call = Call(mf, q, items, t_off, t_ids, excl)
    first = call(0xA5)
    _same(first, want)                                       # nothing of the poison is left: -7777 and NaN are no answers
    _same(call(0x00), first)
    _same(call(0xFF), first)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call.launch()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call.launch()
    for word in (0x5A, 0x00):
        call.poison(word)
        graph.replay()
        torch.cuda.synchronize()
        _same(call.result(), first)


# ---------------------------------------------------------------------------------------------------------- module ----
def _module_batch(mf, cfg):
    rng = np.random.default_rng(12)
    users, items = cfg["num_users"], cfg["num_items"]
    pairs = rng.choice((users - 1) * (items - 1), 3000, replace=False)       # distinct (user, item) pairs, rows 1 ..
    table = mf.data.InteractionTable(pairs // (items - 1) + 1, pairs % (items - 1) + 1, rng.integers(0, 6, pairs.size).astype(np.float32),
                                     rng.integers(0, 10**6, pairs.size))
    who, hist, target = table.eval_sets("val")
    return {"user": {"idx": who.to(DEV)}, "history": tuple(t.to(DEV) for t in hist), "target": tuple(t.to(DEV) for t in target)}


def test_module_logs_the_same_six_and_the_three_new_values(mf, tmp_path):
    cfg = {"num_users": 80, "num_items": 400, "hidden_size": 64, "top_k": 20}
    lit = mf.lightning.MatrixFactorizationLitModule
    topk, posm = lit(cfg), lit({**cfg, "metrics_mode": "positions", "eval_ks": [100, 5000]})
    logged = {}
    for name, m in (("topk", topk), ("positions", posm)):
        m.configure_model(device=DEV)
        if m is posm:
            m.towers.load_state_dict(topk.towers.state_dict())
        m.on_validation_start()
        m.log_dict = functools.partial(logged.__setitem__, name)
    batch = _module_batch(mf, cfg)
    with torch.no_grad():                                   # plant hits: a user's vector points at some of its targets
        t_off, t_ids, _ = batch["target"]
        for r, u in enumerate(batch["user"]["idx"].tolist()):
            own = t_ids[int(t_off[r]): int(t_off[r + 1])][:3]
            if own.numel():
                for m in (topk, posm):
                    m.towers["user"].weight[u] = m.towers["item"].weight[own].sum(dim=0)
    topk.validation_step(batch, 0)
    posm.validation_step(batch, 0)
    names = mf.retrieval.METRIC_NAMES
    assert list(logged["topk"]) == ["val/" + n for n in names]                                    # what it returns today
    assert list(logged["positions"]) == (["val/" + n for n in names] + [f"val/{n}@{k}" for k in (100, 5000) for n in names]
                                         + ["val/MRR", "val/MeanPosition", "val/AUC"])
    t_off, t_ids, rel = (t.cpu().numpy() for t in batch["target"])
    tol = (np.diff(t_off).max() + 4) * EPS
    for n in names:
        assert abs(float(logged["topk"]["val/" + n]) - float(logged["positions"]["val/" + n])) <= tol, n
    assert float(logged["positions"]["val/RetrievalHitRate"]) > 0.5
    index = posm.item_processor.index
    h_off, h_items = (t.cpu().numpy() for t in batch["history"])
    excl = [h_items[a:b].tolist() for a, b in zip(h_off[:-1], h_off[1:])]
    with torch.no_grad():
        queries = posm(batch["user"]["idx"], tower="user").cpu().numpy()
    pos, _, ncand = spec.positions(queries, index.embeddings.cpu().numpy(), t_off, t_ids, excl)
    want = spec.metrics(pos, t_off, rel, ncand, (20, 100, 5000)).mean(axis=0)
    got = np.array([float(v) for v in logged["positions"].values()])
    assert (np.abs(got[:18] - want[:18]) <= tol).all() and abs(got[18] - want[18]) <= tol and abs(got[20] - want[20]) <= tol
    assert abs(got[19] - want[19]) <= EPS * want[19] and want[19] > 0
    posm.save(tmp_path / "model")
    back = lit.load(tmp_path / "model", device=DEV)
    assert back.config == posm.config and back.config.metrics_mode == "positions" and back.config.eval_ks == [100, 5000]
    assert isinstance(back.metrics["val"], mf.retrieval.PositionMetrics) and back.metrics["test"].ks == (20, 100, 5000)
