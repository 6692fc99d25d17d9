"""GPU: the deep top-k engine (csrc/mf_topk_deep.hip, ``ItemIndex.search(path="deep")``, 1 <= k <= 1024) and the metrics
kernel for 64 < k <= 1024.  Scores are compared as uint32 views and rows as integers: equal, never close."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

from oracle import chain, retrieval as oretr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _unit(n, d, gen):
    return torch.nn.functional.normalize(torch.randn(n, d, generator=gen), dim=-1)


def _random_lists(nq, n, gen, lo=0):
    return [sorted(set(torch.randint(lo, lo + n, (int(torch.randint(0, 60, (1,), generator=gen)),), generator=gen).tolist()))
            for _ in range(nq)]


def _same(got, want, what=""):
    (gs, gi), (ws, wi) = got, want
    gs, gi = (x.cpu().numpy() if isinstance(x, torch.Tensor) else x for x in (gs, gi))
    assert np.array_equal(gi, wi), what
    assert np.array_equal(np.ascontiguousarray(gs).view(np.uint32), np.ascontiguousarray(ws).view(np.uint32)), what


def _call(mf, q, items, k, excl=None, idx_base=0, ws="preferred", fill=None):
    """mf_topk_deep through the C ABI on a workspace of the preferred or the minimum size, optionally pre-filled."""
    csr = mf.retrieval._csr
    lib = mf._lib.lib()
    qd, it = q.to(DEV).contiguous(), items.to(DEV).contiguous()
    (nq, d), n = qd.shape, it.shape[0]
    off, ids = csr(excl, nq, DEV)
    nbytes = (lib.mf_topk_deep_ws_bytes if ws == "preferred" else lib.mf_topk_deep_min_ws_bytes)(nq, n, d, k)
    w = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    if fill is not None:
        w.fill_(fill)
    s = torch.empty(nq, k, device=DEV)
    i = torch.empty(nq, k, dtype=torch.int64, device=DEV)
    mf._lib.check(lib.mf_topk_deep(qd.data_ptr(), nq, it.data_ptr(), n, d, k, mf._lib.ptr(off), mf._lib.ptr(ids), idx_base,
                                   w.data_ptr(), nbytes, s.data_ptr(), i.data_ptr(), mf._lib.stream_ptr()))
    return s, i


def _orderable(s):
    u = np.ascontiguousarray(s, dtype=np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))


def _expect(scores, k, excl=None):
    """Top-k of given fp32 scores [Q, N] by the key of include/mf_numerics.h (rank << 32 | ~row), in numpy."""
    nq, n = scores.shape
    keys = (_orderable(scores).astype(np.uint64) << np.uint64(32)) | (~np.arange(n, dtype=np.uint32)).astype(np.uint64)
    out_s, out_i = np.full((nq, k), -np.inf, np.float32), np.full((nq, k), -1, np.int64)
    for r in range(nq):
        kr = keys[r]
        if excl is not None and len(excl[r]):
            kr = np.delete(kr, np.asarray(excl[r], dtype=np.int64))
        top = np.sort(kr)[::-1][:k]
        rows = (~(top & np.uint64(0xFFFFFFFF)).astype(np.uint32)).astype(np.int64)
        out_i[r, : top.size] = rows
        out_s[r, : top.size] = scores[r, rows]
    return out_s, out_i


# ------------------------------------------------------------------------------------------------ 1. the oracle ----
@pytest.mark.parametrize("cfg", [(50, 5000, 64, 100), (1, 3883, 64, 1000), (33, 1000, 128, 65), (7, 300, 32, 128), (40, 2500, 256, 1024),
                                 (130, 4100, 32, 200), (3, 1030, 128, 1024), (5, 90, 64, 100)], ids=lambda c: "x".join(map(str, c)))
def test_deep_topk_bit_exact(mf, cfg):
    nq, n, d, k = cfg
    g = torch.Generator().manual_seed(n)
    q, items = _unit(nq, d, g), _unit(n, d, g)
    items[10] = items[3]                                   # exact score ties -> lowest row first
    excl = _random_lists(nq, n, g)
    want = chain.topk(q.numpy(), items.numpy(), k, excl)
    if k > n:
        assert (want[1][:, n:] == -1).all() and np.isneginf(want[0][:, n:]).all()      # every row is padded
    index = mf.retrieval.ItemIndex(items.to(DEV))
    _same(index.search(q.to(DEV), k, exclude=excl, path="deep"), want)


def test_deep_topk_with_nearly_everything_excluded(mf):
    g = torch.Generator().manual_seed(1)
    nq, n, d, k = 4, 2000, 64, 100
    q, items = _unit(nq, d, g), _unit(n, d, g)
    left = sorted(torch.randperm(n, generator=g)[:10].tolist())
    excl = [[], [r for r in range(n) if r not in left], [5], list(range(n))]           # all but 10 rows; and all of them
    want = chain.topk(q.numpy(), items.numpy(), k, excl)
    got = mf.retrieval.ItemIndex(items.to(DEV)).search(q.to(DEV), k, exclude=excl, path="deep")
    _same(got, want)
    assert sorted(got[1][1, :10].tolist()) == left and (got[1][1, 10:] == -1).all() and (got[1][3] == -1).all()
    assert torch.isneginf(got[0][1, 10:]).all()


def test_deep_topk_idx_base_through_the_c_abi(mf):
    g = torch.Generator().manual_seed(2)
    nq, n, d, k, base = 9, 1500, 64, 130, 1000
    q, items = _unit(nq, d, g), _unit(n, d, g)
    excl = _random_lists(nq, n + 1000, g, lo=base - 500)    # global ids on both sides of [base, base + n)
    assert any(e and e[0] < base for e in excl) and any(e and e[-1] >= base + n for e in excl)
    local = [[y - base for y in e if base <= y < base + n] for e in excl]
    ws, wi = chain.topk(q.numpy(), items.numpy(), k, local)
    _same(_call(mf, q, items, k, excl, idx_base=base), (ws, np.where(wi >= 0, wi + base, -1)))


# --------------------------------------------------------------------------------------- 2. the existing engines ----
@pytest.mark.parametrize("shape", [(150, 20000, 128), (7, 300, 32)], ids=lambda c: "x".join(map(str, c)))
def test_deep_agrees_with_the_tile_engine(mf, shape):
    nq, n, d = shape
    g = torch.Generator().manual_seed(d)
    q, items = _unit(nq, d, g).to(DEV), _unit(n, d, g)
    items[10] = items[3]
    excl = _random_lists(nq, n, g)
    index = mf.retrieval.ItemIndex(items.to(DEV))
    tiles = {k: index.search(q, k, exclude=excl, path="tiles") for k in (64, 33, 1)}
    for k, (ts, ti) in tiles.items():
        ds, di = index.search(q, k, exclude=excl, path="deep")
        assert torch.equal(di, ti) and torch.equal(ds.view(torch.int32), ts.view(torch.int32)), k
    ds, di = index.search(q, 1024, exclude=excl, path="deep")                  # the prefix property
    assert torch.equal(di[:, :64], tiles[64][1]) and torch.equal(ds[:, :64].view(torch.int32), tiles[64][0].view(torch.int32))


# ------------------------------------------------------------------------------------------ 3. several query blocks ----
def test_deep_query_blocks_give_the_same_result(mf):
    nq, n, d, k = 130, 4100, 64, 300
    lib = mf._lib.lib()
    out = (ctypes.c_int64 * 3)()
    assert lib.mf_topk_deep_plan(nq, n, d, k, lib.mf_topk_deep_min_ws_bytes(nq, n, d, k), out) == 0
    assert (out[0], out[1]) == (32, 5) and 5 * 32 > nq                        # five blocks, the last one ragged (2 queries)
    assert lib.mf_topk_deep_plan(nq, n, d, k, lib.mf_topk_deep_ws_bytes(nq, n, d, k), out) == 0 and out[1] == 1
    g = torch.Generator().manual_seed(7)
    q, items = _unit(nq, d, g), _unit(n, d, g)
    items[10] = items[3]
    excl = _random_lists(nq, n, g)
    many = _call(mf, q, items, k, excl, ws="minimum")
    one = _call(mf, q, items, k, excl, ws="preferred")
    assert torch.equal(many[1], one[1]) and torch.equal(many[0], one[0])
    want = chain.topk(q.numpy(), items.numpy(), k, excl)
    _same(many, want)
    _same(one, want)


# ----------------------------------------------------------------------------------------------- 4. radix boundaries ----
def _radix_world():
    """d = 32, one-hot queries +-e0, items[:, 0] = chosen normal floats: a score is exactly that float (times the sign; a
    zero of either sign gives +0.0, as the chain's fmaf(a, b, +0.0) does)."""
    n = 5000
    lo = 0x3F80FD00                                        # 1536 consecutive patterns across 0x3F80FFFF -> 0x3F810000: bytes 1 and 2 of the rank carry
    a = (np.arange(1536, dtype=np.uint32) + np.uint32(lo)).view(np.float32)
    tiny = (np.arange(64, dtype=np.uint32) + np.uint32(0x00800000)).view(np.float32)       # the smallest normals: next to the sign
    vals = np.concatenate([a, -a, np.zeros(5, np.float32), -np.zeros(5, np.float32), tiny, -tiny])
    col = np.full(n, -3.0, np.float32)
    perm = np.random.default_rng(11).permutation(n)
    col[perm[: vals.size]] = vals
    rows_a = np.sort(perm[:1536])
    rows_tiny_pos = np.sort(perm[2 * 1536 + 10: 2 * 1536 + 10 + 64])
    rows_low = np.sort(perm[vals.size:])                   # the rows left at the low constant: the best ones for -e0, so excluded there
    items = np.zeros((n, 32), np.float32)
    items[:, 0] = col
    q = np.zeros((4, 32), np.float32)
    q[:, 0] = (1.0, 1.0, -1.0, 1.0)
    # query 0: the cut inside the positive run; 1: the run excluded -> tiny positives, zeros (ties), tiny negatives, the negated
    # run; 2: the negated run from the other side; 3: the cut between the signs
    excl = [[], rows_a.tolist(), rows_low.tolist(), sorted(rows_a.tolist() + rows_tiny_pos[:40].tolist())]
    scores = (q[:, :1] * col[None, :]) + np.float32(0.0)
    return q, items, excl, scores.astype(np.float32)


@pytest.mark.parametrize("k", [65, 256, 257, 1024])
def test_deep_radix_boundaries(mf, k):
    q, items, excl, scores = _radix_world()
    want = _expect(scores, k, excl)
    assert (want[1] >= 0).all()
    if k == 65:
        assert want[0][1, 63] > 0 and want[0][1, 64] == 0 and want[0][3, 23] > 0 and want[0][3, 34] < 0     # the cuts are where they are meant to be
    if k == 256:
        _same(chain.topk(q, items, k, excl), want, "numpy keys against the oracle")
    _same(mf.retrieval.ItemIndex(torch.from_numpy(items).to(DEV)).search(torch.from_numpy(q).to(DEV), k, exclude=excl, path="deep"), want)


# ----------------------------------------------------------------------------------------------- 5. ties at the cut ----
@pytest.mark.parametrize("k", [100, 1024])
def test_deep_zero_queries_take_the_lowest_rows(mf, k):
    n, d = 6000, 64
    items = _unit(n, d, torch.Generator().manual_seed(5))
    excl = [[0, 2, 5], [], list(range(40)), [n - 1]]
    s, i = mf.retrieval.ItemIndex(items.to(DEV)).search(torch.zeros(4, d, device=DEV), k, exclude=excl, path="deep")
    for r, e in enumerate(excl):
        assert i[r].tolist() == [y for y in range(n) if y not in set(e)][:k], r
    assert (s.view(torch.int32) == 0).all()                 # +0.0


def test_deep_two_score_levels(mf):
    n, d, k = 6000, 32, 1000
    items = torch.zeros(n, d)
    items[::7, 0] = 1.0
    q = torch.zeros(2, d)
    q[:, 0] = 1.0
    upper, lower = list(range(0, n, 7)), [y for y in range(n) if y % 7]
    assert len(upper) == 858
    excl = [[], upper[3:40:5] + lower[:100:3] + lower[500:520]]
    s, i = mf.retrieval.ItemIndex(items.to(DEV)).search(q.to(DEV), k, exclude=excl, path="deep")
    assert i[0].tolist() == upper + lower[:142]
    assert s[0].tolist() == [1.0] * 858 + [0.0] * 142
    up1, lo1 = [y for y in upper if y not in set(excl[1])], [y for y in lower if y not in set(excl[1])]
    assert i[1].tolist() == up1 + lo1[: k - len(up1)]
    _same((s, i), _expect((q @ items.T).numpy(), k, excl))


@pytest.mark.parametrize("k", [100, 1024])
def test_deep_cut_inside_duplicates(mf, k):
    g = torch.Generator().manual_seed(9)
    n, d = 6000, 64
    q, items = _unit(2, d, g), 0.3 * _unit(n, d, g)
    perm = torch.randperm(n, generator=g)
    above, dups = perm[:50], perm[50:3050].sort().values
    items[above] = q[0] * torch.linspace(0.6, 0.9, 50)[:, None]
    items[dups] = 0.5 * q[0]
    want = chain.topk(q.numpy(), items.numpy(), k, None)
    assert want[1][0, 50:].tolist() == dups[: k - 50].tolist()                 # the lowest duplicates win
    _same(mf.retrieval.ItemIndex(items.to(DEV)).search(q.to(DEV), k, path="deep"), want)


# ---------------------------------------------------------------------------------- 6. workspace and determinism ----
def test_deep_ignores_what_the_workspace_held(mf):
    nq, n, d, k = 50, 5000, 64, 100
    g = torch.Generator().manual_seed(n)
    q, items = _unit(nq, d, g), _unit(n, d, g)
    items[10] = items[3]
    excl = _random_lists(nq, n, g)
    ones = _call(mf, q, items, k, excl, fill=0xFF)
    zeros = _call(mf, q, items, k, excl, fill=0)
    again = _call(mf, q, items, k, excl, fill=0)
    short = _call(mf, q, items, k, excl, ws="minimum", fill=0xFF)
    for other in (zeros, again, short):
        assert torch.equal(ones[1], other[1]) and torch.equal(ones[0], other[0])
    _same(ones, chain.topk(q.numpy(), items.numpy(), k, excl))


# ------------------------------------------------------------------------------------------------------ 7. metrics ----
@pytest.mark.parametrize("k", [65, 100, 1024])
def test_deep_retrieval_metrics_match_oracle(mf, k):
    g = torch.Generator().manual_seed(k)
    q, n_items = 97, 3000
    topk = torch.stack([torch.randperm(n_items, generator=g)[:k] for _ in range(q)])
    topk[3, k // 2:] = -1                                     # a query with fewer than k results
    targets, off, ids, rel = [], [0], [], []
    for r in range(q):
        m = int(torch.randint(0, 40, (1,), generator=g)) if r != 5 else 0        # query 5: no targets
        own = torch.randperm(n_items, generator=g)[:m].tolist()
        if m and r % 2 == 0:                                  # make sure some targets are retrieved
            own[: min(m, 3)] = topk[r, : min(m, 3)].tolist()
        if r == 7:                                            # only hits at ranks >= 64: the first ranks of a lane's second round
            own = topk[r, [64, k - 1]].tolist()
        if r == 9 and k > 130:                                # hits on both sides of a 64-rank round
            own = topk[r, [2, 63, 64, 127, 128, k - 1]].tolist()
        own = [i for i in dict.fromkeys(own) if i >= 0]
        rat = torch.randint(0, 6, (len(own),), generator=g).tolist()   # rating 0: listed but not relevant
        if r in (7, 9):
            rat = [max(x, 1) for x in rat]
        targets.append(dict(zip(own, map(float, rat))))
        ids += own
        rel += rat
        off.append(len(ids))
    metric = mf.retrieval.RetrievalMetrics(top_k=k, prefix="val/")
    got = metric.update(topk.to(DEV), torch.tensor(off, device=DEV), torch.tensor(ids, dtype=torch.int64, device=DEV),
                        torch.tensor(rel, dtype=torch.float32, device=DEV)).cpu().numpy()
    want = oretr.retrieval_metrics(topk.numpy(), targets, k)
    assert want[7, 5] == 1.0 / 65 and want[5].sum() == 0
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(float(metric.compute()["val/RetrievalNormalizedDCG"]), want[:, 0].mean(), rtol=1e-5)


# ------------------------------------------------------------------------------------------------------ 8. surface ----
def test_search_surface_serves_deep_k(mf):
    g = torch.Generator().manual_seed(3)
    q, items = _unit(6, 48, g), _unit(700, 48, g)             # dim 48: padded to 64 by ItemIndex
    index = mf.retrieval.ItemIndex(items.to(DEV))
    excl = _random_lists(6, 700, g)
    auto = index.search(q.to(DEV), 100, exclude=excl)
    deep = index.search(q.to(DEV), 100, exclude=excl, path="deep")
    assert torch.equal(auto[0], deep[0]) and torch.equal(auto[1], deep[1])
    pad = lambda x: torch.nn.functional.pad(x, (0, 16)).numpy()   # noqa: E731
    _same(deep, chain.topk(pad(q), pad(items), 100, excl))
    assert ("deep", 6, 100) in index._ws                      # the workspace is kept like the others'
    for path in ("tiles", "scan", "bf16"):
        with pytest.raises(mf.MfHipError):                    # one wavefront holds a row's result there: k <= 64 as before
            index.search(q.to(DEV), 100, path=path)
    with pytest.raises(mf.MfHipError, match="k = 1025 outside 1..1024"):
        index.search(q.to(DEV), 1025)
    with pytest.raises(ValueError, match="'deep'"):
        index.search(q.to(DEV), 100, path="deeper")
    proc = mf.retrieval.ItemProcessor(item_ids=torch.arange(1000, 1700))
    proc.set_index(items.to(DEV))
    df = proc.search(q[0].numpy()[None, :], exclude_item_ids=[1003, 1004], top_k=100)
    assert list(df.columns) == [proc.idx_col, proc.id_col, "score"] and len(df) == 100
    assert not set(df[proc.id_col]) & {1003, 1004} and df["score"].is_monotonic_decreasing
    assert (df[proc.id_col] == df[proc.idx_col] + 1000).all()


def test_module_validates_at_top_k_100(mf):
    m = mf.lightning.MatrixFactorizationLitModule({"num_users": 500, "num_items": 800, "hidden_size": 64, "learning_rate": 0.05,
                                                   "top_k": 100})
    m.configure_model(device=DEV)
    m.on_validation_start()
    g = torch.Generator().manual_seed(4)
    users = torch.arange(1, 41)
    n_items = m.towers["item"].num_embeddings
    hist = [torch.randperm(n_items, generator=g)[: int(torch.randint(0, 30, (1,), generator=g))].sort().values for _ in users]
    tgts = [dict(zip(torch.randperm(n_items, generator=g)[:12].tolist(), torch.randint(1, 6, (12,), generator=g).float().tolist()))
            for _ in users]
    with torch.no_grad():                               # plant hits: a user's vector points at some of its targets
        iw = m.towers["item"].weight
        for r, t in enumerate(tgts):
            m.towers["user"].weight[users[r]] = iw[list(t)[:3]].sum(dim=0)
    csr = lambda lists: (torch.tensor([0] + list(np.cumsum([len(x) for x in lists])), device=DEV),  # noqa: E731
                         torch.cat([torch.as_tensor(list(x), dtype=torch.int64) for x in lists]).to(DEV))
    t_off, t_ids = csr([list(t) for t in tgts])
    t_rel = torch.tensor([v for t in tgts for v in t.values()], device=DEV)
    batch = {"user": {"idx": users.to(DEV)}, "history": csr(hist), "target": (t_off, t_ids, t_rel)}
    m.validation_step(batch, 0)
    got = m.metrics["val"].compute()
    _, rows = m.predict_step(batch, 0)
    assert rows.shape == (40, 100) and not any(set(rows[r].tolist()) & set(hist[r].tolist()) for r in range(len(users)))
    want = oretr.retrieval_metrics(rows.cpu().numpy(), tgts, 100).mean(axis=0)
    np.testing.assert_allclose([float(v) for v in got.values()], want, rtol=1e-5, atol=1e-6)
    assert float(got["val/RetrievalHitRate"]) > 0.5
    m.history[7] = [3, 4, 5]
    df = m.recommend(7, top_k=100, exclude_item_ids=[6])
    assert len(df) == 100 and not set(df["movie_id"]) & {3, 4, 5} and 6 not in set(df["movie_id"]) and df["score"].is_monotonic_decreasing
