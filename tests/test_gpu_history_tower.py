"""GPU: the history-pooled user tower (models.HistoryPoolingTower, mf_pool_forward / mf_pool_backward, mf_sample_history)
against the plain-torch spec of tests/test_history_tower_cpu.py, through the sparse optimisers and the Lightning module."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from oracle import data as odata, losses as ol
from tests.test_history_tower_cpu import spec_pool

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _lists(rng, n_rows, sizes):
    """Lists with padding zeros, out-of-range ids, repeats; one empty list."""
    out = []
    for k, n in enumerate(sizes):
        lst = rng.integers(1, n_rows, n).tolist()
        if n >= 4:  # noqa: PLR2004
            lst[1] = 0
            lst[2] = -3 if k % 2 else n_rows + 5
            lst[3] = lst[0]                              # a repeated item
        out.append(lst)
    out.append([])
    return out


def _segments(lists):
    off = np.cumsum([0] + [len(x) for x in lists])
    items = torch.tensor([i for x in lists for i in x] or [0], dtype=torch.int64, device=DEV)
    off = torch.tensor(off, dtype=torch.int64, device=DEV)
    return off[:-1], off[1:], items


def _padded(lists):
    width = max(1, max(len(x) for x in lists))
    pad = torch.zeros(len(lists), width, dtype=torch.int64)
    for b, x in enumerate(lists):          # right-aligned: padding in front, as zeros anywhere are padding
        if x:
            pad[b, width - len(x):] = torch.tensor(x)
    return pad.to(DEV)


def _tower(mf, n_rows, d, mode, n_i, n_u, max_history=None, seed=0):
    torch.manual_seed(seed)
    item = mf.models.EmbeddingTower(n_rows, d, normalize=n_i, device=DEV)
    return item, mf.models.HistoryPoolingTower(item, pooling_mode=mode, max_history=max_history, normalize=n_u)


@pytest.mark.parametrize("d", [32, 64, 128, 256])
@pytest.mark.parametrize("mode", ["mean", "max"])
def test_forward_matches_spec(mf, d, mode):
    rng = np.random.default_rng(d)
    n_rows = 300
    lists = _lists(rng, n_rows, [1, 5, 17, 64, 65, 200, 3])
    for n_i in (True, False):
        for n_u in (True, False):
            item, tower = _tower(mf, n_rows, d, mode, n_i, n_u)
            want = spec_pool(item.weight.detach().cpu(), lists, mode, n_i, n_u)
            for form in (_segments(lists), _padded(lists)):
                with torch.no_grad():
                    got = tower(form).cpu()
                assert torch.allclose(got, want, atol=1e-5, rtol=0), (mode, d, n_i, n_u)
                assert torch.equal(got[-1], torch.zeros(d))                        # the empty list: exactly 0
                if mode == "max" and not n_u:                # exactly the max over the kernel's own normalised rows
                    for b, lst in enumerate(lists[:-1]):
                        ids = torch.tensor([i for i in lst if 1 <= i < n_rows], device=DEV)
                        with torch.no_grad():
                            rows = item(ids)
                        assert torch.equal(got[b], rows.max(0).values.cpu()), b


@pytest.mark.parametrize("mode", ["mean", "max"])
def test_forward_long_list_and_max_history(mf, mode):
    rng = np.random.default_rng(7)
    n_rows, d = 5000, 128
    lists = [rng.integers(0, n_rows, 30000).tolist(), [3, 4], rng.integers(0, n_rows, 700).tolist(), []]
    item, tower = _tower(mf, n_rows, d, mode, True, True)
    want = spec_pool(item.weight.detach().cpu(), lists, mode, True, True)
    with torch.no_grad():
        got = tower(_segments(lists)).cpu()
    assert torch.allclose(got, want, atol=1e-5, rtol=0)
    for L in (1, 5, 64, 65, 100000):
        _, cut = _tower(mf, n_rows, d, mode, True, True, max_history=L)
        cut.item_tower.weight.data.copy_(item.weight.data)
        want = spec_pool(item.weight.detach().cpu(), lists, mode, True, True, max_history=L)
        with torch.no_grad():
            got_s = cut(_segments(lists)).cpu()
            got_p = cut(_padded(lists)).cpu()
        assert torch.allclose(got_s, want, atol=1e-5, rtol=0), L
        assert torch.allclose(got_p, want, atol=1e-5, rtol=0), L


def _dense_grad(w, lists, mode, n_i, n_u, c, extra=None):
    """Spec gradient of sum(u * c) (+ sum(item_rows(extra_ids) * c2)) w.r.t. the table, in fp64."""
    wt = w.detach().cpu().double().requires_grad_(True)
    loss = (spec_pool(wt, lists, mode, n_i, n_u) * c.double()).sum()
    if extra is not None:
        ids, c2 = extra
        r = wt[ids.cpu()]
        if n_i:
            r = torch.nn.functional.normalize(r, dim=1, eps=1e-12)
        loss = loss + (r * c2.double()).sum()
    loss.backward()
    return wt.grad


def _one_sgd_step(mf, mode, with_items, n_rows, d):
    rng = np.random.default_rng(11)
    lists = _lists(rng, n_rows, [1, 9, 33, 130, 300, 6])
    for n_i, n_u in ((True, True), (False, False), (True, False)):
        item, tower = _tower(mf, n_rows, d, mode, n_i, n_u, seed=5)
        before = item.weight.detach().clone()
        c = torch.randn(len(lists), d)
        u = tower(_segments(lists))
        loss = (u * c.to(DEV)).sum()
        extra = None
        if with_items:
            ids = torch.tensor(rng.integers(0, min(250, n_rows), 200), device=DEV)     # overlaps the lists' ids; includes row 0
            c2 = torch.randn(200, d)
            loss = loss + (item(ids) * c2.to(DEV)).sum()
            extra = (ids, c2)
        loss.backward()
        mf.optim.SparseSGD([item.weight], lr=1.0, weight_decay=0.0).step()
        want = _dense_grad(before, lists, mode, n_i, n_u, c, extra)
        delta = (before - item.weight.detach()).cpu().double()
        touched = want.abs().sum(1) > 0
        assert torch.allclose(delta[touched], want[touched], atol=1e-5, rtol=0), (mode, n_i, n_u)
        untouched = delta.abs().sum(1) == 0
        assert torch.equal(item.weight.detach().cpu()[~touched], before.cpu()[~touched]) or bool(untouched[~touched].all())
        ids_seen = {i for x in lists for i in x if 1 <= i < n_rows} | (set(extra[0].tolist()) if extra else set())
        others = torch.tensor(sorted(set(range(n_rows)) - ids_seen))
        assert torch.equal(item.weight.detach().cpu()[others], before.cpu()[others])        # bit-identical


@pytest.mark.parametrize("mode", ["mean", "max"])
@pytest.mark.parametrize("with_items", [False, True])
def test_backward_one_sgd_step(mf, mode, with_items):
    _one_sgd_step(mf, mode, with_items, 400, 64)


@pytest.mark.parametrize("mode", ["mean", "max"])
@pytest.mark.parametrize("d", [32, 256])
@pytest.mark.parametrize("n_rows", [200, 70000])
def test_backward_one_sgd_step_one_and_three_pass_tables(mf, mode, d, n_rows):
    """The same step on tables whose coalesce sorts in one and in three radix passes (400 rows: two), at the widths the
    run sums lay out differently (d = 32: eight rows per wave, d = 256: one)."""
    _one_sgd_step(mf, mode, True, n_rows, d)


def _zipf_windows(rng, n_rows, batch, mean_len):
    pop = rng.zipf(1.2, size=batch * mean_len * 2) % (n_rows - 1) + 1
    lens = np.minimum(rng.lognormal(np.log(mean_len), 1.0, batch).astype(np.int64), 3000)
    off = np.concatenate([[0], np.cumsum(lens)])
    items = pop[: off[-1]]
    return off, items


def test_backward_zipf_c3_size(mf):
    rng = np.random.default_rng(3)
    n_rows, d, batch = 62424, 128, 8192
    off, items = _zipf_windows(rng, n_rows, batch, 60)
    item, tower = _tower(mf, n_rows, d, "mean", True, True, seed=9)
    before = item.weight.detach().clone()
    c = torch.randn(batch, d, device=DEV) * 1e-2
    ids2 = torch.tensor(rng.integers(1, n_rows, 2 * batch), device=DEV)
    c2 = torch.randn(2 * batch, d, device=DEV) * 1e-2
    hist = (torch.tensor(off[:-1], device=DEV), torch.tensor(off[1:], device=DEV), torch.tensor(items, device=DEV))
    loss = (tower(hist) * c).sum() + (item(ids2) * c2).sum()
    loss.backward()
    mf.optim.SparseSGD([item.weight], lr=1.0, weight_decay=0.0).step()
    delta = (before - item.weight.detach()).double()
    # fp64 reference on 64 rows: the most popular ids and random touched ones
    counts = np.bincount(items, minlength=n_rows)
    rows = np.unique(np.concatenate([np.argsort(-counts)[:32], rng.choice(np.nonzero(counts)[0], 32, replace=False)]))
    w = before.double()
    wn = w / w.norm(dim=1, keepdim=True).clamp_min(1e-12)
    seg = torch.repeat_interleave(torch.arange(batch, device=DEV), torch.tensor(np.diff(off), device=DEV))
    it = torch.tensor(items, device=DEV)
    cnt = torch.bincount(seg, minlength=batch).double()
    p = torch.zeros(batch, d, dtype=torch.float64, device=DEV).index_add_(0, seg, wn[it]) / cnt.clamp_min(1)[:, None]
    inv = 1.0 / p.norm(dim=1, keepdim=True).clamp_min(1e-12)
    uu = p * inv
    cd = c.double()
    gp = (cd - uu * (cd * uu).sum(1, keepdim=True)) * inv                      # normalise backward
    ge = gp[seg] / cnt[seg][:, None]                                         # per entry, w.r.t. the normalised rows
    graw = torch.zeros_like(w).index_add_(0, it, ge).index_add_(0, ids2, c2.double())
    for r in rows.tolist():
        x, uh = w[r], wn[r]
        inv_r = 1.0 / x.norm().clamp_min(1e-12)
        want = (graw[r] - uh * (graw[r] * uh).sum()) * inv_r
        assert torch.allclose(delta[r], want, atol=1e-5, rtol=1e-4), r


def test_two_adam_steps_are_bit_reproducible(mf):
    rng = np.random.default_rng(5)
    n_rows, d = 3000, 128
    off, items = _zipf_windows(rng, n_rows, 512, 40)
    hist = (torch.tensor(off[:-1], device=DEV), torch.tensor(off[1:], device=DEV), torch.tensor(items, device=DEV))
    ids2 = torch.tensor(rng.integers(1, n_rows, 1024), device=DEV)
    c = torch.randn(512, d, device=DEV)
    results = []
    for _ in range(2):
        for mode in ("mean", "max"):
            item, tower = _tower(mf, n_rows, d, mode, True, True, seed=1)
            opt = mf.optim.RowAdam([item.weight], lr=1e-2)
            for _ in range(2):
                loss = (tower(hist) * c).sum() + (item(ids2) * c[:1]).sum()
                loss.backward()
                opt.step()
                opt.zero_grad()
            results.append(item.weight.detach().clone())
    assert torch.equal(results[0], results[2]) and torch.equal(results[1], results[3])


def _small_table(mf, seed=0, n_users=40, n_items=60, n=2000):
    g = torch.Generator().manual_seed(seed)
    user = torch.randint(1, n_users, (n,), generator=g)
    item = torch.randint(1, n_items, (n,), generator=g)
    rating = torch.randint(1, 6, (n,), generator=g).float()
    ts = torch.randint(0, 60 * 24 * 3600, (n,), generator=g)
    return mf.data.InteractionTable(user, item, rating, ts), (user, item, ts)


def test_sampler_windows_follow_the_batch_permutation(mf):
    table, (user, item, ts) = _small_table(mf)
    s = table.sampler(num_items=60, batch_size=64, seed=3, device=DEV, history=True)
    tr = table.sorted_train
    lo, hi = table.history_lo[tr], table.history_hi[tr]
    n = int(tr.sum())
    # oracle rolling windows, in the table's (user, time) order
    want_lists = odata.rolling_history(table.sorted_user.tolist(), table.sorted_item.tolist(), table.sorted_time.tolist(),
                                       4 * 7 * 24 * 3600)
    train_rows = torch.nonzero(tr).reshape(-1).tolist()
    for step in (0, 5, 40):
        b = s.batch(step)
        start, end, items = b["user"]["history"]
        assert items.data_ptr() == s.hist_items.data_ptr()
        for r in range(64):
            p = step * 64 + r
            e = odata.feistel_perm(p % n, n, p // n, 3)
            assert int(start[r]) == int(lo[e]) and int(end[r]) == int(hi[e])
            assert int(b["user"]["idx"][r]) == int(table.pair_user[e])
            got = items[int(start[r]):int(end[r])].tolist()
            assert got == list(want_lists[train_rows[e]]), (step, r)


def _module(mf, **over):
    cfg = {"num_users": 40, "num_items": 60, "hidden_size": 32, "learning_rate": 0.05, "user_tower": "history", **over}
    m = mf.lightning.MatrixFactorizationLitModule(cfg)
    m.configure_model(device=DEV)
    return m


@pytest.mark.parametrize("mode", ["mean", "max"])
def test_module_end_to_end(mf, mode, tmp_path):
    m = _module(mf, pooling_mode=mode, num_negatives=2, train_loss="InfomationNoiseContrastiveEstimationLoss")
    assert isinstance(m.towers["user"], mf.models.HistoryPoolingTower)
    table, _ = _small_table(mf, seed=1)
    s = table.sampler(num_items=60, batch_size=32, seed=0, device=DEV, history=True, pos_pad=64)
    batch = s.batch(0)
    out = m.compute_losses(batch)
    start, end, items = batch["user"]["history"]
    lists = [items[int(a):int(b)].tolist() for a, b in zip(start, end)]
    w = m.towers["item"].weight.detach().cpu()
    u = spec_pool(w, lists, mode, True, True)
    item_idx = torch.cat([batch["item"]["idx"], batch["neg_item"]["idx"]])
    v = torch.nn.functional.normalize(w[item_idx.cpu()], dim=1, eps=1e-12)
    want = ol.all_losses(u, v, batch["target"].cpu(), item_idx=item_idx.cpu(), pos_idx=batch["user"]["pos_idx"].cpu(), num_negatives=2)
    for k in ol.KINDS:
        assert abs(float(out[f"train/{k}"]) - float(want[k])) <= 1e-4 * max(1.0, abs(float(want[k]))), k

    # training: the ordinary three calls and the fused entry point (which falls back) both move the table
    opt = m.configure_optimizers()
    w0 = m.towers["item"].weight.detach().clone()
    loss = m.training_step(batch)
    loss.backward()
    opt.step()
    opt.zero_grad()
    assert not torch.equal(w0, m.towers["item"].weight.detach())
    w1 = m.towers["item"].weight.detach().clone()
    m.fused_training_step(s.batch(1), opt)
    assert m._fused is None and not torch.equal(w1, m.towers["item"].weight.detach())

    # metrics / predict: queries = the pooled eval history, which is also excluded
    m.on_validation_start()
    users, (h_off, h_items), target = table.eval_sets("val")
    ev = {"user": {"idx": users.to(DEV)}, "history": (h_off.to(DEV), h_items.to(DEV)),
          "target": tuple(t.to(DEV) for t in target)}
    scores, rows = m.predict_step(ev)
    w = m.towers["item"].weight.detach().cpu()
    q = spec_pool(w, [h_items[int(a):int(b)].tolist() for a, b in zip(h_off[:-1], h_off[1:])], mode, True, True)
    _, want_rows = m.item_processor.index.search(q.to(DEV), m.config.top_k, exclude_csr=ev["history"])
    assert torch.equal(rows, want_rows)
    m.update_metrics(ev, step_name="val")

    # serving a user who is in no table, history excluded; save / load round trip
    hist = [3, 7, 7, 11]
    rec = m.recommend_with_history(hist, top_k=10)
    assert not set(rec["movie_rn"].tolist()) & set(hist)
    m.history = {5: hist}
    r5 = m.recommend(5, top_k=10)
    assert rec["movie_rn"].tolist() == r5["movie_rn"].tolist()
    m.save(tmp_path / "model")
    m2 = mf.lightning.MatrixFactorizationLitModule.load(tmp_path / "model", device=DEV)
    assert m2.config.user_tower == "history" and m2.config.pooling_mode == mode
    assert isinstance(m2.towers["user"], mf.models.HistoryPoolingTower)
    assert m2.towers["user"].weight is m2.towers["item"].weight
    assert torch.equal(m2.towers["item"].weight, m.towers["item"].weight)
    assert m2.recommend_with_history(hist, top_k=10)["movie_rn"].tolist() == rec["movie_rn"].tolist()


def test_refusals(mf):
    hashed = mf.models.HashEmbeddingTower(100, 32, device=DEV)
    with pytest.raises(ValueError, match="EmbeddingTower"):
        mf.models.HistoryPoolingTower(hashed)
    with pytest.raises(ValueError, match="hashed"):
        mf.models.init_towers(mf.models.ModelConfig(user_tower="history", num_hashes=2), device=DEV)
    with pytest.raises(ValueError, match="table user towers only"):
        mf.distributed.ShardedTrainer(mf, DEV, "sgd", 0, num_users=10, num_items=10, dim=32, comm=object(), user_tower="history")
    towers = mf.models.init_towers(mf.models.ModelConfig(user_tower="history", hidden_size=32), device=DEV)
    opt = mf.optim.SparseSGD(towers.parameters(), lr=0.1)
    fn = mf.losses.PairwiseHingeLoss(num_negatives=2)
    with pytest.raises(mf._lib.MfHipError):
        mf.fused.FusedSmallStep(towers, opt, fn)
