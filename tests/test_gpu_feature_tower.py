"""GPU: the hashed feature-bag towers (models.FeatureBagTower, mf_bag_forward / mf_bag_backward) against the plain-torch
spec of tests/test_feature_tower_cpu.py, through the sparse optimisers, a captured step, a cold-start retrieval world and
the Lightning module."""
from __future__ import annotations

import json

import numpy as np
import pytest
import torch

from oracle import losses as ol
from tests.test_feature_tower_cpu import spec_bag

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
COMBINERS = ("sum", "mean", "sqrtn")


def _lists(rng, R, sizes, weighted):
    """Ragged bags with padding tokens (0, >= R), repeats, one empty bag; weights in [0, 2) with zeros."""
    lists, weights = [], []
    for k, n in enumerate(sizes):
        lst = rng.integers(1, R, n).tolist()
        if n >= 4:  # noqa: PLR2004
            lst[1] = 0
            lst[2] = R + 3 + k
            lst[3] = lst[0]
        lists.append(lst)
        w = (rng.random(n) * 2).astype(np.float32).tolist()
        if n >= 5:  # noqa: PLR2004
            w[4] = 0.0
        weights.append(w)
    return lists, (weights if weighted else None)


def _tower(mf, R, d, combiner, normalize, seed=0, share_with=None):
    torch.manual_seed(seed)
    return mf.models.FeatureBagTower(R, d, combiner=combiner, normalize=normalize, device=DEV, share_with=share_with)


@pytest.mark.parametrize("d", [32, 64, 128, 256])
@pytest.mark.parametrize("combiner", COMBINERS)
@pytest.mark.parametrize("weighted", [False, True])
def test_forward_matches_spec(mf, d, combiner, weighted):
    rng = np.random.default_rng(d + 7 * weighted)
    R = 700
    for sizes in ([1, 3, 7, 0, 12, 64, 2], [1, 65, 130, 0, 9, 5000, 64]):       # the short path, then the chunked path
        lists, weights = _lists(rng, R, sizes, weighted)
        bags = mf.data.FeatureBags.from_lists(lists, weights)
        for normalize in (True, False):
            tower = _tower(mf, R, d, combiner, normalize)
            tower.set_bags(bags)
            w = tower.weight.detach().cpu().double()
            ids = [0, 1, 2, 3, 4, 5, 6, -1, len(lists), 5, 2]                    # out-of-range entity ids: empty bags
            sel = [lists[i] if 0 <= i < len(lists) else [] for i in ids]
            selw = None if weights is None else [weights[i] if 0 <= i < len(lists) else [] for i in ids]
            want = spec_bag(w, sel, selw, combiner, normalize).float()
            with torch.no_grad():
                got = tower(torch.tensor(ids, device=DEV)).cpu()
                got_e = tower.embed(bags).cpu()
            tol = 1e-5 * (1.0 if normalize else max(1.0, float(want.abs().max())))
            assert torch.allclose(got, want, atol=tol, rtol=0), (sizes, normalize, (got - want).abs().max())
            assert torch.allclose(got_e, want[: len(lists)], atol=tol, rtol=0)
            for k in (3, 7, 8):
                assert torch.equal(got[k], torch.zeros(d))                      # empty: exactly 0
            assert torch.equal(got[9], got[5]) and torch.equal(got[10], got[2])  # the order depends on the bag only


def _dense_grad(w, parts):
    """fp64 spec gradient of sum_k sum(spec_bag(parts_k) * c_k) w.r.t. the table."""
    wt = w.detach().cpu().double().requires_grad_(True)
    loss = sum((spec_bag(wt, lists, weights, comb, norm) * c.double().cpu()).sum() for lists, weights, comb, norm, c in parts)
    loss.backward()
    return wt.grad


def _one_sgd_step(mf, combiner, shared, R, d):
    rng = np.random.default_rng(11)
    lists, weights = _lists(rng, R, [1, 9, 33, 0, 130, 6, 2], True)
    lists2, _ = _lists(rng, R, [4, 4, 20, 1], False)
    for normalize in (True, False):
        item = _tower(mf, R, d, combiner, normalize, seed=5)
        item.set_bags(mf.data.FeatureBags.from_lists(lists, weights))
        before = item.weight.detach().clone()
        idx = [0, 1, 2, 3, 4, 5, 6, 2, 9]
        c = torch.randn(len(idx), d, device=DEV)
        loss = (item(torch.tensor(idx, device=DEV)) * c).sum()
        parts = [([lists[i] if i < len(lists) else [] for i in idx], [weights[i] if i < len(lists) else [] for i in idx],
                  combiner, normalize, c)]
        if shared:                               # the user tower on the same table: one coalesced list
            user = _tower(mf, R, d, combiner, normalize, share_with=item)
            user.set_bags(mf.data.FeatureBags.from_lists(lists2))
            c2 = torch.randn(4, d, device=DEV)
            loss = loss + (user(torch.tensor([3, 2, 1, 0], device=DEV)) * c2).sum()
            parts.append(([lists2[i] for i in (3, 2, 1, 0)], None, combiner, normalize, c2))
        loss.backward()
        mf.optim.SparseSGD([item.weight], lr=1.0, weight_decay=0.0).step()
        want = _dense_grad(before, parts)
        delta = (before - item.weight.detach()).cpu().double()
        assert torch.allclose(delta, want, atol=1e-5, rtol=1e-5), (combiner, normalize, (delta - want).abs().max())
        seen = {t for p in parts for x in p[0] for t in x if 1 <= t < R}
        others = torch.tensor(sorted(set(range(R)) - seen))
        assert torch.equal(item.weight.detach().cpu()[others], before.cpu()[others])   # bit-identical


@pytest.mark.parametrize("combiner", COMBINERS)
@pytest.mark.parametrize("shared", [False, True])
def test_backward_one_sgd_step(mf, combiner, shared):
    _one_sgd_step(mf, combiner, shared, 400, 64)


@pytest.mark.parametrize(("R", "d", "combiner"), [(200, 32, "sum"), (200, 256, "mean"), (70000, 32, "sqrtn"), (70000, 256, "sum"),
                                                  (1 << 20, 32, "mean"), (1 << 20, 256, "sqrtn")])
def test_backward_one_sgd_step_one_and_three_pass_tables(mf, R, d, combiner):
    """The same step (both towers on one table) on tables whose coalesce sorts in one and in three radix passes (400
    buckets: two), up to the documented maximum of 2^20 buckets, at d = 32 and d = 256."""
    _one_sgd_step(mf, combiner, True, R, d)


def _catalog(rng, n_ent, R, hot_frac=0.4):
    """C3-shaped bags: 1-12 title tokens + 1-3 genre tokens; token 1 (the hot genre) in hot_frac of the bags."""
    lists = [[]]
    for _ in range(1, n_ent):
        toks = rng.integers(100, R, int(rng.integers(1, 13))).tolist() + rng.integers(2, 30, int(rng.integers(0, 3))).tolist()
        if rng.random() < hot_frac:
            toks.append(1)
        lists.append(toks)
    return lists


def test_backward_c3_size_hot_token(mf):
    rng = np.random.default_rng(3)
    R, d, n_ent, B = 65535, 128, 62424, 16384
    lists = _catalog(rng, n_ent, R)
    bags = mf.data.FeatureBags.from_lists(lists)
    item = _tower(mf, R, d, "mean", True, seed=9)
    item.set_bags(bags)
    before = item.weight.detach().clone()
    idx = torch.tensor(rng.integers(0, n_ent, B), device=DEV)
    c = torch.randn(B, d, device=DEV) * 1e-2
    (item(idx) * c).sum().backward()
    mf.optim.SparseSGD([item.weight], lr=1.0, weight_decay=0.0).step()
    delta = (before - item.weight.detach()).double()
    # fp64 restatement on the device
    off = bags.off.to(DEV)
    lo, ln = off[idx], off[idx + 1] - off[idx]
    seg = torch.repeat_interleave(torch.arange(B, device=DEV), ln)
    pos = torch.arange(int(ln.sum()), device=DEV) - torch.repeat_interleave(torch.cumsum(ln, 0) - ln, ln) + lo[seg]
    tok = bags.tokens.to(DEV)[pos]
    w = before.double()
    cnt = torch.bincount(seg, minlength=B).double()
    p = torch.zeros(B, d, dtype=torch.float64, device=DEV).index_add_(0, seg, w[tok]) / cnt.clamp_min(1)[:, None]
    inv = 1.0 / p.norm(dim=1, keepdim=True).clamp_min(1e-12)
    u = p * inv
    cd = c.double()
    gp = (cd - u * (cd * u).sum(1, keepdim=True)) * inv
    want = torch.zeros_like(w).index_add_(0, tok, gp[seg] / cnt[seg][:, None])
    touched = torch.zeros(R, dtype=torch.bool, device=DEV)
    touched[tok] = True
    assert float((tok == 1).double().mean()) > 0.02                       # the hot token is there ...
    assert int((tok == 1).sum()) > 0.35 * B                               # ... in ~40 % of the bags
    assert torch.allclose(delta[touched], want[touched], atol=1e-5, rtol=1e-4), (delta[touched] - want[touched]).abs().max()
    assert torch.equal(item.weight.detach()[~touched], before[~touched])


def test_two_adam_steps_are_bit_reproducible(mf):
    rng = np.random.default_rng(5)
    R, d = 3000, 128
    lists = _catalog(rng, 2000, R)
    ulists = _catalog(rng, 500, R, hot_frac=0.6)
    idx = torch.tensor(rng.integers(0, 2000, 1024), device=DEV)
    uidx = torch.tensor(rng.integers(0, 500, 512), device=DEV)
    c = torch.randn(1024, d, device=DEV)
    results = []
    for _ in range(2):
        for shared in (False, True):
            item = _tower(mf, R, d, "sqrtn", True, seed=1)
            item.set_bags(mf.data.FeatureBags.from_lists(lists))
            user = _tower(mf, R, d, "sqrtn", True, share_with=item) if shared else None
            if user is not None:
                user.set_bags(mf.data.FeatureBags.from_lists(ulists))
            opt = mf.optim.RowAdam([item.weight], lr=1e-2)
            for _ in range(2):
                loss = (item(idx) * c).sum()
                if user is not None:
                    loss = loss + (user(uidx) * c[:512]).sum()
                loss.backward()
                opt.step()
                opt.zero_grad()
            results.append(item.weight.detach().clone())
    assert torch.equal(results[0], results[2]) and torch.equal(results[1], results[3])
    assert not torch.equal(results[0], results[1])


def _step_fn(mf, towers, opt, loss_fn):
    def fn(batch):
        u = towers["user"](batch["user"])
        v = towers["item"](batch["item"])
        loss = loss_fn(u, v, batch["target"], item_idx=batch["item"], pos_idx=batch["pos"])
        loss.backward()
        opt.step()
        opt.zero_grad()
        return loss.detach()
    return fn


def test_captured_step_replays_bit_identically(mf):
    rng = np.random.default_rng(2)
    n_users, n_items, R, d, B = 300, 800, 4096, 64, 128
    lists, ulists = _catalog(rng, n_items, R), _catalog(rng, n_users, R)

    def batch(k):
        g = torch.Generator().manual_seed(k)
        item = torch.randint(1, n_items, (2 * B,), generator=g)
        pos = torch.randint(1, n_items, (B, 4), generator=g)
        pos[:, 0] = item[:B]
        return {"user": torch.randint(1, n_users, (B,), generator=g).to(DEV), "item": item.to(DEV),
                "target": torch.randint(1, 6, (B,), generator=g).to(DEV), "pos": pos.to(DEV)}

    out = []
    for captured in (False, True):
        cfg = mf.models.ModelConfig(num_users=n_users, num_items=n_items, hidden_size=d, user_tower="features",
                                    item_tower="features", feature_buckets=R)
        torch.manual_seed(0)
        towers = mf.models.init_towers(cfg, device=DEV)
        towers["item"].set_bags(mf.data.FeatureBags.from_lists(lists))
        towers["user"].set_bags(mf.data.FeatureBags.from_lists(ulists))
        opt = mf.optim.RowAdam(towers.parameters(), lr=1e-2)
        fn = _step_fn(mf, towers, opt, mf.losses.InfomationNoiseContrastiveEstimationLoss(num_negatives=0))
        losses = []
        if captured:
            step = mf.graph.CapturedStep(fn, batch(0), optimizers=[opt], warmup=3)
            losses += [float(step(batch(k))) for k in (1, 2, 3)]
        else:
            for _ in range(3):
                fn(batch(0))
            losses += [float(fn(batch(k))) for k in (1, 2, 3)]
        torch.cuda.synchronize()
        out.append((towers["item"].weight.detach().clone(), losses))
    assert torch.equal(out[0][0], out[1][0])
    assert out[0][1] == out[1][1]


def _cold_world(seed=0, n_items=2001, n_users=300, n_genres=10, vocab=300):
    rng = np.random.default_rng(seed)
    genre = np.arange(n_items) % n_genres
    texts = [None] + [json.dumps({"title": " ".join(f"w{x}" for x in rng.integers(0, vocab, rng.integers(1, 6))),
                                  "genres": [f"g{genre[i]}"]}) for i in range(1, n_items)]
    items = np.arange(1, n_items)
    held = np.sort(rng.choice(items, (n_items - 1) // 5, replace=False))
    train = np.setdiff1d(items, held)
    ugenre = np.arange(n_users) % n_genres
    return rng, genre, texts, train, held, ugenre


def _train_cold(mf, item_tower, steps=300, B=256):
    rng, genre, texts, train, held, ugenre = _cold_world()
    n_users, n_items = len(ugenre), len(texts)
    m = mf.lightning.MatrixFactorizationLitModule({"num_users": n_users, "num_items": n_items, "hidden_size": 32,
                                                   "learning_rate": 0.02, "item_tower": item_tower, "feature_buckets": 4096})
    torch.manual_seed(0)
    m.configure_model(device=DEV)
    if item_tower == "features":          # the training catalogue only: held-out items are not registered
        reg = [texts[i] if i in set(train.tolist()) else None for i in range(n_items)]
        m.set_features(item=reg)
    opt = m.configure_optimizers()
    by_genre = [train[genre[train] == g] for g in range(10)]
    fn = mf.losses.InfomationNoiseContrastiveEstimationLoss(num_negatives=0)
    for _ in range(steps):
        users = rng.integers(0, n_users, B)
        items = np.array([rng.choice(by_genre[ugenre[u]]) for u in users])
        it = torch.tensor(items, device=DEV)
        loss = fn(m.towers["user"](torch.tensor(users, device=DEV)), m.towers["item"](it), torch.full((B,), 5, device=DEV),
                  item_idx=it, pos_idx=it[:, None])
        loss.backward()
        opt.step()
        opt.zero_grad()
    return m, genre, texts, held, ugenre


@pytest.mark.parametrize("item_tower", ["features", "table"])
def test_cold_start_retrieves_the_users_genre(mf, item_tower):
    m, genre, texts, held, ugenre = _train_cold(mf, item_tower)
    with torch.no_grad():
        if item_tower == "features":
            m.on_validation_start()                                   # index of the registered catalogue
            n0 = m.item_processor.index.embeddings.shape[0]
            m.add_items([int(i) + 10_000 for i in held], [texts[i] for i in held])
            emb = m.item_processor.index.embeddings[n0:, :32]
            assert emb.shape[0] == len(held)
            assert m.item_processor.row_of(int(held[0]) + 10_000) == n0
        else:
            emb = m.towers["item"](torch.tensor(held, device=DEV))       # never-trained rows
        q = m.towers["user"](torch.arange(len(ugenre), device=DEV))
        top = (q @ emb.T).topk(20, dim=1).indices.cpu().numpy()
    hit = (genre[held[top]] == ugenre[:, None]).mean()
    if item_tower == "features":
        assert hit >= 0.8, hit  # noqa: PLR2004
    else:
        assert hit <= 0.3, hit  # noqa: PLR2004


def _small_table(mf, seed=0, n_users=40, n_items=60, n=2000):
    g = torch.Generator().manual_seed(seed)
    user = torch.randint(1, n_users, (n,), generator=g)
    item = torch.randint(1, n_items, (n,), generator=g)
    rating = torch.randint(1, 6, (n,), generator=g).float()
    ts = torch.randint(0, 60 * 24 * 3600, (n,), generator=g)
    return mf.data.InteractionTable(user, item, rating, ts)


USER = {"gender": "F", "age": 25, "occupation": 3, "zipcode": "10012"}


def test_module_end_to_end(mf, tmp_path):
    n_users, n_items = 40, 60
    item_texts, _ = mf.data.synthetic_item_features(n_items, num_genres=6, vocab=50, seed=2)
    rng = np.random.default_rng(0)
    user_texts = [None] + [json.dumps({"gender": "MF"[k % 2], "age": int(rng.choice([1, 18, 25, 35])),
                                       "occupation": int(rng.integers(0, 21)), "zipcode": f"{rng.integers(10000, 99999)}"})
                           for k in range(1, n_users)]
    cfg = {"num_users": n_users, "num_items": n_items, "hidden_size": 32, "learning_rate": 0.05, "user_tower": "features",
           "item_tower": "features", "feature_buckets": 1000, "feature_combiner": "sqrtn", "num_negatives": 2,
           "train_loss": "InfomationNoiseContrastiveEstimationLoss"}
    m = mf.lightning.MatrixFactorizationLitModule(cfg)
    m.configure_model(device=DEV)
    m.set_features(item=item_texts, user=user_texts)
    assert m.towers["user"].weight is m.towers["item"].weight
    s = _small_table(mf, seed=1).sampler(num_items=n_items, batch_size=32, seed=0, device=DEV, pos_pad=64)
    batch = s.batch(0)
    out = m.compute_losses(batch)
    h = m.feature_hasher()
    w = m.towers["item"].weight.detach().cpu()
    u = spec_bag(w, h.bags([user_texts[i] for i in batch["user"]["idx"].tolist()]).lists(), None, "sqrtn", True)
    item_idx = torch.cat([batch["item"]["idx"], batch["neg_item"]["idx"]])
    v = spec_bag(w, h.bags([item_texts[i] for i in item_idx.tolist()]).lists(), None, "sqrtn", True)
    want = ol.all_losses(u, v, batch["target"].cpu(), item_idx=item_idx.cpu(), pos_idx=batch["user"]["pos_idx"].cpu(), num_negatives=2)
    for k in ol.KINDS:
        assert abs(float(out[f"train/{k}"]) - float(want[k])) <= 1e-4 * max(1.0, abs(float(want[k]))), k

    opt = m.configure_optimizers()
    w0 = m.towers["item"].weight.detach().clone()
    loss = m.training_step(batch)
    loss.backward()
    opt.step()
    opt.zero_grad()
    assert not torch.equal(w0, m.towers["item"].weight.detach())
    w1 = m.towers["item"].weight.detach().clone()
    m.fused_training_step(s.batch(1), opt)                           # falls back to the three calls
    assert m._fused is None and not torch.equal(w1, m.towers["item"].weight.detach())

    m.on_validation_start()
    assert m.item_processor.index.embeddings.shape[0] == n_items
    new_texts = ['{"title":"Brand New Film (2031)","genres":["g0","g3"]}', '{"title":"w3 w4 (1999)","genres":["g1"]}']
    m.add_items([5001, 5002], new_texts)
    rec = m.recommend_with_text(json.dumps(USER, separators=(",", ":")), top_k=10)
    assert rec.equals(m.recommend_with_text(USER, top_k=10))
    assert len(rec) == 10  # noqa: PLR2004
    rec_u = m.recommend(3, top_k=10)
    m.save(tmp_path / "model")
    m2 = mf.lightning.MatrixFactorizationLitModule.load(tmp_path / "model", device=DEV)
    assert m2.config.item_tower == "features" and m2.config.feature_combiner == "sqrtn"
    assert m2.towers["user"].weight is m2.towers["item"].weight
    assert torch.equal(m2.towers["item"].weight, m.towers["item"].weight)
    assert m2.recommend_with_text(USER, top_k=10).equals(rec)
    assert m2.recommend(3, top_k=10)["movie_rn"].tolist() == rec_u["movie_rn"].tolist()
    more = ['{"title":"Another One (2032)","genres":["g2"]}']
    m.add_items([5003], more)
    m2.add_items([5003], more)
    assert m2.recommend_with_text(USER, top_k=12).equals(m.recommend_with_text(USER, top_k=12))
    m2.on_validation_start()                                          # the added items are registered bags now
    assert m2.item_processor.index.embeddings.shape[0] == n_items + 3
    assert torch.equal(m2.item_processor.index.embeddings, m.item_processor.index.embeddings)


def test_refusals_and_fallbacks(mf, tmp_path):
    m = mf.lightning.MatrixFactorizationLitModule({"num_users": 10, "num_items": 10, "hidden_size": 32})
    m.configure_model(device=DEV)
    m.on_validation_start()
    with pytest.raises(ValueError, match="item_tower='features'"):
        m.add_items([100], ['{"title":"x","genres":[]}'])
    with pytest.raises(ValueError, match="user_tower='features'"):
        m.recommend_with_text(USER)
    with pytest.raises(ValueError, match="item_tower='features'"):
        m.set_features(item=[None])
    m.save(tmp_path / "plain")                                       # a directory without feature towers still loads
    m2 = mf.lightning.MatrixFactorizationLitModule.load(tmp_path / "plain", device=DEV)
    assert torch.equal(m2.towers["user"].weight, m.towers["user"].weight)
    with pytest.raises(ValueError, match="table user towers only"):
        mf.distributed.ShardedTrainer(mf, DEV, "sgd", 0, num_users=10, num_items=10, dim=32, comm=object(), user_tower="features")
    towers = mf.models.init_towers(mf.models.ModelConfig(item_tower="features", hidden_size=32, feature_buckets=100), device=DEV)
    with pytest.raises(ValueError, match="set_bags first"):
        towers["item"](torch.tensor([1], device=DEV))
    opt = mf.optim.SparseSGD(towers.parameters(), lr=0.1)
    with pytest.raises(mf._lib.MfHipError):
        mf.fused.FusedSmallStep(towers, opt, mf.losses.PairwiseHingeLoss(num_negatives=2))
    with pytest.raises(mf._lib.MfHipError, match="feature-table rows"):
        lib = mf._lib.lib()
        z = torch.zeros(4, dtype=torch.int64, device=DEV)
        f = torch.zeros(4, 32, device=DEV)
        mf._lib.check(lib.mf_bag_forward(f.data_ptr(), (1 << 20) + 1, 32, None, 1, z.data_ptr(), z.data_ptr(), 1, z.data_ptr(), 4,
                                         None, 1, 1, 1, f.data_ptr(), f.data_ptr(), f.data_ptr(), f.data_ptr(), 1024, None))
