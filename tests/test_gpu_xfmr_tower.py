"""GPU: the transformer user tower (models.HistoryTransformerTower; mf_xfmr_forward / mf_xfmr_backward / mf_xfmr_coalesce)
against the plain-torch spec of tests/test_xfmr_tower_cpu.py and the BertModel fixture, through the optimisers and the module.

Tolerance (every comparison): the reference is the spec run in fp64; the fp32 CPU spec's own error against it on the same
inputs is measured in the same test, and the kernels may err up to 8 x that plus 1e-7, per tensor, in max-abs over the
max-abs of the fp64 value.  Every figure is printed before it is asserted (``pytest -s``)."""
from __future__ import annotations

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.test_xfmr_tower_cpu import load_fixture, random_state, spec_tower

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FACTOR = 8.0


def _check(name: str, got: torch.Tensor, spec32: torch.Tensor, ref64: torch.Tensor) -> float:
    """The rule of the module docstring; returns kernel error / fp32-spec error."""
    ref = ref64.double().cpu()
    scale = max(float(ref.abs().max()), 1e-30) if ref.numel() else 1.0
    e_k = float((got.double().cpu() - ref).abs().max()) / scale if ref.numel() else 0.0
    e_s = float((spec32.double().cpu() - ref).abs().max()) / scale if ref.numel() else 0.0
    ratio = e_k / e_s if e_s > 0 else (0.0 if e_k == 0 else float("inf"))
    print(f"  {name}: kernel {e_k:.3e}  fp32 spec {e_s:.3e}  ratio {ratio:.2f}")
    assert e_k <= FACTOR * e_s + 1e-7, (name, e_k, e_s)
    return ratio


def _segments(lists):
    off = np.cumsum([0] + [len(x) for x in lists])
    items = torch.tensor([i for x in lists for i in x] or [0], dtype=torch.int64, device=DEV)
    off = torch.tensor(off, dtype=torch.int64, device=DEV)
    return off[:-1], off[1:], items


def _padded(lists):
    width = max(1, max(len(x) for x in lists))
    pad = torch.zeros(len(lists), width, dtype=torch.int64)
    for b, x in enumerate(lists):
        if x:
            pad[b, width - len(x):] = torch.tensor(x)
    return pad.to(DEV)


def _lists(rng, n_rows, sizes):
    """Lists with padding zeros, out-of-range ids and repeats; one empty list at the end."""
    out = []
    for k, n in enumerate(sizes):
        lst = rng.integers(1, n_rows, n).tolist()
        if n >= 4:  # noqa: PLR2004
            lst[1] = 0
            lst[2] = -3 if k % 2 else n_rows + 5
            lst[3] = lst[0]
        out.append(lst)
    out.append([])
    return out


def _towers(mf, w, sd, *, heads, act, mode, L, n_i=True, n_u=True):
    rows, h = w.shape
    layers = sum(k.endswith("attention.self.query.weight") for k in sd)
    item = mf.models.EmbeddingTower(rows, h, normalize=n_i, device=DEV)
    with torch.no_grad():
        item.weight.copy_(w.float())
    user = mf.models.HistoryTransformerTower(item, num_hidden_layers=layers, num_attention_heads=heads,
                                             intermediate_size=sd["encoder.layer.0.intermediate.dense.weight"].shape[0], hidden_act=act,
                                             max_position_embeddings=sd["embeddings.position_embeddings.weight"].shape[0],
                                             pooling_mode=mode, max_history=L, normalize=n_u)
    user.load_state_dict({k: v.float() for k, v in sd.items()})
    return item, user


def _world(seed, rows, h, layers, inter, max_pos, pos_std=None):
    g = torch.Generator().manual_seed(seed)
    sd = random_state(g, h, layers, inter, max_pos, pos_std=pos_std, dtype=torch.float64)
    w = torch.randn(rows, h, generator=g, dtype=torch.float64) / h ** 0.5
    return w, sd


# covering subset of d x heads x L x mode x layers x act (every value of every axis appears; both input forms)
FORWARD_CASES = [
    (32, 4, 1, "mean", 1, "gelu", 32), (32, 1, 7, "max", 2, "relu", 64), (32, 2, 16, "cls", 1, "silu", 128), (32, 4, 64, "mean", 2, "gelu_new", 32),
    (64, 4, 16, "max", 1, "gelu", 64), (64, 8, 64, "cls", 2, "relu", 256), (64, 1, 7, "mean", 1, "silu", 96), (64, 2, 1, "max", 2, "gelu_new", 64),
    (128, 4, 64, "max", 1, "gelu", 128), (128, 8, 16, "mean", 2, "relu", 512), (128, 16, 7, "cls", 1, "silu", 64), (128, 2, 1, "mean", 2, "gelu_new", 32),
]


@pytest.mark.parametrize(("d", "heads", "L", "mode", "layers", "act", "inter"), FORWARD_CASES)
def test_forward_matches_spec(mf, d, heads, L, mode, layers, act, inter):
    rng = np.random.default_rng(d + L)
    rows = 300
    w, sd = _world(d + heads, rows, d, layers, inter, 64)
    lists = _lists(rng, rows, [1, 5, 17, 64, 65, 130, 3, 9])
    sd32 = {k: v.float() for k, v in sd.items()}
    for n_i, n_u, padded in ((True, True, False), (False, True, True), (True, False, True), (False, False, False)):
        _, user = _towers(mf, w, sd, heads=heads, act=act, mode=mode, L=L, n_i=n_i, n_u=n_u)
        with torch.no_grad():
            got = user(_padded(lists) if padded else _segments(lists))
        kw = {"heads": heads, "act": act, "mode": mode, "n_i": n_i, "n_u": n_u, "max_history": L}
        ref = spec_tower(w, lists, sd, **kw)
        s32 = spec_tower(w.float(), lists, sd32, **kw)
        assert torch.equal(got[-1].cpu(), torch.zeros(d))                    # the empty list
        _check(f"u d={d} heads={heads} L={L} {mode} layers={layers} {act} n_i={n_i} n_u={n_u} padded={padded}", got, s32, ref)


def _spec_step(w, sd, lists, c, kw, extra, lr, dtype):
    """(u, table delta of one SGD step, dense gradients) of sum(u . c) [+ sum(v . c2)] through the spec, in ``dtype``."""
    wl = w.to(dtype).clone().requires_grad_(True)
    leaf = {k: v.to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    u = spec_tower(wl, lists, leaf, **kw)
    loss = (u * c.to(dtype)).sum()
    if extra is not None:
        ids, c2 = extra
        v = wl[ids]
        loss = loss + ((F.normalize(v, dim=1, eps=1e-12) if kw["n_i"] else v) * c2.to(dtype)).sum()
    loss.backward()
    delta = (wl.detach() - lr * wl.grad) - wl.detach()
    return u.detach(), delta, {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaf.items()}


def _kernel_step(mf, w, sd, hist, c, kw, extra, lr):
    item, user = _towers(mf, w, sd, heads=kw["heads"], act=kw["act"], mode=kw["mode"], L=kw["max_history"], n_i=kw["n_i"], n_u=kw["n_u"])
    u = user(hist)
    loss = (u * c.float().to(DEV)).sum()
    if extra is not None:
        ids, c2 = extra
        loss = loss + (item(ids.to(DEV)) * c2.float().to(DEV)).sum()
    loss.backward()
    before = item.weight.detach().clone()
    mf.optim.SparseSGD([item.weight], lr=lr).step()
    return u.detach(), item.weight.detach() - before, {k: p.grad for k, p in user.named_parameters()}


BACKWARD_CASES = [(32, 4, 16, "mean", 1, "gelu", 32), (64, 8, 7, "max", 2, "relu", 128), (128, 4, 64, "cls", 1, "silu", 256),
                  (64, 1, 64, "mean", 2, "gelu_new", 64), (128, 16, 1, "max", 1, "gelu", 512)]


@pytest.mark.parametrize("with_items", [False, True])
@pytest.mark.parametrize(("d", "heads", "L", "mode", "layers", "act", "inter"), BACKWARD_CASES)
def test_backward_one_sgd_step(mf, d, heads, L, mode, layers, act, inter, with_items):
    rng = np.random.default_rng(d * 3 + L)
    rows = 200
    w, sd = _world(d + L, rows, d, layers, inter, 64)
    lists = _lists(rng, rows, [1, 5, 17, 64, 70, 3, 9, 30])
    g = torch.Generator().manual_seed(d)
    c = torch.randn(len(lists), d, generator=g, dtype=torch.float64)
    extra = (torch.randint(0, rows, (40,), generator=g), torch.randn(40, d, generator=g, dtype=torch.float64)) if with_items else None
    kw = {"heads": heads, "act": act, "mode": mode, "n_i": True, "n_u": True, "max_history": L}
    lr = 0.5
    u64, d64, g64 = _spec_step(w, sd, lists, c, kw, extra, lr, torch.float64)
    u32, d32, g32 = _spec_step(w, sd, lists, c, kw, extra, lr, torch.float32)
    for padded in (False, True):
        u, delta, grads = _kernel_step(mf, w, sd, _padded(lists) if padded else _segments(lists), c, kw, extra, lr)
        print(f"d={d} heads={heads} L={L} {mode} layers={layers} {act} I={inter} items={with_items} padded={padded}")
        _check("u", u, u32, u64)
        _check("table step", delta, d32, d64)
        for k in g64:
            assert grads[k] is not None, k
            _check(k, grads[k], g32[k], g64[k])


def test_fixture_outputs_and_gradients(mf):
    """BertModel's own numbers: the fixture's fp32 values are the thing measured against the fp64 spec."""
    z, cfg, sd, fix_grads = load_fixture()
    x = torch.from_numpy(z["inputs_embeds"])
    mask = torch.from_numpy(z["mask"]).bool()
    c = torch.from_numpy(z["c"])
    B, L, h = x.shape
    # the rows become an item table (row 0 = padding), the histories their ids; rows are used as they are (no normalisation)
    w = torch.cat([torch.zeros(1, h), x.reshape(-1, h)])
    lists = [[1 + b * L + t for t in range(L) if mask[b, t]] for b in range(B)]
    sd64 = {k: v.double() for k, v in sd.items()}
    for mode in ("mean", "max", "cls"):
        kw = {"heads": cfg["heads"], "act": "gelu", "mode": mode, "n_i": False, "n_u": True, "max_history": L}
        item, user = _towers(mf, w, sd, heads=cfg["heads"], act="gelu", mode=mode, L=L, n_i=False, n_u=True)
        u = user(_segments(lists))
        print(f"fixture {mode}")
        u64 = spec_tower(w.double(), lists, sd64, **kw)
        _check("u", u.detach(), torch.from_numpy(z[f"u.{mode}"]), u64)
        if mode != "mean":
            continue
        (u * c.to(DEV)).sum().backward()
        before = item.weight.detach().clone()
        mf.optim.SparseSGD([item.weight], lr=1.0).step()
        dx = (before - item.weight.detach())[1:].reshape(B, L, h)
        _, _, g64 = _spec_step(w, sd, lists, c, kw, None, 1.0, torch.float64)
        wl = w.double().clone().requires_grad_(True)
        (spec_tower(wl, lists, sd64, **kw) * c.double()).sum().backward()
        _check("d inputs_embeds", dx, torch.from_numpy(z["d_inputs_embeds"]), wl.grad[1:].reshape(B, L, h))
        for k, p in user.named_parameters():
            _check(k, p.grad, fix_grads[k], g64[k])


def test_order_matters(mf):
    rows, d, L = 100, 64, 16
    w, sd = _world(7, rows, d, 1, 64, 64, pos_std=0.5)
    hist = [5, 9, 2, 40, 41, 77, 3, 8]
    lists = [hist, hist[::-1]]
    _, user = _towers(mf, w, sd, heads=4, act="gelu", mode="mean", L=L)
    with torch.no_grad():
        u = user(_segments(lists))
    moved = float((u[0] - u[1]).abs().max())
    ref = spec_tower(w, lists, sd, heads=4, act="gelu", mode="mean", n_i=True, n_u=True, max_history=L)
    print(f"transformer: reversed history moves u by {moved:.3e} (spec {float((ref[0] - ref[1]).abs().max()):.3e})")
    assert moved > 1e-2
    item = mf.models.EmbeddingTower(rows, d, device=DEV)
    with torch.no_grad():
        item.weight.copy_(w.float())
        p = mf.models.HistoryPoolingTower(item, pooling_mode="mean")(_segments(lists))
    still = float((p[0] - p[1]).abs().max())
    print(f"history mean: reversed history moves u by {still:.3e}")
    assert still <= 1e-6


def _zipf_lists(rng, rows, batch, mean_len):
    p = 1.0 / np.arange(1, rows) ** 1.1
    p /= p.sum()
    lens = np.minimum(rng.poisson(mean_len, batch), 3 * mean_len)
    lens[:4] = (0, 1, mean_len, 2 * mean_len)
    return [(1 + rng.choice(rows - 1, n, p=p)).tolist() for n in lens]


def test_two_adam_steps_are_bit_reproducible(mf):
    rng = np.random.default_rng(5)
    rows, d, L = 500, 64, 32
    w, sd = _world(11, rows, d, 2, 128, 64)
    lists = _zipf_lists(rng, rows, 512, 24)
    g = torch.Generator().manual_seed(5)
    c = torch.randn(len(lists), d, generator=g)
    ids = torch.randint(1, rows, (700,), generator=g)
    c2 = torch.randn(700, d, generator=g)
    results = []
    for _ in range(2):
        item, user = _towers(mf, w, sd, heads=4, act="gelu", mode="max", L=L)
        towers = torch.nn.ModuleDict({"user": user, "item": item})
        opt = mf.optim.tower_optimizer(towers, "adam", 0.01)
        assert isinstance(opt, mf.optim.TowerOptimizer)
        for step in range(2):
            hist = _segments(lists) if step == 0 else _padded([x[-L:] for x in lists])
            loss = (user(hist) * c.to(DEV)).sum() + (item(ids.to(DEV)) * c2.to(DEV)).sum()
            loss.backward()
            opt.step()
            opt.zero_grad()
        results.append((item.weight.detach().clone(), [p.detach().clone() for p in user.parameters()]))
    assert torch.equal(results[0][0], results[1][0])
    assert not torch.equal(results[0][0].cpu(), w.float())
    for a, b in zip(results[0][1], results[1][1]):
        assert torch.equal(a, b)
    moved = [not torch.equal(a.cpu(), sd[k].float()) for a, k in zip(results[0][1], dict(user.named_parameters()))]
    assert sum(moved) >= len(moved) - 1                # every dense weight stepped (token-type row 1 has no gradient)


def test_backward_zipf_large_batch(mf):
    """B = 8192, L = 32, d = 64: hot items sit in thousands of histories; the coalesced table gradient against the spec."""
    rng = np.random.default_rng(9)
    rows, d, L, B = 5000, 64, 32, 8192
    w, sd = _world(13, rows, d, 1, 64, 64)
    lists = _zipf_lists(rng, rows, B, 20)
    counts = np.bincount(np.concatenate([np.asarray(x[-L:], dtype=np.int64) for x in lists if x]), minlength=rows)
    assert counts.max() > 2000  # noqa: PLR2004
    g = torch.Generator().manual_seed(9)
    c = torch.randn(B, d, generator=g, dtype=torch.float64) / B ** 0.5
    kw = {"heads": 4, "act": "gelu", "mode": "mean", "n_i": True, "n_u": True, "max_history": L}
    extra = (torch.randint(1, rows, (B,), generator=g), torch.randn(B, d, generator=g, dtype=torch.float64) / B ** 0.5)
    u64, d64, g64 = _spec_step(w, sd, lists, c, kw, extra, 1.0, torch.float64)
    u32, d32, g32 = _spec_step(w, sd, lists, c, kw, extra, 1.0, torch.float32)
    u, delta, grads = _kernel_step(mf, w, sd, _segments(lists), c, kw, extra, 1.0)
    print("zipf B=8192 L=32 d=64")
    _check("u", u, u32, u64)
    _check("table step", delta, d32, d64)
    for k in g64:
        _check(k, grads[k], g32[k], g64[k])


def _module(mf, **over):
    cfg = {"num_users": 40, "num_items": 60, "hidden_size": 32, "learning_rate": 0.02, "user_tower": "transformer", "max_history": 8,
           "num_negatives": 2, "train_loss": "InfomationNoiseContrastiveEstimationLoss", **over}
    m = mf.lightning.MatrixFactorizationLitModule(cfg)
    m.configure_model(device=DEV)
    return m


def _last_item_batch(rng, n_items, batch, length):
    """A world where the target depends on the LAST history item only: target = (last * 7 + 3) % (n_items - 1) + 1."""
    hist = rng.integers(1, n_items, (batch, length))
    pos = (hist[:, -1] * 7 + 3) % (n_items - 1) + 1
    neg = rng.integers(1, n_items, batch)
    t = lambda a: torch.tensor(a, dtype=torch.int64, device=DEV)  # noqa: E731
    return {"user": {"idx": t(np.arange(batch) % 39 + 1), "history": t(hist), "pos_idx": t(pos[:, None])},
            "item": {"idx": t(pos)}, "neg_item": {"idx": t(neg)}, "target": torch.ones(batch, device=DEV)}


def test_module_end_to_end(mf, tmp_path):
    m = _module(mf, pooling_mode="cls", num_hidden_layers=2)
    assert isinstance(m.towers["user"], mf.models.HistoryTransformerTower)
    rng = np.random.default_rng(0)
    opt = m.configure_optimizers()
    assert isinstance(opt, mf.optim.TowerOptimizer)
    key = "train/InfomationNoiseContrastiveEstimationLoss"
    probe = _last_item_batch(np.random.default_rng(99), 60, 256, 6)
    with torch.no_grad():
        first = float(m.compute_losses(probe)[key])
    q0 = m.towers["user"].encoder.layer[0].attention.self.query.weight.detach().clone()
    w0 = m.towers["item"].weight.detach().clone()
    for step in range(60):
        batch = _last_item_batch(rng, 60, 128, 6)
        if step % 2:
            m.fused_training_step(batch, opt)              # falls back to the three calls
        else:
            loss = m.training_step(batch)
            loss.backward()
            opt.step()
            opt.zero_grad()
    assert m._fused is None
    with torch.no_grad():
        last = float(m.compute_losses(probe)[key])
    print(f"loss on a held-out batch: {first:.4f} -> {last:.4f}")
    assert last < first - 0.05
    assert not torch.equal(q0, m.towers["user"].encoder.layer[0].attention.self.query.weight.detach())
    assert not torch.equal(w0, m.towers["item"].weight.detach())

    # the losses are the spec's user vectors through the oracle's losses
    from oracle import losses as ol

    batch = _last_item_batch(rng, 60, 32, 6)
    out = m.compute_losses(batch)
    user = m.towers["user"]
    w = m.towers["item"].weight.detach().cpu()
    sd = {k: v.detach().cpu() for k, v in user.state_dict().items()}
    u = spec_tower(w, batch["user"]["history"].tolist(), sd, heads=4, act="gelu", mode="cls", n_i=True, n_u=True, max_history=8)
    item_idx = torch.cat([batch["item"]["idx"], batch["neg_item"]["idx"]]).cpu()
    v = F.normalize(w[item_idx], dim=1, eps=1e-12)
    want = ol.all_losses(u, v, batch["target"].cpu(), item_idx=item_idx, pos_idx=batch["user"]["pos_idx"].cpu(), num_negatives=2)
    for k in ol.KINDS:
        assert abs(float(out[f"train/{k}"]) - float(want[k])) <= 1e-4 * max(1.0, abs(float(want[k]))), k

    # metrics / predict: queries = the encoded eval history, which is also excluded
    m.item_processor.get_index(m)
    off = torch.tensor([0, 3, 3, 8], device=DEV)
    items = torch.tensor([4, 9, 2, 7, 7, 1, 30, 12], device=DEV)
    ev = {"user": {"idx": torch.tensor([1, 2, 3], device=DEV)}, "history": (off, items)}
    _, rows = m.predict_step(ev)
    for b in range(3):
        assert not set(rows[b].tolist()) & set(items[int(off[b]):int(off[b + 1])].tolist())

    # serving a user who is in no table; save / load reproduces it bit for bit
    hist = [3, 7, 7, 11, 20]
    rec = m.recommend_with_history(hist, top_k=10)
    assert not set(rec["movie_rn"].tolist()) & set(hist)
    assert m.recommend_with_history(hist[::-1], top_k=10)["score"].tolist() != rec["score"].tolist()
    m.history = {5: hist}
    assert m.recommend(5, top_k=10)["movie_rn"].tolist() == rec["movie_rn"].tolist()
    m.save(tmp_path / "model")
    m2 = mf.lightning.MatrixFactorizationLitModule.load(tmp_path / "model", device=DEV)
    assert isinstance(m2.towers["user"], mf.models.HistoryTransformerTower) and m2.config.pooling_mode == "cls"
    assert m2.towers["user"].weight is m2.towers["item"].weight
    for (k, a), (_, b) in zip(m.towers.state_dict().items(), m2.towers.state_dict().items()):
        assert torch.equal(a, b), k
    rec2 = m2.recommend_with_history(hist, top_k=10)
    assert rec2["movie_rn"].tolist() == rec["movie_rn"].tolist() and rec2["score"].tolist() == rec["score"].tolist()


def test_refusals(mf):
    with pytest.raises(ValueError, match="EmbeddingTower"):
        mf.models.HistoryTransformerTower(mf.models.HashEmbeddingTower(100, 32, device=DEV))
    with pytest.raises(ValueError, match="table user towers only"):
        mf.distributed.ShardedTrainer(mf, DEV, "sgd", 0, num_users=10, num_items=10, dim=32, comm=object(), user_tower="transformer")
    towers = mf.models.init_towers(mf.models.ModelConfig(user_tower="transformer", hidden_size=32, num_items=50), device=DEV)
    with pytest.raises(mf._lib.MfHipError):
        mf.fused.FusedSmallStep(towers, mf.optim.SparseSGD([towers["item"].weight], lr=0.1), mf.losses.PairwiseHingeLoss(num_negatives=2))
    with pytest.raises(mf._lib.MfHipError, match="dense gradient|2-D"):      # the sparse optimisers do not take the encoder's weights
        p = towers["user"].encoder_parameters()[0]
        p.grad = torch.zeros_like(p)
        mf.optim.SparseSGD([p], lr=0.1).step()
    towers["user"].encoder_parameters()[0].grad = None
    with pytest.raises(mf._lib.MfHipError, match="on the GPU"):
        towers["user"](torch.zeros(2, 4, dtype=torch.int64))
