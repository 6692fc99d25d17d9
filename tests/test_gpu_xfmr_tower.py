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

from tests.test_xfmr_tower_cpu import HARD_CASES, HARD_ROWS, hard_case, load_fixture, random_state, spec_step, spec_tower, tie_world

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FACTOR = 8.0


def _check(name: str, got: torch.Tensor, spec32: torch.Tensor, ref64: torch.Tensor) -> float:
    """The rule of the module docstring; returns kernel error / fp32-spec error."""
    kernel_value_is_finite = bool(torch.isfinite(got).all())
    assert kernel_value_is_finite, name                                      # (nan <= x is False below; this says so by name)
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


_spec_step = spec_step          # (u, table delta of one SGD step, dense gradients) through the spec: tests/test_xfmr_tower_cpu.py


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


def _one_sgd_step(mf, d, heads, L, mode, layers, act, inter, with_items, rows):
    rng = np.random.default_rng(d * 3 + L)
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


@pytest.mark.parametrize("with_items", [False, True])
@pytest.mark.parametrize(("d", "heads", "L", "mode", "layers", "act", "inter"), BACKWARD_CASES)
def test_backward_one_sgd_step(mf, d, heads, L, mode, layers, act, inter, with_items):
    _one_sgd_step(mf, d, heads, L, mode, layers, act, inter, with_items, 200)


@pytest.mark.parametrize(("d", "heads", "L", "mode", "layers", "act", "inter"), [BACKWARD_CASES[0], BACKWARD_CASES[2], BACKWARD_CASES[4]])
def test_backward_one_sgd_step_three_pass_table(mf, d, heads, L, mode, layers, act, inter):
    """The same step on a 70,000-row table: the coalesce sorts in three radix passes (200 rows: one), at the tower's
    narrowest and widest hidden size (32 and 128: it has no d = 256)."""
    _one_sgd_step(mf, d, heads, L, mode, layers, act, inter, True, 70000)


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


# ------------------------------------------------------------------------------------------- second round ----
# The tower at its limits: hard worlds (conditions proven on the CPU: test_xfmr_tower_cpu.test_hard_world_conditions), depth
# 3 and 4, every accepted (hidden, heads) pair, token counts at the engine's boundaries, T = 0, two encodes in one step.
def _step_against_spec(mf, label, w, sd, lists, c, kw, extra, lr, forms=(False, True), ref=None):
    """One SGD step of the kernels (each input form) against the spec under the module's rule; returns the worst ratio."""
    u64, d64, g64 = ref[0] if ref else spec_step(w, sd, lists, c, kw, extra, lr, torch.float64)
    u32, d32, g32 = ref[1] if ref else spec_step(w, sd, lists, c, kw, extra, lr, torch.float32)
    worst = 0.0
    for padded in forms:
        u, delta, grads = _kernel_step(mf, w, sd, _padded(lists) if padded else _segments(lists), c, kw, extra, lr)
        print(f"{label} padded={padded}")
        worst = max(worst, _check("u", u, u32, u64), _check("table step", delta, d32, d64))
        for k in g64:
            assert grads[k] is not None, k
            worst = max(worst, _check(k, grads[k], g32[k], g64[k]))
    return worst


@pytest.mark.parametrize("case", HARD_CASES, ids=lambda case: "-".join(str(x) for x in case))
def test_hard_world_one_sgd_step(mf, case):
    """u, the table step and every encoder gradient on a world whose conditions the CPU file asserts; on ``sharp`` every
    output is finite and every user vector has norm 1 before anything is compared."""
    world = case[0]
    w, sd, lists, c, kw = hard_case(*case)
    assert w.shape[0] == HARD_ROWS
    lr = 0.5
    ref = (spec_step(w, sd, lists, c, kw, None, lr, torch.float64), spec_step(w, sd, lists, c, kw, None, lr, torch.float32))
    if world == "sharp":
        some = torch.tensor([any(1 <= i < HARD_ROWS for i in lst) for lst in lists])
        for padded in (False, True):
            u, delta, grads = _kernel_step(mf, w, sd, _padded(lists) if padded else _segments(lists), c, kw, None, lr)
            for name, t in [("u", u), ("table step", delta), *grads.items()]:
                assert bool(torch.isfinite(t).all()), (name, padded)
            norm = u.double().norm(dim=1).cpu()
            assert float((norm[some] - 1).abs().max()) <= 1e-5 and float(norm[~some].abs().max()) == 0.0, norm  # noqa: PLR2004
    worst = _step_against_spec(mf, " ".join(str(x) for x in case), w, sd, lists, c, kw, None, lr, ref=ref)
    print(f"worst ratio on {world}: {worst:.2f}")


# depth 3 and 4; the (hidden, heads) pairs without a backward case above: (32, 1), (32, 2), (64, 2), (64, 4), (128, 2), (128, 8);
# intermediate sizes 96 and 160 (the GEMM's N tail), 4 h at h = 32 and h = 64, 32 at h = 128
SHAPE_CASES = [(32, 1, 16, "max", 1, "relu", 128), (32, 2, 32, "mean", 2, "silu", 96), (64, 2, 16, "cls", 1, "gelu_new", 256),
               (64, 4, 64, "max", 3, "silu", 160), (128, 2, 64, "mean", 1, "gelu", 32), (128, 8, 16, "max", 4, "relu", 128)]


@pytest.mark.parametrize(("d", "heads", "L", "mode", "layers", "act", "inter"), SHAPE_CASES)
def test_backward_depth_and_shapes(mf, d, heads, L, mode, layers, act, inter):
    rng = np.random.default_rng(d * 5 + heads)
    rows = 200
    w, sd = _world(100 + d + heads, rows, d, layers, inter, 64)
    lists = _lists(rng, rows, [1, 5, 17, 64, 70, 3, 9, 30])
    g = torch.Generator().manual_seed(d + heads)
    c = torch.randn(len(lists), d, generator=g, dtype=torch.float64)
    extra = (torch.randint(0, rows, (40,), generator=g), torch.randn(40, d, generator=g, dtype=torch.float64))
    kw = {"heads": heads, "act": act, "mode": mode, "n_i": True, "n_u": True, "max_history": L}
    _step_against_spec(mf, f"d={d} heads={heads} L={L} {mode} layers={layers} {act} I={inter}", w, sd, lists, c, kw, extra, 0.5)


def _valid_tokens(lists, rows, L):
    return sum(min(L, sum(1 <= i < rows for i in lst)) for lst in lists)


TOKEN_COUNTS = [1, 15, 16, 17, 63, 64, 65, 127, 129, 4095, 4096, 4097, 8193]


@pytest.mark.parametrize("T", TOKEN_COUNTS)
def test_token_count_boundaries(mf, T):
    """Exactly T valid tokens (asserted from the lists): 64-token GEMM tiles, 16-token k-steps, the weight gradient's 256
    slices (their length steps at T = 4096 n; only T = 4095 and 4096 fill the last slice), LayerNorm's 1,024 slices.
    B = 1 for T <= 64, otherwise full lists plus a remainder, with an empty user appended when B would be a multiple of 8."""
    rows, d, L = 300, 32, 64
    rng = np.random.default_rng(T)
    sizes = [L] * (T // L) + ([T % L] if T % L else [])
    lists = [rng.integers(1, rows, n).tolist() for n in sizes]
    if T > L:
        lists[0] = lists[0][:10] + [0, rows, -2] + lists[0][10:]             # padding inside a list does not count
        if len(lists) % 8 == 0:
            lists.append([])
        assert len(lists) % 8
    else:
        assert len(lists) == 1
    assert _valid_tokens(lists, rows, L) == T
    w, sd = _world(T, rows, d, 1, 32, 64)
    g = torch.Generator().manual_seed(T)
    c = torch.randn(len(lists), d, generator=g, dtype=torch.float64) / len(lists) ** 0.5
    kw = {"heads": 2, "act": "gelu", "mode": "max" if T % 2 else "mean", "n_i": True, "n_u": True, "max_history": L}
    _step_against_spec(mf, f"T={T} B={len(lists)}", w, sd, lists, c, kw, None, 0.5, forms=(T <= L,))


def test_full_lists_behind_invalid_entries(mf):
    """Every user keeps exactly L = 64 valid entries that sit behind more than 64 invalid ones: the cut walks back over
    several 64-entry blocks, some of them without a valid entry."""
    rows, d, L = 300, 64, 64
    rng = np.random.default_rng(21)
    bad = lambda n: rng.choice([0, -1, -7, rows, rows + 9], n).tolist()  # noqa: E731
    ids = lambda n: rng.integers(1, rows, n).tolist()  # noqa: E731
    spread = [x for i in ids(L) for x in (i, *bad(2))]                       # 64 valid entries in 192
    lists = [bad(70) + spread + bad(80), ids(100) + bad(130), ids(L) + bad(65), bad(3) + ids(40) + bad(64) + ids(24) + bad(129),
             bad(200) + ids(L) + bad(65)]
    assert _valid_tokens(lists, rows, L) == len(lists) * L
    assert all(sum(1 <= i < rows for i in lst) >= L and len(lst) - max(k for k, i in enumerate(lst) if 1 <= i < rows) > L for lst in lists)
    w, sd = _world(21, rows, d, 1, 64, 64)
    c = torch.randn(len(lists), d, generator=torch.Generator().manual_seed(21), dtype=torch.float64)
    kw = {"heads": 4, "act": "gelu", "mode": "mean", "n_i": True, "n_u": True, "max_history": L}
    _step_against_spec(mf, "full lists behind invalid entries", w, sd, lists, c, kw, None, 0.5)


def test_one_user_holds_every_token(mf):
    rows, d, L = 300, 64, 64
    rng = np.random.default_rng(22)
    lists = [[] if b != 20 else rng.integers(1, rows, L).tolist() for b in range(37)]  # noqa: PLR2004
    lists[3], lists[30] = [0, 0], [rows, -1, 0]
    assert _valid_tokens(lists, rows, L) == L
    w, sd = _world(22, rows, d, 2, 128, 64)
    c = torch.randn(len(lists), d, generator=torch.Generator().manual_seed(22), dtype=torch.float64)
    kw = {"heads": 8, "act": "silu", "mode": "max", "n_i": True, "n_u": True, "max_history": L}
    _step_against_spec(mf, "one user of 37 holds all 64 tokens", w, sd, lists, c, kw, None, 0.5)


@pytest.mark.parametrize("kind", ["sgd", "adam"])
def test_no_valid_token_in_the_batch(mf, kind):
    """T = 0 with t_cap > 0 (a cold batch: every id is 0, negative or >= rows): u is exactly 0, every encoder gradient is
    exactly 0 -- the gradient buffers are uninitialised memory that the kernels must write, so the allocator's free blocks
    are filled with NaN first -- and the optimiser step leaves the table's rows bit-identical."""
    rows, d = 50, 32
    w, sd = _world(3, rows, d, 2, 64, 64)
    lists = [[0, 0, -1], [rows, rows + 7, 0, -5], [0], []]
    c = torch.randn(len(lists), d, generator=torch.Generator().manual_seed(3)).to(DEV)
    for padded, mode in ((False, "max"), (True, "mean")):
        item, user = _towers(mf, w, sd, heads=4, act="gelu", mode=mode, L=16)
        opt = mf.optim.tower_optimizer(torch.nn.ModuleDict({"user": user, "item": item}), kind, 0.05)
        assert isinstance(opt, mf.optim.TowerOptimizer)
        junk = [torch.full_like(p, float("nan")) for p in user.parameters()] + [torch.full((1 << 20,), float("nan"), device=DEV)]
        del junk
        u = user(_padded(lists) if padded else _segments(lists))
        assert torch.equal(u, torch.zeros(len(lists), d, device=DEV))
        (u * c).sum().backward()
        for k, p in user.named_parameters():
            assert p.grad is not None and torch.equal(p.grad, torch.zeros_like(p)), k
        before = item.weight.detach().clone()
        opt.step()
        torch.cuda.synchronize()
        assert torch.equal(item.weight.detach(), before)
        # the step after a cold batch is an ordinary one
        opt.zero_grad()
        (user(_segments([[4, 9, 4], [7]])) * c[:2]).sum().backward()
        opt.step()
        moved = (item.weight.detach() != before).any(1).nonzero().flatten().tolist()
        assert moved == [4, 7, 9]


def _two_encode_spec(w, sd, la, lb, ca, cb, ids, c3, kw, dtype):
    wl = w.to(dtype).clone().requires_grad_(True)
    leaf = {k: v.to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    loss = (spec_tower(wl, la, leaf, **kw) * ca.to(dtype)).sum() + (spec_tower(wl, lb, leaf, **kw) * cb.to(dtype)).sum()
    loss = loss + (F.normalize(wl[ids], dim=1, eps=1e-12) * c3.to(dtype)).sum()
    loss.backward()
    return wl.grad, {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaf.items()}


@pytest.mark.parametrize("kind", ["sgd", "adam"])
def test_two_encodes_in_one_step(mf, kind):
    """One tower applied to two history batches (different B; segments and padded) and the item tower on ids that overlap
    both, one backward, one step: two TransformerHistoryGrad entries on the table, the second coalesce taking the first
    one's -1-padded list as its extra rows; the encoder's gradients are the sums over both encodes.  The table gradient
    is read from the SGD step (lr = 1) or from RowAdam's first moment ((1 - beta1) g after one step); twice, bit for bit."""
    rows, d, L = 120, 64, 16
    rng = np.random.default_rng(31)
    w, sd = _world(31, rows, d, 2, 96, 64)
    la = _lists(rng, rows, [1, 5, 17, 20, 3, 9])
    lb = _lists(rng, rows, [16, 2, 40])
    g = torch.Generator().manual_seed(31)
    ca, cb = (torch.randn(len(x), d, generator=g, dtype=torch.float64) for x in (la, lb))
    seen = [[i for i in lst if 1 <= i < rows] for lst in (la[2], lb[0])]
    ids = torch.cat([torch.tensor(seen[0][:6] + seen[1][-6:]), torch.randint(1, rows, (20,), generator=g)])
    c3 = torch.randn(ids.numel(), d, generator=g, dtype=torch.float64)
    kw = {"heads": 4, "act": "gelu", "mode": "mean", "n_i": True, "n_u": True, "max_history": L}
    dw64, g64 = _two_encode_spec(w, sd, la, lb, ca, cb, ids, c3, kw, torch.float64)
    dw32, g32 = _two_encode_spec(w, sd, la, lb, ca, cb, ids, c3, kw, torch.float32)
    runs = []
    for _ in range(2):
        item, user = _towers(mf, w, sd, heads=4, act="gelu", mode="mean", L=L)
        opt = mf.optim.tower_optimizer(torch.nn.ModuleDict({"user": user, "item": item}), kind, 1.0 if kind == "sgd" else 0.01)
        loss = (user(_segments(la)) * ca.float().to(DEV)).sum() + (user(_padded(lb)) * cb.float().to(DEV)).sum()
        loss = loss + (item(ids.to(DEV)) * c3.float().to(DEV)).sum()
        loss.backward()
        pending = list(item.weight._mf_pending)
        assert sum(isinstance(x, mf.models.TransformerHistoryGrad) for x in pending) == 2 and len(pending) == 3  # noqa: PLR2004
        grads = {k: p.grad.detach().clone() for k, p in user.named_parameters()}
        before = item.weight.detach().clone()
        opt.step()
        if kind == "sgd":
            dw = before - item.weight.detach()
        else:
            state = opt.sparse.state[item.weight]
            dw = state["exp_avg"] / (1.0 - opt.sparse.param_groups[0]["betas"][0])
            touched = (dw64 != 0).any(1)
            assert torch.equal((item.weight.detach() != before).any(1).cpu(), touched)
        runs.append((item.weight.detach().clone(), dw.clone(), grads))
    print(f"two encodes in one step, {kind}")
    _check("table gradient", runs[0][1], dw32, dw64)
    for k in g64:
        _check(k, runs[0][2][k], g32[k], g64[k])
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    for k in g64:
        assert torch.equal(runs[0][2][k], runs[1][2][k]), k


def test_capture_is_refused_and_the_stream_stays_usable(mf):
    rows, d = 60, 32
    w, sd = _world(41, rows, d, 1, 32, 64)
    _, user = _towers(mf, w, sd, heads=4, act="gelu", mode="mean", L=16)
    with torch.no_grad():
        for hist in (_segments([[3, 4, 5], [9]]), _padded([[3, 4, 5], [9]])):   # (segments: before the entry count's host read)
            want = user(hist).clone()
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with pytest.raises(mf._lib.MfHipError, match="capture"):            # raised before any kernel is launched
                with torch.cuda.graph(graph):
                    user(hist)
            del graph
            torch.cuda.synchronize()
            assert not torch.cuda.is_current_stream_capturing()
            assert torch.equal(user(hist), want)


def test_max_pool_ties_go_to_the_first_position(mf):
    """A history that repeats one item under equal position rows: every channel of the max pool is an n-way tie (the CPU
    file shows the rows bit-identical in fp64 and fp32).  The first position wins, in the forward's ``arg`` and in where
    the gradient goes: the step matches the spec (whose max takes the first of equal values), and it is bit-identical to
    the step with cls pooling, which routes the tied user's gradient through position 0 by construction."""
    w, sd, lists = tie_world()
    kw = {"heads": 4, "act": "gelu", "mode": "max", "n_i": True, "n_u": True, "max_history": 16}
    c = torch.randn(len(lists), w.shape[1], generator=torch.Generator().manual_seed(8), dtype=torch.float64)
    _step_against_spec(mf, "max-pool ties", w, sd, lists, c, kw, None, 0.5)
    # the same step with cls pooling routes the gradient through position 0 alone: with ties, max must agree with it for the tied user
    c1 = c.clone()
    c1[1] = 0
    u_max, d_max, g_max = _kernel_step(mf, w, sd, _segments(lists), c1, kw, None, 0.5)
    u_cls, d_cls, g_cls = _kernel_step(mf, w, sd, _segments(lists), c1, {**kw, "mode": "cls"}, None, 0.5)
    assert torch.equal(u_max[0], u_cls[0]) and torch.equal(d_max, d_cls)
    for k in g_max:
        assert torch.equal(g_max[k], g_cls[k]), k
