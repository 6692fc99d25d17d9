"""GPU: training dropout of the transformer user tower (mf_xfmr_forward_dropout / mf_xfmr_backward_dropout) against the
dropout spec of tests/test_xfmr_dropout_cpu.py, whose masks come from the numpy restatement of the generator: the masks are
integers, so the fp32 and the fp64 spec and the kernels drop the same elements.

Tolerance: the rule of tests/test_gpu_xfmr_tower.py (its ``_check``): per tensor, kernel error <= 8 x the fp32 spec's error
against the fp64 spec + 1e-7, in max-abs over the max-abs of the fp64 value.  Every figure is printed before it is asserted.

Shapes (d, heads, L, layers, intermediate): head widths 8, 64 and 16; L = 64 has keys >= 32 (the lane-group mix), L = 33 a
partial group of four keys; 37 users with lengths 0, 1, L and more than L, more than 64 tokens (a GEMM tile boundary and a
partial tile); both input forms."""
from __future__ import annotations

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.test_gpu_xfmr_tower import DEV, _check, _padded, _segments, _towers, _world
from tests.test_xfmr_dropout_cpu import dropout_lists, spec_step_dropout, spec_tower_dropout

pytestmark = pytest.mark.gpu
SHAPES = [(32, 4, 5, 1, 32), (64, 1, 64, 2, 64), (128, 8, 33, 2, 96)]
ROWS = 200
SEED = 20240611


def _case(d, heads, L, layers, inter, mode="mean"):
    rng = np.random.default_rng(d + L)
    w, sd = _world(d + heads + L, ROWS, d, layers, inter, 64)
    lists = dropout_lists(rng, ROWS, L)
    valid = [min(L, sum(1 <= i < ROWS for i in lst)) for lst in lists]
    assert len(lists) == 37 and {0, 1, L} <= set(valid) and sum(valid) > 64 and any(len(x) > L for x in lists)  # noqa: PLR2004
    kw = {"heads": heads, "act": "gelu", "mode": mode, "n_i": True, "n_u": True, "max_history": L}
    return w, sd, lists, kw


def _dropout_towers(mf, w, sd, kw, p_hidden, p_attn, seed=SEED):
    item, user = _towers(mf, w, sd, heads=kw["heads"], act=kw["act"], mode=kw["mode"], L=kw["max_history"], n_i=kw["n_i"], n_u=kw["n_u"])
    user.hidden_dropout_prob, user.attention_probs_dropout_prob = p_hidden, p_attn
    user.manual_seed(seed)
    return item, user.train()


# ------------------------------------------------------------------------------------------- 1. forward ----
@pytest.mark.parametrize("mode", ["mean", "max", "cls"])
@pytest.mark.parametrize(("p_hidden", "p_attn"), [(0.1, 0.1), (0.5, 0.0), (0.0, 0.5), (0.9375, 0.1)])
@pytest.mark.parametrize(("d", "heads", "L", "layers", "inter"), SHAPES)
def test_forward_matches_spec(mf, d, heads, L, layers, inter, p_hidden, p_attn, mode):
    w, sd, lists, kw = _case(d, heads, L, layers, inter, mode)
    drop = {"p_hidden": p_hidden, "p_attn": p_attn, "seed": SEED, "call": 0}
    ref = spec_tower_dropout(w, lists, sd, **kw, **drop)
    s32 = spec_tower_dropout(w.float(), lists, {k: v.float() for k, v in sd.items()}, **kw, **drop)
    _, user = _dropout_towers(mf, w, sd, kw, p_hidden, p_attn)
    with torch.no_grad():
        got = user(_segments(lists))
        assert user.dropout_call == 1
        user.manual_seed(SEED)
        pad = user(_padded(lists))
    assert torch.equal(got, pad)                                             # the masks do not depend on the input form
    assert torch.equal(got[0].cpu(), torch.zeros(d))                         # the empty list
    _check(f"u d={d} heads={heads} L={L} layers={layers} {mode} p=({p_hidden}, {p_attn})", got, s32, ref)
    user.eval()
    with torch.no_grad():
        assert float((user(_segments(lists)) - got).abs().max()) > 1e-3      # noqa: PLR2004  (it did drop)


# ------------------------------------------------------------------------------------- 2. one SGD step ----
def _kernel_step(mf, user, item, hist, c, extra, lr):
    u = user(hist)
    loss = (u * c.float().to(DEV)).sum()
    if extra is not None:
        ids, c2 = extra
        loss = loss + (item(ids.to(DEV)) * c2.float().to(DEV)).sum()
    loss.backward()
    before = item.weight.detach().clone()
    mf.optim.SparseSGD([item.weight], lr=lr).step()
    return u.detach(), item.weight.detach() - before, {k: p.grad for k, p in user.named_parameters()}


@pytest.mark.parametrize("with_items", [False, True])
@pytest.mark.parametrize(("p_hidden", "p_attn"), [(0.1, 0.1), (0.5, 0.5)])
@pytest.mark.parametrize(("d", "heads", "L", "layers", "inter"), SHAPES)
def test_one_sgd_step_matches_spec(mf, d, heads, L, layers, inter, p_hidden, p_attn, with_items):
    """The table rows (grad_x through the coalesce), every encoder parameter and u, both input forms."""
    w, sd, lists, kw = _case(d, heads, L, layers, inter, "max" if d == 64 else "mean")  # noqa: PLR2004
    g = torch.Generator().manual_seed(d)
    c = torch.randn(len(lists), d, generator=g, dtype=torch.float64)
    extra = (torch.randint(0, ROWS, (40,), generator=g), torch.randn(40, d, generator=g, dtype=torch.float64)) if with_items else None
    drop = {"p_hidden": p_hidden, "p_attn": p_attn, "seed": SEED, "call": 0}
    lr = 0.5
    u64, d64, g64 = spec_step_dropout(w, sd, lists, c, kw, extra, lr, torch.float64, drop)
    u32, d32, g32 = spec_step_dropout(w, sd, lists, c, kw, extra, lr, torch.float32, drop)
    for padded in (False, True):
        item, user = _dropout_towers(mf, w, sd, kw, p_hidden, p_attn)
        u, delta, grads = _kernel_step(mf, user, item, _padded(lists) if padded else _segments(lists), c, extra, lr)
        print(f"d={d} heads={heads} L={L} layers={layers} p=({p_hidden}, {p_attn}) items={with_items} padded={padded}")
        _check("u", u, u32, u64)
        _check("table step", delta, d32, d64)
        for k in g64:
            assert grads[k] is not None, k
            _check(k, grads[k], g32[k], g64[k])


# ---------------------------------------------------------------------------------------- 3. off means off ----
def _plain_step(mf, user, item, hist, c):
    u = user(hist)
    (u * c).sum().backward()
    grads = [p.grad.clone() for p in user.parameters()]
    mf.optim.SparseSGD([item.weight], lr=0.5).step()
    return u.detach().clone(), item.weight.detach().clone(), grads


@pytest.mark.parametrize(("d", "heads", "L", "layers", "inter"), SHAPES)
def test_eval_mode_and_zero_probabilities_are_the_old_function(mf, d, heads, L, layers, inter):
    w, sd, lists, kw = _case(d, heads, L, layers, inter)
    c = torch.randn(len(lists), d, generator=torch.Generator().manual_seed(1)).to(DEV)
    hist = _segments(lists)
    item0, user0 = _towers(mf, w, sd, heads=heads, act="gelu", mode="mean", L=L)
    assert user0.training and (user0.hidden_dropout_prob, user0.attention_probs_dropout_prob) == (0.0, 0.0)
    want = _plain_step(mf, user0, item0, hist, c)
    assert user0.dropout_call == 0                                           # nothing to drop: no call number is used

    # a tower built with (0.3, 0.3), in eval mode
    item1 = mf.models.EmbeddingTower(ROWS, d, device=DEV)
    with torch.no_grad():
        item1.weight.copy_(w.float())
    user1 = mf.models.HistoryTransformerTower(item1, num_hidden_layers=layers, num_attention_heads=heads, intermediate_size=inter,
                                              max_history=L, hidden_dropout_prob=0.3, attention_probs_dropout_prob=0.3, dropout_seed=3)
    user1.load_state_dict({k: v.float() for k, v in sd.items()})
    got = _plain_step(mf, user1.eval(), item1, hist, c)
    assert user1.dropout_call == 0
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert all(torch.equal(a, b) for a, b in zip(got[2], want[2]))

    # a train-mode tower at (0, 0) through the new exports
    item2, user2 = _towers(mf, w, sd, heads=heads, act="gelu", mode="mean", L=L)
    start, end, items, n_entries = user2.segments(hist)
    cfg = (layers, heads, inter, 0, 0, L, True, True, (0.0, 0.0, 5, 7))
    u = mf.models._EncodeHistory.apply(user2.weight, start, end, items, n_entries, cfg, *user2.encoder_parameters())
    (u * c).sum().backward()
    grads = [p.grad.clone() for p in user2.parameters()]
    mf.optim.SparseSGD([item2.weight], lr=0.5).step()
    assert torch.equal(u.detach(), want[0]) and torch.equal(item2.weight.detach(), want[1])
    assert all(torch.equal(a, b) for a, b in zip(grads, want[2]))


# ------------------------------------------------------------------------- 4. determinism and freshness ----
def test_two_adam_steps_are_bit_reproducible_and_calls_are_fresh(mf):
    d, heads, L, layers, inter = SHAPES[2]
    w, sd, lists, kw = _case(d, heads, L, layers, inter, "max")
    c = torch.randn(len(lists), d, generator=torch.Generator().manual_seed(2)).to(DEV)
    results = []
    for _ in range(2):
        item, user = _dropout_towers(mf, w, sd, kw, 0.1, 0.1, seed=99)
        opt = mf.optim.tower_optimizer(torch.nn.ModuleDict({"user": user, "item": item}), "adam", 0.01)
        for step in range(2):
            (user(_segments(lists) if step == 0 else _padded(lists)) * c).sum().backward()
            opt.step()
            opt.zero_grad()
        assert user.dropout_call == 2  # noqa: PLR2004
        results.append((item.weight.detach().clone(), [p.detach().clone() for p in user.parameters()]))
    assert torch.equal(results[0][0], results[1][0]) and not torch.equal(results[0][0].cpu(), w.float())
    for a, b in zip(results[0][1], results[1][1]):
        assert torch.equal(a, b)
    # two training forwards of the same batch without reseeding differ; after manual_seed the first one comes back
    _, user = _dropout_towers(mf, w, sd, kw, 0.1, 0.1, seed=99)
    with torch.no_grad():
        a, b = user(_segments(lists)), user(_segments(lists))
        again = user.manual_seed(99)(_segments(lists))
    assert not torch.equal(a, b) and torch.equal(a, again)


def _two_encode_spec(w, sd, la, lb, ca, cb, kw, dtype, p):
    wl = w.to(dtype).clone().requires_grad_(True)
    leaf = {k: v.to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    ua = spec_tower_dropout(wl, la, leaf, **kw, p_hidden=p[0], p_attn=p[1], seed=SEED, call=0)
    ub = spec_tower_dropout(wl, lb, leaf, **kw, p_hidden=p[0], p_attn=p[1], seed=SEED, call=1)
    ((ua * ca.to(dtype)).sum() + (ub * cb.to(dtype)).sum()).backward()
    return ua.detach(), ub.detach(), wl.grad, {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaf.items()}


def test_two_encodes_in_one_step_use_two_calls(mf):
    d, heads, L, layers, inter = SHAPES[0]
    w, sd, lists, kw = _case(d, heads, L, layers, inter)
    la, lb = lists[:20], lists[5:]                                           # overlapping users at other batch indices
    g = torch.Generator().manual_seed(3)
    ca, cb = (torch.randn(len(x), d, generator=g, dtype=torch.float64) for x in (la, lb))
    p = (0.1, 0.1)
    ref = _two_encode_spec(w, sd, la, lb, ca, cb, kw, torch.float64, p)
    s32 = _two_encode_spec(w, sd, la, lb, ca, cb, kw, torch.float32, p)
    item, user = _dropout_towers(mf, w, sd, kw, *p)
    ua, ub = user(_segments(la)), user(_padded(lb))
    assert user.dropout_call == 2  # noqa: PLR2004
    ((ua * ca.float().to(DEV)).sum() + (ub * cb.float().to(DEV)).sum()).backward()
    before = item.weight.detach().clone()
    mf.optim.SparseSGD([item.weight], lr=1.0).step()
    _check("u of call 0", ua.detach(), s32[0], ref[0])
    _check("u of call 1", ub.detach(), s32[1], ref[1])
    _check("table gradient", before - item.weight.detach(), s32[2], ref[2])
    for k, prm in user.named_parameters():
        _check(k, prm.grad, s32[3][k], ref[3][k])


# -------------------------------------------------------------------------------------- 5. the module ----
def test_module_end_to_end(mf, tmp_path):
    cfg = mf.models.ModelConfig(user_tower="transformer", hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1)
    assert (cfg.hidden_dropout_prob, cfg.attention_probs_dropout_prob) == (0.1, 0.1)
    m = mf.lightning.MatrixFactorizationLitModule({"num_users": 40, "num_items": 60, "hidden_size": 32, "learning_rate": 0.02,
                                                   "user_tower": "transformer", "max_history": 8, "num_negatives": 2,
                                                   "train_loss": "InfomationNoiseContrastiveEstimationLoss", "hidden_dropout_prob": 0.1,
                                                   "attention_probs_dropout_prob": 0.1, "dropout_seed": 4})
    m.configure_model(device=DEV)
    user = m.towers["user"]
    assert (user.hidden_dropout_prob, user.attention_probs_dropout_prob, user.dropout_seed, user.training) == (0.1, 0.1, 4, True)
    opt = m.configure_optimizers()
    rng = np.random.default_rng(0)
    t = lambda a: torch.tensor(a, dtype=torch.int64, device=DEV)  # noqa: E731
    w0 = m.towers["item"].weight.detach().clone()
    for _ in range(2):
        hist = rng.integers(1, 60, (64, 6))
        pos = (hist[:, -1] * 7 + 3) % 59 + 1
        batch = {"user": {"idx": t(np.arange(64) % 39 + 1), "history": t(hist), "pos_idx": t(pos[:, None])}, "item": {"idx": t(pos)},
                 "neg_item": {"idx": t(rng.integers(1, 60, 64))}, "target": torch.ones(64, device=DEV)}
        loss = m.training_step(batch)
        assert bool(torch.isfinite(loss))
        loss.backward()
        opt.step()
        opt.zero_grad()
    assert user.dropout_call == 2 and not torch.equal(w0, m.towers["item"].weight.detach())  # noqa: PLR2004

    # serving never drops and leaves the tower's mode as it found it
    m.item_processor.get_index(m)
    hist = [3, 7, 7, 11, 20]
    assert user.training
    rec_train = m.recommend_with_history(hist, top_k=10)
    assert user.training and user.dropout_call == 2  # noqa: PLR2004
    user.eval()
    rec_eval = m.recommend_with_history(hist, top_k=10)
    assert not user.training
    assert rec_train["movie_rn"].tolist() == rec_eval["movie_rn"].tolist() and rec_train["score"].tolist() == rec_eval["score"].tolist()
    user.train()
    m.history = {5: hist}
    assert m.recommend(5, top_k=10)["movie_rn"].tolist() == rec_eval["movie_rn"].tolist() and user.training
    off = torch.tensor([0, 3, 3, 8], device=DEV)
    ev = {"user": {"idx": torch.tensor([1, 2, 3], device=DEV)}, "history": (off, torch.tensor([4, 9, 2, 7, 7, 1, 30, 12], device=DEV))}
    s1, r1 = m.predict_step(ev)
    s2, r2 = m.predict_step(ev)
    assert torch.equal(r1, r2) and torch.equal(s1, s2) and user.training and user.dropout_call == 2  # noqa: PLR2004

    m.save(tmp_path / "model")
    m2 = mf.lightning.MatrixFactorizationLitModule.load(tmp_path / "model", device=DEV)
    u2 = m2.towers["user"]
    assert (m2.config.hidden_dropout_prob, m2.config.attention_probs_dropout_prob, m2.config.dropout_seed) == (0.1, 0.1, 4)
    assert (u2.hidden_dropout_prob, u2.attention_probs_dropout_prob, u2.dropout_seed, u2.dropout_call) == (0.1, 0.1, 4, 0)
    for (k, a), (_, b) in zip(m.towers.state_dict().items(), m2.towers.state_dict().items()):
        assert torch.equal(a, b), k
    assert m2.recommend_with_history(hist, top_k=10)["movie_rn"].tolist() == rec_eval["movie_rn"].tolist()


# ---------------------------------------------------------------------------------------- 6. refusals ----
def test_refusals(mf):
    item = mf.models.EmbeddingTower(50, 32, device=DEV)
    for kw in ({"hidden_dropout_prob": 1.0}, {"hidden_dropout_prob": -0.1}, {"attention_probs_dropout_prob": 1.0},
               {"attention_probs_dropout_prob": -1e-3}):
        with pytest.raises(ValueError, match=next(iter(kw))):
            mf.models.HistoryTransformerTower(item, **kw)
        with pytest.raises(ValueError, match=next(iter(kw))):
            mf.models.ModelConfig(user_tower="transformer", hidden_size=32, **kw)
    # a direct C call with bad probabilities: MF_EINVAL, nothing launched
    user = mf.models.HistoryTransformerTower(item, max_history=8).train()
    lists = [[3, 4, 5], [9]]
    start, end, items, n_entries = user.segments(_segments(lists))
    for bad in ((1.0, 0.0, 0, 0), (0.0, -0.5, 0, 0)):
        cfg = (1, 4, 32, 0, 0, 8, True, True, bad)
        with pytest.raises(mf._lib.MfHipError, match=r"error -1.*\[0, 1\)"):
            mf.models._EncodeHistory.apply(user.weight, start, end, items, n_entries, cfg, *user.encoder_parameters())
    torch.cuda.synchronize()


def test_capture_is_refused_and_the_stream_stays_usable(mf):
    w, sd = _world(41, 60, 32, 1, 32, 64)
    kw = {"heads": 4, "act": "gelu", "mode": "mean", "n_i": True, "n_u": True, "max_history": 16}
    _, user = _dropout_towers(mf, w, sd, kw, 0.1, 0.1)
    lists = [[3, 4, 5], [9]]
    want = spec_tower_dropout(w.float(), lists, {k: v.float() for k, v in sd.items()}, **kw, p_hidden=0.1, p_attn=0.1, seed=SEED, call=0)
    with torch.no_grad():
        for hist in (_segments(lists), _padded(lists)):
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            user.manual_seed(SEED)
            with pytest.raises(mf._lib.MfHipError, match="capture"):            # raised before any kernel is launched
                with torch.cuda.graph(graph):
                    user(hist)
            del graph
            torch.cuda.synchronize()
            assert not torch.cuda.is_current_stream_capturing() and user.dropout_call == 0   # a refused call uses no call number
            got = user(hist)
            assert float((got.cpu() - want).abs().max()) < 1e-4  # noqa: PLR2004
    assert F.normalize(got, dim=1).shape == got.shape
