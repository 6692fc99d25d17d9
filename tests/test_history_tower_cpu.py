"""CPU: the spec of the history-pooled user tower (``spec_pool``, plain torch -- the GPU tests hold the kernels to it), its
configuration surface, the sampler's host-side checks and the new kernels' register budgets."""
from __future__ import annotations

import importlib.util

import pytest
import torch
import torch.nn.functional as F

from tests.conftest import ROOT


def spec_pool(w: torch.Tensor, lists, mode: str, n_i: bool, n_u: bool, max_history: int | None = None) -> torch.Tensor:
    """``[B, d]`` user vectors of the history tower (differentiable in ``w``): ids outside [1, rows) are padding, the last
    ``max_history`` valid entries are kept, r = the (normalised) rows, p = mean or channel-wise max (ties: the first
    entry), u = normalise(p); an empty list gives 0."""
    rows, d = w.shape
    out = []
    for lst in lists:
        valid = [int(i) for i in lst if 1 <= int(i) < rows]
        if max_history is not None:
            valid = valid[-max_history:] if valid else valid
        if not valid:
            p = w.sum() * 0 + torch.zeros(d, dtype=w.dtype)
        else:
            r = w[torch.tensor(valid)]
            if n_i:
                r = F.normalize(r, dim=1, eps=1e-12)
            if mode == "mean":
                p = r.mean(0)
            else:
                m = r.detach().max(0).values
                pos = torch.arange(len(valid))[:, None].expand_as(r)
                first = torch.where(r.detach() == m, pos, len(valid)).min(0).values
                p = r.gather(0, first[None]).squeeze(0)
        out.append(F.normalize(p, dim=0, eps=1e-12) if n_u else p)
    return torch.stack(out)


def test_spec_hand_worked_three_users():
    w = torch.tensor([[9.0, 9.0], [3.0, 4.0], [0.0, 2.0], [1.0, 0.0]])
    lists = [[1, 3, 0], [2, 2, 7], []]           # 0 and 7 (>= 4 rows) are padding; row 0 is never pooled
    mean = spec_pool(w, lists, "mean", True, False)
    assert torch.allclose(mean[0], torch.tensor([(0.6 + 1.0) / 2, 0.8 / 2]))
    assert torch.allclose(mean[1], torch.tensor([0.0, 1.0]))
    assert torch.equal(mean[2], torch.zeros(2))
    mx = spec_pool(w, lists, "max", False, False)
    assert torch.equal(mx[0], torch.tensor([3.0, 4.0])) and torch.equal(mx[1], torch.tensor([0.0, 2.0]))
    u = spec_pool(w, lists, "mean", True, True)
    assert torch.allclose(u[0], F.normalize(torch.tensor([0.8, 0.4]), dim=0))
    assert torch.allclose(spec_pool(w, [[1, 3, 2]], "mean", False, False, max_history=2)[0], torch.tensor([0.5, 1.0]))


def test_spec_max_ties_route_to_the_first_entry():
    w = torch.tensor([[0.0, 0.0], [1.0, 5.0], [1.0, 2.0]], requires_grad=True)
    p = spec_pool(w, [[2, 1, 1]], "max", False, False)
    p.sum().backward()
    # channel 0: rows 2 and 1 tie (1.0): entry 0 (row 2) wins; channel 1: row 1, first of its two copies
    assert torch.equal(w.grad, torch.tensor([[0.0, 0.0], [0.0, 1.0], [1.0, 0.0]]))


@pytest.mark.parametrize("mode", ["mean", "max"])
def test_spec_agrees_with_embedding_bag(mode):
    g = torch.Generator().manual_seed(0)
    w = torch.randn(50, 16, generator=g)
    lists = [torch.randint(1, 50, (n,), generator=g).tolist() for n in (1, 4, 9, 30)]
    flat = torch.tensor([i for x in lists for i in x])
    offsets = torch.tensor([0, *torch.tensor([len(x) for x in lists]).cumsum(0)[:-1].tolist()])
    for n_i in (True, False):
        table = F.normalize(w, dim=1, eps=1e-12) if n_i else w
        bag = F.embedding_bag(flat, table, offsets, mode=mode)
        assert torch.allclose(spec_pool(w, lists, mode, n_i, False), bag, atol=1e-6)
        assert torch.allclose(spec_pool(w, lists, mode, n_i, True), F.normalize(bag, dim=1, eps=1e-12), atol=1e-6)


def test_config_refuses_transformer_and_unknown_pooling_modes(mf):
    for mode in ("cls", "pooler"):
        with pytest.raises(ValueError, match="no transformer"):
            mf.models.ModelConfig(user_tower="history", pooling_mode=mode)
    with pytest.raises(ValueError, match="pooling_mode must be one of"):
        mf.models.ModelConfig(pooling_mode="sum")
    with pytest.raises(ValueError):
        mf.models.ModelConfig(user_tower="bert")
    with pytest.raises(ValueError, match="max_history"):
        mf.models.ModelConfig(max_history=0)
    with pytest.raises(ValueError, match="no transformer"):
        mf.models.HistoryPoolingTower(mf.models.EmbeddingTower(10, 32), pooling_mode="cls")
    cfg = mf.lightning.MatrixFactorizationLitConfig(user_tower="history", pooling_mode="max", max_history=50)
    assert mf.lightning.MatrixFactorizationLitConfig.model_validate(cfg.model_dump()) == cfg


def test_defaults_leave_init_towers_unchanged(mf):
    cfg = mf.models.ModelConfig(num_users=30, num_items=40, hidden_size=32)
    assert (cfg.user_tower, cfg.pooling_mode, cfg.max_history) == ("table", "mean", None)
    torch.manual_seed(0)
    towers = mf.models.init_towers(cfg)
    assert type(towers["user"]) is mf.models.EmbeddingTower and type(towers["item"]) is mf.models.EmbeddingTower
    assert towers["user"].weight.shape == (30, 32) and towers["item"].weight.shape == (40, 32)
    assert len(list(towers.parameters())) == 2


def test_history_towers_share_the_item_table(mf):
    towers = mf.models.init_towers(mf.models.ModelConfig(num_items=40, hidden_size=32, user_tower="history", pooling_mode="max",
                                                         max_history=7))
    user, item = towers["user"], towers["item"]
    assert isinstance(user, mf.models.HistoryPoolingTower) and user.weight is item.weight
    assert (user.pooling_mode, user.max_history) == ("max", 7)
    assert [p is item.weight for p in towers.parameters()] == [True]         # optimised once ...
    assert list(towers.state_dict()) == ["item.weight"]                      # ... and saved once
    with pytest.raises(ValueError, match="EmbeddingTower"):
        mf.models.HistoryPoolingTower(mf.models.HashEmbeddingTower(100, 32))
    with pytest.raises(ValueError, match="hashed"):
        mf.models.init_towers(mf.models.ModelConfig(user_tower="history", num_hashes=2))


def test_sampler_history_host_checks(mf):
    user = torch.tensor([1, 1, 2, 2, 2])
    item = torch.tensor([3, 4, 5, 6, 7])
    target = torch.ones(5)
    pos_off = torch.tensor([0, 0, 2, 5])
    kw = {"num_items": 8, "device": "cpu"}
    S = mf.data.DeviceInteractionSampler
    with pytest.raises(ValueError, match="go together"):
        S(user, item, target, pos_off, item, pair_hist_lo=torch.zeros(5, dtype=torch.int64), **kw)
    with pytest.raises(ValueError, match="one history window per pair"):
        S(user, item, target, pos_off, item, pair_hist_lo=torch.zeros(4), pair_hist_hi=torch.zeros(4), hist_items=item, **kw)
    with pytest.raises(ValueError, match="lo <= hi"):
        S(user, item, target, pos_off, item, pair_hist_lo=torch.zeros(5), pair_hist_hi=torch.full((5,), 9), hist_items=item, **kw)
    with pytest.raises(ValueError, match="lo <= hi"):
        S(user, item, target, pos_off, item, pair_hist_lo=torch.tensor([1, 0, 0, 0, 0]), pair_hist_hi=torch.zeros(5),
          hist_items=item, **kw)
    s = S(user, item, target, pos_off, item, pair_hist_lo=torch.tensor([0, 0, 2, 2, 3]), pair_hist_hi=torch.tensor([0, 1, 2, 3, 4]),
          hist_items=item, user_range=(2, 3), **kw)
    assert s.pair_user.tolist() == [2, 2, 2]
    assert s.pair_hist_lo.tolist() == [2, 2, 3] and s.pair_hist_hi.tolist() == [2, 3, 4]    # filtered with their pairs


def test_interaction_table_sampler_passes_train_windows(mf):
    g = torch.Generator().manual_seed(0)
    n = 300
    table = mf.data.InteractionTable(torch.randint(1, 20, (n,), generator=g), torch.randint(1, 30, (n,), generator=g),
                                     torch.randint(1, 6, (n,), generator=g).float(), torch.randint(0, 10**7, (n,), generator=g))
    s = table.sampler(num_items=30, device="cpu", history=True)
    tr = table.sorted_train
    assert torch.equal(s.pair_hist_lo, table.history_lo[tr]) and torch.equal(s.pair_hist_hi, table.history_hi[tr])
    assert torch.equal(s.hist_items, table.sorted_item)
    assert table.sampler(num_items=30, device="cpu").pair_hist_lo is None


def test_pool_kernels_do_not_spill(mf):
    spec = importlib.util.spec_from_file_location("kernel_resources", ROOT / "tools" / "kernel_resources.py")
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    res = kr.kernel_resources()
    names = ("pool_", "coalesce_", "sample_history_kernel")
    mine = {k: v for k, v in res.items() if any(n in k for n in names)}
    assert len(mine) >= 43, sorted(mine)  # noqa: PLR2004
    for k, v in mine.items():
        assert v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, k
        assert v["private_segment_fixed_size"] == 0, k
