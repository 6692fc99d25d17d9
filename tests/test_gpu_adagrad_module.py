"""GPU: ``optim.RowAdagrad`` through every way a tower reaches a table -- plain towers (the two-table launch, and the two
single calls with ``MF_UPDATE_PAIR=0``), a hashed tower, a history-pooled tower, a feature-bag tower, the transformer tower
through ``tower_optimizer`` -- then a captured step, the Lightning module and the sharded trainer on two ranks.

What a step is held to: right before ``optimizer.step()`` the list every table is about to receive is read off the table
(``optim._pending``: ids, gradient rows, normalised or not), duplicates are summed in fp64 (``_adagrad_spec.coalesce``) and
the specification (tests/_adagrad_spec.py) is applied to the rows and ``sum`` entries the kernel starts from.  With E the
largest elementwise difference between the specification in fp32 and in fp64, the table and ``sum`` after the step may
differ from fp64 by 4 E, floored at one fp32 ulp of the tensor's largest value (the rule of tests/test_gpu_update.py);
every row and ``sum`` entry that no id names keeps its bits.
"""
from __future__ import annotations

import importlib
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import _adagrad_spec as spec
from tests import test_distributed_cpu as tdc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MARGIN = 4


def _sparse(mf, opt):
    return opt.sparse if isinstance(opt, mf.optim.TowerOptimizer) else opt


def _checked_step(mf, opt, forward_backward, tag) -> int:
    """One optimiser step held to the module docstring's rule; returns how many tables it stepped."""
    sparse = _sparse(mf, opt)
    assert type(sparse) is mf.optim.RowAdagrad
    loss = forward_backward()
    assert bool(torch.isfinite(loss)), tag
    snap = []
    for group in sparse.param_groups:
        for p in group["params"]:
            pend = mf.optim._pending(p)
            if pend is None:
                continue
            ids, g, norm = pend
            snap.append((p, group, ids.clone(), g.clone(), bool(norm), p.detach().clone(), sparse.state[p]["sum"].clone()))
    opt.step()
    opt.zero_grad()
    torch.cuda.synchronize()
    for p, group, ids, g, norm, w0, s0 in snap:
        uniq, sums = spec.coalesce(ids, g, p.shape[0])
        assert len(uniq) > 0, tag
        w1, s1 = p.detach(), sparse.state[p]["sum"]
        rows = spec.check_4e(w0[uniq].cpu(), s0[uniq].cpu(), sums, w1[uniq].cpu(), s1[uniq].cpu(), normalized=norm, lr=group["lr"],
                             eps=group["eps"], wd=group["weight_decay"], margin=MARGIN)
        for name, e, dev, bound in rows:
            print(f"ADAGRAD-MODULE-E {tag} rows {tuple(p.shape)} {name}: E {e:.3e} kernel {dev:.3e} bound {bound:.3e}")
        for name, e, dev, bound in rows:
            assert dev <= bound, (tag, name, f"kernel {dev:.3e} > max(4 E = {MARGIN * e:.3e}, one ulp) = {bound:.3e}")
        assert not torch.equal(w1[uniq.to(DEV)], w0[uniq.to(DEV)]) and bool((s1[uniq.to(DEV)] >= s0[uniq.to(DEV)]).all()), tag
        rest = torch.ones(p.shape[0], dtype=torch.bool, device=DEV)
        rest[uniq.to(DEV)] = False
        assert torch.equal(w1[rest].view(torch.int32), w0[rest].view(torch.int32)), (tag, "an untouched row was written")
        assert torch.equal(s1[rest].view(torch.int32), s0[rest].view(torch.int32)), (tag, "an untouched sum entry was written")
    return len(snap)


def _no_table_sized_state(sparse) -> None:
    for group in sparse.param_groups:
        for p in group["params"]:
            state = sparse.state[p]
            assert set(state) == {"sum"} and state["sum"].numel() == p.shape[0] and state["sum"].dtype == torch.float32
            assert not any(torch.is_tensor(v) and v.numel() >= p.numel() for v in state.values())


def _catalog(rng, n_ent, R):
    return [[]] + [rng.integers(1, R, int(rng.integers(1, 9))).tolist() for _ in range(1, n_ent)]


def _world(mf, tower: str, d: int, B: int):
    """(towers, user input of step k, item ids of step k) at a few hundred rows."""
    n_users, n_items, L = 300, 400, 12
    kw = {"num_users": n_users, "num_items": n_items, "hidden_size": d}
    if tower == "hashed":
        kw.update(num_hashes=2, num_users=211, num_items=307)
    elif tower == "history":
        kw.update(user_tower="history")
    elif tower == "features":
        kw.update(user_tower="features", item_tower="features", feature_buckets=1024)
    elif tower == "transformer":
        kw.update(user_tower="transformer", num_attention_heads=4, max_position_embeddings=16)
    torch.manual_seed(3)
    towers = mf.models.init_towers(mf.models.ModelConfig(**kw), device=DEV)
    if tower == "features":
        rng = np.random.default_rng(4)
        towers["item"].set_bags(mf.data.FeatureBags.from_lists(_catalog(rng, n_items, 1024)))
        towers["user"].set_bags(mf.data.FeatureBags.from_lists(_catalog(rng, n_users, 1024)))

    def batch(k):
        g = torch.Generator().manual_seed(100 + k)
        hi = 10_000_000 if tower == "hashed" else n_items
        item = torch.randint(1, hi, (2 * B,), generator=g)
        item[:4] = item[4]                                       # duplicates
        pos = torch.randint(1, hi, (B, 4), generator=g)
        pos[:, 0] = item[:B]
        if tower in ("history", "transformer"):
            user = torch.randint(0, n_items, (B, L), generator=g)   # padded histories (0 = padding)
            user[:, 0] = torch.randint(1, n_items, (B,), generator=g)
        else:
            user = torch.randint(1, 10_000_000 if tower == "hashed" else n_users, (B,), generator=g)
            user[:3] = user[3]
        return {"user": user.to(DEV), "item": item.to(DEV), "target": torch.randint(1, 6, (B,), generator=g).to(DEV), "pos": pos.to(DEV)}

    return towers, batch


def _forward_backward(mf, towers, b):
    fn = mf.losses.InfomationNoiseContrastiveEstimationLoss(num_negatives=0)

    def run():
        loss = fn(towers["user"](b["user"]), towers["item"](b["item"]), b["target"], item_idx=b["item"], pos_idx=b["pos"])
        loss.backward()
        return loss.detach()
    return run


CASES = [("plain", 32, 32, "1"), ("plain", 128, 256, "1"), ("plain", 32, 32, "0"), ("plain", 128, 256, "0"), ("hashed", 32, 64, "1"),
         ("hashed", 128, 256, "1"), ("history", 32, 32, "1"), ("history", 128, 128, "1"), ("features", 32, 64, "1"), ("features", 128, 256, "1"),
         ("transformer", 32, 32, "1"), ("transformer", 128, 64, "1")]


@pytest.mark.parametrize(("tower", "d", "B", "pair_env"), CASES, ids=lambda v: str(v))
def test_three_steps_match_the_specification(mf, monkeypatch, tower, d, B, pair_env):
    monkeypatch.setenv("MF_UPDATE_PAIR", pair_env)
    pair_calls = []
    inner = mf.optim.row_update_pair
    monkeypatch.setattr(mf.optim, "row_update_pair", lambda *a: pair_calls.append(inner(*a)) or pair_calls[-1])
    towers, batch = _world(mf, tower, d, B)
    opt = mf.optim.tower_optimizer(towers, "adagrad", 0.05)
    assert isinstance(opt, mf.optim.TowerOptimizer) == (tower == "transformer")
    sparse = _sparse(mf, opt)
    sparse.param_groups[0]["weight_decay"] = 0.01
    sparse.init_state()
    _no_table_sized_state(sparse)
    two_tables = tower in ("plain", "hashed")
    launched = []                       # per step: the step was ONE two-table launch
    for k in range(3):
        del pair_calls[:]
        stepped = _checked_step(mf, opt, _forward_backward(mf, towers, batch(k)), f"{tower}-d{d}-B{B}-pair{pair_env}-step{k}")
        assert stepped == (2 if two_tables else 1)
        assert pair_calls in ([], [False], [True])      # (a single table: not even asked for)
        launched.append(pair_calls == [True])
    _no_table_sized_state(sparse)
    # two tables of one width in one group: ONE launch (mf_update_pair_adagrad), unless MF_UPDATE_PAIR=0
    assert launched == [two_tables and pair_env == "1"] * 3
    saved = sparse.state_dict()
    again = mf.optim.RowAdagrad([p for g in sparse.param_groups for p in g["params"]])
    again.load_state_dict(saved)
    for p in sparse.state:
        assert torch.equal(again.state[p]["sum"], sparse.state[p]["sum"])


def test_initial_accumulator_value_and_a_zero_gradient_row(mf):
    """``initial_accumulator_value`` fills ``sum``; a touched row whose gradient is zero keeps its value (eps keeps the
    division finite at s = 0)."""
    tower = mf.models.EmbeddingTower(50, 32, normalize=False, device=DEV)
    for init in (0.0, 0.25):
        opt = mf.optim.RowAdagrad(tower.parameters(), lr=0.1, initial_accumulator_value=init)
        opt.init_state()
        w0 = tower.weight.detach().clone()
        ids = torch.tensor([7, 9, 7], device=DEV)
        c = torch.ones(3, 32, device=DEV)
        c[1] = 0.0                                              # row 9: touched, zero gradient
        (tower(ids) * c).sum().backward()
        opt.step()
        s = opt.state[tower.weight]["sum"]
        assert torch.equal(tower.weight.detach()[9], w0[9]) and float(s[9]) == init and bool(torch.isfinite(tower.weight).all())
        assert float(s[7]) == init + 4.0 and float(s[0]) == init          # g = 2 per channel: mean g^2 = 4


def _catalog_features(rng, n_ent, R, hot_frac=0.4):
    lists = [[]]
    for _ in range(1, n_ent):
        toks = rng.integers(100, R, int(rng.integers(1, 13))).tolist() + rng.integers(2, 30, int(rng.integers(0, 3))).tolist()
        if rng.random() < hot_frac:
            toks.append(1)
        lists.append(toks)
    return lists


def test_captured_step_replays_bit_identically(mf):
    """The shape of tests/test_gpu_feature_tower.py's test of the same name, with RowAdagrad and five steps: nothing in the
    update depends on a step number, so the optimiser needs no ``capturable`` switch."""
    rng = np.random.default_rng(2)
    n_users, n_items, R, d, B = 300, 800, 4096, 64, 128
    lists, ulists = _catalog_features(rng, n_items, R), _catalog_features(rng, n_users, R)

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
        opt = mf.optim.RowAdagrad(towers.parameters(), lr=1e-2)
        opt.init_state()
        loss_fn = mf.losses.InfomationNoiseContrastiveEstimationLoss(num_negatives=0)

        def fn(b, towers=towers, opt=opt, loss_fn=loss_fn):
            loss = loss_fn(towers["user"](b["user"]), towers["item"](b["item"]), b["target"], item_idx=b["item"], pos_idx=b["pos"])
            loss.backward()
            opt.step()
            opt.zero_grad()
            return loss.detach()

        losses = []
        if captured:
            step = mf.graph.CapturedStep(fn, batch(0), optimizers=[opt], warmup=3)
            losses += [float(step(batch(k))) for k in (1, 2, 3, 4, 5)]
        else:
            for _ in range(3):
                fn(batch(0))
            losses += [float(fn(batch(k))) for k in (1, 2, 3, 4, 5)]
        torch.cuda.synchronize()
        out.append((towers["item"].weight.detach().clone(), opt.state[towers["item"].weight]["sum"].clone(), losses))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    assert out[0][2] == out[1][2] and float(out[0][1].max()) > 0


def test_lightning_adagrad_takes_the_three_call_path_and_trains(mf):
    """``optimizer="adagrad"`` at the reference's default shape (B = 32: the shape the one-launch step serves for SGD / Adam):
    ``FusedSmallStep`` refuses the optimiser, ``fused_training_step`` runs the three calls, and the tables train."""
    torch.manual_seed(11)
    m = mf.lightning.MatrixFactorizationLitModule({"num_users": 300, "num_items": 400, "learning_rate": 0.05, "optimizer": "adagrad"})
    m.configure_model(device=DEV)
    opt = m.configure_optimizers()
    assert type(opt) is mf.optim.RowAdagrad and opt.param_groups[0]["lr"] == 0.05
    before = {k: m.towers[k].weight.detach().clone() for k in ("user", "item")}
    data = mf.data.SyntheticInteractions(300, 400, max_positives=9, seed=5)
    losses = [float(m.fused_training_step(mf.data.to_device(data.batch(32), DEV), opt)) for _ in range(3)]
    assert m._fused is None                                     # the fallback: training_step + backward + optimizer.step()
    assert all(np.isfinite(losses))
    for k in ("user", "item"):
        w, s = m.towers[k].weight.detach(), opt.state[m.towers[k].weight]["sum"]
        moved = (w != before[k]).any(1)
        assert 0 < int(moved.sum()) < w.shape[0] and bool(torch.isfinite(w).all())
        assert torch.equal(moved, s > 0) and s.shape == (w.shape[0],)      # exactly the touched rows carry state
    assert all(p.grad is None for p in m.towers.parameters())


# --------------------------------------------------------------------------------------------- sharded trainer ----
def _relay_comm(mfd):
    class RelayComm(mfd.TorchComm):
        """torch.distributed (gloo) on host copies, as in tests/test_gpu_distributed.py."""

        def rows(self, x, send_counts, recv_counts):
            return super().rows(x.cpu(), send_counts, recv_counts).to(DEV)

        def counts(self, send):
            return super().counts(send.cpu()).to(DEV)

        def gather(self, x):
            return super().gather(x.cpu()).to(DEV)

        def equal(self, x):
            return super().equal(x.cpu()).to(DEV)

    return RelayComm()


def _sharded_case(rank: int, world: int, out_dir: str) -> None:
    mf = importlib.import_module("matrix-factorization-torch_amd")
    mfd = mf.distributed
    tr = mfd.ShardedTrainer(mf, DEV, "adagrad", 0, num_users=tdc.N_USERS, num_items=tdc.N_ITEMS, dim=tdc.DIM, lr=0.05,
                            kind="PairwiseLogisticLoss", comm=_relay_comm(mfd))
    assert isinstance(tr.ops, mfd.HipOps)
    for name, t in (("user", tr.user_table), ("item", tr.item_table)):
        assert set(tr.state[name]) == {"sum"} and tr.state[name]["sum"].shape == (t.shape[0],)      # no table-sized state
    b = {k: v.to(DEV) for k, v in tdc._batch(rank, world, mfd).items()}
    loss = tr.step(b)
    tr.finish()
    torch.cuda.synchronize()
    torch.save({"user": tr.user_table.cpu(), "item": tr.item_table.cpu(), "user_sum": tr.state["user"]["sum"].cpu(),
                "item_sum": tr.state["item"]["sum"].cpu(), "loss": loss.cpu()}, f"{out_dir}/adagrad_{rank}.pt")


def _worker(rank: int, world: int, port: int, out_dir: str) -> None:
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        _sharded_case(rank, world, out_dir)
    finally:
        dist.destroy_process_group()


def test_sharded_adagrad_world_2_matches_the_single_gpu_run(mf, tmp_path):
    """Two ranks on one card (exchanges relayed over gloo), one step: the shards put back together against ONE
    ``RowAdagrad`` step on whole tables fed both ranks' batches -- both within the 4 E rule of the fp64 specification applied
    to the single-GPU run's coalesced gradients, and ``sum`` entries of untouched rows exactly 0 in both."""
    world = 2
    mp.spawn(_worker, args=(world, tdc._free_port(), str(tmp_path)), nprocs=world, join=True)
    mfd = mf.distributed
    ops = mfd.HipOps(mf)
    std = 1.0 / tdc.DIM ** 0.5
    towers = torch.nn.ModuleDict({"user": mf.models.EmbeddingTower(tdc.N_USERS, tdc.DIM, device=DEV),
                                  "item": mf.models.EmbeddingTower(tdc.N_ITEMS, tdc.DIM, device=DEV)})
    with torch.no_grad():                                         # the virtual tables every shard was cut from
        towers["user"].weight.copy_(ops.init_rows(tdc.N_USERS, tdc.DIM, 0, 1, 0, std, DEV))
        towers["item"].weight.copy_(ops.init_rows(tdc.N_ITEMS, tdc.DIM, 0, 1, 1, std, DEV))
    opt = mf.optim.RowAdagrad(towers.parameters(), **{k: v for k, v in mfd.optimizer_hyper("adagrad", 0.05).items()})
    opt.init_state()
    fn = mf.losses.PairwiseLogisticLoss(num_negatives=0, sigma=1.0, margin=1.0)
    for r in range(world):
        b = {k: v.to(DEV) for k, v in tdc._batch(r, world, mfd).items()}
        fn(towers["user"](b["user"]), towers["item"](b["item"]), b["target"], item_idx=b["item"], pos_idx=b["pos"]).backward()
    snap = {}
    for name in ("user", "item"):
        p = towers[name].weight
        ids, g, norm = mf.optim._pending(p)
        assert norm
        snap[name] = (ids.clone(), g.clone(), p.detach().clone().cpu(), opt.state[p]["sum"].clone().cpu())
    opt.step()
    torch.cuda.synchronize()
    got = [torch.load(f"{tmp_path}/adagrad_{r}.pt") for r in range(world)]
    for name in ("user", "item"):
        p = towers[name].weight
        ids, g, w0, s0 = snap[name]
        uniq, sums = spec.coalesce(ids, g, p.shape[0])
        sharded_w, sharded_s = torch.empty_like(w0), torch.empty_like(s0)
        for r in range(world):
            sharded_w[r::world] = got[r][name]                    # rows are dealt round-robin
            sharded_s[r::world] = got[r][f"{name}_sum"]
        assert torch.equal((sharded_w != w0).any(1), sharded_s > 0)          # the touched rows, and only they
        for run, w1, s1 in (("single", p.detach().cpu(), opt.state[p]["sum"].cpu()), ("sharded", sharded_w, sharded_s)):
            for tensor, e, dev, bound in spec.check_4e(w0[uniq], s0[uniq], sums, w1[uniq], s1[uniq], normalized=True, lr=0.05, eps=1e-10,
                                                       wd=0.0, margin=MARGIN):
                print(f"ADAGRAD-SHARDED-E {run} {name} {tensor}: E {e:.3e} deviation {dev:.3e} bound {bound:.3e}")
                assert dev <= bound, (run, name, tensor, dev, bound)
            rest = torch.ones(p.shape[0], dtype=torch.bool)
            rest[uniq] = False
            assert torch.equal(w1[rest], w0[rest]) and not bool(s1[rest].any()), (run, name)
