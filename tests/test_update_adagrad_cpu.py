"""CPU: row-wise Adagrad up to where a GPU is needed -- the two exports and their host-side refusals, the specification
(tests/_adagrad_spec.py) on hand-worked rows, the Python surface (``optim.RowAdagrad``, ``tower_optimizer``, the Lightning
config), and the sharded trainer on two gloo ranks with the specification injected as the local compute."""
from __future__ import annotations

import ctypes
import importlib
import os
import pathlib
import re

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import embed as oembed
from tests import _adagrad_spec as spec
from tests import test_distributed_cpu as tdc

ROOT = pathlib.Path(__file__).resolve().parents[1]
FAKE = ctypes.c_void_p(0x1000)           # never dereferenced: every refusal is decided before any launch


# ------------------------------------------------------------------------------------------------ the C ABI ----
def test_exports_are_declared_and_bound(mf):
    header = (ROOT / "include" / "mf_hip.h").read_text()
    declared = set(re.findall(r"\b(mf_[a-z0-9_]+)\s*\(", header))
    lib = mf._lib.lib()
    for name, nargs in (("mf_update_adagrad", 14), ("mf_update_pair_adagrad", 23)):
        assert name in declared and name in mf._lib.SIGNATURES and hasattr(lib, name)
        res, args = mf._lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == nargs
        proto = re.search(rf"int {name}\(([^;]*)\);", header).group(1)
        assert len(proto.split(",")) == nargs                          # the binding has the header's argument count


def _single(lib, *, table=FAKE, state=FAKE, n_rows=100, d=32, n=4, lr=0.05, eps=1e-10, wd=0.0, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = lib.mf_update_ws_bytes(n, d)
    return lib.mf_update_adagrad(table, state, n_rows, d, FAKE, n, FAKE, 0, lr, eps, wd, FAKE, ws_bytes, None)


def _pair(lib, *, sum_a=FAKE, sum_b=FAKE, d=32, n_a=4, n_b=4, lr=0.05, eps=1e-10, wd=0.0, short=0):
    wa, wb = lib.mf_update_ws_bytes(max(n_a, 1), d if d in (32, 64, 128, 256) else 32), lib.mf_update_ws_bytes(max(n_b, 1), 32)
    return lib.mf_update_pair_adagrad(d, FAKE, sum_a, 100, FAKE, n_a, FAKE, 0, FAKE, wa, FAKE, sum_b, 100, FAKE, n_b, FAKE, 1, FAKE, wb - short,
                                      lr, eps, wd, None)


def test_host_side_refusals_name_the_export(mf):
    lib, L = mf._lib.lib(), mf._lib
    for kw, rc in (({"state": None}, L.MF_EINVAL), ({"table": None}, L.MF_EINVAL), ({"eps": 0.0}, L.MF_EINVAL), ({"eps": -1e-3}, L.MF_EINVAL),
                   ({"lr": -0.1}, L.MF_EINVAL), ({"wd": -0.1}, L.MF_EINVAL), ({"eps": float("nan")}, L.MF_EINVAL), ({"d": 48}, L.MF_EINVAL),
                   ({"n_rows": 0}, L.MF_EINVAL), ({"n": -1}, L.MF_EINVAL),
                   ({"ws_bytes": lib.mf_update_ws_bytes(4, 32) - 1}, L.MF_ENOSPC), ({"n_rows": 1 << 39}, L.MF_ENOTSUP)):
        assert _single(lib, **kw) == rc, kw
        assert b"mf_update_adagrad:" in lib.mf_last_error(), (kw, lib.mf_last_error())
    assert _single(lib, n=0) == L.MF_OK                                # an empty list: nothing to do, nothing launched
    for kw, rc in (({"sum_a": None}, L.MF_EINVAL), ({"sum_b": None}, L.MF_EINVAL), ({"eps": 0.0}, L.MF_EINVAL), ({"lr": -1.0}, L.MF_EINVAL),
                   ({"wd": -1.0}, L.MF_EINVAL), ({"d": 48}, L.MF_EINVAL), ({"short": 1}, L.MF_ENOSPC), ({"n_a": 0}, L.MF_ENOTSUP),
                   ({"n_b": 0}, L.MF_ENOTSUP), ({"n_a": 65537}, L.MF_ENOTSUP), ({"n_b": 65537}, L.MF_ENOTSUP)):
        assert _pair(lib, **kw) == rc, kw
        assert b"mf_update_pair_adagrad:" in lib.mf_last_error(), (kw, lib.mf_last_error())


# ------------------------------------------------------------------------------------------ the specification ----
@pytest.mark.parametrize("d", [32, 64, 128, 256])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_spec_on_the_exact_row(d, dtype):
    """w0 = 0, g_c = +-4, s0 = 0, lr = 0.5, eps = 4: q = 16, s = 16, w_c = -+ 0.5 * 4 / (4 + 4) = -+0.25, exactly."""
    g = torch.tensor([4.0, -4.0]).repeat(d // 2)[None]
    w, s = spec.adagrad_rows(torch.zeros(1, d), torch.zeros(1), g, normalized=False, lr=0.5, eps=4.0, wd=0.0, dtype=dtype)
    assert w.dtype == dtype and s.tolist() == [16.0]
    assert torch.equal(w, (-g / 16).to(dtype))
    # a second step with the same gradient: s = 32, w = -0.25 - 2 / (sqrt(32) + 4)
    w2, s2 = spec.adagrad_rows(w, s, g, normalized=False, lr=0.5, eps=4.0, wd=0.0, dtype=torch.float64)
    assert s2.tolist() == [32.0]
    torch.testing.assert_close(w2, -g.double() / 16 - 0.5 * g.double() / (32 ** 0.5 + 4), rtol=1e-15, atol=0)


def test_spec_weight_decay_is_coupled():
    """wd = 0.5, w0 = 2 adds exactly 1 to every g_c: g = 3 + 1 = 4, s = 16, w = 2 - 0.5 * 4 / 8 = 1.75; and with an initial
    accumulator of 9: s = 25, w = 2 - 2 / 9."""
    d = 32
    w0, g = torch.full((1, d), 2.0), torch.full((1, d), 3.0)
    w, s = spec.adagrad_rows(w0, torch.zeros(1), g, normalized=False, lr=0.5, eps=4.0, wd=0.5, dtype=torch.float32)
    assert s.tolist() == [16.0] and torch.equal(w, torch.full((1, d), 1.75))
    w, s = spec.adagrad_rows(w0, torch.full((1,), 9.0), g, normalized=False, lr=0.5, eps=4.0, wd=0.5)
    assert s.tolist() == [25.0]
    torch.testing.assert_close(w, torch.full((1, d), 2.0 - 2.0 / 9.0, dtype=torch.float64), rtol=1e-15, atol=0)
    # wd = 0 is skipped, not multiplied: an infinite weight must not poison a zero decay
    w, _ = spec.adagrad_rows(torch.full((1, d), float("inf")), torch.zeros(1), g, normalized=False, lr=0.5, eps=4.0, wd=0.0)
    assert bool(torch.isinf(w).all())


def test_spec_normalised_against_autograd():
    """normalized = 1: the gradient arrives w.r.t. w / max(|w|, 1e-12); autograd through that map in fp64 gives g."""
    gen = torch.Generator().manual_seed(11)
    d, rows = 64, 5
    w0 = torch.randn(rows, d, generator=gen, dtype=torch.float64)
    acc = torch.randn(rows, d, generator=gen, dtype=torch.float64)
    s0 = torch.rand(rows, generator=gen, dtype=torch.float64)
    leaf = w0.clone().requires_grad_()
    unit = leaf / leaf.norm(dim=1, keepdim=True).clamp_min(1e-12)
    (unit * acc).sum().backward()
    lr, eps, wd = spec.f32(0.05), spec.f32(1e-3), spec.f32(0.01)
    g = leaf.grad + wd * w0
    s_want = s0 + (g * g).mean(1)
    w_want = w0 - lr * g / (s_want.sqrt() + eps)[:, None]
    w, s = spec.adagrad_rows(w0, s0, acc, normalized=True, lr=0.05, eps=1e-3, wd=0.01)
    torch.testing.assert_close(s, s_want, rtol=1e-13, atol=0)
    torch.testing.assert_close(w, w_want, rtol=1e-13, atol=1e-15)


def test_spec_update_sums_duplicates_and_skips_bad_ids():
    table, state = torch.zeros(6, 32, dtype=torch.float64), torch.zeros(6, dtype=torch.float64)
    ids = torch.tensor([4, -1, 4, 6, 1])
    grad = torch.stack([torch.full((32,), v) for v in (1.0, float("nan"), 3.0, float("nan"), -4.0)]).double()
    spec.adagrad_update(table, state, ids, grad, normalized=False, lr=0.5, eps=4.0, wd=0.0)
    assert state.tolist() == [0, 16, 0, 0, 16, 0]
    assert torch.equal(table[4], torch.full((32,), -0.25).double()) and torch.equal(table[1], torch.full((32,), 0.25).double())
    assert not table[[0, 2, 3, 5]].any()


# ------------------------------------------------------------------------------------------ the Python surface ----
def test_row_adagrad_arguments(mf):
    p = torch.nn.Parameter(torch.zeros(7, 32))
    opt = mf.optim.RowAdagrad([p])
    assert isinstance(opt, torch.optim.Optimizer) and isinstance(opt, mf.optim._SparseRowOptimizer)
    ref = torch.optim.Adagrad([torch.nn.Parameter(torch.zeros(1))])
    for key in ("lr", "eps", "weight_decay", "initial_accumulator_value"):
        assert opt.defaults[key] == ref.defaults[key], key               # torch.optim.Adagrad's defaults
    for kw in ({"lr": -1.0}, {"eps": 0.0}, {"eps": -1e-3}, {"weight_decay": -0.1}, {"initial_accumulator_value": -1.0}, {"lr": float("nan")}):
        with pytest.raises(ValueError):
            mf.optim.RowAdagrad([p], **kw)
    opt = mf.optim.RowAdagrad([p], lr=0.1, initial_accumulator_value=0.5)
    opt.init_state()
    s = opt.state[p]["sum"]
    assert s.shape == (7,) and s.dtype == torch.float32 and s.tolist() == [0.5] * 7
    assert not any(torch.is_tensor(v) and v.numel() >= p.numel() for v in opt.state[p].values())      # no table-sized state
    s[3] = 2.0
    saved = opt.state_dict()
    again = mf.optim.RowAdagrad([p], lr=0.3)
    again.load_state_dict(saved)
    assert again.param_groups[0]["lr"] == 0.1 and torch.equal(again.state[p]["sum"], s)
    again.init_state()                                                  # (keeps what was loaded)
    assert again.state[p]["sum"][3] == 2.0


def test_tower_optimizer_and_lightning_config(mf):
    towers = mf.models.init_towers(mf.models.ModelConfig(num_users=30, num_items=40, hidden_size=32))
    opt = mf.optim.tower_optimizer(towers, "adagrad", 0.02)
    assert type(opt) is mf.optim.RowAdagrad and opt.param_groups[0]["lr"] == 0.02
    assert len(opt.param_groups[0]["params"]) == 2
    with pytest.raises(ValueError, match="'adam', 'sgd' or 'adagrad'"):
        mf.optim.tower_optimizer(towers, "rmsprop", 0.1)
    cfg = mf.lightning.MatrixFactorizationLitConfig(optimizer="adagrad", num_users=20, num_items=50)
    assert mf.lightning.MatrixFactorizationLitConfig.model_validate(cfg.model_dump()).optimizer == "adagrad"
    module = mf.lightning.MatrixFactorizationLitModule(cfg.model_dump())
    module.configure_model()
    opt = module.configure_optimizers()
    assert type(opt) is mf.optim.RowAdagrad and opt.param_groups[0]["lr"] == cfg.learning_rate
    xf = mf.lightning.MatrixFactorizationLitModule({"user_tower": "transformer", "num_items": 50, "hidden_size": 32, "optimizer": "adagrad"})
    xf.configure_model()
    opt = xf.configure_optimizers()
    assert isinstance(opt, mf.optim.TowerOptimizer) and type(opt.sparse) is mf.optim.RowAdagrad and isinstance(opt.dense, torch.optim.AdamW)
    # the fused one-launch step keeps refusing it: fused_training_step then runs the three calls
    with pytest.raises(mf.MfHipError, match="SparseSGD or optim.RowAdam"):
        mf.fused.FusedSmallStep(towers, mf.optim.RowAdagrad(towers.parameters()), None)
    hyper = mf.distributed.optimizer_hyper("adagrad", 0.05)
    assert hyper == {"lr": 0.05, "eps": 1e-10, "weight_decay": 0.0, "initial_accumulator_value": 0.0}


# ------------------------------------------------------------------------------------------- sharded trainer ----
STEPS = 2


class AdagradOps(tdc.OracleOps):
    """The oracle ops with the Adagrad branch of the specification."""

    def update(self, optimizer, table, state, ids, grad, normalized, step, hyper):
        if optimizer != "adagrad":
            return super().update(optimizer, table, state, ids, grad, normalized, step, hyper)
        spec.adagrad_update(table, state["sum"], ids, grad, normalized=bool(normalized), lr=hyper["lr"], eps=hyper["eps"],
                            wd=hyper["weight_decay"])


def _adagrad_case(rank: int, world: int, out_dir: str) -> None:
    mf = importlib.import_module("matrix-factorization-torch_amd")
    mfd = mf.distributed
    tr = mfd.ShardedTrainer(mf, "cpu", "adagrad", 0, num_users=tdc.N_USERS, num_items=tdc.N_ITEMS, dim=tdc.DIM, ops=AdagradOps(), lr=0.05,
                            kind="PairwiseLogisticLoss")
    for name, t in (("user", tr.user_table), ("item", tr.item_table)):
        assert set(tr.state[name]) == {"sum"} and tr.state[name]["sum"].shape == (t.shape[0],)       # one float per LOCAL row, nothing table-sized
    losses = [tr.step(tdc._batch(rank, world, mfd, "routed", salt=j)) for j in range(STEPS)]
    tr.finish()
    torch.save({"user": tr.user_table, "item": tr.item_table, "user_sum": tr.state["user"]["sum"], "item_sum": tr.state["item"]["sum"],
                "loss": torch.stack(losses)}, f"{out_dir}/adagrad_{rank}.pt")


def _worker(rank: int, world: int, port: int, out_dir: str) -> None:
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        _adagrad_case(rank, world, out_dir)
    finally:
        dist.destroy_process_group()


def test_sharded_adagrad_matches_single_process(mf, tmp_path):
    """Two gloo ranks, example-sharded batches, two steps: the shards put back together equal ONE process applying every
    rank's gradients (from the same pre-step tables) in a single specification update per table -- tables and ``sum``."""
    world = 2
    torch.set_num_threads(1)
    mp.spawn(_worker, args=(world, tdc._free_port(), str(tmp_path)), nprocs=world, join=True)
    mfd = mf.distributed
    std = 1.0 / tdc.DIM ** 0.5
    ut, it = oembed.init_rows(tdc.N_USERS, tdc.DIM, 0, 1, 0, std), oembed.init_rows(tdc.N_ITEMS, tdc.DIM, 0, 1, 1, std)
    us, its = torch.zeros(tdc.N_USERS), torch.zeros(tdc.N_ITEMS)
    ops, hyper = AdagradOps(), mfd.optimizer_hyper("adagrad", 0.05)
    losses = []
    for j in range(STEPS):
        u_ids, u_g, i_ids, i_g = [], [], [], []
        for r in range(world):
            b = tdc._batch(r, world, mfd, "routed", salt=j)
            loss, du, dv = ops.loss_and_grads("PairwiseLogisticLoss", oembed.gather(ut, b["user"], True), oembed.gather(it, b["item"], True),
                                              b["target"], b["item"], b["pos"], None, 0, 1.0, 1.0)
            u_ids.append(b["user"]); u_g.append(du); i_ids.append(b["item"]); i_g.append(dv); losses.append(loss)
        ops.update("adagrad", ut, {"sum": us}, torch.cat(u_ids), torch.cat(u_g), True, j + 1, hyper)
        ops.update("adagrad", it, {"sum": its}, torch.cat(i_ids), torch.cat(i_g), True, j + 1, hyper)
    assert float(us.max()) > 0 and float(its.max()) > 0 and int((us == 0).sum()) > 0       # touched rows moved, untouched ones did not
    got = [torch.load(f"{tmp_path}/adagrad_{r}.pt") for r in range(world)]
    for name, want in (("user", ut), ("item", it), ("user_sum", us), ("item_sum", its)):
        full = torch.empty_like(want)
        for r in range(world):
            full[r::world] = got[r][name]                                # rows are dealt round-robin
        torch.testing.assert_close(full, want, rtol=1e-5, atol=1e-6)
        if name.endswith("_sum"):
            assert torch.equal(full == 0, want == 0), name               # an untouched row keeps its initial value exactly
    for r in range(world):
        torch.testing.assert_close(got[r]["loss"], torch.stack(losses[r::world]), rtol=1.3e-6, atol=1e-5)
