"""GPU: streaming logQ (csrc/mf_logq.hip, ``logq.StreamingLogQ``, the Lightning module's ``logq_mode="streaming"``) against
the numpy rule (tests/_logq_spec.py).

What a step is held to: after EVERY step of a 40-step sequence ``last_seen`` and ``gap`` are bit-equal to the rule's;
``table`` / ``out_logq`` are within 1e-5 absolute of float64 ``-log(gap)`` of the rule (|logq| < ln 2^31 = 21.5, where fp32
values are 1.9e-6 apart: about 5 ulp at the largest magnitude, a tenth of the 1e-4 the loss tests resolve); rows that no id
names keep their bits, and so do guard words past the arrays' ends.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

from tests import _logq_spec as spec

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5
GUARD = 64
NS = (1, 63, 64, 65, 255, 256, 257, 1025, 16_384)
KINDS = ("distinct", "zipf", "one", "stray")
POISON_TABLE = 123.25
WORST = {"logf": 0.0}


def _ids(rng, kind: str, n: int, rows: int) -> np.ndarray:
    if kind == "distinct" and n <= rows:
        return rng.permutation(rows)[:n].astype(np.int64)
    if kind == "one":
        return np.full(n, int(rng.integers(0, rows)), dtype=np.int64)
    p = 1.0 / np.arange(1, rows + 1)
    ids = rng.choice(rows, n, p=p / p.sum()).astype(np.int64)              # Zipf duplicates
    if kind == "stray":                                                   # ids out of range and negative among them
        where = rng.random(n) < 0.3
        stray = rng.choice(np.array([-1, -2**40, rows, rows + 1, 2**31, 2**39 - 1, -rows], dtype=np.int64), n)
        ids = np.where(where, stray, ids)
    return ids


def _steps(count: int) -> list[int]:
    """Strictly increasing step numbers with jumps, one of them above 2^24."""
    rng = np.random.default_rng(7)
    jumps = rng.integers(1, 6, count)
    jumps[count // 2] = (1 << 24) + 3
    return np.cumsum(jumps).tolist()


class Raw:
    """The C ABI on arrays with guard words behind them, next to the rule fed the same calls."""

    def __init__(self, mf, rows: int, alpha: float, hashes: int = 0, seed: int = 0, prior: bool = False) -> None:
        self.mf, self.lib, self.rows, self.alpha, self.hashes, self.seed = mf, mf._lib.lib(), rows, alpha, hashes, seed
        self.spec = spec.Spec(rows, alpha=alpha, num_hashes=hashes, seed=seed)
        size = rows * max(hashes, 1)
        if prior:                        # a state some earlier steps left: half the rows seen at steps 1..3
            rng = np.random.default_rng(rows)
            seen = rng.random(size) < 0.5
            self.spec.last_seen.reshape(-1)[:] = np.where(seen, rng.integers(1, 4, size), 0)
            self.spec.gap.reshape(-1)[:] = np.where(seen, rng.random(size) * 8 + 0.5, 0).astype(np.float32)
        self.last = torch.full((size + GUARD,), -77, dtype=torch.int32, device=DEV)
        self.gap = torch.full((size + GUARD,), -5.5, dtype=torch.float32, device=DEV)
        self.table = torch.full((size + GUARD,), POISON_TABLE, dtype=torch.float32, device=DEV)
        self.last[:size] = torch.from_numpy(self.spec.last_seen.reshape(-1)).to(DEV)
        self.gap[:size] = torch.from_numpy(self.spec.gap.reshape(-1)).to(DEV)
        self.size = size
        self.touched = np.zeros(size, dtype=bool)
        self.t_dev = torch.zeros(1, dtype=torch.int64, device=DEV)

    def update(self, ids: np.ndarray, t: int, *, on_device: bool, want_rows: bool):
        dev_ids = torch.from_numpy(ids).to(DEV)
        out = torch.full((len(ids) + 1,), 9.0, dtype=torch.float32, device=DEV) if want_rows else None
        if on_device:
            self.t_dev.fill_(t)
        rc = self.lib.mf_logq_update(self.last.data_ptr(), self.gap.data_ptr(), self.rows, self.hashes, self.seed,
                                     dev_ids.data_ptr() if len(ids) else None, len(ids), -5 if on_device else t,
                                     self.t_dev.data_ptr() if on_device else None, self.alpha,
                                     self.table.data_ptr() if self.hashes == 0 else None, None if out is None else out.data_ptr(), None)
        self.mf._lib.check(rc)
        want = self.spec.update(ids, t)
        slots, ok = self.spec.slots(ids)
        self.touched[slots[ok].reshape(-1)] = True
        torch.cuda.synchronize()
        if out is not None:
            got = out.cpu().numpy()
            assert got[-1] == 9.0, "the read-out wrote past its n rows"
            self.close(got[:-1], want, f"out_logq at t = {t}")
        return want

    def close(self, got: np.ndarray, want: np.ndarray, what: str) -> None:
        dev = float(np.abs(got.astype(np.float64) - want).max()) if len(want) else 0.0
        WORST["logf"] = max(WORST["logf"], dev)
        assert dev <= TOL, (what, dev)
        assert np.array_equal(got == 0.0, want == 0.0), what                    # exactly 0 where there is no estimate (or gap = 1)

    def check(self, what) -> None:
        last, gap = self.last.cpu().numpy(), self.gap.cpu().numpy()
        assert np.array_equal(last[:self.size], self.spec.last_seen.reshape(-1)), (what, "last_seen")
        assert np.array_equal(gap[:self.size].view(np.int32), self.spec.gap.reshape(-1).view(np.int32)), (what, "gap")
        assert bool((last[self.size:] == -77).all()) and bool((gap[self.size:] == -5.5).all()), (what, "guard words")
        if self.hashes == 0:
            table = self.table.cpu().numpy()
            assert bool((table[self.size:] == POISON_TABLE).all()) and bool((table[:self.size][~self.touched] == POISON_TABLE).all()), what
            rows = np.flatnonzero(self.touched)
            self.close(table[rows], self.spec.logq(rows), f"table {what}")


@pytest.mark.parametrize("on_device", [False, True], ids=["host_t", "t_dev"])
@pytest.mark.parametrize("alpha", [0.01, 0.5, 1.0])
@pytest.mark.parametrize("rows", [1, 33, 1000, 70_001])
def test_direct_mode_forty_steps(mf, rows, alpha, on_device):
    raw = Raw(mf, rows, alpha, prior=True)
    rng = np.random.default_rng(rows + int(alpha * 100))
    steps = _steps(40)
    steps = [t + 3 for t in steps]                           # (behind the prior state's steps)
    peak = 0.0
    for s, t in enumerate(steps):
        n, kind = NS[s % len(NS)], KINDS[s % len(KINDS)]
        ids = _ids(rng, kind, n, rows)
        raw.update(ids, t, on_device=on_device, want_rows=s % 3 != 2)
        raw.check((rows, alpha, s, t, n, kind))
        peak = max(peak, float(raw.spec.gap.max()))
        if s % 5 == 4:                                      # the same t once more: same ids (nothing moves), then other ids
            before = (raw.last.clone(), raw.gap.clone(), raw.table.clone())
            raw.update(ids, t, on_device=on_device, want_rows=True)
            assert all(torch.equal(a, b) for a, b in zip(before, (raw.last, raw.gap, raw.table))), (s, "the same t twice moved something")
            raw.update(_ids(rng, "zipf", 257, rows), t, on_device=on_device, want_rows=True)
            raw.check((rows, alpha, s, t, "same t, other ids"))
    print(f"LOGQ-LOGF rows {rows} alpha {alpha}: largest |fp32 read-out - float64 -log(gap)| so far {WORST['logf']:.3e}")
    assert int(raw.spec.last_seen.max()) > 1 << 24 and peak > 1e5          # (the sequence met the gap above 2^24: alpha 2^24 >= 1.6e5)


def test_sixteen_thousand_copies_of_one_id_and_all_distinct(mf):
    """The two ends of a wave's duplicate handling, with it switched off and at its deepest as well (``mf_logq_set_peel``:
    speed only -- the state is the rule's whatever the setting)."""
    lib = mf._lib.lib()
    try:
        for peel in (0, 1, 4, 8):
            lib.mf_logq_set_peel(peel)
            raw = Raw(mf, 70_001, 0.5)
            rng = np.random.default_rng(peel)
            for s, t in enumerate((1, 2, 5, 6, 40)):
                ids = np.full(16_384, 4242, dtype=np.int64) if s % 2 == 0 else rng.permutation(70_001)[:16_384].astype(np.int64)
                if s == 4:                                   # pairs, triples, ... of equal ids inside every wave
                    ids = np.repeat(rng.permutation(70_001)[:4096], 4).astype(np.int64)[rng.permutation(16_384)]
                raw.update(ids, t, on_device=False, want_rows=True)
                raw.check((peel, s))
    finally:
        lib.mf_logq_set_peel(4)


def test_n_zero_launches_nothing(mf):
    raw = Raw(mf, 33, 0.5, prior=True)
    before = (raw.last.clone(), raw.gap.clone(), raw.table.clone())
    raw.update(np.zeros(0, dtype=np.int64), 9, on_device=False, want_rows=True)
    raw.update(np.zeros(0, dtype=np.int64), 10, on_device=True, want_rows=False)
    assert all(torch.equal(a, b) for a, b in zip(before, (raw.last, raw.gap, raw.table)))


def test_a_device_step_outside_the_range_updates_nothing(mf):
    raw = Raw(mf, 33, 0.5, prior=True)
    before = (raw.last.clone(), raw.gap.clone(), raw.table.clone())
    ids = torch.arange(33, device=DEV)
    for t in (0, -3, 1 << 31, 1 << 40):
        raw.t_dev.fill_(t)
        mf._lib.check(raw.lib.mf_logq_update(raw.last.data_ptr(), raw.gap.data_ptr(), 33, 0, 0, ids.data_ptr(), 33, 1, raw.t_dev.data_ptr(),
                                             0.5, raw.table.data_ptr(), None, None))
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, (raw.last, raw.gap, raw.table)))


def _device_buckets(mf, ids: np.ndarray, hashes: int, seed: int, m: int) -> np.ndarray:
    dev_ids = torch.from_numpy(ids).to(DEV)
    out = torch.empty(len(ids) * hashes, dtype=torch.int64, device=DEV)
    mf._lib.check(mf._lib.lib().mf_hash_buckets(dev_ids.data_ptr(), len(ids), hashes, seed, m, out.data_ptr(), None))
    return out.cpu().numpy().reshape(len(ids), hashes)


@pytest.mark.parametrize("m", [1, 17, 4096])
@pytest.mark.parametrize("hashes", [1, 2, 4])
def test_hashed_mode_forty_steps(mf, hashes, m):
    seed = 1234 + hashes
    raw = Raw(mf, m, 0.5 if m == 17 else 0.05, hashes=hashes, seed=seed)
    rng = np.random.default_rng(hashes * 10_000 + m)
    pool = np.concatenate([rng.integers(0, 2**39, 3000), [0, 1, 2**39 - 1, 2**39 - 2]]).astype(np.int64)
    assert np.array_equal(_device_buckets(mf, pool, hashes, seed, m), spec.hash_buckets(pool, hashes, seed, m))
    p = 1.0 / np.arange(1, len(pool) + 1)
    p /= p.sum()
    for s, t in enumerate(_steps(40)):
        n = NS[s % len(NS)]
        ids = pool[rng.choice(len(pool), n, p=p)]
        if s % 4 == 3:
            ids = np.where(rng.random(n) < 0.25, -rng.integers(1, 2**39, n), ids)          # negative ids are ignored
        want = raw.update(ids, t, on_device=s % 2 == 1, want_rows=True)                     # out_logq == the maximum rule
        raw.check((hashes, m, s, t, n))
        state = (raw.last.clone(), raw.gap.clone())
        probe = np.concatenate([ids[:50], pool[rng.integers(0, len(pool), 50)], [-1]]).astype(np.int64)
        dev_probe = torch.from_numpy(probe).to(DEV)
        got = torch.full((len(probe) + 1,), 9.0, dtype=torch.float32, device=DEV)
        mf._lib.check(raw.lib.mf_logq_lookup(raw.gap.data_ptr(), m, hashes, seed, dev_probe.data_ptr(), len(probe), got.data_ptr(), None))
        got = got.cpu().numpy()
        raw.close(got[:-1], raw.spec.logq(probe), "lookup")
        assert got[-1] == 9.0 and got[len(probe) - 1] == 0.0 and len(want) == n
        assert torch.equal(state[0], raw.last) and torch.equal(state[1], raw.gap), "lookup changed the state"
    if m == 1:
        assert int((raw.spec.last_seen > 0).sum()) == hashes           # everything collides: one bucket per hash


def test_lookup_equals_the_updates_read_out_bit_for_bit(mf):
    for hashes, m in ((0, 1000), (2, 64), (4, 4096)):
        est = mf.StreamingLogQ(m, alpha=0.3, num_hashes=hashes, seed=3, device=DEV)
        g = torch.Generator().manual_seed(hashes)
        for _ in range(6):
            ids = torch.randint(-5, 2000, (777,), generator=g).to(DEV)
            out = est.update(ids)
            state = {k: v.clone() for k, v in est.state_dict().items()}
            assert torch.equal(est.lookup(ids).view(torch.int32), out.view(torch.int32))
            assert all(torch.equal(v, est.state_dict()[k]) for k, v in state.items())
        if hashes == 0:
            assert torch.equal(est.table[ids.clamp(0, m - 1)][(ids >= 0) & (ids < m)], out[(ids >= 0) & (ids < m)])


# ---------------------------------------------------------------------------------------------------- the class ----
def _stream(k: int, hi: int = 5000, n: int = 1500) -> torch.Tensor:
    g = torch.Generator().manual_seed(100 + k)
    return (torch.rand(n, generator=g) ** 3 * hi).to(torch.int64).to(DEV)


def _same(a, b) -> bool:
    sa, sb = a.state_dict(), b.state_dict()
    return set(sa) == set(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)


@pytest.mark.parametrize("hashes", [0, 2])
def test_class_runs_are_identical_reset_and_state_dict(mf, hashes):
    make = lambda: mf.StreamingLogQ(4096, alpha=0.1, num_hashes=hashes, seed=9, device=DEV)      # noqa: E731
    a, b = make(), make()
    outs = []
    for k in range(6):
        oa, ob = a.update(_stream(k)), b.update(_stream(k))
        assert torch.equal(oa.view(torch.int32), ob.view(torch.int32))
        outs.append(oa)
    assert _same(a, b) and int(a.step) == 6 and bool((a.gap > 0).any())
    ref = spec.Spec(4096, alpha=0.1, num_hashes=hashes, seed=9)
    for k in range(6):
        ref.update(_stream(k).cpu().numpy(), k + 1)
    assert np.array_equal(a.last_seen.cpu().numpy(), ref.last_seen) and np.array_equal(a.gap.cpu().numpy().view(np.int32), ref.gap.view(np.int32))
    fresh = make()
    fresh.load_state_dict(a.state_dict())                    # round trip into a fresh instance: it continues bit-equal
    for k in range(6, 9):
        assert torch.equal(fresh.update(_stream(k)).view(torch.int32), a.update(_stream(k)).view(torch.int32))
    assert _same(fresh, a) and int(fresh.step) == 9
    a.reset()
    assert _same(a, make()) and int(a.step) == 0
    for k in range(6):                                       # and from there the same run again
        assert torch.equal(a.update(_stream(k)).view(torch.int32), outs[k].view(torch.int32))
    assert _same(a, b)


@pytest.mark.parametrize("hashes", [0, 2])
def test_captured_update_replays_like_eager_calls(mf, hashes):
    make = lambda: mf.StreamingLogQ(4096, alpha=0.1, num_hashes=hashes, seed=9, device=DEV)      # noqa: E731
    make().update(_stream(0))                                # (the library is loaded and its kernels resident before a capture)
    eager, replayed = make(), make()
    static = _stream(0).clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = replayed.update(static)
    assert int(replayed.step) == 0 and not bool(replayed.last_seen.any())       # a capture runs nothing
    for k in range(5):
        static.copy_(_stream(k))
        graph.replay()
        want = eager.update(_stream(k))
        assert torch.equal(out.view(torch.int32), want.view(torch.int32)), k
    assert _same(eager, replayed) and int(replayed.step) == 5


# ------------------------------------------------------------------------------------------------------ the loss ----
def test_infonce_reads_the_estimators_table_and_rows(mf):
    b, n, d, rows = 64, 128, 64, 500
    g = torch.Generator().manual_seed(4)
    u0 = torch.nn.functional.normalize(torch.randn(b, d, generator=g), dim=1).to(DEV)
    v0 = torch.nn.functional.normalize(torch.randn(n, d, generator=g), dim=1).to(DEV)
    target = torch.randint(1, 6, (b,), generator=g).to(DEV)
    fn = mf.losses.InfomationNoiseContrastiveEstimationLoss(num_negatives=0)

    def run(**kw):
        u, v = u0.clone().requires_grad_(), v0.clone().requires_grad_()
        loss = fn(u, v, target, item_idx=item, pos_idx=pos, **kw)
        loss.backward()
        return loss.detach(), u.grad, v.grad

    for hashes, m in ((0, rows), (2, 64)):
        est = mf.StreamingLogQ(m, alpha=0.2, num_hashes=hashes, seed=1, device=DEV)
        ref = spec.Spec(m, alpha=0.2, num_hashes=hashes, seed=1)
        for k in range(7):
            item = (torch.rand(n, generator=g) ** 2 * rows).to(torch.int64)
            ref.update(item.numpy(), k + 1)
            got_rows = est.update(item.to(DEV))
        item = item.to(DEV)
        pos = item[:b, None].clone()
        want_rows = torch.from_numpy(ref.logq(item.cpu().numpy())).to(torch.float32).to(DEV)
        assert float(want_rows.min()) < -0.5
        if hashes == 0:
            got = run(logq_table=est.table)
            want = run(logq_table=torch.from_numpy(ref.table()).to(torch.float32).to(DEV))
        else:
            got, want = run(logq=got_rows), run(logq=want_rows)
        plain = run()
        assert abs(float(got[0]) - float(plain[0])) > 1e-3                     # (the correction is not a no-op here)
        for x, y, name in zip(got, want, ("loss", "dU", "dV")):
            dev = float((x - y).abs().max())
            print(f"LOGQ-LOSS hashes {hashes} {name}: |estimator - rule| {dev:.3e}")
            assert dev <= TOL, (hashes, name, dev)


# ---------------------------------------------------------------------------------------------------- the module ----
CFG = {"num_users": 300, "num_items": 400, "learning_rate": 0.05, "use_logq": True, "logq_mode": "streaming", "logq_alpha": 0.25,
       "train_loss": "InfomationNoiseContrastiveEstimationLoss"}


def _module(mf, seed=11, **kw):
    torch.manual_seed(seed)
    m = mf.lightning.MatrixFactorizationLitModule({**CFG, **kw})
    m.configure_model(device=DEV)
    return m, m.configure_optimizers()


def _item_idx(batch) -> np.ndarray:
    return torch.cat([batch["item"]["idx"], batch["neg_item"]["idx"]]).cpu().numpy()


def _three_calls(m, opt, batch) -> torch.Tensor:
    loss = m.training_step(batch)
    loss.backward()
    opt.step()
    opt.zero_grad(set_to_none=True)
    return loss.detach()


def _estimator_is(est, ref) -> None:
    assert np.array_equal(est.last_seen.cpu().numpy(), ref.last_seen)
    assert np.array_equal(est.gap.cpu().numpy().view(np.int32), ref.gap.view(np.int32))


def test_module_direct_mode_follows_the_rule_and_validation_advances_nothing(mf):
    m, opt = _module(mf)
    est = m.logq_estimator
    assert isinstance(est, mf.StreamingLogQ) and est.num_hashes == 0 and est.num_buckets == 400 and est.alpha == 0.25
    assert m.logq is est.table and "logq_estimator.gap" in m.state_dict()
    ref = spec.Spec(400, alpha=0.25)
    data = mf.data.SyntheticInteractions(300, 400, max_positives=9, seed=5)
    for k in range(5):
        batch = mf.data.to_device(data.batch(32), DEV)
        val = m.compute_losses(batch, step_name="val")                        # before the step: the estimate as it stands
        assert int(est.step) == k and all(bool(torch.isfinite(v)) for v in val.values())
        m.eval()
        m.compute_losses(batch, step_name="train")                            # not training: nothing advances either
        m.train()
        assert int(est.step) == k
        _three_calls(m, opt, batch)
        ref.update(_item_idx(batch), k + 1)
        assert int(est.step) == k + 1 and m.logq is est.table
        _estimator_is(est, ref)
        dev = float(np.abs(m.logq.cpu().numpy().astype(np.float64) - ref.table()).max())
        assert dev <= TOL, (k, dev)
    assert float(m.logq.min()) < 0.0 and int((m.logq == 0).sum()) > 0          # some rows estimated, some never seen


def test_module_fused_step_updates_the_estimator_ahead_of_the_one_launch(mf):
    (ma, oa), (mb, ob) = _module(mf), _module(mf)
    data = mf.data.SyntheticInteractions(300, 400, max_positives=9, seed=5)
    for k in range(4):
        batch = mf.data.to_device(data.batch(32), DEV)
        want = _three_calls(ma, oa, batch)
        got = mb.fused_training_step(batch, ob)
        assert float(got) == float(want), k
        for name in ("user", "item"):
            assert torch.equal(ma.towers[name].weight, mb.towers[name].weight), (k, name)
        assert _same(ma.logq_estimator, mb.logq_estimator) and torch.equal(ma.logq, mb.logq) and int(mb.logq_estimator.step) == k + 1
    assert mb._fused is not None and mb._fused.fused_steps == 4 and mb._fused.fallback_steps == 0


def test_module_hashed_mode_trains_through_the_three_calls(mf):
    (ma, oa), (mb, ob) = _module(mf, logq_buckets=64, logq_hashes=3), _module(mf, logq_buckets=64, logq_hashes=3)
    est = mb.logq_estimator
    assert est.num_hashes == 3 and est.num_buckets == 64 and mb.logq is None
    ref = spec.Spec(64, alpha=0.25, num_hashes=3, seed=est.seed)
    data = mf.data.SyntheticInteractions(300, 400, max_positives=9, seed=5)
    before = mb.towers["item"].weight.detach().clone()
    for k in range(4):
        batch = mf.data.to_device(data.batch(32), DEV)
        want = _three_calls(ma, oa, batch)
        got = mb.fused_training_step(batch, ob)
        ref.update(_item_idx(batch), k + 1)
        assert mb._fused is None and float(got) == float(want) and bool(torch.isfinite(got))
        _estimator_is(est, ref)
        rows = est.lookup(torch.from_numpy(_item_idx(batch)).to(DEV)).cpu().numpy()
        assert float(np.abs(rows.astype(np.float64) - ref.logq(_item_idx(batch))).max()) <= TOL
        step = int(est.step)
        mb.compute_losses(batch, step_name="val")                             # evaluation: lookup, nothing advances
        assert int(est.step) == step == k + 1
    assert not torch.equal(before, mb.towers["item"].weight) and torch.equal(ma.towers["item"].weight, mb.towers["item"].weight)
    # the rows reach the loss: the same towers without the correction give another loss
    mc, _ = _module(mf, use_logq=False, logq_mode="table")
    mc.towers.load_state_dict(mb.towers.state_dict())
    key = "val/InfomationNoiseContrastiveEstimationLoss"
    with torch.no_grad():
        assert float(mc.compute_losses(batch, step_name="val")[key]) != float(mb.compute_losses(batch, step_name="val")[key])


def test_module_save_and_load_restore_the_estimator(mf, tmp_path):
    for kw in ({}, {"logq_buckets": 128, "logq_hashes": 2}):
        m, opt = _module(mf, **kw)
        data = mf.data.SyntheticInteractions(300, 400, max_positives=9, seed=5)
        for _ in range(3):
            _three_calls(m, opt, mf.data.to_device(data.batch(32), DEV))
        path = tmp_path / f"saved_{len(kw)}"
        m.save(path)
        assert (path / mf.params.LOGQ_PATH).exists()
        back = mf.lightning.MatrixFactorizationLitModule.load(path, device=DEV)
        assert _same(back.logq_estimator, m.logq_estimator) and int(back.logq_estimator.step) == 3
        batch = mf.data.to_device(data.batch(32), DEV)
        ob = back.configure_optimizers()
        assert float(_three_calls(back, ob, batch)) == float(_three_calls(m, opt, batch))      # and goes on from there
        assert _same(back.logq_estimator, m.logq_estimator)
        if not kw:
            assert back.logq is back.logq_estimator.table


def test_table_mode_modules_are_as_before(mf, tmp_path):
    m, opt = _module(mf, logq_mode="table")
    assert m.logq_estimator is None and m.logq is None and not any("logq" in k for k in m.state_dict())
    m.logq = torch.linspace(-3.0, -1.0, 400, device=DEV)
    table = m.logq.clone()
    data = mf.data.SyntheticInteractions(300, 400, max_positives=9, seed=5)
    for _ in range(2):
        m.fused_training_step(mf.data.to_device(data.batch(32), DEV), opt)
    assert m._fused is not None and m._fused.fused_steps == 2 and torch.equal(m.logq, table)
    m.save(tmp_path / "plain")
    assert not (tmp_path / "plain" / mf.params.LOGQ_PATH).exists()
    back = mf.lightning.MatrixFactorizationLitModule.load(tmp_path / "plain", device=DEV)
    assert back.logq_estimator is None and back.logq is None
