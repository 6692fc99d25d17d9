#!/usr/bin/env python3
"""What the streaming logQ estimator costs on the device.

    python tools/logq_probe.py [--out profiles/logq_probe.json]

1. Device microseconds per ``StreamingLogQ.update`` (HIP events around ITERS calls, REGIONS such regions after warm-up; median
   and spread = max - min), n = 16,384 Zipf(1) ids per call, a new batch every call: direct over 62,423 rows and hashed into
   M = 2^20 buckets x 2 hashes; each with the rows read back (two launches) and, direct mode, without (one launch, what the
   Lightning module's step uses); with the wave-level duplicate peel at its default and switched off (``mf_logq_set_peel``);
   and 16,384 copies of one id.  Baseline: the same rule written with torch ops (unique, gather, where, scatter; the hashed
   one takes its buckets from ``mf_hash_buckets``) on the same device; all arms alternate region by region in one process.
2. The C3 training step (InfoNCE + logQ, row-Adam, d = 128, 162,541 users x 62,424 item rows, B = 8192 pairs:
   ``training_step`` + backward + ``optimizer.step``) with ``logq_mode="table"`` against ``"streaming"`` -- alternating regions,
   the overhead in microseconds and in per cent of the step.
"""
from __future__ import annotations

import argparse
import importlib
import json
import pathlib
import statistics
import sys

import torch

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
DEV = "cuda:0"
N_IDS, ROWS, HASHED_M, HASHED_H, ALPHA = 16_384, 62_423, 1 << 20, 2, 0.01
ITERS, REGIONS, WARMUP, POOL = 200, 7, 50, 32


def region_us(fn, iters: int) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for k in range(iters):
        fn(k)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1000.0 / iters


def alternate(arms: dict, iters: int = ITERS, regions: int = REGIONS, warmup: int = WARMUP) -> dict:
    for fn in arms.values():
        for k in range(warmup):
            fn(k)
    torch.cuda.synchronize()
    runs = {name: [] for name in arms}
    for _ in range(regions):
        for name, fn in arms.items():
            runs[name].append(region_us(fn, iters))
    return {name: {"us": statistics.median(r), "spread_us": max(r) - min(r), "min_us": min(r), "regions": len(r), "iters": iters}
            for name, r in runs.items()}


def zipf_batches(rows: int, pool: int = POOL) -> list[torch.Tensor]:
    g = torch.Generator().manual_seed(0)
    p = 1.0 / torch.arange(1, rows + 1, dtype=torch.float64)
    return [torch.multinomial(p, N_IDS, replacement=True, generator=g).to(DEV) for _ in range(pool)]


class TorchRule:
    """The rule with torch ops: distinct slots by ``unique``, then gather / where / scatter."""

    def __init__(self, mf, rows: int, hashes: int) -> None:
        self.mf, self.rows, self.hashes = mf, rows, hashes
        size = rows * max(hashes, 1)
        self.last = torch.zeros(size, dtype=torch.int32, device=DEV)
        self.gap = torch.zeros(size, dtype=torch.float32, device=DEV)
        self.table = torch.zeros(size, dtype=torch.float32, device=DEV)
        self.step = torch.zeros(1, dtype=torch.int64, device=DEV)
        self.offs = torch.arange(max(hashes, 1), device=DEV) * rows

    def slots(self, ids: torch.Tensor) -> torch.Tensor:
        if self.hashes == 0:
            return ids[(ids >= 0) & (ids < self.rows)][:, None]
        out = torch.empty(ids.numel() * self.hashes, dtype=torch.int64, device=DEV)
        self.mf._lib.check(self.mf._lib.lib().mf_hash_buckets(ids.data_ptr(), ids.numel(), self.hashes, 0, self.rows, out.data_ptr(),
                                                              self.mf._lib.stream_ptr()))
        return out.reshape(-1, self.hashes) + self.offs

    def update(self, ids: torch.Tensor, rows: bool = True):
        self.step.add_(1)
        slots = self.slots(ids)
        h = torch.unique(slots)
        old = self.last[h]
        g = (self.step.to(torch.int32) - old).to(torch.float32)
        d = torch.where(old == 0, g, (1.0 - ALPHA) * self.gap[h] + ALPHA * g)
        self.gap[h] = d
        self.last[h] = self.step.to(torch.int32).expand_as(h)
        if self.hashes == 0:
            self.table[h] = -torch.log(d)
        if not rows:
            return None
        x = self.gap[slots]
        return torch.where((x != 0).all(1), -torch.log(x.max(1).values.clamp_min(1e-30)), torch.zeros((), device=DEV))


def update_section(mf) -> dict:
    lib = mf._lib.lib()
    out = {}
    for label, rows, hashes in (("direct_62423", ROWS, 0), (f"hashed_{HASHED_M}x{HASHED_H}", HASHED_M, HASHED_H)):
        batches = zipf_batches(ROWS)
        one = [torch.full((N_IDS,), 4242, dtype=torch.int64, device=DEV)]
        est = {k: mf.StreamingLogQ(rows, alpha=ALPHA, num_hashes=hashes, device=DEV) for k in ("peel4", "peel0", "one4", "one0", "norows")}
        base = TorchRule(mf, rows, hashes)

        def hip(name, peel, pool, rows_back=True):
            def fn(k):
                lib.mf_logq_set_peel(peel)
                est[name].update(pool[k % len(pool)], rows=rows_back)
            return fn

        arms = {"hip_zipf": hip("peel4", 4, batches), "hip_zipf_no_peel": hip("peel0", 0, batches),
                "hip_one_id": hip("one4", 4, one), "hip_one_id_no_peel": hip("one0", 0, one),
                "torch_zipf": lambda k: base.update(batches[k % len(batches)])}
        if hashes == 0:
            arms["hip_zipf_table_only"] = hip("norows", 4, batches, rows_back=False)
        out[label] = alternate(arms)
        lib.mf_logq_set_peel(4)
        # the two implementations were fed the same calls: same state
        same = bool(torch.equal(est["peel4"].last_seen.reshape(-1), est["peel0"].last_seen.reshape(-1))
                    and torch.equal(est["peel4"].gap, est["peel0"].gap))
        out[label]["peel_changes_state"] = not same
        out[label]["torch_gap_max_abs_diff"] = float((est["peel4"].gap.reshape(-1) - base.gap).abs().max())
    return out


def step_section(mf, batch_size: int, steps: int, regions: int) -> dict:
    users, items, d = 162_541, 62_424, 128
    cfg = {"num_users": users, "num_items": items, "hidden_size": d, "train_loss": "InfomationNoiseContrastiveEstimationLoss",
           "num_negatives": 0, "optimizer": "adam", "learning_rate": 0.01, "use_logq": True}
    data = mf.data.SyntheticInteractions(users, items, max_positives=16, seed=0)
    batches = [mf.data.to_device(data.batch(batch_size), DEV) for _ in range(8)]
    arms = {}
    mods = {}
    for mode in ("table", "streaming"):
        torch.manual_seed(0)
        m = mf.lightning.MatrixFactorizationLitModule({**cfg, "logq_mode": mode, "logq_alpha": ALPHA})
        m.configure_model(device=DEV)
        if mode == "table":
            m.logq = mf.logq_from_counts(data.item_probability() * 1e6 + 1).to(DEV)
        opt = m.configure_optimizers()
        mods[mode] = m

        def fn(k, m=m, opt=opt):
            loss = m.training_step(batches[k % len(batches)])
            loss.backward()
            opt.step()
            opt.zero_grad(set_to_none=True)
        arms[mode] = fn
    res = alternate(arms, iters=steps, regions=regions, warmup=10)
    over = res["streaming"]["us"] - res["table"]["us"]
    res["overhead_us"] = over
    res["overhead_percent_of_step"] = 100.0 * over / res["table"]["us"]
    res["config"] = {**cfg, "batch": batch_size, "steps_per_region": steps}
    res["estimator_steps"] = int(mods["streaming"].logq_estimator.step)
    return res


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "logq_probe.json"))
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--regions", type=int, default=REGIONS)
    args = ap.parse_args()
    mf = importlib.import_module("matrix-factorization-torch_amd")
    res = {"device": torch.cuda.get_device_name(0), "n_ids": N_IDS, "alpha": ALPHA, "update_us": update_section(mf),
           "c3_step_us": step_section(mf, args.batch, args.steps, args.regions)}
    pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    pathlib.Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
