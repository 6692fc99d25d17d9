#!/usr/bin/env python3
"""Times the history-pooled user tower (models.HistoryPoolingTower) on an ML-25M-shaped synthetic InteractionTable.

    python tools/history_probe.py [--out profiles/history_probe.json] [--ratings 25000000]

The table: 162,541 users x 62,424 item rows, Zipf item popularity, log-normal user activity, every user's ratings spread
uniformly over a log-normal span of days (fixed seed), split and windowed by data.InteractionTable (4-week rolling
history of every rating).  Batches come from its sampler(history=True): the windows of B = 8192 train pairs.

Reports, with device events after warm-up:
  * the pool forward / backward (mf_pool_forward, the coalesce of mf_pool_backward) at B = 8192, d = 128, mean and max;
    algorithmic bytes = entries x 4d (the row reads) + entries x 8 (the ids) over the kernel time, against 8 TB/s of HBM.
    The 32 MB item table sits in the 256 MiB Infinity Cache, so the rate can exceed the HBM peak;
  * the C3-shaped training step (InfoNCE over the batch's items, CSR positives, row-wise Adam) with the table user tower
    and with the history tower (mean), plus the mf_timing spans of the history step (one `update_rows` launch per step
    shows that the item table's update stays ONE fused launch).
"""
from __future__ import annotations

import argparse
import importlib
import json
import math
import pathlib
import sys

import numpy as np
import torch

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

USERS, ITEMS, DIM, B = 162_541, 62_424, 128, 8192
HBM_TBS = 8.0


def synthetic_table(mf, n_ratings: int, seed: int = 0):
    rng = np.random.default_rng(seed)
    act = rng.lognormal(0.0, 1.2, USERS - 1)
    cnt = np.maximum(1, np.round(act / act.sum() * n_ratings)).astype(np.int64)
    user = np.repeat(np.arange(1, USERS), cnt)
    n = user.size
    item = (rng.zipf(1.15, n) - 1) % (ITEMS - 1) + 1
    span = rng.lognormal(math.log(200.0), 1.5, USERS) * 86400.0          # days over which each user rates
    start = rng.uniform(0, 5 * 365 * 86400.0, USERS)
    ts = (start[user] + rng.uniform(0, 1, n) * span[user]).astype(np.int64)
    rating = rng.integers(1, 6, n).astype(np.float32)
    dev = "cuda"
    t = mf.data.InteractionTable(torch.from_numpy(user).to(dev), torch.from_numpy(item).to(dev), torch.from_numpy(rating).to(dev),
                                 torch.from_numpy(ts).to(dev))
    return t


def time_ms(fn, warmup: int = 5, iters: int = 20) -> float:
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "history_probe.json"))
    ap.add_argument("--ratings", type=int, default=25_000_000)
    args = ap.parse_args()
    mf = importlib.import_module("matrix-factorization-torch_amd")
    lib = mf._lib.lib()
    torch.manual_seed(0)
    table = synthetic_table(mf, args.ratings)
    sampler = table.sampler(num_items=ITEMS, batch_size=B, seed=0, device="cuda", history=True)
    batches = [sampler.batch(i) for i in range(8)]
    lens = torch.cat([(b["user"]["history"][1] - b["user"]["history"][0]) for b in batches]).double()
    res = {"shape": {"users": USERS, "items": ITEMS, "d": DIM, "batch": B, "ratings": int(table.sorted_user.numel()),
                     "train_pairs": int(table.pair_user.numel())},
           "window_len": {"mean": float(lens.mean()), "max": int(lens.max()), "p99": float(lens.quantile(0.99))}}
    print(json.dumps(res))

    # ---- the pool forward / backward alone
    item = mf.models.EmbeddingTower(ITEMS, DIM, device="cuda")
    for mode in ("mean", "max"):
        tower = mf.models.HistoryPoolingTower(item, pooling_mode=mode)
        hist = batches[0]["user"]["history"]
        start, end, items, n_entries = tower.segments(hist)
        code = mf.models.POOLING_MODES.index(mode)

        def fwd():
            return mf.models._PoolRows.apply(item.weight, start, end, items, n_entries, code, 0, True, True)

        with torch.no_grad():
            t_fwd = time_ms(fwd)
        c = torch.randn(B, DIM, device="cuda")
        ids2 = torch.cat([batches[0]["item"]["idx"], batches[0]["neg_item"]["idx"]])
        g2 = torch.randn(ids2.numel(), DIM, device="cuda")

        def bwd():
            u = fwd()
            u.backward(c)
            pend = item.weight._mf_pending
            pend.append((ids2, g2, True))
            out = mf.optim._pending(item.weight)
            pend.clear()
            return out

        t_fb = time_ms(bwd)
        ids_out = bwd()[0]
        algo = n_entries * (4 * DIM + 8)
        res[f"pool_{mode}"] = {"entries": n_entries, "forward_ms": t_fwd, "forward_plus_backward_ms": t_fb,
                               "backward_ms": t_fb - t_fwd, "coalesced_list": int(ids_out.numel()),
                               "unique_ids": int((ids_out >= 0).sum()),
                               "forward_algo_TBps": algo / (t_fwd * 1e-3) / 1e12, "hbm_peak_TBps": HBM_TBS}
        print(json.dumps({mode: res[f"pool_{mode}"]}))

    # ---- the C3-shaped step, table user tower against the history tower
    loss_fn = mf.losses.InfomationNoiseContrastiveEstimationLoss(num_negatives=0)
    for user_tower in ("table", "history"):
        cfg = mf.models.ModelConfig(num_users=USERS, num_items=ITEMS, hidden_size=DIM, user_tower=user_tower)
        towers = mf.models.init_towers(cfg, device="cuda")
        opt = mf.optim.RowAdam(towers.parameters(), lr=1e-3)
        opt.init_state()
        k = [0]

        def step():
            bt = batches[k[0] % len(batches)]
            k[0] += 1
            u = towers["user"](bt["user"]["history"] if user_tower == "history" else bt["user"]["idx"])
            idx = torch.cat([bt["item"]["idx"], bt["neg_item"]["idx"]])
            v = towers["item"](idx)
            loss = loss_fn(u, v, bt["target"], item_idx=idx, pos_csr=bt["user"]["pos_csr"])
            loss.backward()
            opt.step()
            opt.zero_grad()

        ms = time_ms(step, warmup=10, iters=30)
        lib.mf_timing_reset()
        lib.mf_timing_enable(1)
        for _ in range(10):
            step()
        torch.cuda.synchronize()
        lib.mf_timing_enable(0)
        spans = {}
        for name in ("gather_rows", "pool_forward", "pool_backward", "pool_segsum", "update_rows"):
            tot = torch.zeros(1, dtype=torch.float64)
            n = lib.mf_timing_get(name.encode(), mf._lib.ctypes.cast(tot.data_ptr(), mf._lib.ctypes.POINTER(mf._lib.ctypes.c_double)))
            if n:
                spans[name] = {"launches_per_step": n / 10, "ms_per_launch": float(tot) / n}
        res[f"step_{user_tower}"] = {"ms_per_step": ms, "spans": spans}
        print(json.dumps({user_tower: res[f"step_{user_tower}"]}))
    out = pathlib.Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=2))
    print(f"wrote {out}")


if __name__ == "__main__":
    main()
