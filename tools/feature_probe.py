#!/usr/bin/env python3
"""Times the hashed feature-bag towers (models.FeatureBagTower) on an ML-25M-shaped synthetic catalogue.

    python tools/feature_probe.py [--out profiles/feature_probe.json] [--ratings 25000000]

The catalogue: 62,424 items from data.synthetic_item_features (1-3 genres of 20 with a skewed frequency, titles of 1-12
words from 20,000 plus a year), hashed into 65,535 buckets by data.FeatureHasher; d = 128.  The ratings table is
tools/history_probe.py's (Zipf item popularity, log-normal user activity); batches of B = 8192 train pairs, so the item
tower embeds B positives + B negatives = 16,384 bags per step.

Reports, with device events after warm-up:
  * the bag forward and backward alone (mf_bag_forward; mf_bag_backward's coalesce through optim._pending), as HIP-event
    spans of the library (mf_timing) and as wall time of the calls;
  * the C3-shaped training step (InfoNCE, CSR positives, row-wise Adam) with item_tower="table" and "features".
"""
from __future__ import annotations

import argparse
import importlib
import json
import pathlib
import sys

import torch

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

from history_probe import B, DIM, ITEMS, USERS, synthetic_table, time_ms  # noqa: E402

BUCKETS = 65_535


def spans(mf, fn, names, iters=20):
    lib = mf._lib.lib()
    torch.cuda.synchronize()
    lib.mf_timing_reset()
    lib.mf_timing_enable(1)
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    lib.mf_timing_enable(0)
    out = {}
    for name in names:
        tot = torch.zeros(1, dtype=torch.float64)
        n = lib.mf_timing_get(name.encode(), mf._lib.ctypes.cast(tot.data_ptr(), mf._lib.ctypes.POINTER(mf._lib.ctypes.c_double)))
        if n:
            out[name] = {"launches_per_call": n / iters, "us_per_launch": 1e3 * float(tot) / n}
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "feature_probe.json"))
    ap.add_argument("--ratings", type=int, default=25_000_000)
    args = ap.parse_args()
    mf = importlib.import_module("matrix-factorization-torch_amd")
    torch.manual_seed(0)
    texts, _ = mf.data.synthetic_item_features(ITEMS, num_genres=20, vocab=20_000, seed=0)
    bags = mf.data.FeatureHasher(BUCKETS).bags(texts)
    lens = (bags.off[1:] - bags.off[:-1]).double()
    table = synthetic_table(mf, args.ratings)
    sampler = table.sampler(num_items=ITEMS, batch_size=B, seed=0, device="cuda")
    batches = [sampler.batch(i) for i in range(8)]
    res = {"shape": {"items": ITEMS, "buckets": BUCKETS, "d": DIM, "batch_pairs": B, "bags_per_step": 2 * B,
                     "users": USERS, "ratings": int(table.sorted_user.numel())},
           "bag_len": {"mean": float(lens[1:].mean()), "max": bags.max_len}}
    print(json.dumps(res))

    # ---- forward / backward alone
    tower = mf.models.FeatureBagTower(BUCKETS, DIM, combiner="mean", device="cuda")
    tower.set_bags(bags)
    idx = torch.cat([batches[0]["item"]["idx"], batches[0]["neg_item"]["idx"]])
    c = torch.randn(idx.numel(), DIM, device="cuda")

    def fwd():
        return tower(idx)

    def fwd_bwd():
        tower(idx).backward(c)
        out = mf.optim._pending(tower.weight)
        tower.weight._mf_pending.clear()
        return out

    with torch.no_grad():
        t_fwd = time_ms(fwd)
    t_fb = time_ms(fwd_bwd)
    ids_out = fwd_bwd()[0]
    sp = spans(mf, fwd_bwd, ("bag_forward", "bag_backward"))
    res["bag"] = {"forward_us": sp["bag_forward"]["us_per_launch"], "backward_us": sp["bag_backward"]["us_per_launch"],
                  "forward_call_ms": t_fwd, "forward_plus_backward_call_ms": t_fb,
                  "entries": int(lens[idx.cpu()].sum()), "coalesced_list": int(ids_out.numel()),
                  "unique_ids": int((ids_out >= 0).sum())}
    print(json.dumps(res["bag"]))

    # ---- the C3-shaped step: item table against item features
    loss_fn = mf.losses.InfomationNoiseContrastiveEstimationLoss(num_negatives=0)
    for item_tower in ("table", "features"):
        cfg = mf.models.ModelConfig(num_users=USERS, num_items=ITEMS, hidden_size=DIM, item_tower=item_tower,
                                    feature_buckets=BUCKETS)
        towers = mf.models.init_towers(cfg, device="cuda")
        if item_tower == "features":
            towers["item"].set_bags(bags)
        opt = mf.optim.RowAdam(towers.parameters(), lr=1e-3)
        opt.init_state()
        k = [0]

        def step():
            bt = batches[k[0] % len(batches)]
            k[0] += 1
            u = towers["user"](bt["user"]["idx"])
            ii = torch.cat([bt["item"]["idx"], bt["neg_item"]["idx"]])
            v = towers["item"](ii)
            loss = loss_fn(u, v, bt["target"], item_idx=ii, pos_csr=bt["user"]["pos_csr"])
            loss.backward()
            opt.step()
            opt.zero_grad()

        ms = time_ms(step, warmup=10, iters=30)
        res[f"step_{item_tower}"] = {"ms_per_step": ms,
                                     "spans": spans(mf, step, ("gather_rows", "bag_forward", "bag_backward", "update_rows"), 10)}
        print(json.dumps({item_tower: res[f"step_{item_tower}"]}))
    res["target"] = {"forward_us": 30, "backward_us": 150, "step_over_table_ms": 0.25}
    res["feature_step_minus_table_ms"] = res["step_features"]["ms_per_step"] - res["step_table"]["ms_per_step"]
    out = pathlib.Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=2))
    print(f"wrote {out}")


if __name__ == "__main__":
    main()
