#!/usr/bin/env python3
"""Times the transformer tower's serving encode (HistoryTransformerTower.encode) on both of its paths, at the history probe's
world (tools/history_probe.py: the ML-25M-shaped synthetic InteractionTable, history windows of its sampler).

    python tools/xfmr_encode_probe.py [--out profiles/xfmr_encode_probe.json] [--ratings 25000000]

For (d, L, I) in the three shapes of tools/xfmr_probe.py, one layer, 4 heads, mean pooling, and B in {1, 8, 64, 512, 4096, 8192}
users (the first B windows of a batch): the median device time of ``encode(path="fused")`` (mf_xfmr_encode: one launch, no
stash) and of ``encode(path="forward")`` (the training forward's kernels, which is what every serving call ran before) --
device events around ten calls, three such regions after warm-up, the median of the three -- whether the two results are
bit-identical, and the peak of allocated bytes above the baseline during one call of each.  For B = 1 also the wall-clock
time of ``MatrixFactorizationLitModule.recommend_with_history`` end to end (a host clock around calls that end in a device-to-
host copy), with ``path="auto"`` free to take the fused kernel and with it held to the forward.

``largest_B_fused_not_slower`` is the largest measured B at which fused is not slower than forward at all three shapes with
every smaller measured B the same (null when fused loses at B = 1 somewhere; "all" when it wins everywhere): what
``models.XFMR_ENCODE_FUSED_MAX_USERS`` is set from.
"""
from __future__ import annotations

import argparse
import importlib
import importlib.util
import json
import pathlib
import statistics
import sys
import time

import torch

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
_spec = importlib.util.spec_from_file_location("history_probe", ROOT / "tools" / "history_probe.py")
hp = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(hp)

SHAPES = ((64, 32, 64), (128, 32, 128), (128, 64, 512))
BATCHES = (1, 8, 64, 512, 4096, 8192)


def median_ms(fn, regions: int = 3, warmup: int = 10, iters: int = 10) -> float:
    hp.time_ms(fn, warmup=warmup, iters=2)
    return statistics.median(hp.time_ms(fn, warmup=0, iters=iters) for _ in range(regions))


def peak_bytes(fn) -> int:
    fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return int(peak)


def wall_ms(fn, warmup: int = 10, iters: int = 50) -> float:
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    runs = []
    for _ in range(3):
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()                                   # (ends in a device-to-host copy of the result)
        runs.append((time.perf_counter() - t0) / iters * 1e3)
    return statistics.median(runs)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "xfmr_encode_probe.json"))
    ap.add_argument("--ratings", type=int, default=25_000_000)
    args = ap.parse_args()
    mf = importlib.import_module("matrix-factorization-torch_amd")
    torch.manual_seed(0)
    table = hp.synthetic_table(mf, args.ratings)
    sampler = table.sampler(num_items=hp.ITEMS, batch_size=hp.B, seed=0, device="cuda", history=True)
    start, end, items = sampler.batch(0)["user"]["history"]
    res = {"library": str(mf._lib.LIB_PATH), "shape": {"items": hp.ITEMS, "ratings": int(table.sorted_user.numel())}, "cases": []}
    for d, L, inter in SHAPES:
        cfg = {"num_users": 2, "num_items": hp.ITEMS, "hidden_size": d, "user_tower": "transformer", "max_history": L,
               "intermediate_size": inter, "num_hidden_layers": 1, "num_attention_heads": 4, "top_k": 10}
        module = mf.lightning.MatrixFactorizationLitModule(cfg)
        module.configure_model(device="cuda")
        module.item_processor.get_index(module)
        tower = module.towers["user"]
        for b in BATCHES:
            hist = (start[:b].contiguous(), end[:b].contiguous(), items)
            valid = (items >= 1) & (items < hp.ITEMS)
            csum = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), valid.cumsum(0)])
            tokens = int((csum[hist[1]] - csum[hist[0]]).clamp(max=L).sum())
            case = {"d": d, "L": L, "I": inter, "B": b, "tokens": tokens}
            for path in ("fused", "forward"):
                fn = lambda path=path: tower.encode(hist, path=path)  # noqa: E731
                case[f"{path}_ms"] = median_ms(fn)
                case[f"{path}_peak_bytes"] = peak_bytes(fn)
            case["bit_identical"] = bool(torch.equal(tower.encode(hist, path="fused"), tower.encode(hist, path="forward")))
            case["forward_over_fused"] = case["forward_ms"] / case["fused_ms"]
            if b == 1:
                lo, hi = int(start[0]), int(end[0])
                ids = [int(i) for i in items[lo:hi].tolist() if 1 <= int(i) < hp.ITEMS] or [1]
                serve = lambda: module.recommend_with_history(ids, top_k=10)  # noqa: E731
                keep = mf.models.XFMR_ENCODE_FUSED_MAX_USERS
                case["recommend_with_history_wall_ms"] = {}
                for name, limit in (("auto_may_fuse", None), ("forward_only", 0)):
                    mf.models.XFMR_ENCODE_FUSED_MAX_USERS = limit
                    case["recommend_with_history_wall_ms"][name] = wall_ms(serve)
                mf.models.XFMR_ENCODE_FUSED_MAX_USERS = keep
                case["recommend_history_length"] = len(ids)
            res["cases"].append(case)
            print(json.dumps(case), flush=True)
    wins = {b: all(c["fused_ms"] <= c["forward_ms"] for c in res["cases"] if c["B"] == b) for b in BATCHES}
    largest = None
    for b in BATCHES:
        if not wins[b]:
            break
        largest = b
    res["fused_not_slower_at_every_shape"] = wins
    res["largest_B_fused_not_slower"] = "all" if all(wins.values()) else largest
    res["all_bit_identical"] = all(c["bit_identical"] for c in res["cases"])
    out = pathlib.Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=2))
    print(f"wrote {out}")


if __name__ == "__main__":
    main()
