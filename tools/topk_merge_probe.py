#!/usr/bin/env python3
"""Times the merge of deep per-shard lists (``mf_topk_merge_packed_deep``) beside the k <= 64 export on the same input.

    python tools/topk_merge_probe.py [--out profiles/topk_merge_deep_probe.json]

Catalog N = 62,423 x d = 128 (unit rows) dealt round-robin over G shards, G in {2, 8, 16} x k in {100, 1000} x Q in
{1, 32, 1024}.  The input of a cell is what ``ShardedIndex.search`` hands its merge: every shard's ``search(path="deep")`` for
the Q queries, packed by ``mf_topk_pack`` into ``[G][Q][k]`` int64.  Per cell, device microseconds per call -- HIP events around
ITERS calls, REGIONS such regions per arm after every arm has run WARMUP calls, the arms alternating region by region; median,
spread = max - min -- of

  merge_deep    ``mf_topk_merge_packed_deep``
  merge         ``mf_topk_merge_packed`` from the same library, in the cells it accepts (G * k <= 8192)
  deep_shard    ``mf_topk_deep`` on ONE shard (N / G rows) at the same Q and k: the work a rank does before the merge

``merge_over_merge_deep`` is the measured ratio, ``slower_beyond_spread`` says whether the new export's median lies above the old
one's by more than the spread of the old one's own regions, ``merge_share`` is merge_deep / (deep_shard + merge_deep).  In every
shared cell the two exports' outputs are compared bit for bit first.
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

N, D = 62_423, 128
GS, KS, QS = (2, 8, 16), (100, 1000), (1, 32, 1024)
OLD_MAX_KEYS = 8192
ITERS, REGIONS, WARMUP = 30, 7, 10
DEV = "cuda:0"


def region_us(fn, iters: int) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1000.0 / iters


def alternate(arms: dict, iters: int = ITERS, regions: int = REGIONS, warmup: int = WARMUP) -> dict:
    for fn in arms.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    runs = {name: [] for name in arms}
    for _ in range(regions):
        for name, fn in arms.items():
            runs[name].append(region_us(fn, iters))
    return {name: {"us": statistics.median(r), "spread_us": max(r) - min(r), "min_us": min(r), "regions": len(r), "iters": iters}
            for name, r in runs.items()}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "topk_merge_deep_probe.json"))
    args = ap.parse_args()
    mf = importlib.import_module("matrix-factorization-torch_amd")
    lib, L = mf._lib.lib(), mf._lib
    g = torch.Generator().manual_seed(0)
    items = torch.nn.functional.normalize(torch.randn(N, D, generator=g), dim=-1).to(DEV)
    queries = torch.nn.functional.normalize(torch.randn(max(QS), D, generator=g), dim=-1).to(DEV)
    res = {"shape": {"N": N, "d": D, "shards": "rows dealt round-robin", "input": "per-shard search(path='deep') -> mf_topk_pack"},
           "protocol": {"iters": ITERS, "regions": REGIONS, "warmup": WARMUP, "arms": "alternate region by region"}, "cells": []}
    for G in GS:
        shards = [mf.retrieval.ItemIndex(items[s::G].contiguous()) for s in range(G)]
        for k in KS:
            for nq in QS:
                q = queries[:nq].contiguous()
                packed = torch.empty(G, nq, k, dtype=torch.int64, device=DEV)
                for s, shard in enumerate(shards):
                    ps, pl = shard.search(q, k, path="deep")
                    L.check(lib.mf_topk_pack(ps.data_ptr(), pl.data_ptr(), nq * k, G, s, packed[s].data_ptr(), L.stream_ptr()))
                out = {name: (torch.empty(nq, k, device=DEV), torch.empty(nq, k, dtype=torch.int64, device=DEV)) for name in ("merge_deep", "merge")}

                def merge_deep():
                    L.check(lib.mf_topk_merge_packed_deep(packed.data_ptr(), G, nq, k, out["merge_deep"][0].data_ptr(),
                                                          out["merge_deep"][1].data_ptr(), L.stream_ptr()))

                def merge():
                    L.check(lib.mf_topk_merge_packed(packed.data_ptr(), G, nq, k, out["merge"][0].data_ptr(), out["merge"][1].data_ptr(),
                                                     L.stream_ptr()))

                arms = {"merge_deep": merge_deep, "deep_shard": lambda: shards[0].search(q, k, path="deep")}
                cell = {"G": G, "k": k, "Q": nq}
                if G * k <= OLD_MAX_KEYS:
                    arms["merge"] = merge
                    merge_deep()
                    merge()
                    torch.cuda.synchronize()
                    cell["outputs_equal"] = bool(torch.equal(out["merge"][1], out["merge_deep"][1]) and
                                                 torch.equal(out["merge"][0].view(torch.int32), out["merge_deep"][0].view(torch.int32)))
                cell.update(alternate(arms))
                cell["merge_share"] = cell["merge_deep"]["us"] / (cell["deep_shard"]["us"] + cell["merge_deep"]["us"])
                if "merge" in cell:
                    cell["merge_over_merge_deep"] = cell["merge"]["us"] / cell["merge_deep"]["us"]
                    cell["slower_beyond_spread"] = bool(cell["merge_deep"]["us"] > cell["merge"]["us"] + cell["merge"]["spread_us"])
                res["cells"].append(cell)
                print(json.dumps(cell), flush=True)
    out_path = pathlib.Path(args.out)
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
