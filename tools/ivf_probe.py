#!/usr/bin/env python3
"""Times the partitioned search (``PartitionedIndex.search``) beside the exact one, and measures what the probing costs in recall.

    python tools/ivf_probe.py [--out profiles/ivf_probe.json]

Time.  Catalogs 62,423 x 128 and 2^22 x 128 (unit rows), each with the reference's default partition count, built by
``PartitionedIndex.build`` (10 iterations).  Per cell -- Q in {1, 8, 32, 1024} x nprobe in {1, 8, 32} x {no exclusions, 150 per
query} at k = 20 -- device microseconds per call: HIP events around ITERS calls, REGIONS such regions per arm after every arm
has run WARMUP calls, the arms alternating region by region; median, spread = max - min.  The arms:

  cells   ``index.search(q, 20, nprobe=..., path="cells")``: the three stages (centroid search, scan, merge)
  exact   ``ItemIndex.search(q, 20, path="auto")`` on the same rows, from the same library in the same process -- the baseline

``exact_over_cells`` is the measured ratio; ``cells_slower`` says that the partitioned search lost the cell.  ``read_ratio`` is
the catalog's rows over the rows the scan reads per query (the padded rows of the probed cells, averaged over the queries).

Recall.  Recall@20 of ``path="cells"`` against the exact answer, 1,024 queries, nprobe = 1 .. 64, on two catalogs of 2^18 x 64:
uniform random unit rows (no structure to find: the worst case) and a seeded mixture of 1,000 Gaussians (queries drawn from the
same mixture).  Recall is a property of the data; it is reported, nothing here is a pass mark.

Build.  Wall seconds of ``build`` (k-means and layout) and of the first search (which lays out the cell-ordered copy).
"""
from __future__ import annotations

import argparse
import importlib
import json
import pathlib
import statistics
import sys
import time

import numpy as np
import torch

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

D, K = 128, 20
CATALOGS = (62_423, 2**22)
QS, NPROBES, EXCLUDED = (1, 8, 32, 1024), (1, 8, 32), (0, 150)
ITERS, REGIONS, WARMUP = 20, 7, 5
RECALL_N, RECALL_D, RECALL_Q = 2**18, 64, 1024
RECALL_NPROBES = (1, 2, 4, 8, 16, 32, 64)
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


def unit_rows(n: int, d: int, seed: int) -> torch.Tensor:
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.nn.functional.normalize(torch.randn(n, d, generator=g, device=DEV), dim=-1)


def mixture_rows(n: int, d: int, seed: int, centres: torch.Tensor, sigma: float = 0.15) -> torch.Tensor:
    g = torch.Generator(device=DEV).manual_seed(seed)
    which = torch.randint(0, centres.shape[0], (n,), generator=g, device=DEV)
    return torch.nn.functional.normalize(centres[which] + sigma * torch.randn(n, d, generator=g, device=DEV), dim=-1)


def timed_build(mf, rows: torch.Tensor) -> tuple:
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    index = mf.retrieval.PartitionedIndex.build(rows, seed=0)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    index.search(rows[:1], K)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    blocks = (index.cell_blk[1:] - index.cell_blk[:-1]).cpu().numpy()
    info = {"N": rows.shape[0], "d": rows.shape[1], "num_partitions": index.num_partitions, "build_s": t1 - t0, "first_search_s": t2 - t1,
            "max_cell_rows": int(blocks.max()) * 64, "mean_cell_rows": float(blocks.mean()) * 64, "empty_cells": int((blocks == 0).sum())}
    return index, info


def time_catalog(mf, n: int, res: dict) -> None:
    rows = unit_rows(n, D, seed=n % 1000)
    index, info = timed_build(mf, rows)
    res["builds"].append(info)
    print(json.dumps(info), flush=True)
    exact = mf.retrieval.ItemIndex(rows)
    queries = unit_rows(max(QS), D, seed=7)
    g = np.random.default_rng(1)
    blocks = index.cell_blk[1:] - index.cell_blk[:-1]
    for nq in QS:
        q = queries[:nq].contiguous()
        for excluded in EXCLUDED:
            csr = mf.retrieval._csr([g.choice(n, excluded, replace=False) for _ in range(nq)], nq, DEV) if excluded else None
            for nprobe in NPROBES:
                if nprobe > index.num_partitions:
                    continue
                probes = index.coarse.search(q, nprobe)[1]
                cell = {"N": n, "Q": nq, "nprobe": nprobe, "excluded_per_query": excluded, "slices": index.plan(nq, K, nprobe)["slices"],
                        "read_ratio": n / (float(blocks[probes].sum()) * 64 / nq)}
                cell.update(alternate({"cells": lambda: index.search(q, K, exclude_csr=csr, nprobe=nprobe),
                                       "exact": lambda: exact.search(q, K, exclude_csr=csr)}))
                cell["exact_over_cells"] = cell["exact"]["us"] / cell["cells"]["us"]
                cell["cells_slower"] = bool(cell["cells"]["us"] > cell["exact"]["us"])
                res["cells"].append(cell)
                print(json.dumps(cell), flush=True)


def recall(mf, name: str, rows: torch.Tensor, queries: torch.Tensor, res: dict) -> None:
    index, info = timed_build(mf, rows)
    want = index.search(queries, K, path="exact")[1]
    entry = {"data": name, **info, "Q": queries.shape[0], "k": K, "recall_at_20": {}}
    for nprobe in RECALL_NPROBES:
        got = index.search(queries, K, nprobe=nprobe)[1]
        hits = (got.unsqueeze(2) == want.unsqueeze(1)).any(dim=2) & (got >= 0)
        entry["recall_at_20"][str(nprobe)] = float(hits.sum()) / want.numel()
    res["recall"].append(entry)
    print(json.dumps(entry), flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "ivf_probe.json"))
    args = ap.parse_args()
    mf = importlib.import_module("matrix-factorization-torch_amd")
    res = {"protocol": {"k": K, "iters": ITERS, "regions": REGIONS, "warmup": WARMUP, "arms": "alternate region by region",
                        "exact": "ItemIndex.search(path='auto') of the same library"},
           "device": torch.cuda.get_device_name(0), "builds": [], "cells": [], "recall": []}
    for n in CATALOGS:
        time_catalog(mf, n, res)
    recall(mf, "uniform unit rows", unit_rows(RECALL_N, RECALL_D, 3), unit_rows(RECALL_Q, RECALL_D, 4), res)
    centres = unit_rows(1000, RECALL_D, 5)
    recall(mf, "mixture of 1000 Gaussians (sigma 0.15 per coordinate)", mixture_rows(RECALL_N, RECALL_D, 6, centres),
           mixture_rows(RECALL_Q, RECALL_D, 8, centres), res)
    out_path = pathlib.Path(args.out)
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
