#!/usr/bin/env python3
"""Times deep lists from the cells (``PartitionedIndex.search(path="cells_deep")``) beside the exact deep search.

    python tools/ivf_deep_probe.py [--out profiles/ivf_deep_probe.json]

Catalogs 62,423 x 128 (128 cells) and 2^22 x 128 (2,048 cells), unit rows, built by ``PartitionedIndex.build`` (10 iterations).
Per cell -- Q in {1, 32, 1024} x k in {100, 1000} x nprobe in {1, 8, 16} x {no exclusions, 150 per query} -- device microseconds
per call: HIP events around ``iters`` calls, REGIONS such regions per arm after every arm has run WARMUP calls, the arms
alternating region by region; median, spread = max - min.  ``iters`` is chosen per cell so that a region of the slower arm lasts
about REGION_US (1 .. 20 calls).  The arms:

  cells_deep   ``index.search(q, k, nprobe=..., path="cells_deep")``: the three stages (centroid search, scan, merge)
  deep         ``ItemIndex.search(q, k, path="deep")`` on the same rows, from the same library in the same process -- the baseline

``deep_over_cells`` is the measured ratio; ``cells_slower`` says that the partitioned search lost the cell.  ``read_ratio`` is the
catalog's rows over the rows the scan reads per query (the padded rows of the probed cells, averaged over the queries).
``stages_us``: the three stages of ``cells_deep`` timed one by one (the same regions, not alternating); the settles of the
workgroup's buffer are part of ``scan``.

Shallow cost.  At k = 20 and 64, where both scans serve the depth: ``cells_deep`` against ``cells`` (Q and nprobe as above, no
exclusions), the same protocol.
"""
from __future__ import annotations

import argparse
import importlib
import json
import pathlib
import statistics
import sys

import numpy as np
import torch

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

D = 128
CATALOGS = (62_423, 2**22)
QS, KS, NPROBES, EXCLUDED = (1, 32, 1024), (100, 1000), (1, 8, 16), (0, 150)
SHALLOW_KS = (20, 64)
REGIONS, WARMUP, MAX_ITERS, REGION_US = 7, 3, 20, 20_000.0
DEV = "cuda:0"


def region_us(fn, iters: int) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1000.0 / iters


def alternate(arms: dict, regions: int = REGIONS, warmup: int = WARMUP) -> dict:
    for fn in arms.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    slowest = max(region_us(fn, 1) for fn in arms.values())
    iters = int(min(MAX_ITERS, max(1, REGION_US // max(slowest, 1.0))))
    runs = {name: [] for name in arms}
    for _ in range(regions):
        for name, fn in arms.items():
            runs[name].append(region_us(fn, iters))
    return {name: {"us": statistics.median(r), "spread_us": max(r) - min(r), "min_us": min(r), "regions": len(r), "iters": iters}
            for name, r in runs.items()}


def unit_rows(n: int, d: int, seed: int) -> torch.Tensor:
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.nn.functional.normalize(torch.randn(n, d, generator=g, device=DEV), dim=-1)


def stages(mf, index, q, k: int, nprobe: int, csr) -> dict:
    """The stages of ``search(path="cells_deep")`` one by one, on buffers of their own."""
    lib, L = mf._lib.lib(), mf._lib
    nq, n, d = q.shape[0], index.num_items, index.embeddings.shape[1]
    off, ids = csr if csr is not None else (None, None)
    _, probes = index.coarse.search(q, nprobe)
    probes = probes.clone()
    ws = torch.empty(lib.mf_ivf_deep_ws_bytes(nq, nprobe, k, index.max_cell_blocks), dtype=torch.uint8, device=DEV)
    lists = index.plan(nq, k, nprobe, "cells_deep")["lists"]
    scores = torch.empty(nq, k, dtype=torch.float32, device=DEV)
    rows = torch.empty(nq, k, dtype=torch.int64, device=DEV)
    cells = index.cell_blocked()

    def scan():
        L.check(lib.mf_ivf_scan_deep(q.data_ptr(), nq, cells.data_ptr(), index.cell_blk.data_ptr(), index.row_of.data_ptr(), index.row_of.numel(), n,
                                     index.num_partitions, d, index.max_cell_blocks, probes.data_ptr(), nprobe, k, 0, L.ptr(off), L.ptr(ids),
                                     index.idx_base, ws.data_ptr(), ws.numel(), L.stream_ptr()))

    def merge():
        L.check(lib.mf_topk_merge_packed_deep(ws.data_ptr(), lists, nq, k, scores.data_ptr(), rows.data_ptr(), L.stream_ptr()))

    out = {}
    for name, fn in (("coarse", lambda: index.coarse.search(q, nprobe)), ("scan", scan), ("merge", merge)):
        for _ in range(WARMUP):
            fn()
        torch.cuda.synchronize()
        iters = int(min(MAX_ITERS, max(1, REGION_US // max(region_us(fn, 1), 1.0))))
        out[name] = statistics.median(region_us(fn, iters) for _ in range(3))
    return out


def time_catalog(mf, n: int, res: dict) -> None:
    rows = unit_rows(n, D, seed=n % 1000)
    index = mf.retrieval.PartitionedIndex.build(rows, seed=0)
    exact = mf.retrieval.ItemIndex(rows)
    queries = unit_rows(max(QS), D, seed=7)
    g = np.random.default_rng(1)
    blocks = index.cell_blk[1:] - index.cell_blk[:-1]
    info = {"N": n, "d": D, "num_partitions": index.num_partitions, "max_cell_rows": int(blocks.max()) * 64, "mean_cell_rows": float(blocks.float().mean()) * 64}
    res["catalogs"].append(info)
    print(json.dumps(info), flush=True)
    for nq in QS:
        q = queries[:nq].contiguous()
        # 150 distinct rows per query (drawn with spares: a draw without replacement from 2^22 rows costs a pass over them)
        draws = [g.integers(0, n, 400) for _ in range(nq)]
        lists = {0: None, 150: mf.retrieval._csr([x[np.sort(np.unique(x, return_index=True)[1])][:150] for x in draws], nq, DEV)}
        for nprobe in NPROBES:
            probes = index.coarse.search(q, nprobe)[1]
            read_ratio = n / (float(blocks[probes].sum()) * 64 / nq)
            for k in SHALLOW_KS:
                cell = {"N": n, "Q": nq, "k": k, "nprobe": nprobe, "read_ratio": read_ratio}
                cell.update(alternate({"cells_deep": lambda: index.search(q, k, nprobe=nprobe, path="cells_deep"),
                                       "cells": lambda: index.search(q, k, nprobe=nprobe, path="cells")}))
                cell["deep_over_wavefront"] = cell["cells_deep"]["us"] / cell["cells"]["us"]
                res["shallow"].append(cell)
                print(json.dumps(cell), flush=True)
            for k in KS:
                for excluded in EXCLUDED:
                    csr = lists[excluded]
                    cell = {"N": n, "Q": nq, "k": k, "nprobe": nprobe, "excluded_per_query": excluded,
                            "slices": index.plan(nq, k, nprobe, "cells_deep")["slices"], "read_ratio": read_ratio}
                    cell.update(alternate({"cells_deep": lambda: index.search(q, k, exclude_csr=csr, nprobe=nprobe, path="cells_deep"),
                                           "deep": lambda: exact.search(q, k, exclude_csr=csr, path="deep")}))
                    cell["deep_over_cells"] = cell["deep"]["us"] / cell["cells_deep"]["us"]
                    cell["cells_slower"] = bool(cell["cells_deep"]["us"] > cell["deep"]["us"])
                    cell["stages_us"] = stages(mf, index, q, k, nprobe, csr)
                    res["cells"].append(cell)
                    print(json.dumps(cell), flush=True)
                    pathlib.Path(res["out"]).write_text(json.dumps(res, indent=1) + "\n")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "ivf_deep_probe.json"))
    ap.add_argument("--catalogs", default=",".join(map(str, CATALOGS)))
    args = ap.parse_args()
    mf = importlib.import_module("matrix-factorization-torch_amd")
    pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    res = {"protocol": {"regions": REGIONS, "warmup": WARMUP, "iters": f"1..{MAX_ITERS}, a region of the slower arm about {REGION_US:.0f} us",
                        "arms": "alternate region by region", "deep": "ItemIndex.search(path='deep') of the same library"},
           "device": torch.cuda.get_device_name(0), "out": args.out, "catalogs": [], "shallow": [], "cells": []}
    for n in map(int, args.catalogs.split(",")):
        time_catalog(mf, n, res)
    del res["out"]
    pathlib.Path(args.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
