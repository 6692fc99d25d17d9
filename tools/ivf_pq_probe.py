#!/usr/bin/env python3
"""Times the quantised search (``QuantizedIndex.search``) beside the partitioned and the exact one, and measures what the
quantiser costs in recall and saves in memory.  The companion of tools/ivf_probe.py, whose helpers it shares.

    python tools/ivf_pq_probe.py [--out profiles/ivf_pq_probe.json]
    python tools/ivf_pq_probe.py --deep [--catalogs 62423,4194304] [--out profiles/ivf_pq_deep_probe.json]     # path="pq_deep": deep_main

Time.  Catalogs 62,423 x 128 and 2^22 x 128 (unit rows), each with the reference's default partition count and
num_sub_vectors = 16 (the reference's width // 8), built by ``QuantizedIndex.build`` (10 + 10 iterations).  Per cell -- Q in
{1, 8, 32, 1024} x nprobe in {1, 8, 32} x {no exclusions, 150 per query} at k = 20, refine_factor = 4 -- device microseconds per
call: HIP events around ITERS calls, REGIONS such regions per arm after every arm has run WARMUP calls, the arms alternating
region by region; median, spread = max - min.  The arms:

  pq      ``index.search(q, 20, nprobe=..., path="pq")``: the four stages (centroid search, scan, merge, refine)
  cells   ``index.search(q, 20, nprobe=..., path="cells")``: the parent's exact scan of the same cells (``PartitionedIndex``)
  exact   ``ItemIndex.search(q, 20, path="auto")`` on the same rows, from the same library in the same process

``pq_slower_than_cells`` / ``pq_slower_than_exact`` say that the quantised search lost the cell.  ``stages`` splits the pq arm:
each of probes / scan / merge / refine timed alone on the inputs the search hands it (fewer regions).

Recall.  Recall@20 of ``path="pq"`` against the exact answer and against ``path="cells"`` with the same probes, 1,024 queries,
nprobe in {1, 8, 32} x refine_factor in {1, 4, 10}, on the two catalogs of tools/ivf_probe.py (2^18 x 64: uniform unit rows, a
mixture of 1,000 Gaussians), num_sub_vectors = 8.  Recall is a property of the data; it is reported, nothing here is a pass mark.

Memory and build.  Bytes of the codes and codebooks beside the bytes of the cell-ordered fp32 copy they replace; wall seconds
of ``build`` (cells, codebooks) and of the first search (which encodes the rows).
"""
from __future__ import annotations

import argparse
import ctypes
import importlib
import importlib.util
import json
import pathlib
import sys
import time

import numpy as np
import torch

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
_spec = importlib.util.spec_from_file_location("ivf_probe", ROOT / "tools" / "ivf_probe.py")
base = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(base)

D, K, REFINE = 128, 20, 4
CATALOGS = (62_423, 2**22)
QS, NPROBES, EXCLUDED = (1, 8, 32, 1024), (1, 8, 32), (0, 150)
STAGE_REGIONS = 3
RECALL_NPROBES, RECALL_FACTORS = (1, 8, 32), (1, 4, 10)
DEV = base.DEV


def timed_build(mf, rows: torch.Tensor, **kw) -> tuple:
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    index = mf.retrieval.QuantizedIndex.build(rows, seed=0, refine_factor=REFINE, **kw)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    index.search(rows[:1], K)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    npad, d = index.row_of.numel(), rows.shape[1]
    info = {"N": rows.shape[0], "d": d, "num_partitions": index.num_partitions, "num_sub_vectors": index.num_sub_vectors, "dsub": index.dsub,
            "build_s": t1 - t0, "first_search_s": t2 - t1, "code_bytes": index.codes().numel(), "codebook_bytes": index.codebooks.numel() * 4,
            "cell_ordered_fp32_bytes": npad * d * 4, "fp32_copy_over_codes": npad * d * 4 / index.codes().numel()}
    return index, info


def stages(mf, index, q, csr, nprobe: int) -> dict:
    """The four stages of ``path="pq"`` alone, each on the inputs the search gives it."""
    lib, L = mf._lib.lib(), mf._lib
    nq, r = q.shape[0], REFINE * K
    off, ids = csr if csr is not None else (None, None)
    probe_scores, probes = index.coarse.search(q, nprobe)
    plan = (ctypes.c_int64 * 4)()
    L.check(lib.mf_pq_plan(nq, nprobe, r, index.max_cell_blocks, plan))
    ws = L.workspace(lib.mf_pq_ws_bytes(nq, nprobe, r, index.max_cell_blocks), q.device)
    approx = torch.empty(nq, r, dtype=torch.float32, device=DEV)
    cand = torch.empty(nq, r, dtype=torch.int64, device=DEV)
    scores = torch.empty(nq, K, dtype=torch.float32, device=DEV)
    rows = torch.empty(nq, K, dtype=torch.int64, device=DEV)
    n, d = index.embeddings.shape

    def scan():
        L.check(lib.mf_pq_scan(q.data_ptr(), nq, index.codes().data_ptr(), index.codebooks.data_ptr(), index.dsub, index.cell_blk.data_ptr(),
                               index.row_of.data_ptr(), index.row_of.numel(), n, index.num_partitions, d, index.max_cell_blocks,
                               probes.data_ptr(), probe_scores.data_ptr(), nprobe, r, 0, L.ptr(off), L.ptr(ids), index.idx_base, ws.data_ptr(),
                               ws.numel(), L.stream_ptr()))

    def merge():
        L.check(lib.mf_topk_merge_packed_deep(ws.data_ptr(), plan[1], nq, r, approx.data_ptr(), cand.data_ptr(), L.stream_ptr()))

    def refine():
        L.check(lib.mf_pq_refine(q.data_ptr(), nq, index.embeddings.data_ptr(), n, d, cand.data_ptr(), r, K, index.idx_base, scores.data_ptr(),
                                 rows.data_ptr(), L.stream_ptr()))

    scan()
    merge()
    out = base.alternate({"probes": lambda: index.coarse.search(q, nprobe), "scan": scan, "merge": merge, "refine": refine},
                         regions=STAGE_REGIONS)
    return {name: v["us"] for name, v in out.items()}


def distinct_rows(g, n: int, count: int) -> np.ndarray:
    rows = np.unique(g.integers(0, n, count))
    while rows.size < count:
        rows = np.unique(np.concatenate([rows, g.integers(0, n, count - rows.size)]))
    return rows


def time_catalog(mf, n: int, res: dict) -> None:
    rows = base.unit_rows(n, D, seed=n % 1000)
    index, info = timed_build(mf, rows)
    res["builds"].append(info)
    print(json.dumps(info), flush=True)
    exact = mf.retrieval.ItemIndex(rows)
    queries = base.unit_rows(max(QS), D, seed=7)
    g = np.random.default_rng(1)
    for nq in QS:
        q = queries[:nq].contiguous()
        for excluded in EXCLUDED:
            csr = mf.retrieval._csr([distinct_rows(g, n, excluded) for _ in range(nq)], nq, DEV) if excluded else None
            for nprobe in NPROBES:
                if nprobe > index.num_partitions:
                    continue
                cell = {"N": n, "Q": nq, "nprobe": nprobe, "excluded_per_query": excluded, "k": K, "refine_factor": REFINE,
                        "slices": index.plan(nq, K, nprobe)["slices"], "slices_cells": index.plan(nq, K, nprobe, path="cells")["slices"]}
                cell.update(base.alternate({"pq": lambda: index.search(q, K, exclude_csr=csr, nprobe=nprobe),
                                            "cells": lambda: index.search(q, K, exclude_csr=csr, nprobe=nprobe, path="cells"),
                                            "exact": lambda: exact.search(q, K, exclude_csr=csr)}))
                cell["cells_over_pq"] = cell["cells"]["us"] / cell["pq"]["us"]
                cell["exact_over_pq"] = cell["exact"]["us"] / cell["pq"]["us"]
                cell["pq_slower_than_cells"] = bool(cell["pq"]["us"] > cell["cells"]["us"])
                cell["pq_slower_than_exact"] = bool(cell["pq"]["us"] > cell["exact"]["us"])
                cell["stages"] = stages(mf, index, q, csr, nprobe)
                res["cells"].append(cell)
                print(json.dumps(cell), flush=True)


def _recall(got: torch.Tensor, want: torch.Tensor) -> float:
    hits = (got.unsqueeze(2) == want.unsqueeze(1)).any(dim=2) & (got >= 0)
    return float(hits.sum()) / max(1, int((want >= 0).sum()))


def recall(mf, name: str, rows: torch.Tensor, queries: torch.Tensor, res: dict) -> None:
    index, info = timed_build(mf, rows)
    want = index.search(queries, K, path="exact")[1]
    entry = {"data": name, **info, "Q": queries.shape[0], "k": K, "against_exact": {}, "against_cells": {}, "cells_against_exact": {}}
    for nprobe in RECALL_NPROBES:
        cells = index.search(queries, K, nprobe=nprobe, path="cells")[1]
        entry["cells_against_exact"][str(nprobe)] = _recall(cells, want)
        for rf in RECALL_FACTORS:
            got = index.search(queries, K, nprobe=nprobe, refine_factor=rf)[1]
            entry["against_exact"][f"nprobe{nprobe}_rf{rf}"] = _recall(got, want)
            entry["against_cells"][f"nprobe{nprobe}_rf{rf}"] = _recall(got, cells)
    res["recall"].append(entry)
    print(json.dumps(entry), flush=True)


# ------------------------------------------------------------------------------- --deep: path="pq_deep" beside its neighbours ----
DEEP_QS, DEEP_DEPTHS, DEEP_NPROBES, DEEP_SHALLOW = (1, 32, 1024), ((100, 4), (256, 4), (1000, 1)), (1, 8, 16), ((20, 4), (64, 4))
DEEP_WARMUP, DEEP_MAX_ITERS, DEEP_REGION_US = 3, 20, 20_000.0


def deep_alternate(arms: dict, regions: int = base.REGIONS) -> dict:
    """``ivf_probe.alternate`` with the calls of a region chosen per cell: a region of the slowest arm lasts about DEEP_REGION_US."""
    for fn in arms.values():
        for _ in range(DEEP_WARMUP):
            fn()
    torch.cuda.synchronize()
    slowest = max(base.region_us(fn, 1) for fn in arms.values())
    iters = int(min(DEEP_MAX_ITERS, max(1, DEEP_REGION_US // max(slowest, 1.0))))
    return base.alternate(arms, iters=iters, regions=regions, warmup=0)


def deep_stages(mf, index, q, csr, nprobe: int, k: int, rf: int) -> dict:
    """The four stages of ``path="pq_deep"`` one by one, each on the inputs the search hands it."""
    lib, L = mf._lib.lib(), mf._lib
    nq, r = q.shape[0], rf * k
    off, ids = csr if csr is not None else (None, None)
    probe_scores, probes = index.coarse.search(q, nprobe)
    probe_scores, probes = probe_scores.clone(), probes.clone()
    lists = index.plan(nq, k, nprobe, rf, path="pq_deep")["lists"]
    ws = L.workspace(lib.mf_pq_deep_ws_bytes(nq, nprobe, r, index.max_cell_blocks), q.device)
    approx = torch.empty(nq, r, dtype=torch.float32, device=DEV)
    cand = torch.empty(nq, r, dtype=torch.int64, device=DEV)
    scores = torch.empty(nq, k, dtype=torch.float32, device=DEV)
    rows = torch.empty(nq, k, dtype=torch.int64, device=DEV)
    n, d = index.embeddings.shape

    def scan():
        L.check(lib.mf_pq_scan_deep(q.data_ptr(), nq, index.codes().data_ptr(), index.codebooks.data_ptr(), index.dsub, index.cell_blk.data_ptr(),
                                    index.row_of.data_ptr(), index.row_of.numel(), n, index.num_partitions, d, index.max_cell_blocks,
                                    probes.data_ptr(), probe_scores.data_ptr(), nprobe, r, 0, L.ptr(off), L.ptr(ids), index.idx_base,
                                    ws.data_ptr(), ws.numel(), L.stream_ptr()))

    def merge():
        L.check(lib.mf_topk_merge_packed_deep(ws.data_ptr(), lists, nq, r, approx.data_ptr(), cand.data_ptr(), L.stream_ptr()))

    def refine():
        L.check(lib.mf_pq_refine_deep(q.data_ptr(), nq, index.embeddings.data_ptr(), n, d, cand.data_ptr(), r, k, index.idx_base,
                                      scores.data_ptr(), rows.data_ptr(), L.stream_ptr()))

    scan()
    merge()
    out = deep_alternate({"cells": lambda: index.coarse.search(q, nprobe), "scan": scan, "merge": merge, "refine": refine}, regions=STAGE_REGIONS)
    return {name: v["us"] for name, v in out.items()}


def deep_catalog(mf, n: int, res: dict, out_path: pathlib.Path) -> None:
    rows = base.unit_rows(n, D, seed=n % 1000)
    index, info = timed_build(mf, rows)
    res["builds"].append(info)
    print(json.dumps(info), flush=True)
    exact = mf.retrieval.ItemIndex(rows)
    queries = base.unit_rows(max(DEEP_QS), D, seed=7)
    g = np.random.default_rng(1)
    for nq in DEEP_QS:
        q = queries[:nq].contiguous()
        lists = {0: None, 150: mf.retrieval._csr([distinct_rows(g, n, 150) for _ in range(nq)], nq, DEV)}
        for nprobe in DEEP_NPROBES:
            for k, rf in DEEP_SHALLOW:                         # where both quantised paths serve the shape
                cell = {"N": n, "Q": nq, "k": k, "refine_factor": rf, "nprobe": nprobe}
                cell.update(deep_alternate({"pq_deep": lambda: index.search(q, k, nprobe=nprobe, refine_factor=rf, path="pq_deep"),
                                            "pq": lambda: index.search(q, k, nprobe=nprobe, refine_factor=rf, path="pq")}))
                cell["pq_deep_over_pq"] = cell["pq_deep"]["us"] / cell["pq"]["us"]
                res["shallow"].append(cell)
                print(json.dumps(cell), flush=True)
            for k, rf in DEEP_DEPTHS:
                for excluded in EXCLUDED:
                    csr = lists[excluded]
                    cell = {"N": n, "Q": nq, "k": k, "refine_factor": rf, "nprobe": nprobe, "excluded_per_query": excluded,
                            "slices": index.plan(nq, k, nprobe, rf, path="pq_deep")["slices"],
                            "slices_cells_deep": index.plan(nq, k, nprobe, path="cells_deep")["slices"]}
                    cell.update(deep_alternate({
                        "pq_deep": lambda: index.search(q, k, exclude_csr=csr, nprobe=nprobe, refine_factor=rf, path="pq_deep"),
                        "cells_deep": lambda: index.search(q, k, exclude_csr=csr, nprobe=nprobe, path="cells_deep"),
                        "deep": lambda: exact.search(q, k, exclude_csr=csr, path="deep")}))
                    cell["cells_deep_over_pq_deep"] = cell["cells_deep"]["us"] / cell["pq_deep"]["us"]
                    cell["deep_over_pq_deep"] = cell["deep"]["us"] / cell["pq_deep"]["us"]
                    cell["pq_deep_slower_than_cells_deep"] = bool(cell["pq_deep"]["us"] > cell["cells_deep"]["us"])
                    cell["pq_deep_slower_than_deep"] = bool(cell["pq_deep"]["us"] > cell["deep"]["us"])
                    cell["stages_us"] = deep_stages(mf, index, q, csr, nprobe, k, rf)
                    res["cells"].append(cell)
                    print(json.dumps(cell), flush=True)
                    out_path.write_text(json.dumps(res, indent=1) + "\n")


def deep_main(mf, args) -> None:
    """``--deep``: ``path="pq_deep"`` beside ``path="cells_deep"`` of the same index (the parent's exact scan of the same cells,
    which builds the cell-ordered fp32 copy) and ``ItemIndex.search(path="deep")`` on the same rows -- Q in {1, 32, 1024} x
    (top_k, refine_factor) in {(100, 4), (256, 4), (1000, 1)} x nprobe in {1, 8, 16} x {no exclusions, 150 per query}, the arms
    alternating in one process, 7 regions per arm, the calls of a region chosen per cell; the four stages one by one; and at
    (20, 4) and (64, 4) ``pq_deep`` beside ``pq``."""
    out_path = pathlib.Path(args.out if args.out else ROOT / "profiles" / "ivf_pq_deep_probe.json")
    out_path.parent.mkdir(parents=True, exist_ok=True)
    res = {"protocol": {"regions": base.REGIONS, "warmup": DEEP_WARMUP, "stage_regions": STAGE_REGIONS,
                        "iters": f"1..{DEEP_MAX_ITERS}, a region of the slowest arm about {DEEP_REGION_US:.0f} us",
                        "arms": "alternate region by region", "cells_deep": "QuantizedIndex.search(path='cells_deep'): the parent's deep cell scan",
                        "deep": "ItemIndex.search(path='deep') of the same library"},
           "device": torch.cuda.get_device_name(0), "builds": [], "shallow": [], "cells": []}
    for n in map(int, args.catalogs.split(",")):
        deep_catalog(mf, n, res, out_path)
    out_path.write_text(json.dumps(res, indent=1) + "\n")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--deep", action="store_true", help="time path='pq_deep' (profiles/ivf_pq_deep_probe.json)")
    ap.add_argument("--catalogs", default=",".join(map(str, CATALOGS)), help="with --deep: the catalog sizes to time")
    args = ap.parse_args()
    mf = importlib.import_module("matrix-factorization-torch_amd")
    if args.deep:
        deep_main(mf, args)
        return
    args.out = args.out or str(ROOT / "profiles" / "ivf_pq_probe.json")
    res = {"protocol": {"k": K, "refine_factor": REFINE, "iters": base.ITERS, "regions": base.REGIONS, "warmup": base.WARMUP,
                        "stage_regions": STAGE_REGIONS, "arms": "alternate region by region",
                        "cells": "QuantizedIndex.search(path='cells'): PartitionedIndex.search of the same library",
                        "exact": "ItemIndex.search(path='auto') of the same library"},
           "device": torch.cuda.get_device_name(0), "builds": [], "cells": [], "recall": []}
    out_path = pathlib.Path(args.out)
    out_path.parent.mkdir(parents=True, exist_ok=True)
    for n in CATALOGS:
        time_catalog(mf, n, res)
        out_path.write_text(json.dumps(res, indent=1) + "\n")
    recall(mf, "uniform unit rows", base.unit_rows(base.RECALL_N, base.RECALL_D, 3), base.unit_rows(base.RECALL_Q, base.RECALL_D, 4), res)
    centres = base.unit_rows(1000, base.RECALL_D, 5)
    recall(mf, "mixture of 1000 Gaussians (sigma 0.15 per coordinate)", base.mixture_rows(base.RECALL_N, base.RECALL_D, 6, centres),
           base.mixture_rows(base.RECALL_Q, base.RECALL_D, 8, centres), res)
    out_path.write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
