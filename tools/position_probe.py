#!/usr/bin/env python3
"""Times metrics from exact positions (mf_target_positions + mf_position_metrics) against the list path they replace
(mf_topk_deep at k = 1000 + mf_retrieval_metrics), on the same inputs.

    MF_HIP_LIB=path/to/parent/libmf_hip.so python tools/position_probe.py [--out profiles/position_probe.json]      (or --list-lib)

Catalog N = 62,423 x d = 128 (unit rows), Q in {1, 32, 1024}, 1 / 20 / 1000 targets per query (distinct random rows, ratings
1 .. 5), 150 excluded rows per query.  Both paths are called through the C ABI on kept buffers and their preferred
workspaces; per cell, device time per call -- device events around ITERS calls, three such regions after warm-up, the median
and the spread (max - min) -- of the two calls together, and of each alone (``find_ms``, ``metrics_ms``).  The list path runs in a child process on ``MF_HIP_LIB`` / ``--list-lib`` (a build of the parent commit;
default: this build, where the list path's code is the same) and binds only the four exports it calls; the position path
always runs on this tree's build.  ``positions_over_list`` is
the measured ratio; ``max_abs_diff`` compares the six values @1000 of the two paths (reported, not asserted).
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import pathlib
import statistics
import subprocess
import sys

import torch

ROOT = pathlib.Path(__file__).resolve().parents[1]
DEFAULT_LIB = ROOT / "matrix-factorization-torch_amd" / "lib" / "libmf_hip.so"

N, D, K = 62_423, 128, 1000
QS, TS, EXCL = (1, 32, 1024), (1, 20, 1000), 150
DEV = "cuda:0"
vp, i64, sz = ctypes.c_void_p, ctypes.c_int64, ctypes.c_size_t
PARTS = ("ms", "spread_ms", "find_ms", "metrics_ms")      # the two calls together; the search / position call and the metrics call alone


def region_ms(fn, iters: int) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def measure(fn, iters: int = 20, warmup: int = 10, regions: int = 3) -> dict:
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    runs = [region_ms(fn, iters) for _ in range(regions)]
    return {"ms": statistics.median(runs), "spread_ms": max(runs) - min(runs)}


def catalog():
    g = torch.Generator().manual_seed(0)
    return torch.nn.functional.normalize(torch.randn(N, D, generator=g), dim=-1).to(DEV)


def inputs(nq: int, nt: int):
    """The same in both processes: queries, exclusion CSR, target CSR with ratings."""
    g = torch.Generator().manual_seed(1000 * nq + nt)
    q = torch.nn.functional.normalize(torch.randn(nq, D, generator=g), dim=-1).to(DEV)
    rows = torch.stack([torch.randperm(N, generator=g)[: EXCL + nt] for _ in range(nq)])
    excl, tgt = rows[:, :EXCL].sort(dim=1).values, rows[:, EXCL:]
    csr = lambda m: torch.arange(0, (nq + 1) * m, m, dtype=torch.int64).to(DEV)      # noqa: E731
    rel = torch.randint(1, 6, (nq * nt,), generator=g).float()
    return q, (csr(EXCL), excl.reshape(-1).to(DEV)), (csr(nt), tgt.reshape(-1).contiguous().to(DEV), rel.to(DEV))


def check(lib, rc):
    if rc:
        raise RuntimeError(lib.mf_last_error().decode())


def stream():
    return torch.cuda.current_stream().cuda_stream


def list_path(lib, items, q, excl, tgt):
    nq = q.shape[0]
    nbytes = lib.mf_topk_deep_ws_bytes(nq, N, D, K)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    s = torch.empty(nq, K, device=DEV)
    rows = torch.empty(nq, K, dtype=torch.int64, device=DEV)
    out = torch.empty(nq, 6, device=DEV)

    def find():
        check(lib, lib.mf_topk_deep(q.data_ptr(), nq, items.data_ptr(), N, D, K, excl[0].data_ptr(), excl[1].data_ptr(), 0, ws.data_ptr(),
                                    nbytes, s.data_ptr(), rows.data_ptr(), stream()))

    def metrics():
        check(lib, lib.mf_retrieval_metrics(rows.data_ptr(), nq, K, tgt[0].data_ptr(), tgt[1].data_ptr(), tgt[2].data_ptr(), out.data_ptr(),
                                            stream()))
    return find, metrics, out


def positions_path(lib, items, q, excl, tgt):
    nq, nt = q.shape[0], tgt[1].numel()
    nbytes = lib.mf_target_positions_ws_bytes(nq, N, D)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    pos = torch.empty(nt, dtype=torch.int64, device=DEV)
    score = torch.empty(nt, device=DEV)
    ncand = torch.empty(nq, dtype=torch.int64, device=DEV)
    out = torch.empty(nq, 9, device=DEV)
    ks = (ctypes.c_int32 * 1)(K)

    def find():
        check(lib, lib.mf_target_positions(q.data_ptr(), nq, items.data_ptr(), N, D, tgt[0].data_ptr(), tgt[1].data_ptr(), nt,
                                           excl[0].data_ptr(), excl[1].data_ptr(), 0, ws.data_ptr(), nbytes, pos.data_ptr(), score.data_ptr(),
                                           ncand.data_ptr(), stream()))

    def metrics():
        check(lib, lib.mf_position_metrics(pos.data_ptr(), tgt[0].data_ptr(), tgt[2].data_ptr(), ncand.data_ptr(), nq, ks, 1, out.data_ptr(),
                                           stream()))
    return find, metrics, out


def bind(path, names):
    lib = ctypes.CDLL(str(path))
    sig = {
        "mf_last_error": (ctypes.c_char_p, []),
        "mf_topk_deep_ws_bytes": (sz, [i64, i64, ctypes.c_int, ctypes.c_int]),
        "mf_topk_deep": (ctypes.c_int, [vp, i64, vp, i64, ctypes.c_int, ctypes.c_int, vp, vp, i64, vp, sz, vp, vp, vp]),
        "mf_retrieval_metrics": (ctypes.c_int, [vp, i64, ctypes.c_int, vp, vp, vp, vp, vp]),
        "mf_target_positions_ws_bytes": (sz, [i64, i64, ctypes.c_int]),
        "mf_target_positions": (ctypes.c_int, [vp, i64, vp, i64, ctypes.c_int, vp, vp, i64, vp, vp, i64, vp, sz, vp, vp, vp, vp]),
        "mf_position_metrics": (ctypes.c_int, [vp, vp, vp, vp, i64, ctypes.POINTER(ctypes.c_int32), ctypes.c_int, vp, vp]),
    }
    for name in names:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = sig[name]
    return lib


def run(path, which: str) -> list[dict]:
    names = {"list": ("mf_last_error", "mf_topk_deep_ws_bytes", "mf_topk_deep", "mf_retrieval_metrics"),
             "positions": ("mf_last_error", "mf_target_positions_ws_bytes", "mf_target_positions", "mf_position_metrics")}[which]
    lib = bind(path, names)
    items = catalog()
    cells = []
    for nq in QS:
        for nt in TS:
            q, excl, tgt = inputs(nq, nt)
            find, metrics, out = (list_path if which == "list" else positions_path)(lib, items, q, excl, tgt)
            cell = {"Q": nq, "targets": nt, **measure(lambda: (find(), metrics())), "find_ms": measure(find)["ms"],
                    "metrics_ms": measure(metrics)["ms"]}
            cell["values"] = out[:, :6].double().mean(dim=0).tolist()
            cells.append(cell)
            print(json.dumps({which: cell}), file=sys.stderr, flush=True)
    return cells


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "position_probe.json"))
    ap.add_argument("--list-lib", default=os.environ.get("MF_HIP_LIB", str(DEFAULT_LIB)),
                    help="the library the list path is timed on: a build of the parent commit (default: MF_HIP_LIB, else this build)")
    ap.add_argument("--child", choices=("list",), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        print(json.dumps(run(args.list_lib, args.child)))
        return
    # (a child process: two builds of the library do not share one process)
    child = subprocess.run([sys.executable, __file__, "--child", "list", "--list-lib", args.list_lib], check=True, stdout=subprocess.PIPE, text=True)
    lists = json.loads(child.stdout.strip().splitlines()[-1])
    res = {"shape": {"N": N, "d": D, "k": K, "exclusions_per_query": EXCL}, "list_lib": pathlib.Path(args.list_lib).name
           if pathlib.Path(args.list_lib) == DEFAULT_LIB else "parent build", "cells": []}
    for mine, theirs in zip(run(DEFAULT_LIB, "positions"), lists):
        assert (mine["Q"], mine["targets"]) == (theirs["Q"], theirs["targets"])
        cell = {"Q": mine["Q"], "targets": mine["targets"],
                "positions": {k: mine[k] for k in PARTS}, "list_k1000": {k: theirs[k] for k in PARTS},
                "positions_over_list": mine["ms"] / theirs["ms"],
                "max_abs_diff": max(abs(a - b) for a, b in zip(mine["values"], theirs["values"]))}
        res["cells"].append(cell)
        print(json.dumps(cell), flush=True)
    out_path = pathlib.Path(args.out)
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
