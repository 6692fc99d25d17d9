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

    MF_HIP_LIB=path/to/parent/libmf_hip.so python tools/position_probe.py --shards 1,2,8 [--out profiles/sharded_position_probe.json]

``--shards``: the sharded position path instead -- per cell and S, device time of ``mf_target_words`` + ``mf_key_positions`` on ONE
shard of the catalog (shard 0 of S dealt round-robin: N / S rows, the exclusion lists localised, the words those of the whole
catalog), together and each alone; beside it ``mf_target_positions`` on the whole catalog from this build and, in a child
process, from ``MF_HIP_LIB`` / ``--list-lib`` (a build of the parent commit).  ``positions_guard`` puts the two side by side: this
build's median may exceed the parent's by no more than the parent's own spread over its three regions.  The exchange between
the two calls and after them is not in any of these numbers.
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


def shard_path(lib, items, q, excl, tgt, shards: int):
    """Shard 0 of ``shards`` (rows 0, S, 2 S, ..): the two calls of the sharded path; the words are the whole catalog's."""
    nq, nt = q.shape[0], tgt[1].numel()
    part = items[::shards].contiguous()
    n = part.shape[0]
    local = torch.where(excl[1] % shards == 0, excl[1] // shards, torch.full_like(excl[1], -1))
    nbytes = lib.mf_key_positions_ws_bytes(nq, n, D)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    words = torch.empty(nt, dtype=torch.int64, device=DEV)
    mine = torch.empty(nt, dtype=torch.int64, device=DEV)
    above = torch.empty(nt, dtype=torch.int64, device=DEV)
    score = torch.empty(nt, device=DEV)
    ncand = torch.empty(nq, dtype=torch.int64, device=DEV)
    check(lib, lib.mf_target_words(q.data_ptr(), nq, items.data_ptr(), N, D, tgt[0].data_ptr(), tgt[1].data_ptr(), nt, 1, 0, words.data_ptr(),
                                   stream()))

    def find_words():
        check(lib, lib.mf_target_words(q.data_ptr(), nq, part.data_ptr(), n, D, tgt[0].data_ptr(), tgt[1].data_ptr(), nt, shards, 0,
                                       mine.data_ptr(), stream()))

    def count():
        check(lib, lib.mf_key_positions(q.data_ptr(), nq, part.data_ptr(), n, D, tgt[0].data_ptr(), tgt[1].data_ptr(), words.data_ptr(), nt,
                                        shards, 0, excl[0].data_ptr(), local.data_ptr(), ws.data_ptr(), nbytes, above.data_ptr(),
                                        score.data_ptr(), ncand.data_ptr(), stream()))
    return find_words, count


def run_shards(path, shard_counts, with_shards: bool) -> list[dict]:
    """Per cell: ``mf_target_positions`` on the whole catalog and, on this tree's build, the shard calls for every S."""
    names = ("mf_last_error", "mf_target_positions_ws_bytes", "mf_target_positions", "mf_position_metrics")
    lib = bind(path, names + (("mf_target_words", "mf_key_positions_ws_bytes", "mf_key_positions") if with_shards else ()))
    items = catalog()
    cells = []
    for nq in QS:
        for nt in TS:
            q, excl, tgt = inputs(nq, nt)
            find, _, _ = positions_path(lib, items, q, excl, tgt)
            cell = {"Q": nq, "targets": nt, "positions": measure(find)}
            for s in shard_counts if with_shards else ():
                find_words, count = shard_path(lib, items, q, excl, tgt, s)
                cell[f"shards_{s}"] = {**measure(lambda: (find_words(), count())), "words_ms": measure(find_words)["ms"],
                                       "count_ms": measure(count)["ms"], "rows": -(-N // s)}
            cells.append(cell)
            print(json.dumps(cell), file=sys.stderr, flush=True)
    return cells


def main_shards(args) -> None:
    shard_counts = [int(x) for x in args.shards.split(",")]
    child = subprocess.run([sys.executable, __file__, "--child", "positions", "--list-lib", args.list_lib], check=True, stdout=subprocess.PIPE,
                           text=True)
    parent = json.loads(child.stdout.strip().splitlines()[-1])
    res = {"shape": {"N": N, "d": D, "exclusions_per_query": EXCL, "shards": shard_counts, "shard": "0 of S, rows dealt round-robin"},
           "parent_lib": pathlib.Path(args.list_lib).name if pathlib.Path(args.list_lib) == DEFAULT_LIB else "parent build",
           "unit": "ms of device time per call: median of three regions; spread_ms = max - min", "exchange": "not measured", "cells": []}
    for mine, theirs in zip(run_shards(DEFAULT_LIB, shard_counts, True), parent):
        assert (mine["Q"], mine["targets"]) == (theirs["Q"], theirs["targets"])
        over = mine["positions"]["ms"] - theirs["positions"]["ms"]
        cell = {"Q": mine["Q"], "targets": mine["targets"], "parent_positions": theirs["positions"], **{k: v for k, v in mine.items() if k not in ("Q", "targets")},
                "positions_guard": {"slower_by_ms": over, "allowed_ms": theirs["positions"]["spread_ms"], "ok": over <= theirs["positions"]["spread_ms"]}}
        res["cells"].append(cell)
        print(json.dumps(cell), flush=True)
    out_path = pathlib.Path(args.out if args.out != str(ROOT / "profiles" / "position_probe.json") else ROOT / "profiles" / "sharded_position_probe.json")
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text(json.dumps(res, indent=1) + "\n")


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
        "mf_target_words": (ctypes.c_int, [vp, i64, vp, i64, ctypes.c_int, vp, vp, i64, i64, i64, vp, vp]),
        "mf_key_positions_ws_bytes": (sz, [i64, i64, ctypes.c_int]),
        "mf_key_positions": (ctypes.c_int, [vp, i64, vp, i64, ctypes.c_int, vp, vp, vp, i64, i64, i64, vp, vp, vp, sz, vp, vp, vp, vp]),
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
    ap.add_argument("--shards", default=None, help="comma-separated shard counts: time the sharded position path (see above)")
    ap.add_argument("--child", choices=("list", "positions"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child == "positions":
        print(json.dumps(run_shards(args.list_lib, (), False)))
        return
    if args.shards:
        main_shards(args)
        return
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
