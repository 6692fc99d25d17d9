#!/usr/bin/env python3
"""Times the deep top-k engine (mf_topk_deep, ``ItemIndex.search(path="deep")``) against what a user can do without it.

    python tools/topk_deep_probe.py [--out profiles/topk_deep_probe.json]

Catalog N = 62,423 x d = 128 (unit rows), ML-25M-like exclusion lists (20..300 Zipf-distributed item rows per query, as the
benchmark's retrieval leg draws them), Q in {1, 32, 1024} x k in {100, 1000}.  Per cell, device time per call -- device
events around ITERS calls, three such regions after warm-up, the median of the three and their spread (max - min) -- of

  deep          ``search(path="deep")`` on the preferred workspace
  torch         ``torch.topk(q @ E.T with the excluded entries set to -inf, k)`` on the same device: the baseline
  tiles_k64     the fp32 tile engine at k = 64, for context (the deepest list the other engines give)
  scores / select   the scoring pass and the selection pass alone (the library's own event spans around them)

``torch_over_deep`` is the measured ratio.  At Q = 1024 the call is repeated through the C ABI on workspaces that hold slabs of at
most 16 MiB, 64 MiB and the preferred size (16, 4 and 1 query blocks): what the preferred block in csrc/mf_topk_deep.hip is
set from.
"""
from __future__ import annotations

import argparse
import ctypes
import importlib
import json
import pathlib
import statistics
import sys

import torch

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

N, D = 62_423, 128
QS, KS = (1, 32, 1024), (100, 1000)
DEV = "cuda:0"


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


def exclusion_lists(q: int, gen: torch.Generator):
    w = 1.0 / torch.arange(1, N, dtype=torch.float64)          # Zipf over item rows 1 .. N - 1
    pieces, offs = [], [0]
    for n in torch.randint(20, 300, (q,), generator=gen).tolist():
        pieces.append(torch.unique(torch.multinomial(w, n, replacement=True, generator=gen) + 1))
        offs.append(offs[-1] + pieces[-1].numel())
    rows = torch.repeat_interleave(torch.arange(q), torch.tensor([p.numel() for p in pieces]))
    cols = torch.cat(pieces)
    return (torch.tensor(offs, dtype=torch.int64, device=DEV), cols.to(DEV)), rows.to(DEV), cols.to(DEV)


def spans(lib, fn, calls: int = 10) -> dict:
    lib.mf_timing_reset()
    lib.mf_timing_enable(1)
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    out, tot = {}, ctypes.c_double()
    for name in ("topk_deep_scores", "topk_deep_select"):
        lib.mf_timing_get(name.encode(), ctypes.byref(tot))
        out[name.removeprefix("topk_deep_") + "_ms"] = tot.value / calls
    lib.mf_timing_enable(0)
    lib.mf_timing_reset()
    return out


def deep_on_workspace(mf, lib, q, items, k, csr, nbytes: int):
    nq = q.shape[0]
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    s = torch.empty(nq, k, device=DEV)
    i = torch.empty(nq, k, dtype=torch.int64, device=DEV)

    def fn():
        mf._lib.check(lib.mf_topk_deep(q.data_ptr(), nq, items.data_ptr(), N, D, k, csr[0].data_ptr(), csr[1].data_ptr(), 0,
                                       ws.data_ptr(), nbytes, s.data_ptr(), i.data_ptr(), mf._lib.stream_ptr()))
    return fn


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "topk_deep_probe.json"))
    args = ap.parse_args()
    mf = importlib.import_module("matrix-factorization-torch_amd")
    lib = mf._lib.lib()
    g = torch.Generator().manual_seed(0)
    items = torch.nn.functional.normalize(torch.randn(N, D, generator=g), dim=-1).to(DEV)
    index = mf.retrieval.ItemIndex(items)
    out_path = pathlib.Path(args.out)
    res = {"shape": {"N": N, "d": D, "exclusions": "20..300 Zipf rows per query"}, "cells": [], "slab_sizes_at_Q1024": []}
    plan = (ctypes.c_int64 * 3)()
    for nq in QS:
        q = torch.nn.functional.normalize(torch.randn(nq, D, generator=g), dim=-1).to(DEV)
        csr, er, ec = exclusion_lists(nq, g)
        for k in KS:
            pref = lib.mf_topk_deep_ws_bytes(nq, N, D, k)
            if nq == 1024:
                row = (N + 31) // 32 * 32 * 4
                sizes = {"16 MiB": (16 << 20) // row // 32 * 32 * row, "64 MiB": (64 << 20) // row // 32 * 32 * row, "preferred": pref}
                for label, nbytes in sizes.items():
                    assert lib.mf_topk_deep_plan(nq, N, D, k, nbytes, plan) == 0
                    fn = deep_on_workspace(mf, lib, q, items, k, csr, nbytes)
                    res["slab_sizes_at_Q1024"].append({"workspace": label, "k": k, "queries_per_block": plan[0], "blocks": plan[1],
                                                       "slab_mib": plan[2] / 2**20, **measure(fn), **spans(lib, fn)})
                    print(json.dumps(res["slab_sizes_at_Q1024"][-1]), flush=True)

            def deep():
                return index.search(q, k, exclude_csr=csr, path="deep")

            def baseline():
                s = q @ items.T
                s[er, ec] = float("-inf")
                return torch.topk(s, k, dim=1)

            cell = {"Q": nq, "k": k, "deep": measure(deep), "torch": measure(baseline),
                    "tiles_k64": measure(lambda: index.search(q, 64, exclude_csr=csr, path="tiles")), **spans(lib, deep)}
            cell["torch_over_deep"] = cell["torch"]["ms"] / cell["deep"]["ms"]
            # the same rows wherever the baseline's BLAS order does not flip a near-tie: reported, not asserted
            cell["rows_equal_to_torch"] = float((deep()[1] == baseline()[1]).float().mean())
            res["cells"].append(cell)
            print(json.dumps(cell), flush=True)
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
