#!/usr/bin/env python3
"""Times the filtered search (``ItemIndex.search(where=...)`` through a cached ``FilteredView``) beside the only way the parent
commit can answer the same question: every inadmissible row on every query's exclusion list.

    python tools/filter_probe.py --parent-lib path/to/parent/libmf_hip.so [--out profiles/filter_probe.json]

``--parent-lib``: ``libmf_hip.so`` built from the parent commit (``make -C .../csrc LIB=...`` there); without it the baseline
runs on this commit's library (recorded as such -- the engines' kernel text is the same, profiles/filter_digest_*.json).  It is
loaded beside this commit's library in the same process, so the arms can alternate region by region; ``MF_HIP_LIB`` would give
the same library to a process that could time nothing else.

Catalogs 62,423 x 128 and 2^22 x 128 (unit rows), selectivity 1 % / 10 % / 50 % (an allow-mask of exactly round(s N) random rows),
Q = 1 / 32 / 1024, k = 20.  Device microseconds per call: HIP events around ITERS calls, REGIONS such regions per arm after every
arm has run WARMUP calls, the arms alternating region by region; median, spread = max - min.

  view      (b) ``view.search(q, 20)`` on the cached view (``path="auto"``; no exclusion lists: the filter is the whole question)
  baseline  (c) ``ItemIndex.search(q, 20, exclude_csr=...)`` of the parent's library on the whole catalog, the N - M inadmissible
            rows on every query's list, the device CSR built beforehand (host list building is not charged); skipped, and named,
            where those lists would hold more than MAX_BASELINE_ENTRIES entries
  m_rows    the unfiltered search of the view's own M-row index: what the bytes say (b) should approach

  build     (a) ``mf_filter_rows`` + ``mf_gather_rows`` on kept buffers (the host read of M is not in it), and separately the
            derived copies a first search may build: ``blocked`` (few-query scan) and ``bf16`` (prefilter index)

``--no-baseline`` times only ``view`` and ``m_rows`` against each other (no baseline regions, and so none of their list traffic,
between them).  ``view_slower`` says (b) lost the cell beyond (c)'s own spread; ``uncached_us`` = build + view for a filter seen for the first time.
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

D, K = 128, 20
CATALOGS = (62_423, 2**22)
SELECTIVITY = (0.01, 0.10, 0.50)
QS = (1, 32, 1024)
ITERS, REGIONS, WARMUP = 10, 7, 3
MAX_BASELINE_ENTRIES = 2**28         # 2 GiB of list entries per call
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


def second_library(mf, path: str):
    """The parent's library beside ours: the symbols it has, bound with our signatures."""
    handle = ctypes.CDLL(path)
    for name, (res, args) in mf._lib.SIGNATURES.items():
        if hasattr(handle, name):
            fn = getattr(handle, name)
            fn.restype, fn.argtypes = res, args
    return handle


def build_arms(mf, index, mask64: torch.Tensor, view) -> dict:
    lib = mf._lib.lib()
    emb = index.embeddings
    n, d = emb.shape
    m = view.num_items
    rows = torch.empty(n, dtype=torch.int64, device=DEV)
    rank = torch.empty(n, dtype=torch.int32, device=DEV)
    count = torch.empty(1, dtype=torch.int64, device=DEV)
    ws = mf._lib.workspace(lib.mf_filter_ws_bytes(n), DEV)
    sub = torch.empty(m, d, dtype=torch.float32, device=DEV)

    def build():
        mf._lib.check(lib.mf_filter_rows(mask64.data_ptr(), n, 0, 1, 0, ws.data_ptr(), ws.numel(), rows.data_ptr(), rank.data_ptr(),
                                         count.data_ptr(), mf._lib.stream_ptr()))
        mf._lib.check(lib.mf_gather_rows(emb.data_ptr(), n, d, rows.data_ptr(), m, 0, sub.data_ptr(), None, mf._lib.stream_ptr()))

    blocked = torch.empty(lib.mf_topk_blocked_bytes(m, d) // 4, dtype=torch.float32, device=DEV)
    bf16 = torch.empty(lib.mf_topk_bf3_index_bytes(m, d), dtype=torch.uint8, device=DEV)
    src = view.index.embeddings
    return {"build": build,
            "blocked": lambda: mf._lib.check(lib.mf_topk_blocked_build(src.data_ptr(), m, d, blocked.data_ptr(), mf._lib.stream_ptr())),
            "bf16": lambda: mf._lib.check(lib.mf_topk_bf3_build(src.data_ptr(), m, d, bf16.data_ptr(), bf16.numel(), mf._lib.stream_ptr()))}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "filter_probe.json"))
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--no-baseline", action="store_true", help="only the view and the M-row search, alternating: no list traffic between them")
    args = ap.parse_args()
    mf = importlib.import_module("matrix-factorization-torch_amd")
    own = mf._lib.lib()
    parent = second_library(mf, args.parent_lib) if args.parent_lib else own
    res = {"protocol": {"k": K, "d": D, "iters": ITERS, "regions": REGIONS, "warmup": WARMUP, "arms": "alternate region by region",
                        "baseline_library": "parent commit" if args.parent_lib else "this commit (no --parent-lib)",
                        "max_baseline_entries": MAX_BASELINE_ENTRIES},
           "device": torch.cuda.get_device_name(0), "builds": [], "cells": []}
    for n in CATALOGS:
        items = unit_rows(n, D, seed=n % 1000)
        index = mf.retrieval.ItemIndex(items)
        queries = unit_rows(max(QS), D, seed=7)
        for sel in SELECTIVITY:
            m = round(sel * n)
            g = torch.Generator(device=DEV).manual_seed(int(sel * 100))
            mask = torch.zeros(n, dtype=torch.bool, device=DEV)
            mask[torch.randperm(n, generator=g, device=DEV)[:m]] = True
            view = index.filtered(mask)
            assert view.num_items == m
            entry = {"N": n, "M": m, "selectivity": sel, **alternate(build_arms(mf, index, mask.to(torch.int64), view))}
            res["builds"].append(entry)
            print(json.dumps(entry), flush=True)
            outside = torch.nonzero(~mask).flatten()
            for nq in QS:
                q = queries[:nq].contiguous()
                arms = {"view": lambda: view.search(q, K), "m_rows": lambda: view.index.search(q, K)}
                entries = nq * (n - m)
                if entries <= MAX_BASELINE_ENTRIES and not args.no_baseline:
                    csr = (torch.arange(nq + 1, dtype=torch.int64, device=DEV) * (n - m), outside.repeat(nq))

                    def baseline():
                        mf._lib._lib = parent
                        try:
                            return index.search(q, K, exclude_csr=csr)
                        finally:
                            mf._lib._lib = own

                    got, want = view.search(q, K), baseline()
                    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
                    arms["baseline"] = baseline
                big = n > 100_000
                cell = {"N": n, "M": m, "selectivity": sel, "Q": nq, "baseline_entries": entries,
                        **alternate(arms, iters=3 if big else ITERS, regions=5 if big else REGIONS)}
                cell["uncached_us"] = cell["view"]["us"] + entry["build"]["us"]
                if "baseline" in cell:
                    cell["baseline_over_view"] = cell["baseline"]["us"] / cell["view"]["us"]
                    cell["view_slower"] = bool(cell["view"]["us"] > cell["baseline"]["us"] + cell["baseline"]["spread_us"])
                    cell["uncached_slower"] = bool(cell["uncached_us"] > cell["baseline"]["us"] + cell["baseline"]["spread_us"])
                else:
                    cell["baseline_skipped"] = "--no-baseline" if args.no_baseline else f"lists of {entries} entries exceed {MAX_BASELINE_ENTRIES}"
                res["cells"].append(cell)
                print(json.dumps(cell), flush=True)
                del arms
            del view, outside
        del index, items
        torch.cuda.empty_cache()
    out_path = pathlib.Path(args.out)
    out_path.parent.mkdir(parents=True, exist_ok=True)
    head = "".join(f" {json.dumps(k)}: {json.dumps(v)},\n" for k, v in res.items() if k not in ("builds", "cells"))      # one entry per line
    body = ",\n".join(f' "{k}": [\n' + ",\n".join("  " + json.dumps(e) for e in res[k]) + "\n ]" for k in ("builds", "cells"))
    out_path.write_text("{\n" + head + body + "\n}\n")


if __name__ == "__main__":
    main()
