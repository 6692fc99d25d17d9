#!/usr/bin/env python3
"""Times the cell scans filtered in place (``search(allow=...)`` with a ``CellMask``) beside the same filter through a view
(``search(where=...)``), beside the unfiltered cell search, and -- for the quantised index, which takes no view -- beside the only
way the parent commit can answer the question: every inadmissible row on every query's exclusion list.

    python tools/cell_mask_probe.py [--parent-lib path/to/parent/libmf_hip.so] [--out profiles/cell_mask_probe.json]

``--parent-lib``: ``libmf_hip.so`` built from the parent commit, loaded beside this commit's library in the same process so that
the arms can alternate region by region (tools/filter_probe.py); without it the exclusion-list arm runs on this commit's library
(recorded as such -- the unfiltered scans' kernel text is the same, profiles/cell_mask_digest_*.json).

Catalogs 62,423 x 128 (128 cells) and 2^22 x 128 (2,048 cells), unit rows, one seeded build each (``QuantizedIndex.build``, 16
sub-vectors; the partitioned index is built over the same cells); selectivity 1 % / 10 % / 50 % (an allow-mask of exactly
round(s N) random rows) and 100 % (all ones: the pair of the timing condition below); Q = 1 / 32 / 1024, k = 20, nprobe = 8.
Device microseconds per call: HIP events around ITERS calls, REGIONS such regions per arm after every arm has run WARMUP calls,
the arms alternating region by region; median, spread = max - min.

  mask_build   (a) ``index.cell_mask(mask, cache=False)``: the bool mask widened to tag words, one ``mf_filter_cell_bits`` launch
  allow        (b) ``PartitionedIndex.search(q, 20, nprobe=8, allow=cell_mask)``
  view         (c) the same search on the cached view of the same mask (``view.search``: its cells hold only admissible rows)
  view_build   (d) ``PartitionedIndex.search(q, 20, nprobe=8, where=mask)`` with nothing cached: the view's build (compaction,
               gather, host read, the cells and the cell-ordered copy of the view) and the search; few regions, it is slow
  plain        (e) the unfiltered ``search(q, 20, nprobe=8)`` of the same index and library
  pq_allow / pq_plain   (b) and (e) of ``QuantizedIndex.search(path="pq")``
  pq_lists     the parent library's ``path="pq"`` search with the N - M inadmissible rows on every query's exclusion list (device
               CSR built beforehand), where a list holds at most MAX_LIST entries -- skipped and named otherwise

Per cell: ``mask_plus_allow_us`` = (a) + (b) beside ``view_build``; ``allow_over_plain`` = (b) / (e); ``view_faster`` says the cached
view beat the mask beyond the mask's own spread.  The one condition: with the all-ones mask, (b) may exceed (e) by no more than
(e)'s spread -- ``all_ones_within_spread`` (and ``pq_all_ones_within_spread``) of the 100 % cells, from ``pair_allow`` / ``pair_plain``
(``pq_pair_*``): the two arms timed alone in the order b e e b (``alternate_pair`` says why), PAIR_REGIONS regions each;
``*_excess_in_rotation_us`` keeps the difference the five-arm rotation gave.
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

D, K, NPROBE, SUB_VECTORS = 128, 20, 8, 16
CATALOGS = (62_423, 2**22)
SELECTIVITY = (0.01, 0.10, 0.50, 1.0)
QS = (1, 32, 1024)
ITERS, REGIONS, WARMUP = 10, 7, 3
PAIR_REGIONS = 16           # regions per arm of a pair that is compared to within its spread: a spread over 6 says little
MAX_LIST = 2**16            # entries of one query's exclusion list the baseline is asked to walk
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


def alternate_pair(a, b, iters: int, regions: int, warmup: int = WARMUP) -> tuple[dict, dict]:
    """Two arms alone -- (b) and (e) of the condition, passed as ``a`` and ``b`` --, regions in the order b e e b b e e b ..: each arm runs as often behind itself as behind the other, and
    behind nothing else.  In the rotation of all arms above an arm's predecessor is always the same OTHER search -- the quantised
    ``pq_allow`` runs behind the exact cell search, which has just streamed the fp32 cells through the caches, and ``pq_plain``
    behind ``pq_allow``, which has just read the very codes it needs -- so a pair that is to be compared to within its spread is
    timed here."""
    got = alternate({"a": a, "b": b}, iters=1, regions=1, warmup=warmup)      # (warm-up; its one region is dropped)
    del got
    runs = {"a": [], "b": []}
    for r in range(regions):
        for name in (("a", "b") if r % 2 == 0 else ("b", "a")):
            runs[name].append(region_us(a if name == "a" else b, iters))
    return tuple({"us": statistics.median(x), "spread_us": max(x) - min(x), "min_us": min(x), "regions": len(x), "iters": iters}
                 for x in (runs["a"], runs["b"]))


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


def same(a, b) -> bool:
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def write(path: pathlib.Path, res: dict) -> None:
    head = "".join(f" {json.dumps(k)}: {json.dumps(v)},\n" for k, v in res.items() if k not in ("builds", "cells"))      # one entry per line
    body = ",\n".join(f' "{k}": [\n' + ",\n".join("  " + json.dumps(e) for e in res[k]) + "\n ]" for k in ("builds", "cells"))
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text("{\n" + head + body + "\n}\n")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "cell_mask_probe.json"))
    ap.add_argument("--parent-lib", default=None)
    args = ap.parse_args()
    out_path = pathlib.Path(args.out)
    mf = importlib.import_module("matrix-factorization-torch_amd")
    R = mf.retrieval
    own = mf._lib.lib()
    parent = second_library(mf, args.parent_lib) if args.parent_lib else own
    res = {"protocol": {"k": K, "d": D, "nprobe": NPROBE, "num_sub_vectors": SUB_VECTORS, "iters": ITERS, "regions": REGIONS, "warmup": WARMUP,
                        "iters_and_regions": "unless stated per arm: 3 x 5 at N = 2^22 and where a pq_lists arm runs at Q = 1024",
                        "pair_regions": PAIR_REGIONS, "arms": "alternate region by region", "max_list_entries": MAX_LIST,
                        "pq_lists_library": "parent commit" if args.parent_lib else "this commit (no --parent-lib)"},
           "device": torch.cuda.get_device_name(0), "builds": [], "cells": []}
    for n in CATALOGS:
        items = unit_rows(n, D, seed=n % 1000)
        quant = R.QuantizedIndex.build(items, num_sub_vectors=SUB_VECTORS, iters=4, pq_iters=4, seed=0, num_probes=NPROBE)
        part = R.PartitionedIndex.from_assignment(items, quant.centroids, quant.assign, num_probes=NPROBE)
        npad = part.row_of.numel()
        queries = unit_rows(max(QS), D, seed=7)
        big = n > 100_000
        for sel in SELECTIVITY:
            m = round(sel * n)
            g = torch.Generator(device=DEV).manual_seed(int(sel * 100))
            mask = torch.zeros(n, dtype=torch.bool, device=DEV)
            mask[torch.randperm(n, generator=g, device=DEV)[:m]] = True
            cm, cm_q = part.cell_mask(mask), quant.cell_mask(mask)
            view = part.filtered(mask)
            assert view.num_items == m
            skipped_blocks = int((cm.words[0] == 0).sum())
            entry = {"N": n, "M": m, "selectivity": sel, "cells": part.num_partitions, "Npad": npad, "mask_bytes": npad // 8,
                     "view_rows_bytes": m * D * 4, "blocks": npad // 64, "blocks_with_no_admitted_row": skipped_blocks,
                     **alternate({"mask_build": lambda: part.cell_mask(mask, cache=False)})}
            res["builds"].append(entry)
            print(json.dumps(entry), flush=True)
            outside = torch.nonzero(~mask).flatten()
            for nq in QS:
                q = queries[:nq].contiguous()
                arms = {"allow": lambda: part.search(q, K, allow=cm), "view": lambda: view.search(q, K), "plain": lambda: part.search(q, K),
                        "pq_allow": lambda: quant.search(q, K, allow=cm_q), "pq_plain": lambda: quant.search(q, K)}
                assert same(arms["allow"](), arms["view"]())
                cell = {"N": n, "M": m, "selectivity": sel, "Q": nq, "list_entries_per_query": n - m}
                if 0 < n - m <= MAX_LIST:
                    csr = (torch.arange(nq + 1, dtype=torch.int64, device=DEV) * (n - m), outside.repeat(nq))

                    def pq_lists():
                        mf._lib._lib = parent
                        try:
                            return quant.search(q, K, exclude_csr=csr)
                        finally:
                            mf._lib._lib = own

                    assert same(arms["pq_allow"](), pq_lists())
                    arms["pq_lists"] = pq_lists
                else:
                    cell["pq_lists_skipped"] = "no row to exclude" if n == m else f"a list of {n - m} entries exceeds {MAX_LIST}"
                slow = big or "pq_lists" in arms and nq > 32
                cell.update(alternate(arms, iters=3 if slow else ITERS, regions=5 if slow else REGIONS))
                # the uncached view alone: every call builds the view, reads its size back and builds its cells
                cell.update(alternate({"view_build": lambda: part.search(q, K, where=mask)}, iters=2 if big else 5, regions=3, warmup=1))
                cell["mask_plus_allow_us"] = entry["mask_build"]["us"] + cell["allow"]["us"]
                cell["mask_plus_allow_faster_than_view_build"] = bool(cell["mask_plus_allow_us"] < cell["view_build"]["us"])
                cell["allow_over_plain"] = cell["allow"]["us"] / cell["plain"]["us"]
                cell["pq_allow_over_plain"] = cell["pq_allow"]["us"] / cell["pq_plain"]["us"]
                cell["view_faster"] = bool(cell["view"]["us"] + cell["allow"]["spread_us"] < cell["allow"]["us"])
                if "pq_lists" in cell:
                    cell["pq_lists_over_allow"] = cell["pq_lists"]["us"] / cell["pq_allow"]["us"]
                if sel == 1.0:       # the condition's pairs, each alone (alternate_pair); the rotation's figures stay beside them
                    for pre, a, b in (("", "allow", "plain"), ("pq_", "pq_allow", "pq_plain")):
                        cell[pre + "pair_allow"], cell[pre + "pair_plain"] = alternate_pair(arms[a], arms[b], iters=3 if slow else ITERS,
                                                                                         regions=PAIR_REGIONS)
                        cell[pre + "all_ones_excess_us"] = cell[pre + "pair_allow"]["us"] - cell[pre + "pair_plain"]["us"]
                        cell[pre + "all_ones_within_spread"] = bool(cell[pre + "all_ones_excess_us"] <= cell[pre + "pair_plain"]["spread_us"])
                        cell[pre + "all_ones_excess_in_rotation_us"] = cell[a]["us"] - cell[b]["us"]
                res["cells"].append(cell)
                print(json.dumps(cell), flush=True)
                write(out_path, res)
                del arms
            del view, outside, cm, cm_q
        del part, quant, items
        torch.cuda.empty_cache()
    write(out_path, res)


if __name__ == "__main__":
    main()
