"""Time the sparse row updates alone on the bench's id distributions (Zipf item ids + uniform negatives; log-normal users).

    python tools/lab/update_probe.py                                   # mf_update_adam, the four lists (as before)
    python tools/lab/update_probe.py --optimizer adagrad               # mf_update_adagrad
    python tools/lab/update_probe.py --optimizer all --pair --regions 7 --other-lib parent/libmf_hip.so --json out.json
    MF_HIP_LIB=<a -DMF_PROBE build> python tools/lab/update_probe.py --stamps --json stamps.json      # the phases of one workgroup

``--optimizer``: adam | sgd | adagrad | all.  ``--pair``: also the two-table launch (mf_update_pair / mf_update_pair_adagrad) on
the C3 lists (8,192 user ids + 16,384 item ids, d = 128).  ``--other-lib``: a second build of the library (for instance the
parent commit's) whose SGD and Adam are timed on the same lists, its regions alternating with this build's.  Every figure is
device time per call: HIP events around ``--calls`` back-to-back calls, after a warm-up; the median of ``--regions`` regions
with their minimum and maximum.  ``--multi``: also a list of 131,072 ids (the multi-launch path).

``--stamps`` (a library built with -DMF_PROBE): instead of timing, the phase stamps of single Adam launches on the Zipf and the
uniform item list -- for the workgroup with the most keys and for one with the median number, the microseconds from the
workgroup's start to the end of the scan, the sort, pass 0 (thread 0's wave), the barrier behind it and pass 1 (every wave);
the median over ``--regions`` launches.
"""
import argparse
import ctypes
import importlib
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

mf = importlib.import_module("matrix-factorization-torch_amd")
import bench  # noqa: E402

KINDS = ("sgd", "adagrad", "adam")


def load_other(path):
    """A second library, bound with this build's signatures for the exports it has."""
    handle = ctypes.CDLL(os.path.abspath(path))
    for name, (res, args) in mf._lib.SIGNATURES.items():
        if hasattr(handle, name):
            fn = getattr(handle, name)
            fn.restype, fn.argtypes = res, args
    return handle


class Table:
    def __init__(self, rows, d, dev):
        self.rows, self.d = rows, d
        self.w = torch.randn(rows, d, device=dev)
        self.m, self.v = torch.zeros_like(self.w), torch.zeros_like(self.w)
        self.s = torch.zeros(rows, device=dev)

    def state(self, kind):
        return {"sgd": (), "adagrad": (self.s,), "adam": (self.m, self.v)}[kind]


# lr 1e-4, no weight decay, otherwise the optimisers' defaults.  The calls go through optim.row_update / row_update_pair, like a
# step of the optimisers: the workspace comes from torch's caching allocator at every call
HYPER = {kind: mf.distributed.optimizer_hyper(kind, 1e-4, weight_decay=0.0) for kind in KINDS}


def single_call(lib, kind, t, ids, grad):
    return lambda step: mf.optim.row_update(kind, t.w, t.state(kind), ids, grad, False, HYPER[kind], step, lib=lib)


def pair_call(lib, kind, ta, ia, ga, tb, ib, gb):
    def call(step):
        if not mf.optim.row_update_pair(kind, (ta.w, ta.state(kind), ia, ga, False), (tb.w, tb.state(kind), ib, gb, False), HYPER[kind],
                                        step, lib=lib):
            raise SystemExit("the two-table launch was refused (MF_UPDATE_PAIR=0?)")
    return call


def region(calls_of, n_calls, step0):
    """Device microseconds per call of one region: ``calls_of[i % len]`` in turn."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(n_calls):
        calls_of[i % len(calls_of)](step0 + i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n_calls


PHASES = ("scan", "sort", "pass0", "barrier", "pass1")


def stamps(lib, call, n_blocks, reps):
    """Phase durations (us) of the workgroup with the largest m and of one with the median m, medians over `reps` launches."""
    fn = lib.mf_probe_update_stamps
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    buf, khz = (ctypes.c_uint64 * (8 * n_blocks))(), ctypes.c_int(0)
    rows = {"largest": [], "median": []}
    for r in range(reps):
        call(100 + r)
        mf._lib.check(fn(buf, n_blocks, ctypes.byref(khz)))
        wg = [buf[8 * b: 8 * b + 8] for b in range(n_blocks)]
        order = sorted(range(n_blocks), key=lambda b: wg[b][6])
        for which, b in (("largest", order[-1]), ("median", order[n_blocks // 2])):
            t = wg[b]
            ends = [t[i] if t[i] else t[i - 1] for i in range(1, 6)]             # (no second pass: stamps 4 and 5 stay 0)
            ends = [max(e, t[0]) for e in ends]
            prev, cut = t[0], {}
            for name, e in zip(PHASES, ends):
                e = max(e, prev)
                cut[name] = (e - prev) * 1e3 / khz.value
                prev = e
            cut["total"] = (prev - t[0]) * 1e3 / khz.value
            cut["m"] = int(t[6])
            rows[which].append(cut)
    return {which: {k: round(statistics.median(x[k] for x in xs), 2) for k in (*PHASES, "total", "m")} for which, xs in rows.items()}


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--optimizer", default="adam", choices=(*KINDS, "all"))
    ap.add_argument("--pair", action="store_true")
    ap.add_argument("--other-lib", default=None)
    ap.add_argument("--regions", type=int, default=1)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--json", default=None)
    ap.add_argument("--multi", action="store_true")
    ap.add_argument("--stamps", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    d = 128
    libs = {"this": mf._lib.lib()}
    if args.other_lib:
        libs["other"] = load_other(args.other_lib)
    kinds = KINDS if args.optimizer == "all" else (args.optimizer,)
    batches, _ = bench.make_batches(4, 8192, seed=1000, device=dev)
    lists = {"user 8192 (log-normal)": (bench.NUM_USERS, [b["user"] for b in batches]),
             "item 16384 (zipf + uniform)": (bench.NUM_ITEMS, [b["item"] for b in batches]),
             "item 16384 uniform": (bench.NUM_ITEMS, [torch.randint(1, bench.NUM_ITEMS, (16384,), device=dev) for _ in range(4)]),
             "32 ids": (bench.NUM_ITEMS, [torch.randint(1, bench.NUM_ITEMS, (32,), device=dev) for _ in range(4)])}
    if args.multi:
        lists["item 131072 uniform (multi-launch)"] = (bench.NUM_ITEMS, [torch.randint(1, bench.NUM_ITEMS, (131072,), device=dev) for _ in range(4)])
    if args.stamps:
        if not hasattr(libs["this"], "mf_probe_update_stamps"):
            raise SystemExit("--stamps needs a library built with -DMF_PROBE (MF_HIP_LIB=...)")
        out = {"d": d, "launches": max(args.regions, 5), "device": torch.cuda.get_device_name(0), "unit": "us", "lists": {}}
        t = Table(bench.NUM_ITEMS, d, dev)
        for name in ("item 16384 (zipf + uniform)", "item 16384 uniform"):
            ids = lists[name][1][0]
            n = ids.numel()
            grad = torch.randn(n, d, device=dev)
            call = single_call(libs["this"], "adam", t, ids, grad)
            for i in range(10):
                call(i + 1)
            res = out["lists"][name] = stamps(libs["this"], call, 256, max(args.regions, 5))
            for which, row in res.items():
                print(f"{name:30s} {which:8s} m {row['m']:5d}: " + "  ".join(f"{k} {row[k]:6.2f}" for k in (*PHASES, "total")))
        if args.json:
            os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
            with open(args.json, "w") as f:
                json.dump(out, f, indent=1)
        return
    tables = {rows: Table(rows, d, dev) for rows in {r for r, _ in lists.values()}}
    # what to time: name -> {(lib, kind): [one closure per id list]}
    todo = {}
    for name, (rows, ids) in lists.items():
        n = ids[0].numel()
        grad = torch.randn(n, d, device=dev)
        uniq = sum(int(torch.unique(i).numel()) for i in ids) / len(ids)
        top = max(int(torch.bincount(i).max()) for i in ids)
        entry = todo[name] = {"n": n, "unique": uniq, "largest_run": top, "calls": {}}
        for lname, lib in libs.items():
            for kind in kinds:
                if hasattr(lib, f"mf_update_{kind}"):
                    entry["calls"][(lname, kind)] = [single_call(lib, kind, tables[rows], i, grad) for i in ids]
    if args.pair:
        users, items = lists["user 8192 (log-normal)"][1], lists["item 16384 (zipf + uniform)"][1]
        ta, tb = tables[bench.NUM_USERS], tables[bench.NUM_ITEMS]
        ga, gb = torch.randn(8192, d, device=dev), torch.randn(16384, d, device=dev)
        entry = todo["pair: user 8192 + item 16384"] = {"n": 8192 + 16384, "calls": {}}
        for lname, lib in libs.items():
            for kind in kinds:
                if hasattr(lib, "mf_update_pair_adagrad" if kind == "adagrad" else "mf_update_pair"):
                    entry["calls"][(lname, kind)] = [pair_call(lib, kind, ta, ia, ga, tb, ib, gb) for ia, ib in zip(users, items)]
    out = {"d": d, "regions": args.regions, "calls_per_region": args.calls, "device": torch.cuda.get_device_name(0), "lists": {}}
    for name, entry in todo.items():
        for calls_of in entry["calls"].values():                       # warm-up: every (library, kind) of this list
            for i in range(20):
                calls_of[i % len(calls_of)](i + 1)
        torch.cuda.synchronize()
        times = {key: [] for key in entry["calls"]}
        for r in range(args.regions):                                   # the (library, kind) pairs alternate inside every round
            for key, calls_of in entry["calls"].items():
                times[key].append(region(calls_of, args.calls, 21 + r * args.calls))
        res = out["lists"][name] = {k: v for k, v in entry.items() if k != "calls"}
        for (lname, kind), us in times.items():
            med = statistics.median(us)
            res[f"{lname}:{kind}"] = {"median_us": round(med, 2), "min_us": round(min(us), 2), "max_us": round(max(us), 2)}
            extra = ""
            if "unique" in entry:       # bytes the update must move: the gradient rows once, each touched row (and its state) in and out
                per_row = {"sgd": 2 * d * 4, "adagrad": 2 * d * 4 + 8, "adam": 6 * d * 4}[kind]
                moved = (entry["n"] * d * 4 + entry["unique"] * per_row) / 1e9
                extra = f"  ({moved / (med * 1e-6):7.0f} GB/s algorithmic)"
                res[f"{lname}:{kind}"]["algorithmic_GBps"] = round(moved / (med * 1e-6), 1)
            print(f"{name:30s} {lname:5s} {kind:8s} n {entry['n']:6d}: {med:7.1f} us / call  [{min(us):.1f} .. {max(us):.1f}]{extra}")
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
