"""The bf16 retrieval prefilter (csrc/mf_topk_bf3.hip) at the plan geometries its first tests never met: the case table, the
plan read through ``mf_topk_bf3_plan``, the cell every case must land in, and the cases' data.  Host only: read by
tests/test_topk_bf3_plan_cpu.py (cells, plan invariants, what the planted rows do -- by the CPU oracle) and by
tests/test_gpu_topk_prefilter_geometry.py (the searches)."""
from __future__ import annotations

import ctypes
from dataclasses import dataclass, field

import numpy as np
import torch

PLAN_FIELDS = ("NT", "nblk", "XT", "xw", "Qp", "gy", "bs", "nvb_seed", "bpc_seed", "nwg_seed", "bpc", "nwg", "nvals", "windows")
WAVES, BLOCK_ROWS, WINDOW_ROWS, CAND = 8, 128, 65_536, 512     # BF3_WAVES, 32 * BF3_BLOCK, 32 * BF3_PREP_W, BF3_CAND


def plan(lib, nq, n, d):
    out = (ctypes.c_int64 * 16)()
    assert lib.mf_topk_bf3_plan(nq, n, d, out) == 0, (nq, n, d)
    assert out[14] == 0 and out[15] == 0
    return dict(zip(PLAN_FIELDS, list(out)))


@dataclass(frozen=True)
class Case:
    nq: int
    n: int
    d: int
    k: int
    lists: bool
    idx_base: int
    cell: dict                                   # plan field -> exact value, or (">=", bound)
    tail_rows: int | None = None                 # real rows of the last 32-row tile, where the case is about them


# (Q, N, d, k, lists, idx_base) and the cell the name claims.  The cells follow from bf3_plan: they are asserted through the
# export, so a change of the plan that moves a shape out of its cell fails here first -- move the shape, not the cell.
CASES = {
    "two_query_blocks_long_catalog": Case(1030, 70_001, 64, 64, True, 0, dict(
        gy=2, XT=4, xw=8, bs=2, bpc_seed=(">=", 3), bpc=(">=", 5), windows=2), tail_rows=17),
    "d256_two_query_blocks": Case(520, 66_000, 256, 10, True, 11, dict(
        gy=2, XT=2, xw=8, bs=2, bpc_seed=(">=", 3), bpc=(">=", 3), windows=2, NT=2063)),          # NT % 4 = 3: a partial last block
    "seams": Case(260, 70_001, 128, 20, True, 0, dict(gy=1, XT=4, xw=8, bs=2, bpc_seed=2, bpc=3, windows=2), tail_rows=17),
    "one_row_tail_at_the_window_seam": Case(257, 65_537, 128, 20, True, 0, dict(
        gy=1, XT=4, bs=2, bpc_seed=(">=", 2), bpc=(">=", 3), windows=2, NT=2049), tail_rows=1),
    "few_queries_very_long_catalog": Case(40, 140_000, 64, 20, True, 0, dict(
        gy=1, XT=1, xw=2, bs=2, bpc_seed=(">=", 2), bpc=(">=", 5), windows=3, nvals=(">=", 4097))),   # nine trips of the bound's loop
    "three_query_blocks_short_catalog": Case(2100, 4_100, 64, 1, False, 0, dict(
        gy=3, XT=4, xw=8, Qp=3072, bs=1, bpc_seed=1, bpc=1, windows=1)),
    "two_query_blocks_mid_catalog": Case(1100, 33_000, 128, 20, True, 0, dict(
        gy=2, XT=4, xw=8, bs=2, bpc_seed=(">=", 2), bpc=3, windows=1)),
}

# the twelve (d, XT, lists) instantiations of the scan kernels: XT = 1 at Q = 70, XT = 4 (2 at d = 256) at Q = 300
INSTANTIATIONS = [(d, nq, lists) for d in (64, 128, 256) for nq in (70, 300) for lists in (False, True)]
NEVER_LAUNCHED_BEFORE = {(64, 300, False), (128, 300, True), (256, 300, False)}


def instantiation(d, nq, lists):
    return Case(nq, 2_300, d, 20, lists, 0, dict(XT=1 if nq == 70 else (2 if d == 256 else 4), gy=1, bs=1, bpc=1, windows=1))


def check_cell(case: Case, p: dict):
    for name, want in case.cell.items():
        if isinstance(want, tuple):
            assert p[name] >= want[1], (name, p[name], want, p)
        else:
            assert p[name] == want, (name, p[name], want, p)
    if case.tail_rows is not None:
        assert case.n - 32 * (p["NT"] - 1) == case.tail_rows, (case.n, p)


@dataclass
class Data:
    q: torch.Tensor
    items: torch.Tensor
    excl: list | None                            # per query: sorted GLOBAL ids (repeats and ids outside the catalog included)
    special: dict = field(default_factory=dict)  # name -> query: the specially constructed ones
    notes: dict = field(default_factory=dict)    # what the seams case planted where

    def local_lists(self, case: Case, sel):
        """The lists of the queries ``sel`` as the oracle takes them: distinct local rows inside the catalog."""
        if self.excl is None:
            return None
        b, n = case.idx_base, case.n
        return [sorted({y - b for y in self.excl[x] if b <= y < b + n}) for x in sel]


def _unit(n, d, gen):
    return torch.nn.functional.normalize(torch.randn(n, d, generator=gen), dim=-1)


DUP_ROWS = lambda n: (3, n // 2 + 1)             # noqa: E731  (the exact duplicate pair: far apart, other workgroups of the scan)


def build(name: str, case: Case, p: dict) -> Data:
    """Unit rows and queries from a seeded generator; an exact duplicate pair that IS the top of query 6 (the lower row first);
    with lists: 0 .. 300 random sorted global ids per query on both sides of [idx_base, idx_base + N), query 7's list with ids
    below and beyond the catalog and a repeated id, the aligned groups 8 .. 11 = [], L, [], [] and 12 .. 15 = [], [], [], L
    (the prep workgroup deals its four lists' entries by offset comparison)."""
    nq, n, d, base = case.nq, case.n, case.d, case.idx_base
    seed = sum(map(ord, name)) + d + nq
    g = torch.Generator().manual_seed(seed)
    rng = np.random.default_rng(seed)
    q, items = _unit(nq, d, g), _unit(n, d, g)
    a, b = DUP_ROWS(n)
    items[b] = items[a]
    q[6] = items[a]
    data = Data(q, items, None, {"duplicate_pair": 6})
    taken = {a, b}                               # rows with a part to play: no plant may land on another

    def plant(x, rows, scales, noise=0.001):
        rows = [int(r) for r in rows]
        assert not taken & set(rows) and all(0 <= r < n for r in rows), (x, rows)
        taken.update(rows)
        idx = torch.tensor(rows)
        items[idx] = q[x] * torch.as_tensor(scales, dtype=torch.float32)[:, None] + noise * torch.randn(len(rows), d, generator=g)

    if case.lists:
        excl = []
        for _ in range(nq):
            ids = rng.integers(base - 40, base + n + 40, size=int(rng.integers(0, 301)))
            excl.append(sorted(ids.tolist()))
        excl[6] = [y for y in excl[6] if y - base not in (a, b)]
        some = sorted(rng.integers(base, base + n, size=40).tolist())
        excl[7] = sorted([base - 9, base - 1, base + n, base + n + 5] + some + some[:3])          # outside; three ids twice
        long_list = sorted(rng.integers(base, base + n, size=200).tolist())
        for x in range(8, 16):
            excl[x] = list(long_list) if x in (9, 15) else []
        data.excl = excl
        data.special.update(outside_and_repeated=7, empty_before_a_list=8, list_second_of_four=9, empty_before_the_last=14,
                            list_last_of_four=15)

    if name == "one_row_tail_at_the_window_seam":
        last = n - 1                             # row 65,536: the only real row of the tail tile, the only word of window 2
        assert last == WINDOW_ROWS
        taken.add(last)
        items[last] = torch.nn.functional.normalize(q[0] + q[1], dim=0)      # the best row of both queries (score ~0.7)
        data.excl[0] = [y for y in data.excl[0] if y != base + last]
        data.excl[1] = sorted(set(data.excl[1]) | {base + last})
        data.special.update(tail_row_best=0, tail_row_best_and_excluded=1)

    if name == "seams":
        k, bpc = case.k, p["bpc"]
        # query 0: its 24 best rows in odd 128-row blocks -- the seed scan (every second block) never meets them
        odd = [1, 3, 301, p["nblk"] - 2]
        assert all(blk % 2 == 1 and blk < p["nblk"] for blk in odd) and p["bs"] == 2
        rows0 = [blk * BLOCK_ROWS + 21 * j + 5 for blk in odd for j in range(6)]
        plant(0, rows0, np.linspace(0.6, 1.0, len(rows0)))
        data.excl[0] = [y for y in data.excl[0] if y not in set(rows0)]
        # query 1: across the boundary of two chunks of the full scan (its last and the next one's first tile)
        edge = 51 * bpc * BLOCK_ROWS
        rows1 = list(range(edge - 12, edge + 12))
        plant(1, rows1, 1.0 - 0.012 * np.abs(np.arange(-12, 12) + 0.5))
        data.excl[1] = [y for y in data.excl[1] if y not in set(rows1)]
        # query 2: across the seam of the prep windows, the two rows at the seam (its best) excluded
        rows2 = list(range(WINDOW_ROWS - 6, WINDOW_ROWS + 6))
        plant(2, rows2, 1.0 - 0.02 * np.abs(np.arange(-6, 6) + 0.5))
        data.excl[2] = sorted(set(y for y in data.excl[2] if y not in set(rows2)) | {WINDOW_ROWS - 1, WINDOW_ROWS})
        # query 3: the last three rows (the tail tile), the very last -- its best -- excluded
        plant(3, [n - 3, n - 2, n - 1], [0.8, 0.9, 1.0])
        data.excl[3] = sorted(set(y for y in data.excl[3] if y < n - 3) | {n - 1})
        # query 4: zero -- every row ties, the lowest rows that are not excluded win; exclusion words of both windows are read
        q[4] = 0.0
        data.excl[4] = [0, 2, 7, 7, WINDOW_ROWS, WINDOW_ROWS + 1, WINDOW_ROWS + 4, n - 2]
        # query 5: 700 exact copies of one row (more than BF3_CAND survive the lists: the exact path), ten below the window seam
        # and 690 beyond it; five of the first ten and every third of the next sixty are excluded, so the 20 winners are decided by
        # the second window's words
        low = [100 + 97 * i for i in range(10)]
        high = [WINDOW_ROWS + 64 + 6 * i for i in range(690)]
        assert not taken & set(low + high) and high[-1] < n - 3
        taken.update(low + high)
        src = low[0]
        items[torch.tensor(low + high)] = items[src].clone()
        q[5] = items[src]
        gone = low[::2] + high[:60:3]
        data.excl[5] = sorted(gone)
        assert len(low + high) - len(gone) > CAND
        data.special.update(best_rows_in_unsampled_blocks=0, best_rows_across_two_chunks=1, best_rows_across_the_window_seam=2,
                            best_rows_in_the_tail_tile=3, zero_query=4, more_copies_than_candidates=5)
        data.notes.update(rows0=rows0, rows1=rows1, rows2=rows2, edge=edge, low=low, high=high, gone=gone)

    if case.lists:
        ex = data.excl
        assert all(e == sorted(e) for e in ex) and max(map(len, ex)) >= 100
        assert any(e and e[0] < base for e in ex) and any(e and e[-1] >= base + n for e in ex)
        assert any(len(set(e)) < len(e) for e in ex)
        assert [bool(ex[x]) for x in range(8, 16)] == [False, True, False, False, False, False, False, True]
    return data


def oracle_sample(case: Case, p: dict, special: dict, cap: int = 32):
    """The queries checked against the CPU oracle: the first and the last real query of every query workgroup, one query of
    every query-tile set of a workgroup (walking through the set's XT tiles), the specially constructed ones, seeded random
    ones up to ``cap``."""
    nq = case.nq
    per_set = 32 * p["XT"]
    per_wg = per_set * p["xw"]
    assert per_wg * p["gy"] == p["Qp"]
    sel = []
    for wg in range(p["gy"]):
        first, last = wg * per_wg, min(nq, (wg + 1) * per_wg) - 1
        assert first <= last, (wg, p)                                  # (no workgroup of padding queries only)
        sel += [first, last]
        for s in range(p["xw"]):
            if first + s * per_set <= last:                           # (a ragged last workgroup: the sets that hold real queries)
                sel.append(min(last, first + s * per_set + (s % p["XT"]) * 32 + (7 * s + 5) % 32))
    structural = sorted(set(sel) | set(special.values()))
    assert len(structural) <= cap, (len(structural), cap)
    rng = np.random.default_rng(nq)
    rest = [x for x in rng.permutation(nq).tolist() if x not in set(structural)]
    return sorted(structural + rest[: cap - len(structural)])
