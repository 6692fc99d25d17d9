"""What a partitioned search must return, from the oracle the exact engines are already held to, and the cases the CPU and
the GPU tests share.

The spec: ``probes = chain.topk(q, centroids, nprobe)`` (exact, lowest cell on ties); a row is allowed when its cell is probed;
the result is ``chain.topk(q, items, k, exclude = sorted(excluded or not allowed))``.  Rows compare as integers, scores as uint32
views.  Exclusion lists hold GLOBAL rows (``idx_base + row``) as the engines take them; the oracle works on local rows.
"""
from __future__ import annotations

import dataclasses
import functools
import zlib

import numpy as np

from oracle import chain

WIDTHS = (32, 64, 128, 256)


def padded(x: np.ndarray) -> np.ndarray:
    """Zero columns up to the next supported width, as ``ItemIndex`` pads rows and queries."""
    d = next(w for w in WIDTHS if x.shape[1] <= w)
    return np.ascontiguousarray(np.pad(x, ((0, 0), (0, d - x.shape[1]))), dtype=np.float32)


def probes(q, centroids, nprobe: int) -> np.ndarray:
    return chain.topk(padded(q), padded(centroids), nprobe)[1]


def not_allowed(assign: np.ndarray, probed: np.ndarray) -> list[np.ndarray]:
    """Per query, the local rows whose cell is not probed."""
    return [np.nonzero(~np.isin(assign, p[p >= 0]))[0] for p in probed]


def expected(q, items, centroids, assign, k: int, nprobe: int, exclude=None, idx_base: int = 0):
    """``(scores [Q, k] fp32, GLOBAL rows [Q, k] int64)`` with the -inf / -1 tail."""
    n = items.shape[0]
    barred = not_allowed(assign, probes(q, centroids, nprobe))
    lists = []
    for i, b in enumerate(barred):
        mine = np.asarray([] if exclude is None else exclude[i], dtype=np.int64) - idx_base
        lists.append(np.union1d(mine[(mine >= 0) & (mine < n)], b).tolist())
    s, r = chain.topk(padded(q), padded(items), k, lists)
    return s, np.where(r >= 0, r + idx_base, -1)


@dataclasses.dataclass
class Case:
    name: str
    items: np.ndarray          # [N, dim]
    centroids: np.ndarray      # [C, dim]
    assign: np.ndarray         # [N] int64
    q: np.ndarray              # [Q, dim]
    k: int
    nprobe: int
    exclude: list | None       # per query, GLOBAL rows
    idx_base: int = 0

    @property
    def sizes(self) -> np.ndarray:
        return np.bincount(self.assign, minlength=self.centroids.shape[0])

    @property
    def max_cell_blocks(self) -> int:
        return int(((self.sizes + 63) // 64).max())

    def expected(self):
        return expected(self.q, self.items, self.centroids, self.assign, self.k, self.nprobe, self.exclude, self.idx_base)


def _unit(x):
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def _lists(rng, nq: int, n: int, lengths, idx_base: int = 0):
    """Exclusion lists whose lengths cycle through ``lengths`` (capped at n), distinct global rows, not sorted."""
    return [(rng.choice(n, min(lengths[i % len(lengths)], n), replace=False) + idx_base).tolist() for i in range(nq)]


def make(name, dim, n, nq, c, nprobe, k, *, sizes=None, lengths=(0, 1, 17), idx_base=0) -> Case:
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    items = _unit(rng.standard_normal((n, dim)))
    centroids = _unit(rng.standard_normal((c, dim)))
    if sizes is None:
        assign = rng.integers(0, c, n).astype(np.int64)
    else:
        assert len(sizes) == c and sum(sizes) == n
        assign = rng.permutation(np.repeat(np.arange(c, dtype=np.int64), sizes))
    q = _unit(rng.standard_normal((nq, dim)))
    excl = None if lengths is None else _lists(rng, nq, n, lengths, idx_base)
    return Case(name, items, centroids, assign, q, k, nprobe, excl, idx_base)


def _spread(total: int, parts: int) -> list[int]:
    return [total // parts + (i < total % parts) for i in range(parts)]


@functools.lru_cache(maxsize=None)
def cases() -> dict[str, Case]:
    out: list[Case] = []
    for d in WIDTHS:                                                                   # every width, several blocks per cell
        out.append(make(f"width{d}", d, 1000, 33, 16, 3, 20))
    out.append(make("one_cell_one_row_list", 32, 33, 1, 1, 1, 1))
    out.append(make("fewer_rows_than_k", 64, 33, 70, 4, 4, 64))                         # N < k: every list ends in a tail
    out.append(make("long_lists", 128, 2500, 70, 37, 3, 20, lengths=(0, 1, 17, 1025)))
    out.append(make("all_cells_k64", 256, 2500, 1, 37, 37, 64))
    out.append(make("sliced_cells", 64, 2500, 3, 4, 3, 64, lengths=(0, 17, 1025)))           # ~10 blocks per cell: two slices each
    out.append(make("k1_many_queries", 64, 1000, 70, 16, 1, 1, lengths=None))
    out.append(make("idx_base", 64, 1000, 33, 4, 3, 20, idx_base=1000))
    out.append(make("padded_width", 48, 1000, 33, 16, 3, 20))

    # cells of 0, 1, 63, 64 and 65 rows; query 0 is the empty cell's centroid, so that cell is probed at nprobe = 3 too
    sizes = [0, 1, 63, 64, 65] + _spread(1000 - 193, 11)
    for nprobe in (3, 16):
        c = make(f"cell_sizes_nprobe{nprobe}", 64, 1000, 33, 16, nprobe, 20, sizes=sizes)
        c.q[0] = c.centroids[0]
        out.append(c)

    # one cell of 2,560 rows (40 blocks), alone under the probe of a single query: the plan slices it
    c = make("big_cell", 128, 2620, 1, 4, 1, 20, sizes=[2560, 10, 20, 30], lengths=(17,))
    c.q[0] = c.centroids[0]
    out.append(c)

    # all but three rows of the probed cells excluded: three entries, then the tail
    c = make("all_but_three", 64, 1000, 3, 4, 1, 20, lengths=None)
    c.exclude = []
    for p in probes(c.q, c.centroids, 1):
        inside = np.nonzero(np.isin(c.assign, p))[0]
        c.exclude.append(inside[3:].tolist())
    out.append(c)

    # 300 identical rows dealt over the four cells, the query is that row: equal scores across cells, lowest row first
    c = make("ties_across_cells", 64, 1000, 2, 4, 3, 64, lengths=(0, 5))
    c.items[:300] = c.items[0]
    c.assign[:300] = np.arange(300) % 4
    c.q[0] = c.items[0]
    out.append(c)

    # two identical centroids: the lower cell is the one probed
    c = make("twin_centroids", 64, 1000, 33, 4, 1, 20)
    c.centroids[2] = c.centroids[1]
    c.q[:8] = _unit(c.centroids[1] + 0.05 * c.q[:8])
    out.append(c)

    c = make("zero_query", 32, 1000, 3, 16, 3, 20)                                        # every score 0: rows in order, cells 0, 1, 2
    c.q[1] = 0.0
    out.append(c)
    return {c.name: c for c in out}


def plan_slices(nq: int, nprobe: int, k: int, max_cell_blocks: int, merge_keys: int = 8192) -> int:
    """The documented rule of ``mf_ivf_plan`` and ``mf_pq_plan`` (include/mf_hip.h): about 1,024 workgroups, a block per wave in
    a slice of the largest cell at least, ``nprobe * S * k`` within the merge's keys (8,192 for ``mf_topk_merge_packed``),
    ``1 <= S <= max_cell_blocks``."""
    want = -(-1024 // (nq * nprobe))
    s = min(want, max(1, max_cell_blocks // 4), merge_keys // (nprobe * k), max_cell_blocks)
    return max(1, s)
