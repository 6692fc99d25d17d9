"""What the deep cell scan (csrc/mf_ivf_deep.hip, ``PartitionedIndex.search(path="cells_deep")``) is held to beyond
tests/_ivf_spec.py, shared by tests/test_ivf_deep_cpu.py, tests/test_gpu_ivf_deep.py and tests/test_gpu_ivf_deep_settles.py: the
buffer's constants read out of the source, the buffer's bookkeeping ("kept / waiting / threshold", with admission) restated in a
few lines, the one-cell catalog whose scan settles several times, the deep case set, and the catalog whose long cell settles
under masks, exclusion lists and ties.  The result spec itself is ``_ivf_spec.expected`` -- it takes any k."""
from __future__ import annotations

import functools
import pathlib
import re
import zlib

import numpy as np

from oracle import chain
from tests import _ivf_spec as ivf

ROOT = pathlib.Path(__file__).resolve().parents[1]
SOURCE = ROOT / "matrix-factorization-torch_amd" / "csrc" / "mf_ivf_deep.hip"
MERGE_KEYS = 16384          # MF_TOPK_MERGE_DEEP_MAX_KEYS: G * k keys of a query in the deep merge
MAX_K = 1024                # MF_TOPK_DEEP_MAX_K
DEPTHS = (1, 64, 65, 128, 129, 256, 257, 512, 513, 1000, 1024)


@functools.lru_cache(maxsize=None)
def constants() -> dict[str, int]:
    """``static constexpr int IVFD_* = <number>;`` of the unit's header part (IVFD_PASS is written as a product there)."""
    text = SOURCE.read_text()
    out = {name: int(value) for name, value in re.findall(r"static constexpr int (IVFD_\w+) = (\d+);", text)}
    assert "static constexpr int IVFD_PASS = 64 * MF_CELLS_NW;" in text
    out["IVFD_PASS"] = 256
    return out


def kept(k: int) -> int:
    """``ivfd_kept``: the power of two >= k, ``IVFD_KP_MIN`` at least."""
    kp = constants()["IVFD_KP_MIN"]
    while kp < k:
        kp *= 2
    return kp


def capacity(kp: int) -> int:
    """``ivfd_capacity``: the keys of the buffer a scan with kept part ``kp`` uses."""
    return max(4 * kp, constants()["IVFD_BUF_MIN"])


def room_of(k: int) -> int:
    """Waiting keys behind which another pass still fits at depth k: 1664 / 1536 / 1280 / 2816 in the four kept classes."""
    kp = kept(k)
    return capacity(kp) - kp - constants()["IVFD_PASS"]


def walk(scores: np.ndarray, k: int, admitted: np.ndarray | None = None, rows: np.ndarray | None = None, room: int | None = None) -> dict:
    """The buffer of one workgroup over the rows of its slice in cell order (``scores``: one per position): passes of
    ``IVFD_PASS`` positions; a row's key waits when it beats the bound and is admitted; when more than ``capacity - kept -
    IVFD_PASS`` keys wait, a settle keeps the k best and the bound becomes the k-th of them (0 while fewer are held).
    ``admitted``: a bool per position -- a row that the mask clears or the exclusion list names is not admitted, and never
    waits.  ``rows``: the global row per position; the key is ``(score, -row)``, so equal scores break by row.  Without the
    two, every row is admitted, the row is the position, and ``settles`` holds per settle ``(keys waiting, the bound was live
    before it)``; with either, ``(keys waiting, the bound was live, begun inside the loop, sort length)`` -- inside the loop:
    more than ``room`` keys waited after a pass; the sort length: the power of two >= kept + waiting, ``IVFD_SORT_MIN`` at
    least -- and ``rows`` beside ``best``.  ``best``: the positions the walk keeps, best first.  ``room``: another class's
    threshold, to show that a case tells the classes apart (the buffer's capacity is then not asserted)."""
    c = constants()
    kp = kept(k)
    plain = admitted is None and rows is None
    scores = np.asarray(scores, dtype=np.float32)
    n = scores.size
    admitted = np.ones(n, dtype=bool) if admitted is None else np.asarray(admitted, dtype=bool)
    rows = np.arange(n, dtype=np.int64) if rows is None else np.asarray(rows, dtype=np.int64)
    assert admitted.shape == rows.shape == (n,)
    fits = room is None
    room = room_of(k) if room is None else room
    held: list[tuple[float, int, int]] = []                  # (score, -row, position): the larger tuple is the better key
    waiting: list[tuple[float, int, int]] = []
    bound = None
    settles = []

    def settle(inside):
        nonlocal held, waiting, bound
        length = c["IVFD_SORT_MIN"]
        while length < kp + len(waiting):
            length *= 2
        settles.append((len(waiting), bound is not None) if plain else (len(waiting), bound is not None, inside, length))
        assert not fits or kp + len(waiting) <= capacity(kp) <= c["IVFD_BUF"]
        held = sorted(held + waiting, reverse=True)[:k]
        waiting = []
        bound = held[k - 1] if len(held) >= k else None

    for p0 in range(0, n, c["IVFD_PASS"]):
        p1 = min(p0 + c["IVFD_PASS"], n)
        enters = admitted[p0:p1].copy()
        if bound is not None:
            s, r = scores[p0:p1], rows[p0:p1]
            enters &= (s > np.float32(bound[0])) | ((s == np.float32(bound[0])) & (r < -bound[1]))
        waiting += [(float(scores[p]), -int(rows[p]), int(p)) for p in p0 + np.flatnonzero(enters)]
        if len(waiting) > room:
            settle(True)
    if waiting:
        settle(False)
    out = {"settles": settles, "best": [p for _, _, p in held]}
    if not plain:
        out["rows"] = [-r for _, r, _ in held]
    return out


# ---------------------------------------------------------------------------------------- the cell of several settles ----
SETTLE_DIM = 32
SETTLE_ORDERS = ("ascending", "descending", "shuffled")


def settle_rows() -> int:
    """Rows of the one-cell catalog: three times the buffer's capacity and a ragged rest (a last block of 40 rows)."""
    return 3 * constants()["IVFD_BUF"] + 1000


def settle_scores(order: str) -> np.ndarray:
    """Distinct fp32 scores in (0, 1] along the cell order.  The catalog's row i is ``scores[i] * e0`` and the query ``e0``, so
    the chain's score of row i is ``fma(scores[i], 1, 0)`` and then sums of zeros: ``scores[i]`` to the bit."""
    n = settle_rows()
    up = (np.arange(1, n + 1, dtype=np.float64) / n).astype(np.float32)
    assert np.unique(up).size == n
    if order == "ascending":
        return up
    if order == "descending":
        return up[::-1].copy()
    return up[np.random.default_rng(7).permutation(n)]


def top_of(scores: np.ndarray, lo: int, hi: int, k: int) -> np.ndarray:
    """numpy's top-k of rows ``[lo, hi)``: score descending, row ascending; the rows, at most k."""
    rows = np.arange(lo, hi)
    order = np.lexsort((rows, -scores[lo:hi].astype(np.float64)))
    return rows[order[:k]]


# ------------------------------------------------------------------------------------------------------ the case set ----
@functools.lru_cache(maxsize=None)
def cases() -> dict[str, ivf.Case]:
    out = [
        ivf.make("deep_w32_k65", 32, 1000, 33, 16, 3, 65),
        ivf.make("deep_w48_k128", 48, 1000, 33, 16, 8, 128),                            # a padded width
        ivf.make("deep_w64_k129", 64, 2500, 70, 37, 3, 129, lengths=(0, 1, 17, 1025)),
        ivf.make("deep_w128_k256_all_cells", 128, 2500, 1, 37, 37, 256),
        ivf.make("deep_w256_k257_all_cells", 256, 1000, 33, 16, 16, 257),
        ivf.make("deep_k512", 64, 5000, 3, 16, 8, 512),
        ivf.make("deep_k513_all_cells", 32, 5000, 33, 16, 16, 513),
        ivf.make("deep_k1000_tail", 64, 2500, 3, 4, 1, 1000),                          # about 610 rows under the probe: a tail
        ivf.make("deep_k1024", 128, 5000, 1, 8, 8, 1024, lengths=(1025,)),
        ivf.make("deep_k1", 64, 1000, 70, 16, 1, 1, lengths=None),
        ivf.make("deep_k64_fewer_rows", 64, 33, 70, 4, 4, 64),
        ivf.make("deep_idx_base", 64, 1000, 33, 4, 3, 100, idx_base=1000),
        ivf.make("deep_nprobe16_of_37", 64, 2500, 33, 37, 16, 65),
    ]
    sizes = [0, 1, 63, 64, 65] + ivf._spread(1000 - 193, 11)
    for nprobe in (3, 16):                     # query 0 is the empty cell's centroid: that cell is probed at nprobe = 3 too
        c = ivf.make(f"deep_cell_sizes_nprobe{nprobe}", 64, 1000, 33, 16, nprobe, 100, sizes=sizes)
        c.q[0] = c.centroids[0]
        out.append(c)
    c = ivf.make("deep_all_but_three", 64, 1000, 3, 4, 1, 100, lengths=None)
    c.exclude = []
    for p in ivf.probes(c.q, c.centroids, 1):
        c.exclude.append(np.nonzero(np.isin(c.assign, p))[0][3:].tolist())
    out.append(c)
    # 1,100 identical rows dealt over four cells of 625 rows (ten blocks: two slices each), the query is that row
    c = ivf.make("deep_ties_k1024", 64, 2500, 2, 4, 4, 1024, sizes=[625] * 4, lengths=(0, 5))
    c.items[:1100] = c.items[0]
    c.assign[:1100] = np.arange(1100) % 4
    c.q[0] = c.items[0]
    out.append(c)
    c = ivf.make("deep_zero_query", 32, 1000, 3, 16, 3, 100)                            # every score 0: rows in order, cells 0, 1, 2
    c.q[1] = 0.0
    out.append(c)
    return {c.name: c for c in out}


# ------------------------------------------------------------- the long cell under masks, lists and ties ----
# tests/test_gpu_ivf_deep_settles.py: a catalog whose long cell fills the buffer again and again with real dot products, the
# masks over that cell's POSITIONS, the exclusion lists, and the cell of identical rows behind a shuffled ``row_of``.
SETTLE_DEPTHS = (100, 200, 500, 1000)        # one per kept class 128 / 256 / 512 / 1024
SETTLE_BASE = 30
SETTLE_CELL = 1
SETTLE_FIRST_BLOCK = 3                       # 150 rows lie ahead of the long cell: its first mask word


def settle_sizes() -> tuple[int, int, int]:
    return 150, settle_rows(), 70


@functools.lru_cache(maxsize=None)
def settle_catalog(d: int) -> ivf.Case:
    """Three cells of 150, ``settle_rows()`` and 70 random unit rows of width ``d``, dealt to the cells by a seeded permutation
    (a row is not its position), ``idx_base = 30``.  Centroid 1 is a unit vector c; the long cell's vectors are laid into its
    rows so that the chain score with query 0 ascends along the cell order (the index keeps a cell in ascending row order).
    Queries: c (every pass beats the bound), -c (nothing does after the first k; the chain's score of -c is the negated score
    to the bit) and a random unit vector pulled towards c (a shuffled order).  -c probes another cell: an export-level test gives
    the probes itself, a search leaves query 1 to the short cell it probes.  Read only."""
    sizes = settle_sizes()
    n = sum(sizes)
    rng = np.random.default_rng(4000 + d)
    items = ivf._unit(rng.standard_normal((n, d)))
    centroids = ivf._unit(rng.standard_normal((len(sizes), d)))
    assign = rng.permutation(np.repeat(np.arange(len(sizes), dtype=np.int64), sizes))
    c = centroids[SETTLE_CELL]
    q = np.stack([c, -c, ivf._unit(0.5 * c[None] + ivf._unit(rng.standard_normal((1, d))))[0]]).astype(np.float32)
    inside = np.flatnonzero(assign == SETTLE_CELL)
    vectors = items[inside]
    items[inside] = vectors[np.argsort(chain.scores(q[:1], vectors)[0], kind="stable")]
    for a in (items, centroids, assign, q):
        a.setflags(write=False)
    return ivf.Case(f"settle_{d}", items, centroids, assign, q, SETTLE_DEPTHS[0], 1, None, SETTLE_BASE)


@functools.lru_cache(maxsize=None)
def long_rows(d: int) -> np.ndarray:
    """The local row at every position of the long cell, ascending."""
    return np.flatnonzero(settle_catalog(d).assign == SETTLE_CELL)


@functools.lru_cache(maxsize=None)
def long_scores(d: int) -> np.ndarray:
    """``[3, settle_rows()]`` fp32: the chain score of every query with the row at every position of the long cell."""
    c = settle_catalog(d)
    out = chain.scores(c.q, c.items[long_rows(d)])
    out.setflags(write=False)
    return out


def _whole_blocks(n: int, keep) -> np.ndarray:
    return np.repeat([bool(keep(j)) for j in range(-(-n // 64))], 64)[:n]


# name -> (positions of the long cell, rng) -> bool per position; every row of the other cells is admitted
SETTLE_MASKS = {
    "all": lambda n, rng: np.ones(n, dtype=bool),
    "half": lambda n, rng: rng.random(n) < 0.5,                             # dense random
    "every other block": lambda n, rng: _whole_blocks(n, lambda j: j % 2 == 0),     # in every pass two waves skip and two append
    "one block in five": lambda n, rng: _whole_blocks(n, lambda j: j % 5 != 4),     # one block in five CLEARED: in four passes of
    #                                                          five one wave has a zero word and skips while the other three append
    "late": lambda n, rng: np.arange(n) >= 3000,                            # 46 zero words first: the bound goes live late
    "last block only": lambda n, rng: np.arange(n) >= n - n % 64,           # 40 rows: a tail at every depth
    "none": lambda n, rng: np.zeros(n, dtype=bool),
}


@functools.lru_cache(maxsize=None)
def settle_mask(name: str) -> np.ndarray:
    """The family's mask over the POSITIONS of the long cell, seeded by its name: the same at every width.  Read only."""
    out = SETTLE_MASKS[name](settle_rows(), np.random.default_rng(zlib.crc32(name.encode())))
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def settle_ok(name: str, d: int) -> np.ndarray:
    """The same mask per local ROW of the catalog of width ``d``, as ``cell_mask`` takes it.  Read only."""
    ok = np.ones(settle_catalog(d).items.shape[0], dtype=bool)
    ok[long_rows(d)] = settle_mask(name)
    ok.setflags(write=False)
    return ok


def best_first(scores: np.ndarray, rows: np.ndarray, admitted: np.ndarray, lo: int, hi: int) -> np.ndarray:
    """The admitted positions of ``[lo, hi)``, best first: score descending, row ascending."""
    at = lo + np.flatnonzero(admitted[lo:hi])
    return at[np.lexsort((rows[at], -scores[at].astype(np.float64)))]


SETTLE_LISTS = ("the best 2k", "long and scattered", "all but three")


@functools.lru_cache(maxsize=None)
def settle_lists(family: str, d: int, k: int, mask: str = "all") -> tuple[tuple[int, ...], ...]:
    """Per query an exclusion list of GLOBAL rows in no order.  ``the best 2k``: the query's 2k best rows of the long cell
    that the mask admits (a kernel that lets an excluded key move its bound returns a short list).  ``long and scattered``:
    1,025 rows of the long cell, 40 of the other cells, ``idx_base - 1`` and ``idx_base + N``.  ``all but three``: every row of
    the long cell that the mask admits but three."""
    c = settle_catalog(d)
    rows, admitted = long_rows(d), settle_mask(mask)
    n = c.items.shape[0]
    out = []
    for i in range(c.q.shape[0]):
        rng = np.random.default_rng(zlib.crc32(f"{family} {d} {k} {mask} {i}".encode()))
        if family == "the best 2k":
            mine = rows[best_first(long_scores(d)[i], rows, admitted, 0, rows.size)[: 2 * k]]
        elif family == "long and scattered":
            others = np.flatnonzero(c.assign != SETTLE_CELL)
            mine = np.concatenate([rng.choice(rows, 1025, replace=False), rng.choice(others, 40, replace=False), [-1, n]])
        else:
            assert family == "all but three"
            mine = rows[admitted]
            mine = np.delete(mine, rng.choice(mine.size, 3, replace=False))
        out.append(tuple((rng.permutation(mine) + c.idx_base).tolist()))
    return tuple(out)


def settle_admitted(d: int, mask: str, lists=None) -> np.ndarray:
    """bool ``[3, settle_rows()]``: the positions of the long cell that the mask admits and the query's list does not name."""
    c = settle_catalog(d)
    out = np.tile(settle_mask(mask), (c.q.shape[0], 1))
    if lists is not None:
        for i, mine in enumerate(lists):
            out[i] &= ~np.isin(long_rows(d) + c.idx_base, np.asarray(mine, dtype=np.int64))
    return out


def settle_expected(d: int, k: int, mask: str = "all", lists=None):
    """The oracle's answer when every query probes the long cell alone (what the export is given): ``chain.topk`` with the
    rows of the other cells, the rows the mask clears and the query's list excluded -- ``(scores [3, k], GLOBAL rows [3, k])``.
    For queries 0 and 2 this is ``_ivf_spec.expected`` at ``nprobe = 1``."""
    c = settle_catalog(d)
    n = c.items.shape[0]
    barred = np.flatnonzero((c.assign != SETTLE_CELL) | ~settle_ok(mask, d))
    every = []
    for i in range(c.q.shape[0]):
        mine = np.asarray([] if lists is None else lists[i], dtype=np.int64) - c.idx_base
        every.append(np.union1d(mine[(mine >= 0) & (mine < n)], barred).tolist())
    s, r = chain.topk(c.q, c.items, k, every)
    return s, np.where(r >= 0, r + c.idx_base, -1)


# ---- the cell of identical rows: equal scores under a live bound, the row not monotone in the position
TIE_DEPTHS = (100, 500, 1000)


@functools.lru_cache(maxsize=None)
def tie_catalog(d: int = 64) -> ivf.Case:
    """One cell of ``settle_rows()`` copies of one unit row; the query is that row.  ``idx_base = 30``."""
    rng = np.random.default_rng(d)
    row = ivf._unit(rng.standard_normal((1, d)))
    n = settle_rows()
    return ivf.Case(f"settle_ties_{d}", np.repeat(row, n, axis=0), row.copy(), np.zeros(n, dtype=np.int64), row.copy(), TIE_DEPTHS[0], 1, None,
                    SETTLE_BASE)


@functools.lru_cache(maxsize=None)
def tie_row_of() -> np.ndarray:
    """A seeded shuffle of the rows over the cell's positions, -1 at the padding: the ``row_of`` the export is given in place of
    the index's (the blocked rows are identical, whatever the order).  The shuffle leans downwards -- the row at position p
    is about n - p, give or take the buffer's 4,096 -- so neither rows nor keys are monotone in the position, and pass after
    pass holds better tied keys: the buffer fills again and again under a live bound.  Through the index a later pass never
    holds a better tied key."""
    n = settle_rows()
    rng = np.random.default_rng(11)
    out = np.full(-(-n // 64) * 64, -1, dtype=np.int64)
    out[np.argsort(np.arange(n) + rng.uniform(0, constants()["IVFD_BUF"], n))] = np.arange(n - 1, -1, -1)
    out.setflags(write=False)
    return out
