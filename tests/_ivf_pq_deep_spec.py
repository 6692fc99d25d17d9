"""What the deep quantised search (``QuantizedIndex.search(path="pq_deep")``, ``mf_pq_scan_deep``, ``mf_pq_refine_deep``) is held
to beyond tests/_ivf_pq_spec.py, shared by tests/test_ivf_pq_deep_cpu.py and tests/test_gpu_ivf_pq_deep.py: the deep case set
(top_k beyond 64, R up to 1,024) and the one-cell catalog whose scan settles several times under a live bound.  The result spec
itself is ``_ivf_pq_spec.candidates`` / ``refine`` / ``search`` -- they take any depth; the buffer's bookkeeping is
``_ivf_deep_spec.walk``."""
from __future__ import annotations

import functools

import numpy as np

from oracle import chain
from tests import _ivf_deep_spec as deep
from tests import _ivf_pq_spec as spec
from tests import _ivf_spec as ivf

MERGE_KEYS = deep.MERGE_KEYS
MAX_R = 1024
DEPTHS = deep.DEPTHS                     # the class boundaries of ivfd_kept, as candidate depths


# ------------------------------------------------------------------------------------------------------ the case set ----
# name -> (ivf.make's arguments, its keywords, sub-vector length, refine factor, codebook iterations)
_CASES = {
    "pqd_w32_k65": (("pqd_w32_k65", 32, 1000, 33, 16, 3, 65), {}, 4, 1, 1),
    "pqd_w32_m2": (("pqd_w32_m2", 32, 1000, 33, 16, 3, 100), {}, 16, 4, 1),                      # M = 2: two code bytes per row
    "pqd_w48_k100": (("pqd_w48_k100", 48, 1000, 33, 16, 8, 100), {}, 8, 4, 1),                   # a padded width
    "pqd_w64_k256": (("pqd_w64_k256", 64, 2500, 70, 37, 3, 256), {"lengths": (0, 1, 17, 1025)}, 16, 4, 1),
    "pqd_w128_k1000": (("pqd_w128_k1000", 128, 2500, 1, 37, 16, 1000), {}, 8, 1, 1),
    "pqd_w256_m32_k1024": (("pqd_w256_m32_k1024", 256, 1000, 33, 16, 8, 1024), {}, 8, 1, 0),
    "pqd_w256_m64_k1024": (("pqd_w256_m64_k1024", 256, 2500, 3, 16, 16, 1024), {}, 4, 1, 0),      # 16 * 1,024 keys: the merge's all
    "pqd_fewer_rows": (("pqd_fewer_rows", 64, 33, 70, 4, 4, 100), {}, 8, 4, 1),
    "pqd_idx_base": (("pqd_idx_base", 64, 1000, 33, 4, 3, 100), {"idx_base": 1000}, 4, 4, 1),
    "pqd_idx_base_no_lists": (("pqd_idx_base_no_lists", 64, 1000, 33, 4, 3, 100), {"idx_base": 1000, "lengths": None}, 4, 4, 1),
    "pqd_k1000_tail": (("pqd_k1000_tail", 64, 2500, 3, 4, 1, 1000), {}, 8, 1, 1),                 # about 610 rows under the probe
    "pqd_nprobe64_k256": (("pqd_nprobe64_k256", 64, 2500, 3, 64, 64, 256), {}, 8, 1, 1),          # 64 * 256 keys: the merge's all
}


@functools.lru_cache(maxsize=None)
def cases() -> dict[str, spec.PqCase]:
    out = {}
    for name, (args, kw, dsub, rf, iters) in _CASES.items():
        out[name] = spec.PqCase(ivf.make(*args, **kw), dsub, rf, iters)
    sizes = [0, 1, 63, 64, 65] + ivf._spread(1000 - 193, 11)           # query 0 is the empty cell's centroid: that cell is probed
    c = ivf.make("pqd_cell_sizes", 64, 1000, 33, 16, 3, 100, sizes=sizes)
    c.q[0] = c.centroids[0]
    out[c.name] = spec.PqCase(c, 8, 4)
    # 1,100 identical rows dealt over four cells of 625 rows with ONE centroid four times: identical residuals, codes and bases,
    # so identical approximate scores across cells and slices -- the row alone orders them
    c = ivf.make("pqd_ties_r1024", 64, 2500, 2, 4, 4, 1024, sizes=[625] * 4, lengths=(0, 5))
    c.items[:1100] = c.items[0]
    c.assign[:1100] = np.arange(1100) % 4
    c.centroids[1:] = c.centroids[0]
    c.q[0] = c.items[0]
    out[c.name] = spec.PqCase(c, 8, 1)
    c = ivf.make("pqd_zero_query", 32, 1000, 3, 16, 3, 100)                # every approximate score 0 for query 1
    c.q[1] = 0.0
    out[c.name] = spec.PqCase(c, 8, 4)
    return out


def per_row_approx(c: spec.PqCase, query: int = 0) -> np.ndarray:
    """The approximate score of every row of a ONE-cell catalog for one query (``_ivf_pq_spec``'s arithmetic)."""
    b = c.base
    qp, cp = ivf.padded(b.q), ivf.padded(b.centroids)
    assert cp.shape[0] == 1
    base, _ = chain.topk(qp[query: query + 1], cp, 1)
    lut = spec.tables(qp[query: query + 1], c.books)[0]
    return spec._approx(lut, base[0], b.assign, c.codes, np.arange(b.items.shape[0]))


# ------------------------------------------------------------------------------------- the cell of several settles ----
LONG_ORDERS = deep.SETTLE_ORDERS
LONG_DEPTHS = (100, 1000, 1024)
LONG_BASE = 30
LONG_BLOCKS = 208


class LongCell(spec.PqCase):
    """A ``PqCase`` with given codebooks (``QuantizedIndex.from_codebooks``): the codes follow the rows."""

    def __init__(self, base, dsub, books):
        super().__init__(base, dsub, 1)
        self.__dict__["books"] = books


@functools.lru_cache(maxsize=None)
def long_cell(order: str) -> LongCell:
    """One cell of ``deep.settle_rows()`` = 13,288 rows of width 32 (four sub-vectors of 8), one query, ``idx_base = 30``, with
    codebooks fixed before the rows are ordered: along the cell order (one cell: position = row) the spec's approximate score of
    the query is ascending, descending or shuffled.  Ties are allowed; the row breaks them.  Read only."""
    n = deep.settle_rows()
    rng = np.random.default_rng(9000)
    items = ivf._unit(rng.standard_normal((n, 32)))
    centroid = ivf._unit(rng.standard_normal((1, 32)))
    q = ivf._unit(centroid + 0.5 * ivf._unit(rng.standard_normal((1, 32))))
    assign = np.zeros(n, dtype=np.int64)
    books = spec.build_codebooks(spec.residuals(items, centroid, assign), 4, 0)
    first = LongCell(ivf.Case("long", items, centroid, assign, q, 1, 1, None, LONG_BASE), 8, books)
    approx = per_row_approx(first)
    by = np.argsort(approx, kind="stable")
    if order == "descending":
        by = by[::-1]
    elif order == "shuffled":
        by = np.random.default_rng(9001).permutation(n)
    else:
        assert order == "ascending"
    out = LongCell(ivf.Case(f"long_{order}", np.ascontiguousarray(items[by]), centroid, assign, q, 1, 1, None, LONG_BASE), 8, books)
    for a in (out.base.items, centroid, assign, q, books):
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def long_approx(order: str) -> np.ndarray:
    out = per_row_approx(long_cell(order))
    out.setflags(write=False)
    return out


def long_slices(r: int) -> tuple[int, int, int]:
    """The slicings of the 208-block cell the GPU test runs at depth r: one, the planned number for one query and one probe,
    the largest the merge takes."""
    return 1, spec.plan_slices(1, 1, r, LONG_BLOCKS), min(LONG_BLOCKS, MERGE_KEYS // r)


def packed(score: np.ndarray, grow: np.ndarray) -> np.ndarray:
    """The packed entries (include/mf_hip.h) of scores and GLOBAL rows: the score's bits << 32 | the row, as int64."""
    bits = np.ascontiguousarray(score, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((bits << np.uint64(32)) | np.asarray(grow, dtype=np.int64).astype(np.uint64)).view(np.int64)


def long_lists(order: str, r: int, slices: int, admitted: np.ndarray | None = None) -> np.ndarray:
    """``[slices, r]`` packed entries: what ``mf_pq_scan_deep`` leaves for the one query and probe, list by list -- slice s holds
    the blocks ``[208 s / S, 208 (s + 1) / S)``, its r best admitted keys (approximate score descending, row ascending), then
    "none" (-1)."""
    approx, n = long_approx(order), deep.settle_rows()
    admitted = np.ones(n, dtype=bool) if admitted is None else admitted
    out = np.full((slices, r), -1, dtype=np.int64)
    for s in range(slices):
        lo, hi = min(n, 64 * (LONG_BLOCKS * s // slices)), min(n, 64 * (LONG_BLOCKS * (s + 1) // slices))
        rows = lo + np.flatnonzero(admitted[lo:hi])
        best = rows[np.argsort(spec.keys(approx[rows], rows + LONG_BASE))[::-1][:r]]
        out[s, : best.size] = packed(approx[best], best + LONG_BASE)
    return out
