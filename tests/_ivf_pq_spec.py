"""What the quantised index (``retrieval.QuantizedIndex``, csrc/mf_pq.hip) must compute, restated in numpy on the oracle's
chain (``oracle.chain.scores`` on sub-vectors zero-padded to 8 channels), and the cases the CPU and the GPU tests share --
those of tests/_ivf_spec.py, each with a sub-vector length, a refine factor and seeded codebooks.

With D the stored width, ``dsub`` in {4, 8, 16}, ``M = D / dsub``, codebooks ``B[M][256][dsub]``:
  residual   r = x - centroid[cell]                                        one fp32 subtraction per channel
  code[m]    = argmax_j (chain(r[m], B[m][j]) - 0.5f * chain(B[m][j], B[m][j])), lowest j on ties
  lut[m][j]  = chain(q[m], B[m][j])
  approx     = ((base + lut[0][code_0]) + lut[1][code_1]) + ...,  base = chain(q, centroid[cell])
  candidates = the admissible rows of the probed cells by (approx descending, global row ascending), the first R
  result     = the candidates by (chain(q, x) descending, global row ascending), the first k, then the -inf / -1 tail
Rows compare as integers, scores as uint32 views.
"""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

from oracle import chain
from tests import _ivf_spec as ivf

F32 = np.float32
SUB_LENGTHS = (4, 8, 16)


# ------------------------------------------------------------------------------------------------ the arithmetic ----
def _pad8(x: np.ndarray) -> np.ndarray:
    w = -(-x.shape[1] // 8) * 8
    return np.ascontiguousarray(np.pad(x, ((0, 0), (0, w - x.shape[1]))), dtype=F32)


def sub(x: np.ndarray, m: int, dsub: int) -> np.ndarray:
    """Sub-vector m of every row, as the chain takes it."""
    return _pad8(x[:, m * dsub : (m + 1) * dsub])


def residuals(items: np.ndarray, centroids: np.ndarray, assign: np.ndarray) -> np.ndarray:
    return (ivf.padded(items) - ivf.padded(centroids)[assign]).astype(F32)


def half_norms(books: np.ndarray) -> np.ndarray:
    """``h[m][j] = 0.5f * chain(B[m][j], B[m][j])``."""
    return np.stack([F32(0.5) * np.diagonal(chain.scores(_pad8(b), _pad8(b))) for b in books]).astype(F32)


def encode(res: np.ndarray, books: np.ndarray) -> np.ndarray:
    """``codes [N, M]`` uint8 of residuals ``[N, D]``."""
    m, _, dsub = books.shape
    h = half_norms(books)
    out = np.empty((res.shape[0], m), dtype=np.uint8)
    for j in range(m):
        s = (chain.scores(sub(res, j, dsub), _pad8(books[j])) - h[j][None, :]).astype(F32)
        out[:, j] = np.argmax(s, axis=1)                                   # the first of equal maxima: the lowest code
    return out


def tables(q: np.ndarray, books: np.ndarray) -> np.ndarray:
    """``lut [Q, M, 256]``."""
    m, _, dsub = books.shape
    return np.stack([chain.scores(sub(q, j, dsub), _pad8(books[j])) for j in range(m)], axis=1).astype(F32)


def keys(score: np.ndarray, row: np.ndarray) -> np.ndarray:
    """``mf_key_retrieval``: larger is better -- score descending, then row ascending."""
    u = np.ascontiguousarray(score, dtype=F32).view(np.uint32)
    ordered = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint64)
    return (ordered << np.uint64(32)) | (~np.asarray(row, dtype=np.int64).astype(np.uint32)).astype(np.uint64)


def _tailed(score, row, width):
    s = np.full(width, -np.inf, dtype=F32)
    r = np.full(width, -1, dtype=np.int64)
    n = min(width, len(row))
    s[:n], r[:n] = score[:n], row[:n]
    return s, r


def _approx(lut_q, base_of, assign, codes, rows):
    acc = base_of[assign[rows]]
    for j in range(codes.shape[1]):
        acc = (acc + lut_q[j, codes[rows, j]]).astype(F32)                  # plain fp32 adds in ascending m
    return acc


def candidates(q, items, centroids, assign, books, codes, r: int | None, nprobe: int, exclude=None, idx_base: int = 0):
    """``(approx [Q, R] fp32, GLOBAL rows [Q, R] int64)``, the -inf / -1 tail; ``r=None``: every admissible probed row, as lists."""
    qp, cp = ivf.padded(q), ivf.padded(centroids)
    base, cells = chain.topk(qp, cp, nprobe)
    lut = tables(qp, books)
    out_s, out_r = [], []
    for i in range(qp.shape[0]):
        base_of = np.zeros(cp.shape[0], dtype=F32)
        base_of[cells[i]] = base[i]
        rows = np.nonzero(np.isin(assign, cells[i]))[0]
        if exclude is not None:
            rows = rows[~np.isin(rows + idx_base, np.asarray(exclude[i], dtype=np.int64))]
        acc = _approx(lut[i], base_of, assign, codes, rows)
        order = np.argsort(keys(acc, rows + idx_base))[::-1]
        s, g = acc[order], rows[order] + idx_base
        if r is not None:
            s, g = _tailed(s, g, r)
        out_s.append(s)
        out_r.append(g)
    return (out_s, out_r) if r is None else (np.stack(out_s), np.stack(out_r))


def refine(q, items, cand_rows, k: int, idx_base: int = 0):
    """``(scores [Q, k] fp32, GLOBAL rows [Q, k] int64)``: the candidates by their exact chain score."""
    qp, ip = ivf.padded(q), ivf.padded(items)
    out_s, out_r = [], []
    for i in range(qp.shape[0]):
        g = np.asarray(cand_rows[i], dtype=np.int64)
        g = g[g >= 0]
        exact = chain.scores(qp[i : i + 1], ip[g - idx_base])[0] if g.size else np.zeros(0, dtype=F32)
        order = np.argsort(keys(exact, g))[::-1]
        s, r = _tailed(exact[order], g[order], k)
        out_s.append(s)
        out_r.append(r)
    return np.stack(out_s), np.stack(out_r)


def search(q, items, centroids, assign, books, codes, k: int, refine_factor: int | None, nprobe: int, exclude=None, idx_base: int = 0):
    """``refine_factor=None``: every admissible probed row is a candidate."""
    r = None if refine_factor is None else refine_factor * k
    _, rows = candidates(q, items, centroids, assign, books, codes, r, nprobe, exclude, idx_base)
    return refine(q, items, rows, k, idx_base)


def build_codebooks(res: np.ndarray, m: int, pq_iters: int) -> np.ndarray:
    """The seeded build on training residuals ``[T, D]`` (all rows of a catalog of at most 65,536): codeword j of every
    sub-space starts as the sub-vector of row ``j mod T``; an iteration encodes the rows and replaces every codeword by the
    mean of its sub-vectors -- added in row order in fp32, from 0, then divided by the count; an empty one stays."""
    t, d = res.shape
    dsub = d // m
    books = res[np.arange(256) % t].reshape(256, m, dsub).transpose(1, 0, 2).copy()
    for _ in range(pq_iters):
        codes = encode(res, books)
        for j in range(m):
            part = res[:, j * dsub : (j + 1) * dsub]
            for c in np.unique(codes[:, j]):
                mine = part[codes[:, j] == c]
                total = np.add.accumulate(np.concatenate([np.zeros((1, dsub), F32), mine]), axis=0, dtype=F32)[-1]
                books[j, c] = total / F32(mine.shape[0])
    return books


def layout(assign: np.ndarray, c: int) -> tuple[np.ndarray, np.ndarray]:
    """``(cell_blk [C + 1], row_of [Npad])`` of ``retrieval.partition_layout``."""
    sizes = np.bincount(assign, minlength=c)
    cell_blk = np.concatenate([[0], np.cumsum((sizes + 63) // 64)]).astype(np.int64)
    row_of = np.full(64 * int(cell_blk[-1]), -1, dtype=np.int64)
    for cell in range(c):
        rows = np.nonzero(assign == cell)[0]
        row_of[64 * cell_blk[cell] : 64 * cell_blk[cell] + rows.size] = rows
    return cell_blk, row_of


def device_codes(codes: np.ndarray, row_of: np.ndarray) -> np.ndarray:
    """``codes [N, M]`` in the cell-ordered layout of include/mf_hip.h: ``[64-row block][M / U][64][U]`` bytes, U = min(M, 4),
    code 0 at padding positions."""
    m = codes.shape[1]
    u = min(m, 4)
    at = np.zeros((row_of.size, m), dtype=np.uint8)
    at[row_of >= 0] = codes[row_of[row_of >= 0]]
    return np.ascontiguousarray(at.reshape(-1, 64, m // u, u).transpose(0, 2, 1, 3)).reshape(-1)


def plan_slices(nq: int, nprobe: int, r: int, max_cell_blocks: int) -> int:
    """The documented rule of ``mf_pq_plan``: that of ``mf_ivf_plan`` with R for k and the 16,384 keys of the deep merge."""
    return ivf.plan_slices(nq, nprobe, r, max_cell_blocks, merge_keys=16384)


# ----------------------------------------------------------------------------------------------------- the cases ----
@dataclasses.dataclass
class PqCase:
    base: ivf.Case
    dsub: int
    refine_factor: int
    pq_iters: int = 1

    @property
    def name(self) -> str:
        return self.base.name

    @property
    def width(self) -> int:
        return ivf.padded(self.base.items).shape[1]

    @property
    def m(self) -> int:
        return self.width // self.dsub

    @property
    def r(self) -> int:
        return self.refine_factor * self.base.k

    @functools.cached_property
    def residuals(self) -> np.ndarray:
        return residuals(self.base.items, self.base.centroids, self.base.assign)

    @functools.cached_property
    def books(self) -> np.ndarray:
        return build_codebooks(self.residuals, self.m, self.pq_iters)

    @functools.cached_property
    def codes(self) -> np.ndarray:
        return encode(self.residuals, self.books)

    def _args(self):
        c = self.base
        return c.q, c.items, c.centroids, c.assign, self.books, self.codes

    def candidates(self, r: int | None = -1):
        c = self.base
        return candidates(*self._args(), self.r if r == -1 else r, c.nprobe, c.exclude, c.idx_base)

    def expected(self, refine_factor: int | None = -1):
        c = self.base
        rf = self.refine_factor if refine_factor == -1 else refine_factor
        return search(*self._args(), c.k, rf, c.nprobe, c.exclude, c.idx_base)


# (sub-vector length, refine factor) of every shared case: R = refine_factor * k takes 1, 20, 80 and 256 among others
_GEOMETRY = {
    "width32": (4, 4), "width64": (8, 4), "width128": (16, 4), "width256": (4, 1),
    "one_cell_one_row_list": (16, 1), "fewer_rows_than_k": (16, 4), "long_lists": (8, 4), "all_cells_k64": (16, 4),
    "sliced_cells": (8, 4), "k1_many_queries": (8, 1), "idx_base": (4, 4), "padded_width": (8, 4),
    "cell_sizes_nprobe3": (8, 4), "cell_sizes_nprobe16": (16, 1), "big_cell": (8, 4), "all_but_three": (8, 4),
    "ties_across_cells": (8, 4), "twin_centroids": (4, 4), "zero_query": (8, 4),
}


@functools.lru_cache(maxsize=None)
def cases() -> dict[str, PqCase]:
    base = ivf.cases()
    assert set(base) == set(_GEOMETRY)
    return {name: PqCase(c, *_GEOMETRY[name]) for name, c in base.items()}


# ------------------------------------------------------------------------------------- the scan's steady state ----
def scan_trace(q, items, centroids, assign, books, codes, r: int, exclude=None, idx_base: int = 0, query: int = 0) -> dict:
    """How ``pq_scan_kernel`` walks the best cell of one query when the cell is ONE slice (csrc/mf_pq.hip): passes of four 64-row
    blocks; a key has to beat the bound ``tau`` (0 until a settle has left R keys) before it is looked up in the exclusion
    list; what stays waits behind the kept keys; the buffer is settled -- the R best kept, their R-th the new bound -- inside
    the loop when more than 512 keys wait, and after it when any do.  Returns the counts the tests assert on and the list the
    walk ends with, which must be the first R candidates whatever the path taken."""
    qp, cp = ivf.padded(q), ivf.padded(centroids)
    base, cells = chain.topk(qp[query : query + 1], cp, 1)
    _, row_of = layout(assign, cp.shape[0])
    cell_blk, _ = layout(assign, cp.shape[0])
    lo, hi = 64 * int(cell_blk[cells[0, 0]]), 64 * int(cell_blk[cells[0, 0] + 1])
    at = row_of[lo:hi]
    rows = at[at >= 0]
    base_of = np.zeros(cp.shape[0], dtype=F32)
    base_of[cells[0]] = base[0]
    key = np.zeros(at.size, dtype=np.uint64)
    key[at >= 0] = keys(_approx(tables(qp[query : query + 1], books)[0], base_of, assign, codes, rows), rows + idx_base)
    barred = np.zeros(at.size, dtype=bool)
    if exclude is not None:
        barred[at >= 0] = np.isin(rows + idx_base, np.asarray(exclude[query], dtype=np.int64))
    kept = np.zeros(0, dtype=np.uint64)
    waiting: list = []
    tau = np.uint64(0)
    out = {"passes": 0, "settles_in_loop": 0, "lookups": 0, "turned_away_by_the_bound": 0, "excluded_hits": 0, "excluded_hits_under_a_bound": 0}

    def settle():
        nonlocal kept, waiting, tau
        kept = np.sort(np.concatenate([kept, np.asarray(waiting, dtype=np.uint64)]))[::-1][:r]
        tau = kept[r - 1] if kept.size >= r else np.uint64(0)
        waiting = []

    for p0 in range(0, at.size, 256):
        k, b = key[p0 : p0 + 256], barred[p0 : p0 + 256]
        beats = k > tau                                                    # (padding has key 0: never)
        out["passes"] += 1
        out["lookups"] += int(beats.sum())
        out["turned_away_by_the_bound"] += int(((k != 0) & ~beats).sum())
        out["excluded_hits"] += int((beats & b).sum())
        out["excluded_hits_under_a_bound"] += int((beats & b).sum()) if tau else 0
        waiting += k[beats & ~b].tolist()
        if len(waiting) > 512:
            settle()
            out["settles_in_loop"] += 1
    out["settle_after_the_loop"] = len(waiting) > 0
    if waiting:
        settle()
    out["keys"] = kept
    return out


@functools.lru_cache(maxsize=None)
def steady_cases() -> dict[str, PqCase]:
    """Cells of 2,560 rows (40 blocks: ten passes) scanned as ONE slice, which the shared cases never are (their slices have
    at most six blocks: two passes, no bound, one settle).  ``steady``: the big cell of ``big_cell`` with a list of 150
    exclusions that holds every other one of its 60 best candidates.  ``steady_tail``: the first 768 rows of the cell lie
    near the query and the other 1,792 opposite it, so the settle after the third pass is the last thing that happens -- the
    walk ends with nothing waiting.  ``steady_many``: 1,024 queries on that catalog, where the plan itself gives one slice."""
    out = {}
    c = PqCase(ivf.cases()["big_cell"], 8, 4)
    base = ivf.Case(**{**c.base.__dict__, "name": "steady"})
    c = PqCase(base, 8, 4)
    _, best = c.candidates(60)
    rng = np.random.default_rng(60)
    base.exclude = [np.concatenate([best[0][::2], rng.choice(np.setdiff1d(np.arange(2620), best[0]), 120, replace=False)]).tolist()]
    out["steady"] = PqCase(base, 8, 4)

    rng = np.random.default_rng(61)
    base = ivf.make("steady_tail", 64, 2620, 1, 4, 1, 20, sizes=[2560, 10, 20, 30], lengths=None)
    base.assign = np.concatenate([np.zeros(2560, np.int64), np.repeat(np.arange(1, 4), [10, 20, 30])])
    base.q[0] = base.centroids[0]
    noise = rng.standard_normal((2560, 64)).astype(F32) / 8
    sign = np.where(np.arange(2560) < 768, 1.0, -1.0).astype(F32)[:, None]
    base.items[:2560] = ivf._unit(sign * base.centroids[0] + noise)
    base.exclude = [rng.choice(768, 100, replace=False).tolist()]
    out["steady_tail"] = PqCase(base, 8, 4)

    many = ivf.Case(**{**base.__dict__, "name": "steady_many"})
    many.q = ivf._unit(base.centroids[0] + rng.standard_normal((1024, 64)).astype(F32) / 16)
    many.exclude = [rng.choice(2620, (0, 1, 100)[i % 3], replace=False).tolist() for i in range(1024)]
    out["steady_many"] = PqCase(many, 8, 4)
    return out
