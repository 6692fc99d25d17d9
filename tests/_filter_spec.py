"""The filtered search's index arithmetic restated in numpy (csrc/mf_filter.hip, include/mf_hip.h "Filtered search over item
tags"): the predicate, the ascending compaction, the two maps into a view and the map out of it.  Integers only: every
comparison against the kernels is an equality."""
from __future__ import annotations

import numpy as np

U64 = 1 << 64


def admits(tags, any_of: int = 0, all_of: int = 0, none_of: int = 0) -> np.ndarray:
    """bool [N]: ``(t & all_of) == all_of and (any_of == 0 or t & any_of) and not t & none_of`` on the 64-bit patterns."""
    t = np.asarray(tags, dtype=np.int64).view(np.uint64)
    any_of, all_of, none_of = (np.uint64(m % U64) for m in (any_of, all_of, none_of))
    ok = (t & all_of) == all_of
    if any_of:
        ok &= (t & any_of) != 0
    return ok & ((t & none_of) == 0)


def compact(ok) -> tuple[np.ndarray, np.ndarray]:
    """``(rows int64 [M] ascending, rank int32 [N]: the row's slot in rows, or -1)``."""
    ok = np.asarray(ok, dtype=bool)
    rows = np.flatnonzero(ok).astype(np.int64)
    rank = np.full(ok.size, -1, dtype=np.int32)
    rank[rows] = np.arange(rows.size, dtype=np.int32)
    return rows, rank


def remap(ids, idx_base: int, rank) -> np.ndarray:
    """Global rows -> slots; -1 for a row outside ``[idx_base, idx_base + N)`` or outside the view."""
    r = np.asarray(ids, dtype=np.int64) - idx_base
    inside = (r >= 0) & (r < len(rank))
    out = np.full(r.shape, -1, dtype=np.int64)
    out[inside] = np.asarray(rank)[r[inside]]
    return out


def map_lists(off, ids, idx_base: int, rank) -> tuple[np.ndarray, np.ndarray]:
    """An exclusion CSR inside the view: per query the entries the view holds, in their order, as slots."""
    off = np.asarray(off, dtype=np.int64)
    slots = remap(np.asarray(ids, dtype=np.int64)[: off[-1]], idx_base, rank)
    keep = slots >= 0
    kept_before = np.concatenate([[0], np.cumsum(keep)]).astype(np.int64)
    return kept_before[off], slots[keep]


def unmap(idx, rows, idx_base: int) -> np.ndarray:
    """Slots -> global rows; a negative slot stays -1."""
    idx = np.asarray(idx, dtype=np.int64)
    out = np.full(idx.shape, -1, dtype=np.int64)
    ok = idx >= 0
    out[ok] = idx_base + np.asarray(rows, dtype=np.int64)[idx[ok]]
    return out


def extended_lists(exclude, nq: int, ok, idx_base: int) -> list[list[int]]:
    """The oracle's exclusion lists: every query's own list plus every GLOBAL row the filter does not admit."""
    out_rows = (np.flatnonzero(~np.asarray(ok, dtype=bool)) + idx_base).tolist()
    return [[*(exclude[i] if exclude is not None else []), *out_rows] for i in range(nq)]
