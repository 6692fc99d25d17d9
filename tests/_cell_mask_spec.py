"""The allow bitmap of the cell scans restated in numpy (``mf_filter_cell_bits`` of csrc/mf_filter.hip, ``retrieval.CellMask``):
one 64-bit word per 64-row block of a cell-ordered catalog.  The predicate is ``tests/_filter_spec.admits``; what a search with
such a mask must return is stated through ``_filter_spec.extended_lists`` -- the same search with every inadmissible global row
appended to every query's exclusion list.  Integers only: every comparison against the kernel is an equality."""
from __future__ import annotations

import numpy as np

from tests import _filter_spec

admits = _filter_spec.admits
extended_lists = _filter_spec.extended_lists


def layout(assign, num_cells: int) -> tuple[np.ndarray, np.ndarray]:
    """``(cell_blk int64 [C + 1], row_of int64 [Npad])`` of ``retrieval.partition_layout``: the rows by cell, ascending inside a
    cell, every cell padded to whole 64-row blocks, -1 at the padding positions."""
    assign = np.asarray(assign, dtype=np.int64)
    blocks = [(int((assign == c).sum()) + 63) // 64 for c in range(num_cells)]
    cell_blk = np.concatenate([[0], np.cumsum(blocks)]).astype(np.int64)
    row_of = np.full(int(cell_blk[-1]) * 64, -1, dtype=np.int64)
    for c in range(num_cells):
        rows = np.flatnonzero(assign == c)
        row_of[cell_blk[c] * 64: cell_blk[c] * 64 + rows.size] = rows
    return cell_blk, row_of


def words(ok, row_of) -> np.ndarray:
    """int64 ``[Npad // 64]``, the bit patterns of the words: bit ``lane`` of word ``blk`` is set iff ``r = row_of[blk * 64 + lane]
    >= 0`` and ``ok[r]``."""
    ok, row_of = np.asarray(ok, dtype=bool), np.asarray(row_of, dtype=np.int64)
    assert row_of.size % 64 == 0
    bit = (row_of >= 0) & ok[np.clip(row_of, 0, None)]
    out = np.zeros(row_of.size // 64, dtype=np.uint64)
    for lane in range(64):
        out |= bit[lane::64].astype(np.uint64) << np.uint64(lane)
    return out.view(np.int64)
