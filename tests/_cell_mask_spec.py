"""The allow bitmap of the cell scans restated in numpy (``mf_filter_cell_bits`` of csrc/mf_filter.hip, ``retrieval.CellMask``):
one 64-bit word per 64-row block of a cell-ordered catalog.  The predicate is ``tests/_filter_spec.admits``; what a search with
such a mask must return is stated through ``_filter_spec.extended_lists`` -- the same search with every inadmissible global row
appended to every query's exclusion list.  Integers only: every comparison against the kernel is an equality."""
from __future__ import annotations

import functools
import zlib

import numpy as np

from tests import _filter_spec
from tests import _ivf_pq_spec as pq
from tests import _ivf_spec as ivf

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


# ------------------------------------------------------------------- slices longer than one strip of mask words ----
# ``pq_scan_allow_kernel`` (csrc/mf_pq_scan.inc) does not read its mask word by word: lane l holds the word of block
# ``strip0 + l`` (a strip: 64 words, 16 passes of four waves), a second strip is asked for ahead, and once ``blk0 - strip0 >=
# 64`` the kernel rotates.  What follows is the catalog whose slices are long enough to rotate, the masks that tell a strip
# from its neighbours, and the rotation itself in integers.
LONG_CELL_SIZES = (40, 8230, 70, 100)      # cell 1: 129 blocks from block 1 on, 38 rows in the last
LONG_CELL = 1
LONG_IDX_BASE = 30
LONG_NQ = 5


@functools.lru_cache(maxsize=None)
def long_cell_case(d: int, dsub: int) -> pq.PqCase:
    """8,440 rows in four cells, the second of 8,230 rows: ``c0 = 1``, so no strip load of its slices is 64-word aligned in the
    mask.  Five queries near that cell's centroid (nprobe = 1 probes it), seeded untrained codebooks, ``idx_base = 30``."""
    base = ivf.make(f"long_cell_{d}", d, sum(LONG_CELL_SIZES), LONG_NQ, len(LONG_CELL_SIZES), 1, 20, sizes=list(LONG_CELL_SIZES), lengths=None)
    rng = np.random.default_rng(d)
    base.q = ivf._unit(base.centroids[LONG_CELL] + rng.standard_normal((LONG_NQ, d)).astype(np.float32) / 16)
    base.idx_base = LONG_IDX_BASE
    return pq.PqCase(base, dsub, 4, pq_iters=0)


def long_cell_queries(d: int, nq: int) -> np.ndarray:
    """``nq`` more seeded queries that probe the long cell."""
    c = long_cell_case(d, 8).base
    rng = np.random.default_rng(d + nq)
    return ivf._unit(c.centroids[LONG_CELL] + rng.standard_normal((nq, d)).astype(np.float32) / 16)


def _long(cell_blk) -> tuple[int, int]:
    """``(c0, nb)`` of the cell with the most blocks."""
    nb = np.diff(np.asarray(cell_blk, dtype=np.int64))
    return int(cell_blk[int(nb.argmax())]), int(nb.max())


def _of_blocks(row_of, cell_blk, rng, blocks, density=None) -> np.ndarray:
    """ok[n]: the rows of the long cell's blocks ``blocks`` (relative to its first), each with probability ``density[j]`` where
    given, and a random half of the rows of every other cell."""
    row_of = np.asarray(row_of, dtype=np.int64)
    c0, nb = _long(cell_blk)
    ok = np.zeros(int(row_of.max()) + 1, dtype=bool)
    outside = np.concatenate([row_of[: c0 * 64], row_of[(c0 + nb) * 64:]])
    outside = outside[outside >= 0]
    ok[outside[rng.random(outside.size) < 0.5]] = True
    for j in blocks:
        rows = row_of[(c0 + j) * 64: (c0 + j + 1) * 64]
        rows = rows[rows >= 0]
        ok[rows if density is None else rows[rng.random(rows.size) < density[j]]] = True
    return ok


def _third_strip(row_of, cell_blk, rng):
    return _of_blocks(row_of, cell_blk, rng, [128])


def _second_strip(row_of, cell_blk, rng):
    return _of_blocks(row_of, cell_blk, rng, range(64, 128))


def _not_first_strip(row_of, cell_blk, rng):
    return _of_blocks(row_of, cell_blk, rng, range(64, _long(cell_blk)[1]))


def _strip_edges(row_of, cell_blk, rng):
    return _of_blocks(row_of, cell_blk, rng, [63, 64, 127, 128])


def _two_bits(row_of, cell_blk, rng):
    ok = _of_blocks(row_of, cell_blk, rng, [])
    c0, _ = _long(cell_blk)
    ok[[int(row_of[(c0 + 64) * 64 + 63]), int(row_of[(c0 + 128) * 64])]] = True
    return ok


def _alternate_blocks(row_of, cell_blk, rng):
    return _of_blocks(row_of, cell_blk, rng, range(0, _long(cell_blk)[1], 2))


def _sparse_blocks(row_of, cell_blk, rng):
    nb = _long(cell_blk)[1]
    picked = np.flatnonzero(rng.random(nb) < 0.2)
    return _of_blocks(row_of, cell_blk, rng, picked, density=rng.random(nb))


def _half(row_of, cell_blk, rng):
    return _of_blocks(row_of, cell_blk, rng, range(_long(cell_blk)[1]), density=np.full(_long(cell_blk)[1], 0.5))


# name -> (row_of, cell_blk, rng) -> ok[n]; block numbers are those of the long cell, 0 .. 128
MASK_FAMILIES = {
    "third_strip": _third_strip,            # block 128 alone: 38 rows, fewer than R = 80
    "second_strip": _second_strip,          # blocks 64 .. 127
    "not_first_strip": _not_first_strip,    # everything but blocks 0 .. 63
    "strip_edges": _strip_edges,            # blocks 63, 64, 127, 128
    "two_bits": _two_bits,                  # lane 63 of block 64 and lane 0 of block 128
    "alternate_blocks": _alternate_blocks,  # odd blocks 0, even blocks whole: in every pass two waves skip and two read
    "sparse_blocks": _sparse_blocks,        # one block in five at a random density, the rest 0: passes without a reader
    "half": _half,                          # dense random
}


@functools.lru_cache(maxsize=None)
def long_cell_layout(d: int) -> tuple[np.ndarray, np.ndarray]:
    """``layout`` of the long-cell catalog of width ``d`` (the same ``cell_blk`` at every width, another deal of the rows)."""
    c = long_cell_case(d, 8 if d < 256 else 4).base
    return layout(c.assign, c.centroids.shape[0])


@functools.lru_cache(maxsize=None)
def family_ok(name: str, d: int) -> np.ndarray:
    """The family's mask on the long-cell catalog of width ``d``, seeded by its name.  Read only."""
    cell_blk, row_of = long_cell_layout(d)
    ok = MASK_FAMILIES[name](row_of, cell_blk, np.random.default_rng(zlib.crc32(name.encode())))
    ok.setflags(write=False)
    return ok


def strip_walk(cell_blk, cell: int, S: int, slice: int, words, rotate: bool = True) -> dict:  # noqa: A002, N803
    """The walk of ``pq_scan_allow_kernel`` over slice ``slice`` of ``S`` of cell ``cell``, as far as the mask goes: blocks
    ``[b0, b1)`` in passes of four (wave w of a pass has block ``blk0 + w``); lane l of a strip holds ``words[first + l]`` where
    ``first + l < b1``, else 0; the strips at ``b0`` and ``b0 + 64`` are loaded before the loop, and a pass that finds ``blk0 -
    strip0 >= 64`` moves on -- ``strip0 += 64``, the strip ahead becomes the current one, the next is loaded at ``strip0 + 64``.
    A wave's word is lane ``blk - strip0`` of the current strip; it reads its block where ``blk < b1`` and the word is not 0.
    ``rotate=False``: a kernel that keeps its first strip for ever (the lane number taken modulo 64, as the hardware takes it).

    ``seen``: the cell-ordered positions ``blk * 64 + lane`` whose bit the walk finds set.  ``mixed_passes``: passes in which
    some of the four waves read and some do not (a zero word, or a block past the end) -- they still meet at the barriers.
    ``blocks_in_last_strip``: the blocks of the slice from the last ``strip0`` on, 64 at the most."""
    cell_blk = [int(b) for b in cell_blk]
    words = [int(w) for w in np.asarray(words, dtype=np.int64).view(np.uint64)]
    c0, nb = cell_blk[cell], cell_blk[cell + 1] - cell_blk[cell]
    b0, b1 = c0 + nb * slice // S, c0 + nb * (slice + 1) // S

    def load(first):
        return [words[first + lane] if first + lane < b1 else 0 for lane in range(64)]

    strip0, strip, strip_next = b0, load(b0), load(b0 + 64)
    out = {"seen": set(), "passes": 0, "rotations": 0, "blocks_read": 0, "blocks_skipped": 0, "passes_without_a_reader": 0, "mixed_passes": 0}
    for blk0 in range(b0, b1, 4):
        if rotate and blk0 - strip0 >= 64:
            strip0 += 64
            strip, strip_next = strip_next, load(strip0 + 64)
            out["rotations"] += 1
        readers = 0
        for blk in range(blk0, blk0 + 4):
            if blk >= b1:
                continue
            word = strip[(blk - strip0) % 64]
            out["blocks_read" if word else "blocks_skipped"] += 1
            readers += word != 0
            out["seen"].update(blk * 64 + lane for lane in range(64) if word >> lane & 1)
        out["passes"] += 1
        out["passes_without_a_reader"] += readers == 0
        out["mixed_passes"] += 0 < readers < 4
    out["blocks_in_last_strip"] = min(64, b1 - strip0)
    return out
