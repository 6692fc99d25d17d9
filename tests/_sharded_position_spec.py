"""Plain numpy restatement of positions over a row-sharded catalog (``mf_target_words`` + ``mf_key_positions``, include/mf_hip.h;
``ShardedIndex.positions``): what each shard computes from its own rows, and how the shards' answers combine.  TEST
INFRASTRUCTURE -- the package does not import it.

A shard is ``(stride, offset, n)``: its local row l is global row ``l * stride + offset``, l < n.  Global order: order word
(``mf_orderable`` of the chain score) descending, then global row ascending -- tests/_position_spec.py's on the whole catalog.
"""
from __future__ import annotations

import numpy as np

from oracle import chain
from tests import _position_spec as spec


def round_robin(n: int, shards: int) -> list[tuple[int, int, int]]:
    return [(shards, s, len(range(s, n, shards))) for s in range(shards)]


def contiguous(n: int, shards: int) -> list[tuple[int, int, int]]:
    """Blocks of uneven sizes (the first ``n % shards`` hold one row more), none empty for ``n >= shards``."""
    sizes = [n // shards + (1 if s < n % shards else 0) for s in range(shards)]
    return [(1, int(sum(sizes[:s])), sizes[s]) for s in range(shards)]


def rows_of(shard) -> np.ndarray:
    stride, offset, n = shard
    return np.arange(n, dtype=np.int64) * stride + offset


def bound(g: int, shard) -> int:
    """L: the number of the shard's rows whose global row is below g (exact integers)."""
    stride, offset, n = shard
    g = int(g)
    if g < offset:
        return 0
    return min(-((offset - g) // stride), n)                 # ceil((g - offset) / stride)


def local_row(g: int, shard) -> int:
    """The shard's row that IS global row g, or -1."""
    stride, offset, n = shard
    d = int(g) - offset
    return d // stride if d >= 0 and d % stride == 0 and d // stride < n else -1


def shard_words(scores, tgt_off, tgt_idx, shard) -> np.ndarray:
    """int64 [T]: the order word of every entry whose row the shard holds (``scores`` [Q, n]: its rows' chain scores), else 0."""
    words = np.zeros(len(tgt_idx), dtype=np.int64)
    order = spec.orderable(scores).reshape(scores.shape)
    for r in range(scores.shape[0]):
        for e in range(int(tgt_off[r]), int(tgt_off[r + 1])):
            l = local_row(tgt_idx[e], shard)
            if l >= 0:
                words[e] = int(order[r, l])
    return words


def shard_counts(scores, tgt_off, tgt_idx, words, shard, exclude_local=None):
    """``(above int64 [T], score fp32 [T], ncand int64 [Q])`` of one shard; ``exclude_local``: per query LOCAL rows (any)."""
    nq, n = scores.shape
    above = np.full(len(tgt_idx), -1, dtype=np.int64)
    score = np.full(len(tgt_idx), -np.inf, dtype=np.float32)
    ncand = np.zeros(nq, dtype=np.int64)
    for r in range(nq):
        slab = spec.orderable(scores[r]).astype(np.int64)
        if exclude_local is not None and len(exclude_local[r]):
            ex = np.asarray(exclude_local[r], dtype=np.int64)
            slab[ex[(ex >= 0) & (ex < n)]] = 0
        ncand[r] = int((slab != 0).sum())
        for e in range(int(tgt_off[r]), int(tgt_off[r + 1])):
            tw = int(words[e])
            l = local_row(tgt_idx[e], shard)
            if tw == 0 or (l >= 0 and slab[l] == 0):
                continue
            L = bound(tgt_idx[e], shard)
            above[e] = int((slab > tw).sum()) + int((slab[:L] == tw).sum())
            score[e] = np.array([tw ^ 0xFFFFFFFF if not tw & 0x80000000 else tw & 0x7FFFFFFF], dtype=np.uint32).view(np.float32)[0]
    return above, score, ncand


def combine(parts):
    """[(above, score, ncand) per shard] -> (pos, score, ncand) of the whole catalog."""
    above = np.stack([p[0] for p in parts])
    none = (above < 0).any(axis=0)
    pos = np.where(none, -1, above.sum(axis=0))
    score = np.where(none, np.float32(-np.inf), parts[0][1]).astype(np.float32)
    return pos, score, np.stack([p[2] for p in parts]).sum(axis=0)


def sharded_positions(q, items, shards, tgt_off, tgt_idx, exclude=None):
    """Per shard: words, bounds, counts and ncand from ``oracle.chain.scores`` of the shard's own rows; then the maximum of the
    words over the shards, and the combination.  ``exclude``: per query GLOBAL rows (any, also outside the catalog)."""
    q, items = np.asarray(q, dtype=np.float32), np.asarray(items, dtype=np.float32)
    tgt_off, tgt_idx = np.asarray(tgt_off, dtype=np.int64), np.asarray(tgt_idx, dtype=np.int64)
    scores = [chain.scores(q, np.ascontiguousarray(items[rows_of(sh)])) for sh in shards]
    words = np.stack([shard_words(sc, tgt_off, tgt_idx, sh) for sc, sh in zip(scores, shards)]).max(axis=0)
    parts = []
    for sc, sh in zip(scores, shards):
        local = None if exclude is None else [[local_row(g, sh) for g in ex] for ex in exclude]
        parts.append(shard_counts(sc, tgt_off, tgt_idx, words, sh, local))
    return combine(parts)
