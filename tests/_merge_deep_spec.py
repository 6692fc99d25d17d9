"""The deep merge written out in numpy (``mf_topk_merge_deep`` / ``mf_topk_merge_packed_deep``, csrc/mf_topk.hip): the 64-bit
retrieval key, the order the merged list has for ANY ordered lists -- key descending, then list number ascending, then position
ascending -- and the kernel's rank rule, which must give that order without sorting."""
from __future__ import annotations

import numpy as np

ALL_ONES = np.uint32(0xFFFFFFFF)


def keys(scores: np.ndarray, rows: np.ndarray) -> np.ndarray:
    """uint64 keys of (score, global row) entries, 0 for none (row < 0): order word of the score << 32 | ~row."""
    bits = np.ascontiguousarray(scores, dtype=np.float32).view(np.uint32)
    hi = np.where(bits & np.uint32(0x80000000), ~bits, bits | np.uint32(0x80000000)).astype(np.uint64)
    lo = (~(rows & 0xFFFFFFFF).astype(np.uint32)).astype(np.uint64)
    return np.where(rows >= 0, (hi << np.uint64(32)) | lo, np.uint64(0))


def entries(key: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """(scores fp32, rows int64) of keys; -inf / -1 for key 0."""
    hi = (key >> np.uint64(32)).astype(np.uint32)
    bits = np.where(hi & np.uint32(0x80000000), hi & np.uint32(0x7FFFFFFF), ~hi)
    rows = (~(key & np.uint64(0xFFFFFFFF)).astype(np.uint32)).astype(np.int64)
    none = key == 0
    return np.where(none, np.float32(-np.inf), bits.view(np.float32)).astype(np.float32), np.where(none, -1, rows)


def packed(scores: np.ndarray, rows: np.ndarray) -> np.ndarray:
    """The exchange form ``mf_topk_pack`` writes for GLOBAL rows: score bits << 32 | row, -1 for none."""
    bits = np.ascontiguousarray(scores, dtype=np.float32).view(np.uint32).astype(np.uint64)
    word = (bits << np.uint64(32)) | (rows & 0xFFFFFFFF).astype(np.uint64)
    return np.where(rows >= 0, word.view(np.int64), -1)


def merge_sorted(key: np.ndarray, k: int) -> np.ndarray:
    """``key`` [G, kk] of one query -> the first k keys by (key descending, list ascending, position ascending), 0-padded."""
    g, kk = key.shape
    flat = key.reshape(-1)
    lists, places = np.divmod(np.arange(g * kk), kk)
    there = flat != 0
    order = sorted(np.flatnonzero(there).tolist(), key=lambda t: (-int(flat[t]), int(lists[t]), int(places[t])))[:k]
    out = np.zeros(k, dtype=np.uint64)
    out[: len(order)] = flat[order]
    return out


def merge_ranked(key: np.ndarray, k: int) -> np.ndarray:
    """The kernel's rule: entry e of list g goes to column e + sum over earlier lists of #{keys >= x} + sum over later lists of
    #{keys > x}; every column below min(m, k) must be written exactly once, the rest stays 0."""
    g, kk = key.shape
    out = np.zeros(k, dtype=np.uint64)
    written = np.zeros(k, dtype=np.int64)
    for a in range(g):
        for e in range(kk):
            x = key[a, e]
            if x == 0:
                continue
            rank = e
            for b in range(g):
                if b < a:
                    rank += int((key[b] >= x).sum())
                elif b > a:
                    rank += int((key[b] > x).sum())
            if rank < k:
                out[rank] = x
                written[rank] += 1
    m = int((key != 0).sum())
    assert written[: min(m, k)].tolist() == [1] * min(m, k) and not written[min(m, k):].any(), written
    return out
