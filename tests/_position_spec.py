"""Plain numpy restatement (fp64 / int64) of ``mf_target_positions`` and ``mf_position_metrics`` (include/mf_hip.h): what the
tests of the position path compare against.  TEST INFRASTRUCTURE -- the package does not import it.

Order: a query's admissible rows (0 <= y < N, y + idx_base not on its exclusion list) by the retrieval key of
include/mf_numerics.h -- ``mf_orderable(chain score) << 32 | ~row``, larger is better -- so score descending, row ascending.
Scores are ``oracle.chain.scores``: the fmaf chain the kernels compute bit for bit.
"""
from __future__ import annotations

import numpy as np

from oracle import chain

NAMES = ("RetrievalNormalizedDCG", "RetrievalRecall", "RetrievalPrecision", "RetrievalMAP", "RetrievalHitRate", "RetrievalMRR")
UNCUT = ("MRR", "MeanPosition", "AUC")


def orderable(s) -> np.ndarray:
    u = np.ascontiguousarray(s, dtype=np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))


def keys(scores_row) -> np.ndarray:
    n = scores_row.shape[-1]
    return (orderable(scores_row).astype(np.uint64) << np.uint64(32)) | (~np.arange(n, dtype=np.uint32)).astype(np.uint64)


def orders(scores, exclude=None, idx_base: int = 0) -> list[np.ndarray]:
    """Per query the admissible LOCAL rows, best first.  ``exclude``: per query GLOBAL rows (any, also outside the catalog)."""
    nq, n = scores.shape
    out = []
    for r in range(nq):
        adm = np.ones(n, dtype=bool)
        if exclude is not None and len(exclude[r]):
            e = np.asarray(exclude[r], dtype=np.int64) - idx_base
            adm[e[(e >= 0) & (e < n)]] = False
        rows = np.nonzero(adm)[0]
        out.append(rows[np.argsort(keys(scores[r])[rows], kind="stable")[::-1]])
    return out


def positions_from_scores(scores, tgt_off, tgt_idx, exclude=None, idx_base: int = 0):
    """``(pos int64 [T], score fp32 [T], ncand int64 [Q])`` from given fp32 scores [Q, N]."""
    nq, n = scores.shape
    tgt_off, tgt_idx = np.asarray(tgt_off, dtype=np.int64), np.asarray(tgt_idx, dtype=np.int64)
    pos = np.full(tgt_idx.shape, -1, dtype=np.int64)
    score = np.full(tgt_idx.shape, -np.inf, dtype=np.float32)
    ncand = np.zeros(nq, dtype=np.int64)
    for r, order in enumerate(orders(scores, exclude, idx_base)):
        place = np.full(n, -1, dtype=np.int64)
        place[order] = np.arange(order.size)
        ncand[r] = order.size
        for e in range(int(tgt_off[r]), int(tgt_off[r + 1])):
            y = int(tgt_idx[e]) - idx_base
            if 0 <= y < n and place[y] >= 0:
                pos[e], score[e] = place[y], scores[r, y]
    return pos, score, ncand


def positions(q, items, tgt_off, tgt_idx, exclude=None, idx_base: int = 0):
    return positions_from_scores(chain.scores(np.asarray(q), np.asarray(items)), tgt_off, tgt_idx, exclude, idx_base)


def metrics(pos, tgt_off, tgt_rel, ncand, ks) -> np.ndarray:
    """[Q, 6 len(ks) + 3] in fp64: per k the six values of ``NAMES``, then ``UNCUT``."""
    pos, tgt_off, ncand = (np.asarray(x, dtype=np.int64) for x in (pos, tgt_off, ncand))
    tgt_rel = np.asarray(tgt_rel, dtype=np.float64)
    nq, nk = ncand.size, len(ks)
    out = np.zeros((nq, 6 * nk + 3), dtype=np.float64)
    for q in range(nq):
        p, r = pos[tgt_off[q]: tgt_off[q + 1]], tgt_rel[tgt_off[q]: tgt_off[q + 1]]
        relevant = r > 0
        if not relevant.any():
            continue
        rank = np.empty(r.size, dtype=np.int64)                       # among the ratings, descending, list order among equals
        rank[np.argsort(-r, kind="stable")] = np.arange(r.size)
        placed = relevant & (p >= 0)
        above = np.array([int((placed & (p < pe)).sum()) for pe in p], dtype=np.int64)      # relevant targets placed above
        for i, k in enumerate(ks):
            ideal = (r[rank < k] / np.log2(rank[rank < k] + 2.0)).sum()
            got = (p >= 0) & (p < k)
            dcg = (r[got] / np.log2(p[got] + 2.0)).sum()
            hit = placed & (p < k)
            nh = int(hit.sum())
            o = out[q, 6 * i: 6 * i + 6]
            o[0] = dcg / ideal if ideal > 0 else 0.0
            o[1] = nh / int(relevant.sum())
            o[2] = nh / k
            if nh:
                o[3] = ((above[hit] + 1) / (p[hit] + 1)).mean()
                o[4] = 1.0
                o[5] = 1.0 / (p[hit].min() + 1)
        n_adm = int(placed.sum())
        if n_adm:
            o = out[q, 6 * nk:]
            o[0] = 1.0 / (p[placed].min() + 1)
            o[1] = p[placed].mean()
            o[2] = (1.0 - (p[placed] - above[placed]) / max(int(ncand[q]) - n_adm, 1)).mean()
    return out
