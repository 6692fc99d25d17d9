"""Inputs of the retrieval-metrics tests around k = 64, where the kernel goes from one rank per lane to several
(tests/test_gpu_topk_merge.py; tests/golden/make_metrics_seam_golden.py writes the k <= 64 outputs once)."""
from __future__ import annotations

import numpy as np

KS = (1, 63, 64, 65, 128, 1024)
GOLDEN_KS = (1, 63, 64)            # one rank per lane: the outputs are pinned bit for bit
Q = 7
N_ITEMS = 5000


def seam_case(k: int):
    """``(topk [Q, k] int64, offsets [Q + 1], target ids, target ratings, targets as dicts)``.  Query 0 has no targets; 1 has
    half its list empty and more missed targets than free slots; 2 retrieved min(60, k - 1) items and misses ten targets,
    which take ranks 60 .. 69 -- across rank 64 when k allows; 3 found every target; 4 has tied ratings (zeros among them);
    5 and 6 are random, 6 with a hundred targets (more than one per lane) and a short list."""
    g = np.random.default_rng(1000 + k)
    topk = np.stack([g.permutation(N_ITEMS)[:k] for _ in range(Q)]).astype(np.int64)
    topk[1, k // 2:] = -1
    n2 = min(60, k - 1)
    topk[2, n2:] = -1
    topk[6, (3 * k) // 4:] = -1
    targets = []
    for r in range(Q):
        got = [int(i) for i in topk[r] if i >= 0]
        fresh = [int(i) for i in g.permutation(N_ITEMS) if int(i) not in set(got)]
        if r == 0:
            own, rat = [], []
        elif r == 1:
            own = fresh[: k // 2 + 5] + got[:2]
            rat = g.integers(1, 6, len(own)).tolist()
        elif r == 2:
            own = got[:2] + fresh[:10]
            rat = g.integers(1, 6, len(own)).tolist()
        elif r == 3:
            own = got[:: max(1, k // 9)]
            rat = g.integers(1, 6, len(own)).tolist()
        elif r == 4:
            own = got[1::3][:12] + fresh[:6]
            rat = [3, 3, 0, 3, 5, 5, 0, 3][: len(own)] + [3] * max(0, len(own) - 8)
        else:
            m = 25 if r == 5 else 100
            own = list(dict.fromkeys(got[: m // 3] + fresh[: m - m // 3]))
            rat = g.integers(0, 6, len(own)).tolist()
        order = g.permutation(len(own))                      # list order is the rank order of missed targets: not sorted
        own, rat = [own[i] for i in order], [float(rat[i]) for i in order]
        targets.append(dict(zip(own, rat)))
    off = np.cumsum([0] + [len(t) for t in targets]).astype(np.int64)
    ids = np.array([i for t in targets for i in t], dtype=np.int64)
    rel = np.array([v for t in targets for v in t.values()], dtype=np.float32)
    return topk, off, ids, rel, targets
