"""The streaming logQ rule (include/mf_hip.h ``mf_logq_update``) restated in numpy float32 -- what the device
state is held to bit for bit.

State per bucket h: ``last_seen[h]`` (int32, 0 = never) and ``gap[h]`` (fp32, 0 = never); a step number t >= 1, strictly
increasing.  One update with the ids of a batch touches every DISTINCT bucket once::

    old = last_seen[h];  g = float32(t - old)                  (round to nearest even)
    gap[h] = g                                  if old == 0
             fl(fl((1 - a) gap[h]) + fl(a g))   otherwise      (1 - a computed once in fp32)
    last_seen[h] = t

A bucket whose ``last_seen`` already is t is left alone (a second update with the same t changes nothing).  Read-out:
``logq(id) = -log(D)``; direct mode (``num_hashes = 0``) D = gap[id], ids outside [0, n_buckets) ignored and read 0.0;
hashed mode D = the largest gap among the id's ``num_hashes`` buckets, negative ids ignored; any bucket never seen: 0.0.
"""
from __future__ import annotations

import numpy as np

GOLDEN_GAMMA = np.uint64(0x9E3779B97F4A7C15)


def splitmix64(z: np.ndarray) -> np.ndarray:
    """SplitMix64's output function (include/mf_numerics.h ``mf_splitmix64``; splitmix64(GOLDEN_GAMMA) = 0xE220A8397B1DCDAF is
    the known answer of tests/test_host_cpu.py)."""
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def hash_buckets(ids, num_hashes: int, seed: int, n_buckets: int) -> np.ndarray:
    """``[n, num_hashes]`` buckets of every id (``mf_hash_bucket``)."""
    ids = np.asarray(ids, dtype=np.int64).astype(np.uint64)
    with np.errstate(over="ignore"):
        z = ids[:, None] + np.uint64(seed) + (np.arange(num_hashes, dtype=np.uint64)[None, :] + np.uint64(1)) * GOLDEN_GAMMA
    return (splitmix64(z) % np.uint64(n_buckets)).astype(np.int64)


class Spec:
    def __init__(self, n_buckets: int, *, alpha: float = 0.01, num_hashes: int = 0, seed: int = 0, bucket_fn=None) -> None:
        self.n_buckets, self.num_hashes, self.seed = int(n_buckets), int(num_hashes), int(seed)
        self.alpha = np.float32(alpha)
        self.keep = np.float32(1.0) - self.alpha
        self.bucket_fn = bucket_fn                      # (ids, num_hashes, seed, n_buckets) -> [n, H]; default: hash_buckets
        shape = (self.n_buckets,) if self.num_hashes == 0 else (self.num_hashes, self.n_buckets)
        self.last_seen = np.zeros(shape, dtype=np.int32)
        self.gap = np.zeros(shape, dtype=np.float32)

    def slots(self, ids) -> tuple[np.ndarray, np.ndarray]:
        """(flat slot of every (id, hash) [n, max(H, 1)], valid [n])."""
        ids = np.asarray(ids, dtype=np.int64).reshape(-1)
        if self.num_hashes == 0:
            ok = (ids >= 0) & (ids < self.n_buckets)
            return np.where(ok, ids, 0)[:, None], ok
        ok = ids >= 0
        fn = self.bucket_fn or hash_buckets
        b = np.asarray(fn(np.where(ok, ids, 0), self.num_hashes, self.seed, self.n_buckets), dtype=np.int64).reshape(-1, self.num_hashes)
        return b + np.arange(self.num_hashes, dtype=np.int64)[None, :] * self.n_buckets, ok

    def update(self, ids, t: int) -> np.ndarray:
        slots, ok = self.slots(ids)
        last, gap = self.last_seen.reshape(-1), self.gap.reshape(-1)
        h = np.unique(slots[ok].reshape(-1))
        h = h[last[h] != np.int32(t)]
        old = last[h]
        g = (np.int64(t) - old.astype(np.int64)).astype(np.float32)        # int -> float32: round to nearest even
        avg = (self.keep * gap[h]).astype(np.float32) + (self.alpha * g).astype(np.float32)
        gap[h] = np.where(old == 0, g, avg.astype(np.float32))
        last[h] = np.int32(t)
        return self.logq(ids)

    def gap_of(self, ids) -> np.ndarray:
        """D of every id (0.0 = no estimate)."""
        slots, ok = self.slots(ids)
        x = self.gap.reshape(-1)[slots]
        return np.where(ok & (x != 0).all(axis=1), x.max(axis=1), np.float32(0.0)).astype(np.float32)

    def logq(self, ids) -> np.ndarray:
        """float64 ``-log(D)`` (0.0 where there is no estimate): what the fp32 read-out is compared with."""
        d = self.gap_of(ids).astype(np.float64)
        return np.where(d > 0, -np.log(np.where(d > 0, d, 1.0)), 0.0)

    def table(self) -> np.ndarray:
        return self.logq(np.arange(self.n_buckets))


def inclusion_probability(p: np.ndarray, n_pos: int, n_neg: int) -> np.ndarray:
    """P(item j is among n_pos draws from p and n_neg uniform draws over len(p) items)."""
    m = len(p)
    return 1.0 - (1.0 - p) ** n_pos * (1.0 - 1.0 / m) ** n_neg
