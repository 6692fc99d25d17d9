"""What the deep cell scan (csrc/mf_ivf_deep.hip, ``PartitionedIndex.search(path="cells_deep")``) is held to beyond
tests/_ivf_spec.py, shared by tests/test_ivf_deep_cpu.py and tests/test_gpu_ivf_deep.py: the buffer's constants read out of the
source, the buffer's bookkeeping ("kept / waiting / threshold") restated in a few lines, the one-cell catalog whose scan settles
several times, and the deep case set.  The result spec itself is ``_ivf_spec.expected`` -- it takes any k."""
from __future__ import annotations

import functools
import pathlib
import re

import numpy as np

from tests import _ivf_spec as ivf

ROOT = pathlib.Path(__file__).resolve().parents[1]
SOURCE = ROOT / "matrix-factorization-torch_amd" / "csrc" / "mf_ivf_deep.hip"
MERGE_KEYS = 16384          # MF_TOPK_MERGE_DEEP_MAX_KEYS: G * k keys of a query in the deep merge
MAX_K = 1024                # MF_TOPK_DEEP_MAX_K
DEPTHS = (1, 64, 65, 128, 129, 256, 257, 512, 513, 1000, 1024)


@functools.lru_cache(maxsize=None)
def constants() -> dict[str, int]:
    """``static constexpr int IVFD_* = <number>;`` of the unit's header part (IVFD_PASS is written as a product there)."""
    text = SOURCE.read_text()
    out = {name: int(value) for name, value in re.findall(r"static constexpr int (IVFD_\w+) = (\d+);", text)}
    assert "static constexpr int IVFD_PASS = 64 * MF_CELLS_NW;" in text
    out["IVFD_PASS"] = 256
    return out


def kept(k: int) -> int:
    """``ivfd_kept``: the power of two >= k, ``IVFD_KP_MIN`` at least."""
    kp = constants()["IVFD_KP_MIN"]
    while kp < k:
        kp *= 2
    return kp


def capacity(kp: int) -> int:
    """``ivfd_capacity``: the keys of the buffer a scan with kept part ``kp`` uses."""
    return max(4 * kp, constants()["IVFD_BUF_MIN"])


def walk(scores: np.ndarray, k: int) -> dict:
    """The buffer of one workgroup over the rows of its slice in cell order (``scores``: one per row, all distinct, every row
    admitted): passes of ``IVFD_PASS`` rows; a row's key waits when it beats the bound; when more than ``capacity - kept -
    IVFD_PASS`` keys wait, a settle keeps the k best and the bound becomes the k-th of them (0 while fewer are held).
    ``settles``: per settle ``(keys waiting, the bound was live before it)``; ``best``: the positions the walk keeps, best
    first."""
    c = constants()
    kp = kept(k)
    room = capacity(kp) - kp - c["IVFD_PASS"]
    held: list[tuple[float, int]] = []                       # (score, -position): the larger tuple is the better key
    waiting: list[tuple[float, int]] = []
    bound = None
    settles = []

    def settle():
        nonlocal held, waiting, bound
        settles.append((len(waiting), bound is not None))
        assert kp + len(waiting) <= capacity(kp) <= c["IVFD_BUF"]
        held = sorted(held + waiting, reverse=True)[:k]
        waiting = []
        bound = held[k - 1] if len(held) >= k else None

    for p0 in range(0, len(scores), c["IVFD_PASS"]):
        for pos in range(p0, min(p0 + c["IVFD_PASS"], len(scores))):
            key = (float(scores[pos]), -pos)
            if bound is None or key > bound:
                waiting.append(key)
        if len(waiting) > room:
            settle()
    if waiting:
        settle()
    return {"settles": settles, "best": [-p for _, p in held]}


# ---------------------------------------------------------------------------------------- the cell of several settles ----
SETTLE_DIM = 32
SETTLE_ORDERS = ("ascending", "descending", "shuffled")


def settle_rows() -> int:
    """Rows of the one-cell catalog: three times the buffer's capacity and a ragged rest (a last block of 40 rows)."""
    return 3 * constants()["IVFD_BUF"] + 1000


def settle_scores(order: str) -> np.ndarray:
    """Distinct fp32 scores in (0, 1] along the cell order.  The catalog's row i is ``scores[i] * e0`` and the query ``e0``, so
    the chain's score of row i is ``fma(scores[i], 1, 0)`` and then sums of zeros: ``scores[i]`` to the bit."""
    n = settle_rows()
    up = (np.arange(1, n + 1, dtype=np.float64) / n).astype(np.float32)
    assert np.unique(up).size == n
    if order == "ascending":
        return up
    if order == "descending":
        return up[::-1].copy()
    return up[np.random.default_rng(7).permutation(n)]


def top_of(scores: np.ndarray, lo: int, hi: int, k: int) -> np.ndarray:
    """numpy's top-k of rows ``[lo, hi)``: score descending, row ascending; the rows, at most k."""
    rows = np.arange(lo, hi)
    order = np.lexsort((rows, -scores[lo:hi].astype(np.float64)))
    return rows[order[:k]]


# ------------------------------------------------------------------------------------------------------ the case set ----
@functools.lru_cache(maxsize=None)
def cases() -> dict[str, ivf.Case]:
    out = [
        ivf.make("deep_w32_k65", 32, 1000, 33, 16, 3, 65),
        ivf.make("deep_w48_k128", 48, 1000, 33, 16, 8, 128),                            # a padded width
        ivf.make("deep_w64_k129", 64, 2500, 70, 37, 3, 129, lengths=(0, 1, 17, 1025)),
        ivf.make("deep_w128_k256_all_cells", 128, 2500, 1, 37, 37, 256),
        ivf.make("deep_w256_k257_all_cells", 256, 1000, 33, 16, 16, 257),
        ivf.make("deep_k512", 64, 5000, 3, 16, 8, 512),
        ivf.make("deep_k513_all_cells", 32, 5000, 33, 16, 16, 513),
        ivf.make("deep_k1000_tail", 64, 2500, 3, 4, 1, 1000),                          # about 610 rows under the probe: a tail
        ivf.make("deep_k1024", 128, 5000, 1, 8, 8, 1024, lengths=(1025,)),
        ivf.make("deep_k1", 64, 1000, 70, 16, 1, 1, lengths=None),
        ivf.make("deep_k64_fewer_rows", 64, 33, 70, 4, 4, 64),
        ivf.make("deep_idx_base", 64, 1000, 33, 4, 3, 100, idx_base=1000),
        ivf.make("deep_nprobe16_of_37", 64, 2500, 33, 37, 16, 65),
    ]
    sizes = [0, 1, 63, 64, 65] + ivf._spread(1000 - 193, 11)
    for nprobe in (3, 16):                     # query 0 is the empty cell's centroid: that cell is probed at nprobe = 3 too
        c = ivf.make(f"deep_cell_sizes_nprobe{nprobe}", 64, 1000, 33, 16, nprobe, 100, sizes=sizes)
        c.q[0] = c.centroids[0]
        out.append(c)
    c = ivf.make("deep_all_but_three", 64, 1000, 3, 4, 1, 100, lengths=None)
    c.exclude = []
    for p in ivf.probes(c.q, c.centroids, 1):
        c.exclude.append(np.nonzero(np.isin(c.assign, p))[0][3:].tolist())
    out.append(c)
    # 1,100 identical rows dealt over four cells of 625 rows (ten blocks: two slices each), the query is that row
    c = ivf.make("deep_ties_k1024", 64, 2500, 2, 4, 4, 1024, sizes=[625] * 4, lengths=(0, 5))
    c.items[:1100] = c.items[0]
    c.assign[:1100] = np.arange(1100) % 4
    c.q[0] = c.items[0]
    out.append(c)
    c = ivf.make("deep_zero_query", 32, 1000, 3, 16, 3, 100)                            # every score 0: rows in order, cells 0, 1, 2
    c.q[1] = 0.0
    out.append(c)
    return {c.name: c for c in out}
