"""Cases and reference for the direct tests of the sparse row update (csrc/mf_update.h and the update half of
csrc/mf_embed.hip), driven through ``mf_update_sgd`` / ``mf_update_adam`` / ``mf_update_pair``: tests/test_gpu_update.py
runs them on the GPU, tests/test_update_cpu.py checks the plan.

A case is ``(n, n_rows, d, layout)``.  A layout is a list of run lengths for one **target** (a hash bucket of the
one-launch path; the whole list of the multi-launch path), plus filler entries in the other buckets and out-of-range ids
(-1, -7, n_rows, n_rows + 9: skipped by every path, sorted behind the valid ids by both sorts of the multi-launch path).
Keys sort by (id, batch position), so with the target's ids taken ascending, run k's head sits at sorted position
``sum(count[:k])`` of the target's list whatever the batch order: a layout places every head and every end on a chosen
position.  ``indices`` scatters the entries over the batch in a seeded random order.

Which bucket an id falls in, how many buckets a call has and which sort regime a bucket of m keys takes are MIRRORED here
from mf_update.h (``fused_bucket_bits``, ``fused_bucket``, the three branches of ``fused_update_body``), and which sort a
multi-launch call gets from ``sort_packed_posbits`` of mf_embed.hip.  The regime a case reaches is therefore planned, not
observed on the device: tests/test_update_cpu.py reads the constants out of the header and fails when they move.

Exact values: every gradient element is an integer in [-M, M] drawn per (position, channel), the initial rows are integers
in [-W, W], and ``M * longest run + W < 2^24``: every fp32 partial sum, and the SGD row ``w0 - sum g`` at lr = 1, is exact
in any order.
"""
from __future__ import annotations

import dataclasses
import functools

import numpy as np
import torch

# ---- mirrored from csrc/mf_update.h (tests/test_update_cpu.py compares them with the header) ----
FUSED_MAX_N = 65536
FUSED_CAP = 8192
FUSED_RANK_MAX = 512
FUSED_MAX_BITS = 8
RUN_CHUNK = 32
HASH_MULT = 0x9E3779B1
NF_ADAM = 12
NF_SGD = 16

WIDTHS = (32, 64, 128, 256)
MULTI_WIDTHS = (32, 256)
BUCKET_SIZES = (1, 2, 32, 33, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 8191, 8192, 8193)
N_EDGES = (1, 32, 33, 64, 65, 4096, 4097, 8192, 8193, 65535, 65536)
ROW_LENGTHS = tuple(range(1, 34))                  # each with its head at residue 0
TABLE_LENGTHS = (1, 2, 31, 32, 33, 63, 64, 65)     # each with its head at residues 0, 1, 31
TABLE_RESIDUES = (0, 1, 31)
LADDER_X = tuple(nf * a + b for nf in (NF_ADAM, NF_SGD) for a, b in ((1, -1), (1, 0), (1, 1), (2, 0), (2, 1)))
MULTI = ((65537, 32767, "packed"), (65537, 32768, "generic"), (131072, 16383, "packed"), (131072, 40000, "generic"))
# the regime each bucket size is there for, written down by hand (not computed by `regime`)
_B = lambda p: ("regime", "bitonic", p)                                            # noqa: E731
PLANNED_REGIME = {1: ("regime", "rank"), 2: ("regime", "rank"), 32: ("regime", "rank"), 33: ("regime", "rank"), 511: ("regime", "rank"),
                  512: ("regime", "rank"), 513: _B(1024), 1023: _B(1024), 1024: _B(1024), 1025: _B(2048), 2047: _B(2048), 2048: _B(2048),
                  2049: _B(4096), 8191: _B(8192), 8192: _B(8192), 8193: ("regime", "overflow")}
EXACT_LIMIT = 1 << 24
W0_MAX = 1000                                      # |initial table value|
N_ROWS = 40000                                     # the one-launch cases' table (the largest: 40,000 x 256)


def fused_bucket_bits(n: int) -> int:
    bits = 0
    while bits < FUSED_MAX_BITS and (32 << bits) < n:
        bits += 1
    return bits


def fused_bucket(ids, bits: int):
    ids = np.asarray(ids, dtype=np.int64)
    if bits == 0:
        return np.zeros(ids.shape, dtype=np.int64)
    return (((ids & 0xFFFFFFFF) * HASH_MULT) & 0xFFFFFFFF) >> (32 - bits)


def regime(m: int) -> tuple:
    """("rank",) | ("bitonic", padded size) | ("overflow",): the branch of fused_update_body a bucket of m keys takes."""
    if m <= FUSED_RANK_MAX:
        return ("rank",)
    if m <= FUSED_CAP:
        p = 1024
        while p < m:
            p <<= 1
        return ("bitonic", p)
    return ("overflow",)


def sort_packed_posbits(n: int, id_limit: int) -> int:
    """mf_embed.hip: the position bits if the packed 32-bit sort applies to (n keys, ids below id_limit), else -1."""
    if n <= 0 or n > (1 << 20) or id_limit <= 0:
        return -1
    posbits = 0
    while (1 << posbits) < n:
        posbits += 1
    return posbits if ((id_limit + 1) << posbits) <= (1 << 32) else -1


def multi_sort(n: int, n_rows: int) -> str:
    return "packed" if sort_packed_posbits(n, n_rows) >= 0 else "generic"


# ------------------------------------------------------------------------------------------------ layouts ----
class _Placer:
    """Lays runs down at chosen sorted positions; filler runs (fresh ids, at most 29 long) move the position.  `pins`:
    ``(position, [lengths])`` -- runs that must start at an absolute position; a pin is laid as soon as the next run
    would pass it."""

    def __init__(self, pins=()) -> None:
        self.counts: list[int] = []
        self.pos = 0
        self.pins = sorted(pins)

    def _lay(self, length: int) -> None:
        self.counts.append(length)
        self.pos += length

    def _fill_to(self, target: int) -> None:
        assert self.pos <= target, (self.pos, target)
        while self.pos < target:
            self._lay(min(29, target - self.pos))

    def _pins_before(self, end: int) -> None:
        while self.pins and end > self.pins[0][0]:
            at, lengths = self.pins.pop(0)
            self._fill_to(at)
            for length in lengths:
                self._lay(length)

    def run(self, length: int) -> None:
        self._pins_before(self.pos + length)
        self._lay(length)

    def head_at(self, r: int, length: int) -> None:
        """A run of `length` whose head is == r (mod RUN_CHUNK)."""
        self._pins_before(self.pos + (r - self.pos) % RUN_CHUNK + length)
        fill = (r - self.pos) % RUN_CHUNK
        if fill:
            self._lay(fill)
        self._lay(length)

    def finish(self) -> list[int]:
        """Lays the pins left, then ends the list on a multiple of RUN_CHUNK with a run of 27 whose head is at residue 5: it
        ends on the last key, and its next chunk boundary equals m."""
        self._pins_before(1 << 60)
        self.head_at(0, 5)
        self._lay(27)
        assert self.pos % RUN_CHUNK == 0
        return self.counts


def placement_counts(which: str) -> list[int]:
    """"A": the first run (preceded by nothing); every length 1..33 at residue 0; the residue-by-length table; heads at
    1023 and 1024; a run across 2048.  "B" (a head at 1024 and a run across 1024 exclude each other): the table again and a
    run across 1024."""
    if which == "A":
        p = _Placer(pins=[(1023, [1, 40]), (2040, [20])])
        p.run(3)
        for length in ROW_LENGTHS:
            p.head_at(0, length)
    else:
        p = _Placer(pins=[(1010, [40])])
        p.run(3)
    for length in TABLE_LENGTHS:
        for r in TABLE_RESIDUES:
            p.head_at(r, length)
    return p.finish()


def ladder_counts(extra: int, residue: int) -> list[int]:
    """Runs of a first chunk (32 - residue rows) and x further whole chunks, plus `extra` rows, for every x of LADDER_X;
    the last run ends on the list's last key."""
    p = _Placer()
    p.run(3)
    for x in LADDER_X:
        p.head_at(residue, (RUN_CHUNK - residue) + x * RUN_CHUNK + extra)
    return p.counts


def random_counts(rng, total: int, max_runs: int) -> list[int]:
    """`total` entries in at most max_runs runs: a random composition (short and long runs)."""
    if total == 0:
        return []
    k = int(max(1, min(max_runs, total)))
    cuts = np.sort(rng.choice(np.arange(1, total), size=k - 1, replace=False)) if k > 1 else np.zeros(0, np.int64)
    return np.diff(np.concatenate([[0], cuts, [total]])).astype(np.int64).tolist()


@dataclasses.dataclass(frozen=True)
class Spec:
    name: str
    family: str
    n: int                             # entries of the call, out-of-range ones included
    n_rows: int
    d: int
    targets: tuple                     # ((bucket or None, (count, ...)), ...): None = the whole list (multi-launch)
    n_bad: int = 0
    seed: int = 0
    claims: tuple = ()                 # what the layout is there for; tests/test_update_cpu.py checks each
    ids: tuple = ()                    # the first target's ids, if not the default choice of target_ids

    @property
    def multi(self) -> bool:
        return self.n > FUSED_MAX_N

    @property
    def bits(self) -> int:
        return fused_bucket_bits(self.n)

    @property
    def n_fill(self) -> int:
        return self.n - self.n_bad - sum(sum(c) for _, c in self.targets)

    def counts(self, t: int = 0) -> np.ndarray:
        return np.array(self.targets[t][1], dtype=np.int64)

    def heads(self, t: int = 0) -> np.ndarray:
        c = self.counts(t)
        return np.concatenate([[0], np.cumsum(c)[:-1]]).astype(np.int64)


def claim_holds(spec: Spec, claim: tuple) -> bool:
    """Recomputed from the target's counts alone."""
    kind = claim[0]
    counts, heads = spec.counts(), spec.heads()
    ends = heads + counts
    m = int(counts.sum())
    if kind == "m":                                      # ("m", m): the target's size
        return m == claim[1]
    if kind == "regime":                                 # ("regime", "rank") | ("regime", "bitonic", padded size) | ("regime", "overflow")
        return regime(m) == tuple(claim[1:])
    if kind == "n":
        return spec.n == claim[1]
    if kind == "runs>":                                  # many runs, not one
        return len(counts) > claim[1]
    if kind == "one_run":
        return len(counts) == 1
    if kind == "head":                                   # ("head", L, r): a run of length L with head == r (mod 32)
        return bool(((counts == claim[1]) & (heads % RUN_CHUNK == claim[2])).any())
    if kind == "head_at":                                # ("head_at", position)
        return bool((heads == claim[1]).any())
    if kind == "across":                                 # ("across", position): head < position < end
        return bool(((heads < claim[1]) & (ends > claim[1])).any())
    if kind == "first":                                  # the first run: preceded by nothing
        return int(heads[0]) == 0
    if kind == "ends_last":                              # a run ends on the list's last key, behind other runs
        return len(counts) > 1 and int(ends[-1]) == m
    if kind == "long_ends_last":                         # ... a run of several chunks
        return int(ends[-1]) == m and int(counts[-1]) > RUN_CHUNK
    if kind == "chunk_end_is_m":                         # a run whose next chunk boundary equals m
        return bool(((heads // RUN_CHUNK + 1) * RUN_CHUNK == m).any())
    if kind == "ladder":                                 # ("ladder", x, extra, r)
        _, x, extra, r = claim
        return bool(((heads % RUN_CHUNK == r) & (counts == (RUN_CHUNK - r) + x * RUN_CHUNK + extra)).any())
    if kind == "longest":                                # ("longest", L): a run of exactly L, not first, not last
        at = np.nonzero(counts == claim[1])[0]
        return len(at) > 0 and 0 < int(at[0]) < len(counts) - 1
    if kind == "block":                                  # a run of exactly 32 on a boundary
        return bool(((counts == RUN_CHUNK) & (heads % RUN_CHUNK == 0)).any())
    if kind == "bad_behind":                             # out-of-range entries behind the last valid position
        return spec.n_bad > 0
    if kind == "no_bad":                                 # the last run ends at n - 1
        return spec.n_bad == 0 and spec.n_fill == 0
    if kind == "two_overflow":
        return len(spec.targets) == 2 and all(sum(c) > FUSED_CAP for _, c in spec.targets)
    if kind == "sort":                                   # ("sort", "packed" | "generic")
        return spec.multi and multi_sort(spec.n, spec.n_rows) == claim[1]
    raise ValueError(claim)


def _placement_claims(which: str) -> list[tuple]:
    claims = [("first",), ("ends_last",), ("chunk_end_is_m",)]
    claims += [("head", length, r) for length in TABLE_LENGTHS for r in TABLE_RESIDUES]
    if which == "A":
        claims += [("head", length, 0) for length in ROW_LENGTHS]
        claims += [("head_at", 1023), ("head_at", 1024), ("across", 2048)]
    else:
        claims += [("across", 1024)]
    return claims


def _bucket(bits: int, k: int = 5) -> int:
    """The target bucket: in the middle of the range, so that filled calls have keys in lower and in higher buckets."""
    return ((1 << bits) * k) // 8


def _one(name, family, d, counts, n_fill=0, n_bad=0, seed=0, claims=(), n_rows=N_ROWS, k=5) -> Spec:
    n = int(sum(counts)) + n_fill + n_bad
    return Spec(name, family, n, n_rows, d, ((_bucket(fused_bucket_bits(n), k), tuple(int(c) for c in counts)),), n_bad=n_bad,
                seed=seed, claims=(("m", int(sum(counts))), *claims))


def ids_of_bucket(n_rows: int, bits: int, bucket: int) -> np.ndarray:
    ids = np.arange(n_rows, dtype=np.int64)
    return ids[fused_bucket(ids, bits) == bucket]


def _max_runs(n: int, n_rows: int = N_ROWS) -> int:
    """Ids a bucket of a call of n entries certainly has (the hash spreads 40,000 consecutive ids within 4 % of even)."""
    return int(0.9 * n_rows) >> fused_bucket_bits(n)


@functools.lru_cache(maxsize=None)
def specs() -> tuple[Spec, ...]:
    out: list[Spec] = []
    # bucket sizes: every key of the call in one bucket (and four out-of-range ids); filled for two widths above 2,000
    for mi, m in enumerate(BUCKET_SIZES):
        for di, d in enumerate(WIDTHS):
            seed = 1000 + 4 * mi + di
            rng = np.random.default_rng(seed)
            n_bad = 0 if m <= 2 else 4
            n_fill = 500 if m >= 2047 and d in (64, 256) else 0
            if m <= 33:
                counts, claims = [m], [("one_run",)]
            else:
                counts = random_counts(rng, m, min(_max_runs(m + n_bad + n_fill), m // 40 + 3))
                claims = [("runs>", 3)]
            out.append(_one(f"bucket-{m}-d{d}", "bucket", d, counts, n_fill, n_bad, seed, [PLANNED_REGIME[m], *claims]))
    for di, d in enumerate(WIDTHS):
        out.append(_one(f"bucket-9000-one-run-d{d}", "bucket", d, [9000], 0, 4, 1100 + di, [("regime", "overflow"), ("one_run",)]))
        # two buckets over 8192 in one call of 65,536: their segments of the global lists must not overlap
        rng = np.random.default_rng(1200 + di)
        a, b = random_counts(rng, 8193, 100), random_counts(rng, 8300, 90)
        bits = fused_bucket_bits(65536)
        out.append(Spec(f"two-overflow-d{d}", "bucket", 65536, N_ROWS, d, ((_bucket(bits, 2), tuple(a)), (_bucket(bits, 6), tuple(b))),
                        n_bad=16, seed=1200 + di, claims=(("m", 8193), ("regime", "overflow"), ("n", 65536), ("two_overflow",))))
    # n on the bucket-count edges: a target of two runs (one longer than a chunk), the rest spread over every bucket
    for ni, n in enumerate(N_EDGES):
        for di, d in enumerate(WIDTHS):
            n_bad = 4 if n >= 32 else 0
            counts = [1] if n == 1 else [5, 23] if n <= 33 else [7, 37]
            out.append(_one(f"n-{n}-d{d}", "n", d, counts, n - n_bad - sum(counts), n_bad, 2000 + 4 * ni + di, [("regime", "rank"), ("n", n)]))
    # run placement inside one sorted list (A: ~2,500 keys; B: ~1,400), the rest of 4,000 entries in other buckets
    for which in "AB":
        counts = placement_counts(which)
        for di, d in enumerate(WIDTHS):
            out.append(_one(f"placement-{which}-d{d}", "placement", d, counts, 4000 - sum(counts) - 8, 8, 3000 + di + 10 * (which == "B"),
                            [_B(4096 if which == "A" else 2048), *_placement_claims(which)]))
    # the second-pass ladder: 1 + x chunks, x around NF and 2 NF for both NF; + one row; a short first chunk
    for extra in (0, 1):
        for residue in (0, 5):
            counts = ladder_counts(extra, residue)
            claims = [_B(8192)] + [("ladder", x, extra, residue) for x in LADDER_X] + [("long_ends_last",)]
            for di, d in enumerate(WIDTHS):
                out.append(_one(f"ladder-e{extra}-r{residue}-d{d}", "ladder", d, counts, 300, 4, 4000 + di + 10 * extra + 20 * residue, claims))
    # multi-launch: placement A in the global sorted order, a run of 9,000, a run of exactly 32 on a boundary, random runs,
    # and a run of 70 on the last valid position
    for ci, (n, n_rows, sort) in enumerate(MULTI):
        for di, d in enumerate(MULTI_WIDTHS):
            seed = 5000 + 2 * ci + di
            rng = np.random.default_rng(seed)
            n_bad = 0 if (n, n_rows, d) == (131072, 16383, 256) else 37
            p = _Placer()
            p.counts = placement_counts("A")
            p.pos = sum(p.counts)
            p.run(9000)
            p.head_at(0, 32)
            rest = n - n_bad - p.pos - 70
            counts = p.counts + random_counts(rng, rest, min(n_rows - len(p.counts) - 1, rest // 5)) + [70]
            claims = _placement_claims("A")[:1] + _placement_claims("A")[3:] + [
                ("n", n), ("sort", sort), ("longest", 9000), ("block",), ("long_ends_last",), ("bad_behind",) if n_bad else ("no_bad",)]
            out.append(Spec(f"multi-{n}-{n_rows}-d{d}", "multi", n, n_rows, d, ((None, tuple(int(c) for c in counts)),), n_bad=n_bad,
                            seed=seed, claims=tuple(claims)))
    names = [s.name for s in out]
    assert len(set(names)) == len(names)
    return tuple(out)


def spec_named(name: str) -> Spec:
    return next(s for s in specs() if s.name == name)


# mf_update_pair: table A one bucket (n_a = 20), table B 256 buckets of which one overflows (n_b = 8193); the same ids
PAIR_N_A, PAIR_N_B = 20, 8193


@functools.lru_cache(maxsize=None)
def pair_specs() -> tuple[tuple[Spec, Spec], ...]:
    out = []
    for di, d in enumerate(MULTI_WIDTHS):
        rng = np.random.default_rng(6100 + di)
        b_counts = random_counts(rng, 8192, 60) + [1]                   # 8,193 entries, none out of range: every key in one bucket
        b = _one(f"pair-b-d{d}", "pair", d, b_counts, 0, 0, 6100 + di, [("regime", "overflow"), ("n", PAIR_N_B)])
        tb = target_ids(b)                                              # A's three ids are ids of B's list
        a = dataclasses.replace(_one(f"pair-a-d{d}", "pair", d, [1, 13, 2], 0, 4, 6000 + di, [("regime", "rank"), ("n", PAIR_N_A)]),
                                ids=(int(tb[0]), int(tb[len(tb) // 2]), int(tb[-1])))
        out.append((a, b))
    return tuple(out)


# ------------------------------------------------------------------------------------------------- inputs ----
def target_ids(spec: Spec, t: int = 0) -> np.ndarray:
    """The ids of target t's runs, ascending: spread over the table's ids that hash to the bucket, the first and the last one
    included (multi-launch: over the whole table, 0 and n_rows - 1 included)."""
    bucket, counts = spec.targets[t]
    if spec.ids and t == 0:
        assert len(spec.ids) == len(counts) and list(spec.ids) == sorted(set(spec.ids))
        return np.array(spec.ids, dtype=np.int64)
    pool = np.arange(spec.n_rows, dtype=np.int64) if bucket is None else ids_of_bucket(spec.n_rows, spec.bits, bucket)
    assert len(counts) <= len(pool), (spec.name, len(counts), len(pool))
    pick = np.unique(np.linspace(0, len(pool) - 1, num=len(counts)).round().astype(np.int64))
    if len(pick) < len(counts):                                             # (rounding met twice: fill from the front)
        pick = np.union1d(pick, np.setdiff1d(np.arange(len(pool)), pick)[: len(counts) - len(pick)])
    return pool[pick]


def bad_ids(spec: Spec) -> np.ndarray:
    return np.resize(np.array([-1, -7, spec.n_rows, spec.n_rows + 9], dtype=np.int64), spec.n_bad)


def indices(spec: Spec) -> np.ndarray:
    """The id list of the call: the targets' runs, filler ids of the other buckets (drawn with repeats), out-of-range ids,
    in a seeded random order."""
    rng = np.random.default_rng(spec.seed)
    parts = [np.repeat(target_ids(spec, t), spec.counts(t)) for t in range(len(spec.targets))]
    if spec.n_fill:
        ids = np.arange(spec.n_rows, dtype=np.int64)
        b = fused_bucket(ids, spec.bits)
        pool = ids[~np.isin(b, [bk for bk, _ in spec.targets])]
        assert len(pool) > 0, spec.name
        parts.append(rng.choice(pool, size=spec.n_fill, replace=True))
    parts.append(bad_ids(spec))
    idx = np.concatenate(parts)
    assert len(idx) == spec.n, (spec.name, len(idx))
    return idx[rng.permutation(spec.n)]


def magnitude(idx: np.ndarray, n_rows: int) -> int:
    """M of the module docstring, from the longest run of the list."""
    valid = idx[(idx >= 0) & (idx < n_rows)]
    longest = int(np.bincount(valid).max()) if len(valid) else 1
    return int(min(1000, (EXACT_LIMIT - 1 - W0_MAX) // longest))


def build(spec: Spec, steps: int = 2) -> dict:
    """The raw inputs of the call as numpy arrays: ids, one gradient per step (integers; NaN in the rows of out-of-range
    ids, which no path may read into a sum), the initial table (integers, no zero row)."""
    idx = indices(spec)
    rng = np.random.default_rng(spec.seed + 77)
    m = magnitude(idx, spec.n_rows)
    bad = (idx < 0) | (idx >= spec.n_rows)
    grads = []
    for _ in range(steps):
        g = rng.integers(-m, m + 1, size=(spec.n, spec.d), dtype=np.int32).astype(np.float32)
        g[bad] = np.nan
        grads.append(g)
    w0 = rng.integers(-W0_MAX, W0_MAX + 1, size=(spec.n_rows, spec.d), dtype=np.int32).astype(np.float32)
    w0[:, 0] = np.where(w0[:, 0] == 0, 1, w0[:, 0])
    return {"n": spec.n, "n_rows": spec.n_rows, "d": spec.d, "idx": idx, "grads": grads, "w0": w0, "M": m}


# ---------------------------------------------------------------------------------------------- reference ----
def reference(idx, grad, n_rows: int) -> tuple[torch.Tensor, torch.Tensor]:
    """(unique valid ids ascending, int64 sums of their gradient rows): an index_add over the valid entries, compact (one row
    per id present).  Reads nothing but the raw inputs."""
    idx = torch.as_tensor(idx)
    grad = torch.as_tensor(grad)
    valid = (idx >= 0) & (idx < n_rows)
    uniq, inv = torch.unique(idx[valid], return_inverse=True)
    rows = grad[valid]
    as_int = rows.to(torch.int64)
    assert torch.equal(as_int.to(rows.dtype), rows), "the exact cases' gradients are integers"
    sums = torch.zeros(len(uniq), grad.shape[1], dtype=torch.int64, device=idx.device)
    sums.index_add_(0, inv, as_int)
    return uniq, sums


def presummed(uniq: torch.Tensor, sums: torch.Tensor, n_rows: int, pad_to: int = 0) -> tuple[torch.Tensor, torch.Tensor]:
    """The list of unique ids with the exact summed rows (fp32: every sum is below 2^24), padded with out-of-range ids (NaN
    rows) up to pad_to entries so that a multi-launch case's pre-summed list takes the multi-launch path too."""
    g = sums.to(torch.float32)
    assert torch.equal(g.to(torch.int64), sums)
    n_pad = max(0, pad_to - len(uniq))
    if n_pad == 0:
        return uniq, g
    pad = torch.tensor([-1, -7, n_rows, n_rows + 9], dtype=torch.int64, device=uniq.device).repeat(n_pad // 4 + 1)[:n_pad]
    return torch.cat([uniq, pad]), torch.cat([g, torch.full((n_pad, g.shape[1]), float("nan"), dtype=torch.float32, device=g.device)])
