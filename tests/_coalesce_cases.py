"""Cases and reference for the direct tests of the shared gradient coalesce (csrc/mf_coalesce.h, mf_coalesce.hip), driven
through ``mf_pool_backward``: tests/test_gpu_coalesce.py runs them on the GPU, tests/test_coalesce_cpu.py checks the plan.

A case is a **run layout**: ``[(id, count), ...]`` ascending in id.  The sort is stable and padding keys sort last, so the
head of run k sits at sorted position ``sum(count[:k])`` whatever the entry order: a layout places every head and every
end on a chosen position.  ``build`` scatters the entries in a seeded random order over the explicit rows (extras) and
the pooled entries of hand-made owners, sprinkles padding entries, and returns the raw ABI inputs as numpy arrays.
``reference`` reads nothing but those inputs and follows the header comment of ``mf_pool_backward`` in include/mf_hip.h.

Exact cases: every gradient value is an integer in [-M, M] times 1, 1/2 or 1/4, with ``4 M * longest run < 2^24``, so
that four times any partial sum is an integer below 2^24: every fp32 sum is exact in any order.
"""
from __future__ import annotations

import dataclasses
import functools

import numpy as np
import torch

LENGTHS = (1, 2, 3, 4, 5, 31, 32, 33, 1023, 1024, 1025, 32767, 32768, 32769)       # run lengths of the issue's table
HEADS = ((0, 32), (1, 32), (31, 32), (1023, 1024))                                 # head position == r (mod m)
ENTRY_COUNTS = (1, 2, 255, 256, 257, 4095, 4096, 4097, 8192, 3 * 4096 + 1, 64 * 4096 - 1, 64 * 4096, 64 * 4096 + 1)
TABLES = (2, 255, 256, 257, 65535, 65536, 65537, 1 << 20)                          # n_rows
WIDTHS = (32, 64, 128, 256)
PASS_TABLE = {1: 255, 2: 257, 3: 65537}                                            # the table a family uses per pass count
EXACT_LIMIT = 1 << 24
RADIX_TILE = 4096
SCAN_SWEEP = 16384                                                                 # counters per sweep of the scan kernel


def radix_passes(n_rows: int) -> int:
    """The rule of coalesce_sort's comment: keys 0 .. n_rows (n_rows marks an entry that carries nothing), 8-bit digits."""
    bits = 1
    while (1 << bits) <= n_rows:
        bits += 1
    return (bits + 7) // 8


def id_pool(n_rows: int, k: int, pooled_only: bool = False) -> list[int]:
    """k ids of the table, ascending.  In order of priority: 0 (valid as an extra id only), 1, n_rows - 1, 2 (1 and 2 differ in
    the bottom digit only), 1 + top (1 and 1 + top differ in the top digit only; top = 256^(passes - 1)), the ids around
    top, then ids spread over the table."""
    top = 1 << (8 * (radix_passes(n_rows) - 1))
    first = [0, 1, n_rows - 1, 2, 1 + top, top, top - 1, top + 1, 1 + 2 * top, 1 + 3 * top, n_rows - 2]
    spread = [int(x) for x in np.linspace(0, n_rows - 1, num=min(2 * k, n_rows))]
    ids: list[int] = []
    seen = set()
    for i in first + spread + list(range(min(n_rows, 3 * k + 16))):
        if 0 <= i < n_rows and i not in seen and not (pooled_only and i == 0):
            seen.add(i)
            ids.append(i)
        if len(ids) == k:
            break
    assert len(ids) == k, (n_rows, k)
    return sorted(ids)


class _Placer:
    """Lays runs down at chosen sorted positions; filler runs (fresh ids) move the position."""

    def __init__(self) -> None:
        self.counts: list[int] = []
        self.pos = 0

    def run(self, length: int) -> None:
        self.counts.append(length)
        self.pos += length

    def head_at(self, r: int, m: int, length: int) -> None:
        fill = (r - self.pos) % m
        if fill:
            self.run(fill)
        self.run(length)

    def end_at(self, m: int, length: int) -> None:
        self.head_at((-length) % m, m, length)

    def layout(self, n_rows: int) -> list[tuple[int, int]]:
        return list(zip(id_pool(n_rows, len(self.counts)), self.counts))


def boundary_counts(lengths=LENGTHS) -> list[int]:
    """Every length at every head residue of HEADS; runs that end exactly on a 32 / 1024 / 32768 boundary (head inside a
    unit); runs that start exactly on one and go past the next; a run across a 4096 tile edge."""
    p = _Placer()
    p.run(3)                                                     # the first valid run: preceded by nothing
    for length in lengths:
        for r, m in HEADS:
            p.head_at(r, m, length)
    top = max(lengths)
    for m in (32, 1024, 32768):
        if m < top:
            p.end_at(m, m // 2 + 3)                              # ends on the boundary, head inside the unit
            p.end_at(m, m + 5)                                   # ... and after crossing one
            p.head_at(0, m, m + 1)                               # the head is a block start; one entry in the next block
            p.head_at(0, m, m)                                   # exactly one block
    p.head_at(RADIX_TILE - 6, RADIX_TILE, 33)                    # across a tile edge
    p.head_at(RADIX_TILE - 1, RADIX_TILE, 2)                     # the edge between the run's two entries
    p.head_at(0, RADIX_TILE, 1)                                  # a head that is a tile's first position
    p.run(4)
    return p.counts


def random_counts(rng, n_valid: int, max_runs: int) -> list[int]:
    """n_valid entries in at most max_runs runs: a random composition (short and long runs)."""
    if n_valid == 0:
        return []
    k = int(min(max_runs, n_valid, max(1, n_valid // 7)))
    cuts = np.sort(rng.choice(np.arange(1, n_valid), size=k - 1, replace=False)) if k > 1 else np.zeros(0, np.int64)
    return np.diff(np.concatenate([[0], cuts, [n_valid]])).astype(np.int64).tolist()


@dataclasses.dataclass(frozen=True)
class Spec:
    name: str
    family: str
    n_rows: int
    d: int
    layout: tuple                      # ((id, count), ...) ascending in id
    mode: int = 0                      # 0: mean with count in {1, 2, 4}; 1: max with a hand-made arg
    owners: str = "mixed"              # "one" (B = 1), "each" (one entry per owner), "mixed" (0, 1, many; empties everywhere)
    values: str = "exact"              # "exact" | "float"
    source: str = "both"               # "both" | "extras" (pooled: nothing) | "pooled" (extra_* null, n_extra = 0)
    n_pad: int = 0                     # padding entries sprinkled among the valid ones
    seed: int = 0
    claims: tuple = ()                 # what the layout is there for; tests/test_coalesce_cpu.py checks each

    @property
    def counts(self) -> np.ndarray:
        return np.array([c for _, c in self.layout], dtype=np.int64)

    @property
    def n_valid(self) -> int:
        return int(self.counts.sum())

    @property
    def n(self) -> int:
        return self.n_valid + self.n_pad

    @property
    def heads(self) -> np.ndarray:
        return np.concatenate([[0], np.cumsum(self.counts)[:-1]]).astype(np.int64) if self.layout else np.zeros(0, np.int64)

    @property
    def longest(self) -> int:
        return int(self.counts.max()) if self.layout else 1

    @property
    def magnitude(self) -> int:
        """M of the module docstring: the largest |integer| of an exact case's gradient values."""
        return int(min(1000, (EXACT_LIMIT - 1) // (4 * self.longest)))

    @property
    def passes(self) -> int:
        return radix_passes(self.n_rows)


def claim_holds(spec: Spec, claim: tuple) -> bool:
    """Recomputed from the counts alone."""
    kind = claim[0]
    heads, counts = spec.heads, spec.counts
    ends = heads + counts
    if kind == "head":                                   # ("head", L, r, m): a run of length L with head == r (mod m)
        _, length, r, m = claim
        return bool(((counts == length) & (heads % m == r)).any())
    if kind == "end":                                    # ("end", m): a run that ends on a multiple of m, head inside a unit
        m = claim[1]
        return bool(((ends % m == 0) & (heads % m != 0)).any())
    if kind == "start":                                  # ("start", m): a head on a multiple of m, the run longer than m
        m = claim[1]
        return bool(((heads % m == 0) & (counts > m)).any())
    if kind == "block":                                  # ("block", m): a run that is exactly one aligned block of m
        m = claim[1]
        return bool(((heads % m == 0) & (counts == m)).any())
    if kind == "tile":                                   # a run across a 4096 edge, its head not on the edge
        return bool(((heads // RADIX_TILE != (ends - 1) // RADIX_TILE) & (heads % RADIX_TILE != 0)).any())
    if kind == "n":                                      # ("n", n): the entry count, padding included
        return spec.n == claim[1]
    if kind == "longest>":
        return spec.longest > claim[1] and spec.n > claim[1] and len(spec.layout) >= 3 and \
            int(np.argmax(counts)) not in (0, len(counts) - 1)
    if kind == "saturated":                              # every id of the table, n >= n_rows
        return [i for i, _ in spec.layout] == list(range(spec.n_rows)) and spec.n >= spec.n_rows
    if kind == "last_at_end":                            # no padding: the last run ends at n - 1
        return spec.n_pad == 0 and spec.n_valid > 0
    if kind == "padding_follows":
        return spec.n_pad > 0 and spec.n_valid > 0
    if kind == "nothing":
        return spec.n_valid == 0 and spec.n_pad > 0
    if kind == "ids":                                    # runs on 0, 1, n_rows - 1 and digit neighbours
        ids = {i for i, _ in spec.layout}
        top = 1 << (8 * (spec.passes - 1))
        want = {0, 1, spec.n_rows - 1}
        if spec.n_rows > 2:
            want |= {2}                                  # 1, 2: the bottom digit only
        if spec.passes > 1 and 1 + top < spec.n_rows:
            want |= {1 + top}                            # 1, 1 + top: the top digit only
        return want <= ids
    if kind == "scan_sweeps":                            # ("scan_sweeps", k): the histogram (256 per tile) takes k sweeps
        tiles = -(-max(spec.n, 1) // RADIX_TILE)
        return -(-256 * tiles // SCAN_SWEEP) == claim[1]
    raise ValueError(claim)


def _boundary_spec(name, family, n_rows, d, lengths, **kw) -> Spec:
    counts = boundary_counts(lengths)
    p = _Placer()
    p.counts = counts
    claims = [("head", length, r, m) for length in lengths for r, m in HEADS]
    claims += [c for m in (32, 1024, 32768) if m < max(lengths) for c in (("end", m), ("start", m), ("block", m))]
    claims += [("tile",), ("last_at_end",) if kw.get("n_pad", 0) == 0 else ("padding_follows",)]
    return Spec(name, family, n_rows, d, tuple(p.layout(n_rows)), claims=tuple(claims), **kw)


def _random_spec(name, family, n_rows, d, n, seed, claims=(), n_pad=None, **kw) -> Spec:
    rng = np.random.default_rng(seed)
    n_pad = (n // 16 if n >= 16 else 0) if n_pad is None else n_pad
    pooled_only = kw.get("source", "both") == "pooled"
    counts = random_counts(rng, n - n_pad, min(n_rows - pooled_only, 4000))
    ids = id_pool(n_rows, len(counts), pooled_only)
    return Spec(name, family, n_rows, d, tuple(zip(ids, counts)), seed=seed, n_pad=n_pad, claims=(("n", n), *claims), **kw)


@functools.lru_cache(maxsize=None)
def specs() -> tuple[Spec, ...]:
    out: list[Spec] = []
    owners3, medium = ("mixed", "one", "each"), tuple(x for x in LENGTHS if x <= 1025)   # noqa: PLR2004
    # boundaries: every run length x head residue, ends / starts on unit boundaries, tile edges; every d x pass count
    for pi, (ps, n_rows) in enumerate(PASS_TABLE.items()):
        for di, d in enumerate(WIDTHS):
            k = pi + di
            out.append(_boundary_spec(f"boundaries-p{ps}-d{d}", "boundaries", n_rows, d, LENGTHS, mode=k % 2, owners=owners3[k % 2],
                                      n_pad=0 if k % 3 == 0 else 37 + k, seed=100 + k))
            out.append(_boundary_spec(f"float-p{ps}-d{d}", "float", n_rows, d, medium, values="float", mode=(k + 1) % 2,
                                      owners=owners3[(k + 1) % 3], n_pad=0 if k % 3 == 1 else 21 + k, seed=200 + k))
    out.append(_boundary_spec("float-long-p3-d32", "float", 65537, 32, LENGTHS, values="float", n_pad=5, seed=250))
    out.append(_boundary_spec("float-long-p1-d256", "float", 255, 256, LENGTHS, values="float", mode=1, n_pad=5, seed=251))
    # tables: every n_rows of the issue at every d; runs on 0, 1, n_rows - 1 and digit neighbours
    for ti, n_rows in enumerate(TABLES):
        for di, d in enumerate(WIDTHS):
            k = ti + di
            out.append(_random_spec(f"table-{n_rows}-d{d}", "tables", n_rows, d, 3000 + 17 * k, 300 + k, claims=(("ids",),),
                                    mode=k % 2, owners=owners3[k % 3]))
    # entry counts: each n under a 1-, 2- and 3-pass table, at d = 32 and 256 (and 64 / 128 in turn)
    for ni, n in enumerate(ENTRY_COUNTS):
        for j, d in enumerate((32, 256, (64, 128)[ni % 2])):
            ps = (ni + j) % 3 + 1
            sweeps = -(-256 * -(-n // RADIX_TILE) // SCAN_SWEEP)
            out.append(_random_spec(f"count-{n}-p{ps}-d{d}", "counts", PASS_TABLE[ps], d, n, 400 + 3 * ni + j,
                                    claims=(("scan_sweeps", sweeps),), mode=(ni + j) % 2,
                                    owners="each" if n <= 8192 and j == 0 else "mixed"))        # noqa: PLR2004
    # the top level: one run of more than 2^20 entries, short runs before and after it.  These are most of the file's wall
    # time, so there is one per distinct code path: the two ends of the run sums' lane layout, an odd and an even pass count.
    for ps, d in ((3, 32), (2, 256)):
        n_rows = PASS_TABLE[ps]
        ids = id_pool(n_rows, 7)
        counts = [5, 32, (1 << 20) + 4097 + ps, 33, 1]
        lay = tuple(zip([ids[1], ids[2], ids[len(ids) // 2], ids[-2], ids[-1]], counts))
        out.append(Spec(f"giant-p{ps}-d{d}", "giant", n_rows, d, lay, mode=0, owners="mixed", n_pad=9, seed=500 + ps,
                        claims=(("longest>", 1 << 20), ("n", sum(counts) + 9))))
    # saturation: every id of the table present, n >= n_rows: U == capacity, no -1 slot
    for n_rows in (255, 257):
        for di, d in enumerate(WIDTHS):
            rng = np.random.default_rng(600 + n_rows + d)
            lay = tuple((i, int(c)) for i, c in enumerate(rng.integers(1, 6, n_rows)))
            out.append(Spec(f"saturated-{n_rows}-d{d}", "saturated", n_rows, d, lay, mode=di % 2, owners=owners3[di % 3],
                            n_pad=di * 3, seed=600 + di, claims=(("saturated",),)))
    # nothing valid: only padding entries
    for si, source in enumerate(("extras", "pooled", "both")):
        for d, n_rows in ((32, 255), (256, 65537), (64, 257)):
            out.append(Spec(f"nothing-{source}-{n_rows}-d{d}", "nothing", n_rows, d, (), mode=si % 2, source=source,
                            n_pad=(1, 70, 4097)[si], seed=700 + si, claims=(("nothing",),)))
    # owners and modes: every owner shape under both modes, every pass count
    for oi, owners in enumerate(owners3):
        for mode in (0, 1):
            for ps, d in ((1, 256), (2, 32), (3, 128)):
                out.append(_random_spec(f"owners-{owners}-m{mode}-p{ps}-d{d}", "owners", PASS_TABLE[ps], d, 6000 + oi, 800 + oi + 3 * mode,
                                        mode=mode, owners=owners))
    # the smallest table: ids 0 and 1 only
    for d in WIDTHS:
        out.append(Spec(f"two-rows-d{d}", "tables", 2, d, ((0, 33), (1, 1025)), mode=d // 32 % 2, n_pad=8, seed=900 + d,
                        claims=(("ids",), ("head", 1025, 1, 32))))
        out.append(Spec(f"two-rows-pooled-d{d}", "tables", 2, d, ((1, 4097),), source="pooled", owners="each", n_pad=3, seed=950 + d,
                        claims=(("n", 4100),)))
    names = [s.name for s in out]
    assert len(set(names)) == len(names)
    return tuple(out)


HOST_BOUND_CASES = ("float-p1-d32", "float-p2-d256", "float-p3-d64", "float-p3-d32", "float-p1-d256", "float-p2-d128")


def spec_named(name: str) -> Spec:
    return next(s for s in specs() if s.name == name)


# ------------------------------------------------------------------------------------------------- inputs ----
def _sprinkle(rng, valid: np.ndarray, pads: list[int], n_pad: int) -> np.ndarray:
    """`valid` in order with n_pad padding ids at random places."""
    out = np.empty(len(valid) + n_pad, dtype=np.int64)
    at = np.zeros(len(out), dtype=bool)
    at[rng.choice(len(out), size=n_pad, replace=False)] = True
    out[at] = np.resize(np.array(pads, dtype=np.int64), n_pad) if n_pad else []
    out[~at] = valid
    return out


def _owner_lengths(rng, total: int, owners: str) -> np.ndarray:
    if owners == "one" or total == 0:
        return np.array([total], dtype=np.int64)
    if owners == "each":
        return np.ones(total, dtype=np.int64)
    draw = rng.choice(np.array([0, 0, 1, 1, 2, 3, 7, 40, 300, 5000]), size=total // 50 + 16)
    cs = np.cumsum(draw)
    if cs[-1] < total:
        mid = np.concatenate([draw, [total - cs[-1]]])
    else:
        k = int(np.searchsorted(cs, total))                       # the first owner that reaches the total: cut it there
        mid = draw[: k + 1].copy()
        mid[-1] -= cs[k] - total
    half = len(mid) // 2
    return np.concatenate([np.zeros(3, np.int64), mid[:half], np.zeros(4, np.int64), mid[half:], np.zeros(3, np.int64)]).astype(np.int64)


def build(spec: Spec) -> dict:
    """The ABI inputs of one call (numpy; `torch_inputs` moves them): see the module docstring."""
    rng = np.random.default_rng(spec.seed)
    n_rows, d = spec.n_rows, spec.d
    ids = np.repeat(np.array([i for i, _ in spec.layout], dtype=np.int64), spec.counts) if spec.layout else np.zeros(0, np.int64)
    ids = ids[rng.permutation(len(ids))]                                             # the entry order
    if spec.source == "extras":
        to_extra = np.ones(len(ids), dtype=bool)
    elif spec.source == "pooled":
        assert not (ids == 0).any()
        to_extra = np.zeros(len(ids), dtype=bool)
    else:
        to_extra = (ids == 0) | (rng.random(len(ids)) < 0.3)
    pad_e = {"extras": spec.n_pad, "pooled": 0, "both": spec.n_pad // 3}[spec.source]
    pad_p = spec.n_pad - pad_e
    extra_ids = _sprinkle(rng, ids[to_extra], [-1, n_rows], pad_e)
    pooled = _sprinkle(rng, ids[~to_extra], [0, -3, n_rows, n_rows + 5, 2 ** 40], pad_p)
    # owners: lengths, entry numbering (repeats for empty owners), list positions with gaps (as after a max_history cut)
    lengths = _owner_lengths(rng, len(pooled), spec.owners)
    n_own = len(lengths)
    ent_off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    gaps = rng.choice(np.array([0, 0, 1, 3]), size=n_own)
    lo = (ent_off[:-1] + np.cumsum(gaps)).astype(np.int64)
    owner_of = np.repeat(np.arange(n_own), lengths)
    junk = 1 if n_rows > 1 else 0                                                    # a VALID id between the owners' ranges
    items = np.full(len(pooled) + int(gaps.sum()) + 2, junk, dtype=np.int64)
    items[lo[owner_of] + (np.arange(len(pooled)) - ent_off[owner_of])] = pooled
    # gradients
    m = spec.magnitude
    if spec.values == "exact":
        grad_p = rng.integers(-m, m + 1, size=(n_own, d)).astype(np.float32)
        extra_grad = rng.integers(-m, m + 1, size=(len(extra_ids), d)).astype(np.float32)
    else:
        grad_p = rng.standard_normal((n_own, d), dtype=np.float32)
        extra_grad = rng.standard_normal((len(extra_ids), d), dtype=np.float32)
    extra_grad[(extra_ids < 0) | (extra_ids >= n_rows)] = np.nan                     # rows the call must never read into a sum
    count = rng.choice(np.array([1, 2, 4], dtype=np.int32), size=n_own)
    arg = None
    if spec.mode == 1:                                                               # each channel picks one of the owner's valid entries
        valid = (pooled >= 1) & (pooled < n_rows)
        valid_h = np.nonzero(valid)[0]
        nv = np.bincount(owner_of[valid], minlength=n_own)
        vstart = np.concatenate([[0], np.cumsum(nv)])[:-1]
        pick = np.minimum((rng.random((n_own, d)) * nv[:, None]).astype(np.int64), np.maximum(nv[:, None] - 1, 0))
        has = nv > 0
        arg = np.full((n_own, d), -1, dtype=np.int32)
        if len(valid_h):
            chosen = valid_h[np.minimum(vstart[:, None] + pick, len(valid_h) - 1)] - ent_off[:-1, None]
            arg[has] = chosen[has].astype(np.int32)
    inp = {"n_rows": n_rows, "d": d, "mode": spec.mode, "items": items, "B": n_own, "lo": lo, "ent_off": ent_off, "count": count,
           "arg": arg, "grad_p": grad_p, "n_entries": int(ent_off[-1]), "extra_ids": extra_ids, "extra_grad": extra_grad,
           "n_extra": len(extra_ids)}
    if spec.source == "pooled":
        assert len(extra_ids) == 0
        inp["extra_ids"] = inp["extra_grad"] = None
    return inp


def input_bytes(inp: dict) -> int:
    return sum(v.nbytes for v in inp.values() if isinstance(v, np.ndarray))


def torch_inputs(inp: dict, device) -> dict:
    return {k: torch.from_numpy(v).to(device) if isinstance(v, np.ndarray) else v for k, v in inp.items()}


# ---------------------------------------------------------------------------------------------- reference ----
def entry_ids(t: dict) -> tuple[torch.Tensor, torch.Tensor]:
    """(id, valid) of every entry, extras first, as the header numbers them."""
    n_rows, n_own = t["n_rows"], t["B"]
    dev = t["items"].device
    h = torch.arange(int(t["ent_off"][n_own]), device=dev)
    owner = torch.searchsorted(t["ent_off"][:n_own].contiguous(), h, right=True) - 1           # the last b with ent_off[b] <= h
    pooled = t["items"][t["lo"][owner] + (h - t["ent_off"][owner])]
    if t["n_extra"]:
        ex = t["extra_ids"]
        return torch.cat([ex, pooled]), torch.cat([(ex >= 0) & (ex < n_rows), (pooled >= 1) & (pooled < n_rows)])
    return pooled, (pooled >= 1) & (pooled < n_rows)


def entry_rows(t: dict, q0: int, q1: int) -> torch.Tensor:
    """fp32 gradient rows of entries [q0, q1): an explicit row; grad_p[b] / count[b] (mode 0; count a power of two here, so
    the quotient is exact); grad_p[b] on the channels where arg[b] names the entry (mode 1)."""
    n_extra, n_own = t["n_extra"], t["B"]
    parts = []
    if q0 < n_extra:
        parts.append(t["extra_grad"][q0:min(q1, n_extra)])
    if q1 > n_extra:
        h = torch.arange(max(q0, n_extra) - n_extra, q1 - n_extra, device=t["items"].device)
        owner = torch.searchsorted(t["ent_off"][:n_own].contiguous(), h, right=True) - 1
        g = t["grad_p"][owner]
        if t["mode"] == 0:
            parts.append(g / t["count"][owner].float()[:, None])
        else:
            j = (h - t["ent_off"][owner]).to(torch.int32)
            parts.append(torch.where(t["arg"][owner] == j[:, None], g, torch.zeros_like(g)))
    return torch.cat(parts) if len(parts) > 1 else parts[0]


def reference(t: dict, chunk: int = 1 << 16):
    """(unique valid ids ascending, their fp64 sums, the fp64 sums of |g|, the run lengths): per id, the index_add_ of the
    issue, kept compact (one row per id present, not per table row) so that a 2^20-row table costs nothing."""
    ids, valid = entry_ids(t)
    uniq, inv, counts = torch.unique(ids[valid], return_inverse=True, return_counts=True)
    slot = torch.full_like(ids, -1)
    slot[valid] = inv
    want = torch.zeros(len(uniq), t["d"], dtype=torch.float64, device=ids.device)
    mass = torch.zeros_like(want)
    for q0 in range(0, len(ids), chunk):
        q1 = min(q0 + chunk, len(ids))
        v = valid[q0:q1]
        if bool(v.any()):
            r = entry_rows(t, q0, q1)[v].double()
            want.index_add_(0, slot[q0:q1][v], r)
            mass.index_add_(0, slot[q0:q1][v], r.abs())
    return uniq, want, mass, counts


def gamma(run_len: torch.Tensor) -> torch.Tensor:
    """(L - 1) u / (1 - (L - 1) u), u = 2^-24: the bound of an fp32 sum of L terms in any order (Higham, ASNA 4.2)."""
    u = 2.0 ** -24
    k = (run_len.double() - 1) * u
    return k / (1 - k)
