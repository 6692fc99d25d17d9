"""CPU: positions over a row-sharded catalog -- the host side of ``mf_target_words`` / ``mf_key_positions`` (csrc/mf_topk_deep.hip:
exports, workspace sizes, every refusal, the new kernels' resources, the record that the refactor left the existing kernels
alone), the numpy spec of the sharded rule (tests/_sharded_position_spec.py) against the unsharded one
(tests/_position_spec.py), and ``ShardedIndex.positions`` / ``compute(comm=...)`` over gloo with the oracle as local compute."""
from __future__ import annotations

import ctypes
import importlib
import importlib.util
import json
import os
import pathlib

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import _position_spec as spec
from tests import _sharded_position_spec as sspec
from tests import test_distributed_cpu as tdc

ROOT = pathlib.Path(__file__).resolve().parents[1]
FAKE = ctypes.c_void_p(0x1000)
BIG = ctypes.c_size_t(2**40)
EXPORTS = ("mf_target_words", "mf_key_positions_ws_bytes", "mf_key_positions_min_ws_bytes", "mf_key_positions")


# --------------------------------------------------------------------------------------------- exports and refusals ----
def test_exports_are_declared_bound_and_present(mf):
    lib = mf._lib.lib()
    header = (ROOT / "include" / "mf_hip.h").read_text()
    for name in EXPORTS:
        assert hasattr(lib, name) and name in mf._lib.SIGNATURES and name + "(" in header, name


def test_workspace_is_the_positions(mf):
    lib = mf._lib.lib()
    for q in (1, 31, 32, 33, 1024, 65_536):
        for n in (1, 31, 33, 62_423, 8_400_000):
            for d in (32, 64, 128, 256):
                assert lib.mf_key_positions_ws_bytes(q, n, d) == lib.mf_target_positions_ws_bytes(q, n, d) > 0, (q, n, d)
                assert lib.mf_key_positions_min_ws_bytes(q, n, d) == lib.mf_target_positions_min_ws_bytes(q, n, d) > 0, (q, n, d)
    for q, n, d in ((0, 10, 64), (-1, 10, 64), (4, 0, 64), (4, 10, 48), (4, 1 << 31, 64), (4, 40_000_000, 64)):
        assert lib.mf_key_positions_ws_bytes(q, n, d) == 0 and lib.mf_key_positions_min_ws_bytes(q, n, d) == 0, (q, n, d)


@pytest.fixture
def words(mf):
    lib = mf._lib.lib()

    def run(q=FAKE, Q=4, items=FAKE, N=1000, d=64, to=FAKE, ti=FAKE, nt=10, stride=1, offset=0, out=FAKE):
        rc = lib.mf_target_words(q, Q, items, N, d, to, ti, nt, stride, offset, out, None)
        return rc, (lib.mf_last_error() if rc else b"")

    return run


@pytest.fixture
def count(mf):
    lib = mf._lib.lib()

    def run(q=FAKE, Q=4, items=FAKE, N=1000, d=64, to=FAKE, ti=FAKE, tw=FAKE, nt=10, stride=1, offset=0, eo=None, ei=None, ws=FAKE, wsb=BIG,
            oa=FAKE, os_=FAKE, oc=FAKE):
        rc = lib.mf_key_positions(q, Q, items, N, d, to, ti, tw, nt, stride, offset, eo, ei, ws, wsb, oa, os_, oc, None)
        return rc, (lib.mf_last_error() if rc else b"")

    return run


@pytest.mark.parametrize("kw", [dict(q=None), dict(items=None), dict(to=None), dict(ti=None), dict(out=None), dict(Q=0), dict(Q=-3), dict(N=0),
                                dict(N=-1), dict(nt=-1), dict(stride=0), dict(stride=-2), dict(offset=-1)], ids=str)
def test_words_refuses_bad_arguments(mf, words, kw):
    rc, msg = words(**kw)
    assert rc == mf._lib.MF_EINVAL and msg.startswith(b"mf_target_words: bad argument"), (kw, rc, msg)


def test_words_other_refusals_and_their_order(mf, words):
    E = mf._lib
    for kw, code, text in ((dict(d=48), E.MF_EINVAL, b"mf_target_words: embedding width 48 not in {32,64,128,256}"),
                           (dict(d=16), E.MF_EINVAL, b"mf_target_words: embedding width 16 not in {32,64,128,256}"),
                           (dict(N=1 << 31), E.MF_ENOTSUP, b"mf_target_words: item indices must fit 32 bits"),
                           # pointers and sizes, then the width, then 32-bit rows
                           (dict(q=None, d=48), E.MF_EINVAL, b"mf_target_words: bad argument"),
                           (dict(stride=0, N=1 << 31), E.MF_EINVAL, b"mf_target_words: bad argument"),
                           (dict(d=48, N=1 << 31), E.MF_EINVAL, b"mf_target_words: embedding width 48")):
        rc, msg = words(**kw)
        assert rc == code and msg.startswith(text), (kw, rc, msg)


@pytest.mark.parametrize("kw", [dict(q=None), dict(items=None), dict(to=None), dict(ti=None), dict(tw=None), dict(ws=None), dict(oa=None),
                                dict(os_=None), dict(oc=None), dict(Q=0), dict(Q=-3), dict(N=0), dict(N=-1), dict(nt=-1), dict(stride=0),
                                dict(stride=-2), dict(offset=-1)], ids=str)
def test_key_positions_refuses_bad_arguments(mf, count, kw):
    rc, msg = count(**kw)
    assert rc == mf._lib.MF_EINVAL and msg.startswith(b"mf_key_positions: bad argument"), (kw, rc, msg)


@pytest.mark.parametrize("kw,code,text", [
    (dict(d=48), "MF_EINVAL", b"mf_key_positions: embedding width 48 not in {32,64,128,256}"),
    (dict(d=16), "MF_EINVAL", b"mf_key_positions: embedding width 16 not in {32,64,128,256}"),
    (dict(eo=FAKE), "MF_EINVAL", b"mf_key_positions: excl_off/excl_idx mismatch"),
    (dict(ei=FAKE), "MF_EINVAL", b"mf_key_positions: excl_off/excl_idx mismatch"),
    (dict(N=1 << 31), "MF_ENOTSUP", b"mf_key_positions: item indices must fit 32 bits"),
    (dict(N=40_000_000), "MF_ENOTSUP", b"mf_key_positions: a 32-query score slab of 40000000 columns exceeds the descriptor limit"),
    (dict(wsb=ctypes.c_size_t(0)), "MF_ENOSPC", b"mf_key_positions: workspace too small"),
], ids=lambda x: str(x) if isinstance(x, dict) else None)
def test_key_positions_refusals_have_the_positions_codes(mf, count, kw, code, text):
    rc, msg = count(**kw)
    assert rc == getattr(mf._lib, code) and msg.startswith(text), (kw, rc, msg)


def test_key_positions_refusal_order_and_the_workspace_floor(mf, count):
    E, lib = mf._lib, mf._lib.lib()
    low = lib.mf_key_positions_min_ws_bytes(4, 1000, 64)
    rc, msg = count(wsb=ctypes.c_size_t(low - 1))
    assert rc == E.MF_ENOSPC and msg.startswith(b"mf_key_positions: workspace too small")
    # pointers and sizes (the shard map among them), width, 32-bit rows, the exclusion pair, geometry, workspace: mf_target_positions' order
    for kw, code, text in ((dict(q=None, d=48), E.MF_EINVAL, b"bad argument"), (dict(nt=-1, N=1 << 31), E.MF_EINVAL, b"bad argument"),
                           (dict(stride=0, d=48), E.MF_EINVAL, b"bad argument"), (dict(offset=-1, wsb=ctypes.c_size_t(0)), E.MF_EINVAL, b"bad argument"),
                           (dict(d=48, N=1 << 31), E.MF_EINVAL, b"embedding width 48"), (dict(N=1 << 31, eo=FAKE), E.MF_ENOTSUP, b"must fit 32 bits"),
                           (dict(eo=FAKE, wsb=ctypes.c_size_t(0)), E.MF_EINVAL, b"excl_off/excl_idx mismatch"),
                           (dict(N=40_000_000, wsb=ctypes.c_size_t(0)), E.MF_ENOTSUP, b"descriptor limit")):
        rc, msg = count(**kw)
        assert rc == code and text in msg, (kw, rc, msg)


# ------------------------------------------------------------------------------------------------- kernel resources ----
def test_new_kernels_have_no_spill_and_no_scratch():
    s = importlib.util.spec_from_file_location("kernel_resources", ROOT / "tools" / "kernel_resources.py")
    kr = importlib.util.module_from_spec(s)
    s.loader.exec_module(kr)
    res = kr.kernel_resources()
    count = {n: r for n, r in res.items() if "shard_key_count_kernel" in n}
    words = {n: r for n, r in res.items() if "shard_words_kernel" in n}
    assert len(count) == 1 and len(words) == 4, (sorted(count), sorted(words))       # one counting kernel; one words kernel per width
    for name, r in {**count, **words}.items():
        assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, (name, r)
        assert r["group_segment_fixed_size"] <= 64 * 1024, (name, r)
        for taken in ("target_positions_kernel", "position_metrics_kernel", "topk_deep_", "retrieval_metrics_kernel"):
            assert taken not in name, name                   # existing tests count kernels by these names


def test_the_refactor_is_on_record():
    """profiles/sharded_positions_digest_{parent,branch}.json: ``tools/kernel_resources.py --text-digest
    --only=target_positions_kernel,topk_deep_`` on a build of the parent commit and of this one.  Every kernel of the parent is
    there on the branch; where a kernel's instruction text is not reproduced, DESIGN says so by name and points at the timing
    that stands in for it (profiles/sharded_position_probe.json)."""
    parent, branch = (json.loads((ROOT / "profiles" / f"sharded_positions_digest_{which}.json").read_text()) for which in ("parent", "branch"))
    assert set(parent) == set(branch) and len(parent) == 7, sorted(parent)          # select, excl, four slab widths, positions
    design = (ROOT / "DESIGN.md").read_text()
    for name in parent:
        kernel = name.split("(")[0].split()[-1].split("<")[0]
        if parent[name]["text_sha256"] == branch[name]["text_sha256"]:
            continue
        assert kernel == "target_positions_kernel", name    # the engines' kernels are not touched by the refactor
        assert f"`{kernel}`'s instruction text is not reproduced" in design, name
        assert (ROOT / "profiles" / "sharded_position_probe.json").exists()
        for fld in ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size"):
            assert branch[name][fld] == 0, (name, fld)
        assert branch[name]["group_segment_fixed_size"] == parent[name]["group_segment_fixed_size"]
        assert branch[name]["vgpr_count"] <= parent[name]["vgpr_count"] and branch[name]["sgpr_count"] <= parent[name]["sgpr_count"], name


# ------------------------------------------------------------------------------------- the spec of the sharded rule ----
def _unit(n, d, gen):
    return torch.nn.functional.normalize(torch.randn(n, d, generator=gen), dim=-1).numpy()


def _planted(n, d=32, nq=6, seed=0):
    """Queries, catalog, target CSR and exclusion lists with every planted case: a run of equal scores that spans the shards, a
    zero query, targets that are excluded, outside the catalog on both sides and duplicated, an empty list."""
    g = torch.Generator().manual_seed(seed + n)
    rng = np.random.default_rng(seed + n)
    q, items = _unit(nq, d, g), _unit(n, d, g)
    run = np.sort(rng.choice(n, size=min(n, max(3, n // 3)), replace=False))
    items[run] = items[run[0]]                                # equal scores in every query: the global row decides
    q[1] = 0.0                                                # every score +0: the whole catalog is one run
    excl = [sorted(set(rng.integers(-3, n + 3, int(rng.integers(0, max(2, n // 4)))).tolist())) for _ in range(nq)]
    excl[3] = list(range(n))                                  # nothing admissible
    lists = []
    for r in range(nq):
        own = rng.integers(0, n, int(rng.integers(1, 12))).tolist() + run[:4].tolist() + [int(run[-1])]
        own += [y for y in excl[r] if 0 <= y < n][:2]         # excluded
        own += [-1, -5, n, n + 7, own[0], own[0]]             # outside on both sides; duplicates
        lists.append(own)
    lists[4] = []
    t_off = np.cumsum([0] + [len(x) for x in lists])
    t_ids = np.array([y for x in lists for y in x], dtype=np.int64)
    return q, items, t_off, t_ids, excl


@pytest.mark.parametrize("deal", [sspec.round_robin, sspec.contiguous], ids=lambda f: f.__name__)
@pytest.mark.parametrize("shards", [1, 2, 3, 8])
@pytest.mark.parametrize("n", [9, 101])
def test_the_sharded_rule_equals_positions_on_the_whole_catalog(n, shards, deal):
    q, items, t_off, t_ids, excl = _planted(n)
    layout = deal(n, shards)
    assert sorted(np.concatenate([sspec.rows_of(sh) for sh in layout]).tolist()) == list(range(n))
    if n == 9 and shards == 8:
        assert min(sh[2] for sh in layout) == 1               # a shard of one row
    for ex in (excl, None):
        want = spec.positions(q, items, t_off, t_ids, ex)
        got = sspec.sharded_positions(q, items, layout, t_off, t_ids, ex)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2])
        assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
    assert (want[0] == -1).any() and (want[0] >= 0).any()
    zero = want[0][t_off[1]: t_off[2]]                        # the zero query without exclusions: a row's place is its number
    assert np.array_equal(zero, np.where((t_ids[t_off[1]: t_off[2]] >= 0) & (t_ids[t_off[1]: t_off[2]] < n), t_ids[t_off[1]: t_off[2]], -1))


def test_hand_worked_bounds():
    rr = (4, 1, 5)                                            # round-robin, shard 1 of 4: global rows 1, 5, 9, 13, 17
    assert [sspec.bound(g, rr) for g in (-7, 0, 1, 2, 5, 6, 8, 9, 17, 18, 1000)] == [0, 0, 0, 1, 1, 2, 2, 2, 4, 5, 5]
    assert [sspec.local_row(g, rr) for g in (-7, 0, 1, 2, 5, 17, 21)] == [-1, -1, 0, -1, 1, 4, -1]
    blk = (1, 10, 3)                                          # a contiguous block: global rows 10, 11, 12
    assert [sspec.bound(g, blk) for g in (-1, 9, 10, 11, 12, 13, 99)] == [0, 0, 0, 1, 2, 3, 3]
    assert [sspec.local_row(g, blk) for g in (9, 10, 12, 13)] == [-1, 0, 2, -1]
    one = (8, 7, 1)                                           # a shard of one row: global row 7
    assert [sspec.bound(g, one) for g in (0, 7, 8, 15)] == [0, 0, 1, 1]
    # counts: the shard's rows hold words 5 5 3 5 0 (row 4 excluded); a target with word 5 from elsewhere
    scores = np.array([[1.0, 1.0, 0.5, 1.0, 1.0]], dtype=np.float32)
    w = int(spec.orderable(np.float32(1.0)))
    for g, above in ((0, 0), (1, 0), (3, 1), (5, 1), (7, 2), (11, 2), (14, 3), (16, 3), (17, -1), (18, 3), (99, 3)):
        got = sspec.shard_counts(scores, [0, 1], [g], [w], rr, [[4]])
        assert got[0].tolist() == [above] and got[2].tolist() == [4], (g, got)
    low = int(spec.orderable(np.float32(0.5)))                # below the 1.0s, tied with row 2 (global row 9)
    assert [sspec.shard_counts(scores, [0, 1], [g], [low], rr, [[4]])[0][0] for g in (8, 9, 10)] == [3, 3, 4]
    assert sspec.shard_counts(scores, [0, 1], [3], [0], rr)[0].tolist() == [-1]          # word 0: no shard holds the row


# ------------------------------------------------------------------------------------------------- gloo plumbing ----
class SpecOps(tdc.OracleOps):
    """``OracleOps`` + the two shard calls of the position path, by the numpy spec."""

    @staticmethod
    def _shard(items, stride, offset):
        return (int(stride), int(offset), items.shape[0])

    @staticmethod
    def _lists(csr, nq):
        off, ids = (t.numpy() for t in csr)
        return [ids[off[r]: off[r + 1]].tolist() for r in range(nq)]

    def target_words(self, queries, items, targets_csr, stride, offset):
        scores = spec.chain.scores(queries.numpy(), items.numpy())
        t_off, t_ids = (t.numpy() for t in targets_csr)
        return torch.from_numpy(sspec.shard_words(scores, t_off, t_ids, self._shard(items, stride, offset)))

    def key_positions(self, queries, items, targets_csr, words, stride, offset, exclude_local_csr):
        scores = spec.chain.scores(queries.numpy(), items.numpy())
        t_off, t_ids = (t.numpy() for t in targets_csr)
        local = None if exclude_local_csr is None else self._lists(exclude_local_csr, queries.shape[0])
        return tuple(torch.from_numpy(x) for x in sspec.shard_counts(scores, t_off, t_ids, words.numpy(), self._shard(items, stride, offset), local))


TARGET_LENGTHS = (0, 1, 3, 9, 20)


def _case_inputs(rank: int):
    """What ``tdc._topk_case`` draws (catalog, queries, exclusion lists), and target lists of 0, 1, 3, 9 and 20 entries."""
    g = torch.Generator().manual_seed(5)
    items = torch.nn.functional.normalize(torch.randn(tdc.N_ITEMS, tdc.DIM, generator=g), dim=-1)
    gq = torch.Generator().manual_seed(50 + rank)
    q = torch.nn.functional.normalize(torch.randn(5, tdc.DIM, generator=gq), dim=-1)
    excl = [sorted(set(torch.randint(0, tdc.N_ITEMS, (int(n),), generator=gq).tolist())) for n in (0, 3, 9, 1, 20)]
    rng = np.random.default_rng(70 + rank)
    lists = [rng.integers(-2, tdc.N_ITEMS + 2, n).tolist() for n in TARGET_LENGTHS]
    lists[2][0] = excl[2][0]                                  # an excluded target
    lists[4][1] = lists[4][0]                                 # a duplicate
    rel = rng.integers(0, 6, sum(TARGET_LENGTHS)).astype(np.float32)
    return items, q, excl, lists, rel


def _csr(lists):
    off = torch.tensor([0] + list(np.cumsum([len(e) for e in lists])), dtype=torch.int64)
    return off, torch.tensor([i for e in lists for i in e], dtype=torch.int64)


def _positions_case(rank: int, world: int, out_dir: str) -> None:
    mf = importlib.import_module("matrix-factorization-torch_amd")
    mfd = mf.distributed
    items, q, excl, lists, rel = _case_inputs(rank)
    e_off, e_ids = _csr(excl)
    targets = _csr(lists)
    index = mfd.ShardedIndex(items[rank::world].contiguous(), rank, tdc.N_ITEMS, stride=world, ops=SpecOps())
    exact = index.positions(q, targets, exclude_csr=(e_off, e_ids))
    padded = mfd.ShardedIndex(items[rank::world].contiguous(), rank, tdc.N_ITEMS, stride=world, ops=SpecOps())
    capped = padded.positions(q, targets, exclude_csr=(e_off, e_ids.clone()), exclude_capacity=40, target_capacity=40)
    assert all(torch.equal(a, b) for a, b in zip(exact, capped))
    bare = index.positions(q, targets)                        # no exclusion lists
    with pytest.raises(ValueError, match="target_capacity"):
        padded.positions(q, targets, target_capacity=8)
    with pytest.raises(ValueError, match="exclude_capacity"):
        padded.positions(q, targets, exclude_csr=(e_off, e_ids.clone()), exclude_capacity=8, target_capacity=40)
    with pytest.raises(ValueError, match="one target list per query"):
        index.positions(q[:4], targets)
    none = index.positions(q, (torch.zeros(6, dtype=torch.int64), torch.zeros(0, dtype=torch.int64)), exclude_csr=(e_off, e_ids))
    assert none[0].numel() == 0 and none[1].numel() == 0 and torch.equal(none[2], exact[2])
    # the search beside it still gathers (and caches) the same exclusion lists
    s, i = index.search(q, tdc.K, exclude_csr=(e_off, e_ids))
    # metrics: this rank's own means, and the means over all ranks' queries -- the same numbers on every rank
    pm = mf.retrieval.PositionMetrics((3, 20))
    rm = mf.retrieval.RetrievalMetrics(tdc.K)
    comm = mfd.TorchComm()
    assert all(float(v) == 0.0 for m in (pm, rm) for v in m.compute(comm=comm).values())          # nobody has seen a query
    per_query = torch.from_numpy(spec.metrics(exact[0].numpy(), targets[0].numpy(), rel, exact[2].numpy(), (3, 20))).to(torch.float32)
    pm._sum, pm._n = per_query.sum(dim=0, dtype=torch.float64), 5        # (``update`` is a device kernel: feed its sums)
    list_rows = torch.from_numpy(np.random.default_rng(rank).random((5, 6))).to(torch.float32)
    rm._sum, rm._n = list_rows.sum(dim=0, dtype=torch.float64), 5
    if rank == world - 1:                                     # the last rank saw twice the queries
        pm._sum, pm._n, rm._sum, rm._n = pm._sum * 2, 10, rm._sum * 2, 10
    torch.save({"exact": exact, "bare": bare, "s": s, "i": i, "pm_own": pm.compute(), "pm_all": pm.compute(comm=comm), "rm_all": rm.compute(comm=comm),
                "pm_rows": per_query, "rm_rows": list_rows}, f"{out_dir}/pos_{rank}.pt")


def _worker(rank: int, world: int, port: int, fn: str, out_dir: str) -> None:
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        globals()[fn](rank, world, out_dir)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 4])
def test_sharded_index_positions_equal_the_whole_catalog(tmp_path, world):
    torch.set_num_threads(1)
    mp.spawn(_worker, args=(world, tdc._free_port(), "_positions_case", str(tmp_path)), nprocs=world, join=True)
    got = [torch.load(f"{tmp_path}/pos_{r}.pt") for r in range(world)]
    seen = 0
    for r in range(world):
        items, q, excl, lists, _ = _case_inputs(r)
        off, ids = (t.numpy() for t in _csr(lists))
        for name, ex in (("exact", excl), ("bare", None)):
            want = spec.positions(q.numpy(), items.numpy(), off, ids, ex)
            pos, score, ncand = (t.numpy() for t in got[r][name])
            assert np.array_equal(pos, want[0]) and np.array_equal(ncand, want[2]), (r, name)
            assert np.array_equal(score.view(np.uint32), want[1].view(np.uint32)), (r, name)
        seen += int((want[0] >= 0).sum())
        assert (spec.positions(q.numpy(), items.numpy(), off, ids, excl)[0] == -1).any()
        ws, wi = spec.chain.topk(q.numpy(), items.numpy(), tdc.K, excl)
        assert np.array_equal(got[r]["i"].numpy(), wi) and np.array_equal(got[r]["s"].numpy().view(np.uint32), ws.view(np.uint32))
    assert seen > 20 * world
    # compute(comm=...): the mean over every rank's queries (the last rank's counted twice), the same on every rank
    weight = [2.0 if r == world - 1 else 1.0 for r in range(world)]
    for key, rows in (("pm_all", "pm_rows"), ("rm_all", "rm_rows")):
        total = sum(w * got[r][rows].double().sum(dim=0) for r, w in enumerate(weight)) / (5 * sum(weight))
        for r in range(world):
            vals = torch.stack(list(got[r][key].values())).double()
            torch.testing.assert_close(vals, total, rtol=1e-6, atol=1e-7)          # (fp64 sums, rounded to fp32 once)
            assert list(got[r][key]) == list(got[0][key])
    own = torch.stack(list(got[0]["pm_own"].values())).double()
    torch.testing.assert_close(own, got[0]["pm_rows"].double().mean(dim=0), rtol=1e-6, atol=1e-7)      # without a comm: as before
