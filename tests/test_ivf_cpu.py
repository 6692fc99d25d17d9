"""CPU: the host side of the partitioned index (csrc/mf_ivf.hip, ``retrieval.PartitionedIndex``) -- the exports, every refusal
and their order (all decided before any launch, so never-dereferenced fake pointers do), the plan over its whole domain, the
layout function on hand-made assignments, the kernels' resources from the code object's notes, the config fields, and the spec
on every GPU case, with the properties the GPU assertions lean on."""
from __future__ import annotations

import ctypes
import importlib.util
import itertools
import pathlib

import numpy as np
import pytest
import torch

from tests import _ivf_spec as spec

ROOT = pathlib.Path(__file__).resolve().parents[1]
FAKE = ctypes.c_void_p(0x1000)
EXPORTS = {"mf_ivf_ws_bytes": "size_t", "mf_ivf_plan": "int", "mf_ivf_scan": "int", "mf_ivf_cell_mean": "int"}


def test_exports_are_declared_bound_documented_and_present(mf):
    lib = mf._lib.lib()
    header = (ROOT / "include" / "mf_hip.h").read_text()
    guide = (ROOT / "INTEGRATION.md").read_text()
    for name, ret in EXPORTS.items():
        assert hasattr(lib, name) and name in mf._lib.SIGNATURES and f"{ret} {name}(" in header and name in guide, name
    assert "mf_ivf.hip" in (ROOT / "matrix-factorization-torch_amd" / "csrc" / "Makefile").read_text()


# ------------------------------------------------------------------------------------------------------ refusals ----
def _scan(lib, **kw):
    a = dict(q=FAKE, Q=4, blocked=FAKE, cell_blk=FAKE, row_of=FAKE, Npad=1024, N=1000, C=8, d=64, mcb=4, probes=FAKE, nprobe=3, k=20,
             S=0, eo=None, ei=None, base=0, ws=FAKE, ws_bytes=1 << 30)
    a.update(kw)
    rc = lib.mf_ivf_scan(a["q"], a["Q"], a["blocked"], a["cell_blk"], a["row_of"], a["Npad"], a["N"], a["C"], a["d"], a["mcb"], a["probes"],
                         a["nprobe"], a["k"], a["S"], a["eo"], a["ei"], a["base"], a["ws"], a["ws_bytes"], None)
    return rc, (lib.mf_last_error() if rc else b"")


# (what is wrong, the code, a piece of the text) in the documented order: a fault further up wins over every one below it
FAULTS = (
    (dict(q=None), "MF_EINVAL", b"mf_ivf_scan: bad argument"),
    (dict(k=65), "MF_ENOTSUP", b"k = 65 outside 1..64"),
    (dict(nprobe=9), "MF_ENOTSUP", b"nprobe = 9 outside 1..8"),
    (dict(d=48), "MF_EINVAL", b"embedding width 48 not in {32,64,128,256}"),
    (dict(base=2**32 - 999), "MF_ENOTSUP", b"item indices must fit 32 bits"),
    (dict(S=137, mcb=256, Npad=16384), "MF_ENOTSUP", b"nprobe * S * k too large"),        # 3 * 137 * 20 = 8,220 keys
    (dict(ws_bytes=16), "MF_ENOSPC", b"workspace too small"),
    (dict(eo=FAKE), "MF_EINVAL", b"excl_off/excl_idx mismatch"),
)


def test_each_refusal_has_its_code_and_text(mf):
    lib, E = mf._lib.lib(), mf._lib
    for kw, code, text in FAULTS:
        rc, msg = _scan(lib, **kw)
        assert rc == getattr(E, code) and text in msg, (kw, rc, msg)
    for kw in (dict(blocked=None), dict(cell_blk=None), dict(row_of=None), dict(probes=None), dict(ws=None), dict(Q=0), dict(N=0), dict(C=0),
               dict(Npad=960), dict(Npad=1000), dict(mcb=0), dict(mcb=17), dict(S=-1)):
        rc, msg = _scan(lib, **kw)
        assert rc == E.MF_EINVAL and b"mf_ivf_scan: bad argument" in msg, (kw, rc, msg)
    for kw, text in ((dict(k=0), b"k = 0 outside"), (dict(nprobe=0), b"nprobe = 0 outside"), (dict(C=100, nprobe=65), b"outside 1..64"),
                     (dict(Npad=2**31, N=2**31 - 5, mcb=4), b"32 bits"), (dict(base=-1), b"32 bits"), (dict(S=5), b"too large"),
                     (dict(ei=FAKE), b"mismatch")):
        rc, msg = _scan(lib, **kw)
        assert rc in (E.MF_ENOTSUP, E.MF_EINVAL) and text in msg, (kw, rc, msg)


def test_which_of_two_faults_wins(mf):
    lib, E = mf._lib.lib(), mf._lib
    for (i, (kw_a, code, text)), (j, (kw_b, _, _)) in itertools.combinations(enumerate(FAULTS), 2):
        if set(kw_a) & set(kw_b):
            continue                                     # (both faults need the same argument: not one call)
        rc, msg = _scan(lib, **kw_a, **kw_b)
        assert rc == getattr(E, code) and text in msg, (i, j, rc, msg)


def test_the_boundaries_are_accepted(mf):
    """k = 64 with nprobe = 64 (4,096 keys), idx_base + N = 2^32 and an exact workspace pass every check: where there is no
    device the launch itself then fails, past every refusal."""
    lib, E = mf._lib.lib(), mf._lib
    if torch.cuda.is_available():
        return                      # (a launch on fake pointers is only harmless where there is no device: tests/test_gpu_ivf.py runs real ones)
    for kw in (dict(C=64, nprobe=64, k=64, S=2), dict(base=2**32 - 1000), dict(ws_bytes=3 * 4 * 20 * 8, S=1), dict(S=4)):
        rc, msg = _scan(lib, **kw)
        assert rc == E.MF_ELAUNCH, (kw, rc, msg)


def test_cell_mean_refusals(mf):
    lib, E = mf._lib.lib(), mf._lib
    for args in ((None, 10, 64, FAKE, FAKE, 2, 1, FAKE), (FAKE, 0, 64, FAKE, FAKE, 2, 1, FAKE), (FAKE, 10, 64, FAKE, FAKE, 0, 1, FAKE),
                 (FAKE, 10, 64, None, FAKE, 2, 1, FAKE), (FAKE, 10, 64, FAKE, FAKE, 2, 1, None)):
        assert lib.mf_ivf_cell_mean(*args, None) == E.MF_EINVAL and b"mf_ivf_cell_mean: bad argument" in lib.mf_last_error(), args
    assert lib.mf_ivf_cell_mean(FAKE, 10, 48, FAKE, FAKE, 2, 1, FAKE, None) == E.MF_EINVAL and b"width 48" in lib.mf_last_error()


# ---------------------------------------------------------------------------------------------------------- plan ----
def test_plan_over_its_domain(mf):
    lib, E = mf._lib.lib(), mf._lib
    out = (ctypes.c_int64 * 4)()
    sliced = 0
    for nq, nprobe, k, mcb in itertools.product((1, 2, 8, 32, 33, 1024, 100_000), (1, 3, 8, 32, 64), (1, 20, 64), (1, 3, 4, 40, 96, 5000, 200_000)):
        assert lib.mf_ivf_plan(nq, nprobe, k, mcb, out) == E.MF_OK
        s, g, wgs, nbytes = out
        assert 1 <= s <= mcb and nprobe * s * k <= 8192, (nq, nprobe, k, mcb, s)
        assert s == spec.plan_slices(nq, nprobe, k, mcb) and g == nprobe * s and wgs == nq * g and nbytes == g * nq * k * 8
        assert nbytes <= lib.mf_ivf_ws_bytes(nq, nprobe, k, mcb) < nbytes + 256
        sliced += s > 1
    assert sliced > 50
    assert lib.mf_ivf_plan(1, 8, 20, 96, out) == E.MF_OK and out[0] == 24              # the serving shape: 192 workgroups of 4 blocks
    assert lib.mf_ivf_plan(1, 8, 20, 96, None) == E.MF_EINVAL and lib.mf_last_error() == b"mf_ivf_plan: out is NULL"
    for bad in ((0, 8, 20, 96), (1, 0, 20, 96), (1, 65, 20, 96), (1, 8, 0, 96), (1, 8, 65, 96), (1, 8, 20, 0)):
        assert lib.mf_ivf_plan(*bad, out) == E.MF_EINVAL and lib.mf_ivf_ws_bytes(*bad) == 0, bad


# -------------------------------------------------------------------------------------------------------- layout ----
def _check_layout(mf, assign, c):
    a = torch.as_tensor(assign, dtype=torch.int64)
    perm, cell_blk, row_of = mf.retrieval.partition_layout(a, c)
    sizes = np.bincount(assign, minlength=c)
    assert perm.dtype == cell_blk.dtype == row_of.dtype == torch.int64
    assert cell_blk.tolist() == [0] + np.cumsum((sizes + 63) // 64).tolist()
    assert row_of.numel() == 64 * int(cell_blk[-1])
    want_perm = []
    for cell in range(c):
        rows = np.nonzero(np.asarray(assign) == cell)[0]                     # ascending: the stable order
        want_perm += rows.tolist()
        lo, hi = 64 * int(cell_blk[cell]), 64 * int(cell_blk[cell + 1])
        assert row_of[lo : lo + rows.size].tolist() == rows.tolist() and (row_of[lo + rows.size : hi] == -1).all(), cell
    assert perm.tolist() == want_perm
    assert sorted(row_of[row_of >= 0].tolist()) == list(range(len(assign)))
    return cell_blk, row_of


def test_layout_on_hand_made_assignments(mf):
    cell_blk, row_of = _check_layout(mf, [2, 0, 2, 2, 5, 0], 7)                # empty cells 1, 3, 4, 6; a one-row cell
    assert cell_blk.tolist() == [0, 1, 1, 2, 2, 2, 3, 3] and row_of[:3].tolist() == [1, 5, -1] and row_of[64:68].tolist() == [0, 2, 3, -1]
    cell_blk, row_of = _check_layout(mf, [0] * 64 + [1] * 64, 2)               # cells of exactly 64: no padding at all
    assert cell_blk.tolist() == [0, 1, 2] and (row_of >= 0).all()
    cell_blk, _ = _check_layout(mf, [1] * 65 + [0], 3)                         # 65 rows: a second block; the last cell empty
    assert cell_blk.tolist() == [0, 1, 3, 3]
    rng = np.random.default_rng(0)
    _check_layout(mf, rng.integers(0, 37, 2500), 37)
    _check_layout(mf, np.zeros(33, np.int64), 1)
    for bad, c in (([0, 3], 3), ([-1, 0], 2), ([], 2), ([0], 0)):
        with pytest.raises(ValueError):
            mf.retrieval.partition_layout(torch.tensor(bad, dtype=torch.int64), c)
    assert [mf.retrieval.default_num_partitions(n) for n in (1, 2, 33, 62_423, 2**22, 12_500_000)] == [1, 1, 4, 128, 2048, 2048]


# ----------------------------------------------------------------------------------------------------- resources ----
def test_the_new_kernels_have_no_spill_no_scratch_and_little_lds():
    s = importlib.util.spec_from_file_location("kernel_resources", ROOT / "tools" / "kernel_resources.py")
    kr = importlib.util.module_from_spec(s)
    s.loader.exec_module(kr)
    table = kr.kernel_resources()
    scan = {n: r for n, r in table.items() if "ivf_scan_kernel" in n}
    assert sorted(int(n.split("<")[1].split(">")[0]) for n in scan) == [32, 64, 128, 256], sorted(scan)
    mean = {n: r for n, r in table.items() if "ivf_cell_mean_kernel" in n}
    assert len(mean) == 1
    for name, r in {**scan, **mean}.items():
        assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, (name, r)
        assert r["group_segment_fixed_size"] <= 160 * 1024 and r["max_flat_workgroup_size"] == 256, (name, r)
    for name, r in scan.items():
        # per wave 192 keys and two lists of 64, and the 256 keys of the join: 12 KiB; registers for two workgroups per SIMD
        assert r["group_segment_fixed_size"] == 12 * 1024 and r["vgpr_count"] + r["agpr_count"] <= 128, (name, r)


# -------------------------------------------------------------------------------------------------------- config ----
def test_config_fields_and_round_trip(mf):
    cfg_cls = mf.lightning.MatrixFactorizationLitConfig
    base = dict(num_users=10, num_items=20)
    cfg = cfg_cls(**base)
    assert (cfg.index_type, cfg.num_partitions, cfg.num_probes, cfg.index_seed) == ("exact", None, 8, 0)
    cfg = cfg_cls(**base, index_type="partitioned", num_partitions=4, num_probes=3, index_seed=7)
    again = cfg_cls.model_validate(cfg.model_dump())
    assert again == cfg and again.model_dump()["index_type"] == "partitioned" and again.num_partitions == 4
    for bad in (dict(index_type="ivf"), dict(num_partitions=0), dict(num_probes=0), dict(num_probes=65), dict(index_seed=-1)):
        with pytest.raises(ValueError):
            cfg_cls(**base, **bad)
    proc = mf.lightning.MatrixFactorizationLitModule(cfg)._item_processor()
    assert (proc.index_type, proc.num_partitions, proc.num_probes, proc.index_seed) == ("partitioned", 4, 3, 7)
    with pytest.raises(ValueError, match="index_type"):
        mf.retrieval.ItemProcessor(index_type="hnsw")


def test_cpu_tensors_are_refused(mf):
    c = spec.cases()["width32"]
    t = [torch.from_numpy(x) for x in (c.items, c.centroids, c.assign)]
    with pytest.raises(mf._lib.MfHipError, match="must live on the GPU"):
        mf.retrieval.PartitionedIndex.from_assignment(*t)
    with pytest.raises(mf._lib.MfHipError, match="must live on the GPU"):
        mf.retrieval.PartitionedIndex.build(t[0], 4)
    with pytest.raises(mf._lib.MfHipError, match="must live on the GPU"):
        mf.retrieval.ItemProcessor(index_type="partitioned").set_index(t[0])


# ------------------------------------------------------------------------------------------------ the case set ----
@pytest.fixture(scope="module")
def results():
    return {name: (c, *c.expected()) for name, c in spec.cases().items()}


def test_the_spec_on_every_case(results):
    for name, (c, s, r) in results.items():
        nq, n = c.q.shape[0], c.items.shape[0]
        assert s.shape == r.shape == (nq, c.k) and s.dtype == np.float32 and r.dtype == np.int64, name
        probed = spec.probes(c.q, c.centroids, c.nprobe)
        for i in range(nq):
            got = r[i][r[i] >= 0] - c.idx_base
            assert np.isin(c.assign[got], probed[i]).all(), (name, i)                         # only probed cells ...
            if c.exclude is not None:
                assert not np.isin(got + c.idx_base, c.exclude[i]).any(), (name, i)          # ... and nothing excluded
            filled = int((r[i] >= 0).sum())
            assert (r[i][filled:] == -1).all() and np.isneginf(s[i][filled:]).all(), (name, i)
            inside = np.isin(c.assign, probed[i]) & ~np.isin(np.arange(n) + c.idx_base, [] if c.exclude is None else c.exclude[i])
            assert filled == min(c.k, int(inside.sum())), (name, i)


def test_the_case_set_holds_what_the_gpu_assertions_lean_on(mf, results):
    cs = spec.cases()
    assert {c.items.shape[1] for c in cs.values()} >= {32, 48, 64, 128, 256}
    assert {c.items.shape[0] for c in cs.values()} >= {33, 1000, 2500} and {c.q.shape[0] for c in cs.values()} >= {1, 33, 70}
    assert {c.centroids.shape[0] for c in cs.values()} >= {1, 4, 16, 37} and {c.k for c in cs.values()} == {1, 20, 64}
    assert {c.nprobe for c in cs.values()} >= {1, 3} and any(c.nprobe == c.centroids.shape[0] > 1 for c in cs.values())
    assert {len(e) for c in cs.values() if c.exclude for e in c.exclude} >= {0, 1, 17, 1025}
    assert any(c.idx_base > 0 and c.exclude for c in cs.values())
    assert set(cs["cell_sizes_nprobe3"].sizes[:5].tolist()) == {0, 1, 63, 64, 65}
    # a tail
    _, s, r = results["all_but_three"]
    assert ((r >= 0).sum(axis=1) == 3).all() and np.isneginf(s[:, 3:]).all()
    assert (results["fewer_rows_than_k"][2][:, -1] == -1).all()
    # an empty cell under the probe, at nprobe = 3 as well
    for name in ("cell_sizes_nprobe3", "cell_sizes_nprobe16"):
        c = cs[name]
        assert c.sizes[0] == 0 and spec.probes(c.q, c.centroids, c.nprobe)[0, 0] == 0, name
    # equal scores across cells: the 64 lowest of the 300 twin rows that lie in the three probed cells, in row order
    c, s, r = results["ties_across_cells"]
    probed = spec.probes(c.q, c.centroids, c.nprobe)[0]
    twins = [row for row in range(300) if c.assign[row] in probed]
    assert r[0].tolist() == twins[:64] and len({c.assign[row] for row in twins[:64]}) == 3 and len(set(s[0].view(np.uint32).tolist())) == 1
    # twin centroids: the lower cell
    c = cs["twin_centroids"]
    assert (spec.probes(c.q, c.centroids, 1)[:8, 0] == 1).all()
    # the zero query: rows in order from cells 0, 1, 2
    c, s, r = results["zero_query"]
    assert spec.probes(c.q, c.centroids, 3)[1].tolist() == [0, 1, 2] and not s[1].any()
    assert r[1].tolist() == [row for row in range(c.items.shape[0]) if c.assign[row] < 3 and row not in c.exclude[1]][:20]
    # both plan geometries
    lib = mf._lib.lib()
    out = (ctypes.c_int64 * 4)()
    slices = {}
    for name, c in cs.items():
        assert lib.mf_ivf_plan(c.q.shape[0], c.nprobe, c.k, c.max_cell_blocks, out) == 0
        slices[name] = out[0]
    assert slices["big_cell"] == 10 and cs["big_cell"].sizes[0] == 2560 and spec.probes(cs["big_cell"].q, cs["big_cell"].centroids, 1)[0, 0] == 0
    assert slices["width64"] == 1 and sum(s > 1 for s in slices.values()) >= 2
