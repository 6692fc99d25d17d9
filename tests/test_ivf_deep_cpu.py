"""CPU: the host side of the deep cell scan (csrc/mf_ivf_deep.hip, ``PartitionedIndex.search(path="cells_deep")``) -- the four
exports, every refusal of the two scans and of the plan with their order (all decided before any launch: never-dereferenced fake
pointers do), the plan over its domain, the kernels' resources from the code objects' notes, the buffer's constants read from
the source with what the GPU test of several settles leans on, ``default_path``, the Python refusals, the deep case set, and the
digest record."""
from __future__ import annotations

import ctypes
import importlib.util
import itertools
import json
import pathlib

import numpy as np
import pytest
import torch

from tests import _ivf_deep_spec as deep
from tests import _ivf_spec as spec

ROOT = pathlib.Path(__file__).resolve().parents[1]
FAKE = ctypes.c_void_p(0x1000)
EXPORTS = {"mf_ivf_deep_ws_bytes": "size_t", "mf_ivf_deep_plan": "int", "mf_ivf_scan_deep": "int", "mf_ivf_scan_deep_allow": "int"}


def test_exports_are_declared_bound_documented_and_present(mf):
    lib = mf._lib.lib()
    header = (ROOT / "include" / "mf_hip.h").read_text()
    guide = (ROOT / "INTEGRATION.md").read_text()
    for name, ret in EXPORTS.items():
        assert hasattr(lib, name) and name in mf._lib.SIGNATURES and f"{ret} {name}(" in header and name in guide, name
    assert " mf_ivf_deep.hip " in (ROOT / "matrix-factorization-torch_amd" / "csrc" / "Makefile").read_text()
    sig = mf._lib.SIGNATURES
    assert sig["mf_ivf_scan_deep"] == sig["mf_ivf_scan"] and sig["mf_ivf_scan_deep_allow"] == sig["mf_ivf_scan_allow"]
    assert sig["mf_ivf_deep_plan"] == sig["mf_ivf_plan"] and sig["mf_ivf_deep_ws_bytes"] == sig["mf_ivf_ws_bytes"]
    assert mf._lib.MF_TOPK_DEEP_MAX_K == deep.MAX_K and mf._lib.MF_TOPK_MERGE_DEEP_MAX_KEYS == deep.MERGE_KEYS


# ------------------------------------------------------------------------------------------------------ refusals ----
def _scan(lib, allow, **kw):
    a = dict(q=FAKE, Q=4, blocked=FAKE, cell_blk=FAKE, row_of=FAKE, Npad=1024, N=1000, C=8, d=64, mcb=4, probes=FAKE, nprobe=3, k=100,
             S=0, eo=None, ei=None, base=0, words=FAKE, n_masks=1, of=None, ws=FAKE, ws_bytes=1 << 30)
    a.update(kw)
    head = (a["q"], a["Q"], a["blocked"], a["cell_blk"], a["row_of"], a["Npad"], a["N"], a["C"], a["d"], a["mcb"], a["probes"], a["nprobe"], a["k"],
            a["S"], a["eo"], a["ei"], a["base"])
    if allow:
        rc = lib.mf_ivf_scan_deep_allow(*head, a["words"], a["n_masks"], a["of"], a["ws"], a["ws_bytes"], None)
    else:
        rc = lib.mf_ivf_scan_deep(*head, a["ws"], a["ws_bytes"], None)
    return rc, (lib.mf_last_error() if rc else b"")


# (what is wrong, the code, a piece of the text) in the documented order: a fault further up wins over every one below it
FAULTS = (
    (dict(q=None), "MF_EINVAL", b"bad argument"),
    (dict(k=1025), "MF_ENOTSUP", b"k = 1025 outside 1..1024"),
    (dict(nprobe=9), "MF_ENOTSUP", b"nprobe = 9 outside 1..8"),
    (dict(d=48), "MF_EINVAL", b"embedding width 48 not in {32,64,128,256}"),
    (dict(base=2**32 - 999), "MF_ENOTSUP", b"item indices must fit 32 bits"),
    (dict(S=55, mcb=256, Npad=16384), "MF_ENOTSUP", b"nprobe * S * k too large"),         # 3 * 55 * 100 = 16,500 keys
    (dict(ws_bytes=16), "MF_ENOSPC", b"workspace too small"),
    (dict(eo=FAKE), "MF_EINVAL", b"excl_off/excl_idx mismatch"),
)
ALLOW_FAULTS = ((dict(words=None), "MF_EINVAL", b"bad allow argument"), (dict(n_masks=2**31), "MF_ENOTSUP", b"words exceed 2^31"))


@pytest.mark.parametrize("allow", [False, True])
def test_each_refusal_has_its_code_and_text(mf, allow):
    lib, E = mf._lib.lib(), mf._lib
    who = b"mf_ivf_scan_deep_allow: " if allow else b"mf_ivf_scan_deep: "
    for kw, code, text in FAULTS + (ALLOW_FAULTS if allow else ()):
        if "n_masks" in kw:
            kw = {**kw, "of": FAKE}
        rc, msg = _scan(lib, allow, **kw)
        assert rc == getattr(E, code) and msg.startswith(who) and text in msg, (kw, rc, msg)
    for kw in (dict(blocked=None), dict(cell_blk=None), dict(row_of=None), dict(probes=None), dict(ws=None), dict(Q=0), dict(N=0), dict(C=0),
               dict(Npad=960), dict(Npad=1000), dict(mcb=0), dict(mcb=17), dict(S=-1)):
        rc, msg = _scan(lib, allow, **kw)
        assert rc == E.MF_EINVAL and who + b"bad argument" in msg, (kw, rc, msg)
    for kw, text in ((dict(k=0), b"k = 0 outside 1..1024"), (dict(nprobe=0), b"nprobe = 0 outside"), (dict(C=100, nprobe=65), b"outside 1..64"),
                     (dict(Npad=2**31, N=2**31 - 5, mcb=4), b"32 bits"), (dict(base=-1), b"32 bits"), (dict(S=5), b"too large"),
                     (dict(ei=FAKE), b"mismatch"), (dict(C=64, nprobe=17, k=1024, S=1), b"nprobe * S * k too large"),
                     (dict(C=64, nprobe=64, k=257, S=1), b"nprobe * S * k too large")):
        rc, msg = _scan(lib, allow, **kw)
        assert rc in (E.MF_ENOTSUP, E.MF_EINVAL) and text in msg, (kw, rc, msg)
    if allow:
        for kw in (dict(n_masks=0), dict(n_masks=2, of=None)):
            rc, msg = _scan(lib, True, **kw)
            assert rc == E.MF_EINVAL and b"bad allow argument" in msg, (kw, rc, msg)


@pytest.mark.parametrize("allow", [False, True])
def test_which_of_two_faults_wins(mf, allow):
    lib, E = mf._lib.lib(), mf._lib
    faults = FAULTS + (ALLOW_FAULTS[:1] if allow else ())
    for (i, (kw_a, code, text)), (j, (kw_b, _, _)) in itertools.combinations(enumerate(faults), 2):
        if set(kw_a) & set(kw_b):
            continue                                     # (both faults need the same argument: not one call)
        rc, msg = _scan(lib, allow, **kw_a, **kw_b)
        assert rc == getattr(E, code) and text in msg, (i, j, rc, msg)


def test_the_boundaries_are_accepted(mf):
    """k = 1024 with nprobe = 16 and k = 256 with nprobe = 64 (16,384 keys), idx_base + N = 2^32 and an exact workspace pass every
    check: where there is no device the launch itself then fails, past every refusal."""
    lib, E = mf._lib.lib(), mf._lib
    if torch.cuda.is_available():
        return                      # (a launch on fake pointers is only harmless where there is no device: tests/test_gpu_ivf_deep.py runs real ones)
    for allow in (False, True):
        for kw in (dict(C=64, nprobe=16, k=1024, S=1), dict(C=64, nprobe=64, k=256, S=1), dict(base=2**32 - 1000),
                   dict(ws_bytes=3 * 4 * 100 * 8, S=1), dict(S=4), dict(k=1), dict(k=65)):
            rc, msg = _scan(lib, allow, **kw)
            assert rc == E.MF_ELAUNCH, (allow, kw, rc, msg)


# ---------------------------------------------------------------------------------------------------------- plan ----
def test_plan_over_its_domain(mf):
    lib, E = mf._lib.lib(), mf._lib
    out = (ctypes.c_int64 * 4)()
    sliced = beyond = 0
    for nq, nprobe, k, mcb in itertools.product((1, 2, 8, 32, 33, 1024, 100_000), (1, 3, 8, 16, 17, 64), (1, 64, 65, 100, 256, 257, 1000, 1024),
                                                (1, 3, 4, 40, 96, 5000, 200_000)):
        assert lib.mf_ivf_deep_plan(nq, nprobe, k, mcb, out) == E.MF_OK
        s, g, wgs, nbytes = out
        assert 1 <= s <= mcb, (nq, nprobe, k, mcb, s)
        if nprobe * k <= deep.MERGE_KEYS:
            assert nprobe * s * k <= deep.MERGE_KEYS, (nq, nprobe, k, mcb, s)
        else:
            assert s == 1                                  # (planned with one slice; the scan refuses the shape)
            beyond += 1
        assert s == spec.plan_slices(nq, nprobe, k, mcb, merge_keys=deep.MERGE_KEYS) and g == nprobe * s and wgs == nq * g and nbytes == g * nq * k * 8
        assert nbytes <= lib.mf_ivf_deep_ws_bytes(nq, nprobe, k, mcb) < nbytes + 256
        sliced += s > 1
    assert sliced > 100 and beyond > 0
    assert lib.mf_ivf_deep_plan(1, 8, 100, 32, out) == E.MF_OK and out[0] == 8            # 2^22 rows in 2,048 cells: 64 workgroups of 4 blocks
    assert lib.mf_ivf_deep_plan(1, 8, 1000, 32, out) == E.MF_OK and out[0] == 2           # 16,384 // 8,000
    assert lib.mf_ivf_deep_plan(1, 8, 100, 96, None) == E.MF_EINVAL and lib.mf_last_error() == b"mf_ivf_deep_plan: out is NULL"
    for bad in ((0, 8, 100, 96), (1, 0, 100, 96), (1, 65, 100, 96), (1, 8, 0, 96), (1, 8, 1025, 96), (1, 8, 100, 0)):
        assert lib.mf_ivf_deep_plan(*bad, out) == E.MF_EINVAL and lib.mf_ivf_deep_ws_bytes(*bad) == 0, bad
        assert b"k in 1..1024 and nprobe in 1..64" in lib.mf_last_error()
    # the wavefront scan's plan keeps its limits
    assert lib.mf_ivf_plan(1, 8, 65, 96, out) == E.MF_EINVAL and lib.mf_ivf_ws_bytes(1, 8, 65, 96) == 0


# ----------------------------------------------------------------------------------------------------- resources ----
def test_the_new_kernels_have_no_spill_no_scratch_and_lds_for_two_workgroups():
    s = importlib.util.spec_from_file_location("kernel_resources", ROOT / "tools" / "kernel_resources.py")
    kr = importlib.util.module_from_spec(s)
    s.loader.exec_module(kr)
    table = kr.kernel_resources()
    c = deep.constants()
    for stem in ("ivf_scan_deep_kernel<", "ivf_scan_deep_allow_kernel<"):
        scan = {n: r for n, r in table.items() if stem in n}
        assert sorted(int(n.split("<")[1].split(">")[0]) for n in scan) == [32, 64, 128, 256], (stem, sorted(scan))
        for name, r in scan.items():
            assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0 and r["max_flat_workgroup_size"] == 256, (name, r)
            # the buffer and four counts; static, within the 64 KiB of a kernel without an attribute, two workgroups in a CU's 160 KiB
            assert r["group_segment_fixed_size"] == c["IVFD_BUF"] * 8 + 16 <= 64 * 1024, (name, r)
            assert 2 * r["group_segment_fixed_size"] <= 160 * 1024 and r["vgpr_count"] + r["agpr_count"] <= 256, (name, r)


# ----------------------------------------------------------------------------------------------------- constants ----
def test_the_constants_and_the_cell_of_several_settles():
    c = deep.constants()
    assert c == {"IVFD_PASS": 256, "IVFD_KP_MIN": 128, "IVFD_KP_MAX": 1024, "IVFD_BUF_MIN": 2048, "IVFD_BUF": 4096, "IVFD_SORT_MIN": 512}
    assert [deep.kept(k) for k in (1, 64, 128, 129, 256, 257, 512, 513, 1000, 1024)] == [128, 128, 128, 256, 256, 512, 512, 1024, 1024, 1024]
    assert [deep.capacity(kp) for kp in (128, 256, 512, 1024)] == [2048, 2048, 2048, 4096] and deep.capacity(c["IVFD_KP_MAX"]) == c["IVFD_BUF"]
    for kp in (128, 256, 512, 1024):                       # a pass's keys always fit behind the threshold, and the shortest sort covers kp
        assert deep.capacity(kp) - kp - c["IVFD_PASS"] >= c["IVFD_PASS"] and c["IVFD_SORT_MIN"] <= deep.capacity(kp)
    n = deep.settle_rows()
    assert n >= 3 * c["IVFD_BUF"] and n % 64 == 40
    for order in deep.SETTLE_ORDERS:
        scores = deep.settle_scores(order)
        assert scores.dtype == np.float32 and np.unique(scores).size == n and scores.min() > 0
        for k in (100, 1000, 1024):
            w = deep.walk(scores, k)
            live = [waiting for waiting, bound in w["settles"] if bound]
            assert w["best"] == deep.top_of(scores, 0, n, k).tolist(), (order, k)
            assert w["settles"][0][1] is False and w["settles"][0][0] >= k
            if order == "ascending":                       # every key beats the bound: the buffer fills again and again
                assert len(live) >= 3 and min(live[:-1]) > deep.capacity(deep.kept(k)) - deep.kept(k) - c["IVFD_PASS"], (order, k, w["settles"])
            elif order == "descending":                    # none after the first k: one settle, or a last one with nothing new kept
                assert len(w["settles"]) == 1 or sum(live) == 0, (order, k, w["settles"])
            else:
                assert len(live) >= 1 and 0 < sum(live) < n - k, (order, k, w["settles"])
    # a slice of the cell at the planned geometry settles too: 52 slices of four blocks at k = 100 do not, S = 1 does
    assert len(deep.walk(deep.settle_scores("ascending")[:256], 100)["settles"]) == 1


# -------------------------------------------------------------------------------------------------------- python ----
def test_default_path_and_the_python_refusals(mf):
    R = mf.retrieval
    assert R.ItemIndex.PATHS == ("auto", "scan", "tiles", "bf16", "deep")
    exact, cells, quant = (object.__new__(cls) for cls in (R.ItemIndex, R.PartitionedIndex, R.QuantizedIndex))
    assert [exact.default_path(k) for k in (1, 64, 65, 1024)] == ["auto"] * 4
    assert [cells.default_path(k) for k in (1, 64, 65, 100, 1024)] == ["cells", "cells", "cells_deep", "cells_deep", "cells_deep"]
    assert [quant.default_path(k) for k in (1, 64, 65)] == ["pq"] * 3
    # refused before the queries are looked at: an index that holds nothing but its cell count has nothing to launch with
    cells.num_probes, cells.num_partitions = 8, 64
    for top_k, nprobe, text in ((0, 8, "1..1024"), (1025, 8, "1..1024"), (1025, 1, "1..1024"), (1024, 17, "must not exceed 16384"),
                                (257, 64, "must not exceed 16384"), (100, 65, "nprobe must be in 1..64"), (100, 0, "nprobe must be")):
        with pytest.raises(ValueError, match=text):
            cells.search(None, top_k, nprobe=nprobe, path="cells_deep")
    with pytest.raises(ValueError, match="1..64"):
        cells.search(None, 65, path="cells")
    with pytest.raises(ValueError, match="no bitmap route"):
        cells.search(None, 100, path="deep", allow=object())
    with pytest.raises(ValueError, match="give one of them"):
        cells.search(None, 100, path="cells_deep", allow=object(), where=object())
    quant.num_probes, quant.num_partitions, quant.refine_factor = 8, 64, 4
    with pytest.raises(ValueError):
        quant.search(None, 100, path="pq")
    with pytest.raises(ValueError, match="1..1024"):
        quant.search(None, 1025, path="cells_deep")


# ------------------------------------------------------------------------------------------------ the case set ----
def test_the_case_set_holds_what_the_gpu_assertions_lean_on(mf):
    cs = deep.cases()
    assert {c.k for c in cs.values()} >= set(deep.DEPTHS)
    assert {c.items.shape[1] for c in cs.values()} >= {32, 48, 64, 128, 256}
    assert {c.items.shape[0] for c in cs.values()} >= {33, 1000, 2500, 5000} and {c.q.shape[0] for c in cs.values()} >= {1, 33, 70}
    assert {c.nprobe for c in cs.values()} >= {1, 3, 8, 16} and sum(c.nprobe == c.centroids.shape[0] > 1 for c in cs.values()) >= 3
    assert {len(e) for c in cs.values() if c.exclude for e in c.exclude} >= {0, 1, 17, 1025} and any(c.exclude is None for c in cs.values())
    assert any(c.idx_base == 1000 and c.exclude for c in cs.values())
    assert all(c.nprobe * c.k <= deep.MERGE_KEYS for c in cs.values())
    for name in ("deep_cell_sizes_nprobe3", "deep_cell_sizes_nprobe16"):
        c = cs[name]
        assert c.sizes[:5].tolist() == [0, 1, 63, 64, 65] and spec.probes(c.q, c.centroids, c.nprobe)[0, 0] == 0, name
    # a tail in every list: 607 .. 615 rows under the one probe
    c = cs["deep_k1000_tail"]
    s, r = c.expected()
    filled = (r >= 0).sum(axis=1)
    assert (filled >= 600).all() and (filled < 1000).all() and np.isneginf(s[0, filled[0]:]).all() and (r[0, filled[0]:] == -1).all()
    s, r = cs["deep_all_but_three"].expected()
    assert ((r >= 0).sum(axis=1) == 3).all()
    # the twins: 1,024 of 1,100 equal scores, rows ascending, from all four cells; both plan geometries among the cases
    c = cs["deep_ties_k1024"]
    s, r = c.expected()
    assert r[0].tolist() == list(range(1024)) and len(set(s[0].view(np.uint32).tolist())) == 1 and set(c.assign[:1024].tolist()) == {0, 1, 2, 3}
    lib = mf._lib.lib()
    out = (ctypes.c_int64 * 4)()
    slices = {}
    for name, c in cs.items():
        assert lib.mf_ivf_deep_plan(c.q.shape[0], c.nprobe, c.k, c.max_cell_blocks, out) == 0
        slices[name] = out[0]
    assert slices["deep_ties_k1024"] == 2 and slices["deep_k1000_tail"] >= 2 and slices["deep_w32_k65"] == 1
    assert sum(s > 1 for s in slices.values()) >= 3 and sum(s == 1 for s in slices.values()) >= 3


# ---------------------------------------------------------------------------------------------------- the record ----
def test_the_digest_record_shows_the_parents_kernels_unchanged():
    """profiles/ivf_deep_digest_{parent,branch}.json: ``tools/kernel_resources.py --text-digest`` of the parent's library and of
    this one with one ``--only=`` list, the branch's record cut to the kernels the parent's names (``--names-of=``): every kernel of
    mf_ivf.hip, mf_pq.hip, mf_filter.hip and the top-k units.  The two records are equal: same kernels, same instruction text, same
    resource figures -- the deep scan stands beside them."""
    parent = json.loads((ROOT / "profiles" / "ivf_deep_digest_parent.json").read_text())
    branch = json.loads((ROOT / "profiles" / "ivf_deep_digest_branch.json").read_text())
    assert branch == parent and all(len(v["text_sha256"]) == 64 for v in parent.values())
    count = lambda unit: sum(unit in k for k in parent)  # noqa: E731
    assert count("ivf_scan_kernel<") == 4 and count("ivf_scan_allow_kernel<") == 4 and count("ivf_cell_mean_kernel") == 1
    assert count("pq_scan_kernel<") == 12 and count("pq_scan_allow_kernel<") == 12 and count("pq_encode_kernel") == 3 and count("pq_refine_kernel") == 4
    for unit in ("filter_mark_kernel", "filter_pack_kernel", "filter_remap_kernel", "filter_unmap_kernel", "filter_lists_count_kernel",
                 "filter_lists_scan_kernel", "filter_lists_write_kernel", "filter_cell_bits", "topk_small_scan_kernel", "topk_small_mfma_scan_kernel",
                 "bf3_scan_kernel", "bf3_final_kernel", "topk_deep_slab_kernel", "topk_deep_select_kernel", "topk_merge_kernel",
                 "topk_merge_deep_kernel", "topk_pack_kernel", "select_kernel", "select_seed_kernel", "target_positions_kernel"):
        assert count(unit) >= 1, unit
    assert not any("scan_deep" in k for k in parent)
    # the library that is built now has every one of them under the same name, and the deep scans beside them
    s = importlib.util.spec_from_file_location("kernel_resources", ROOT / "tools" / "kernel_resources.py")
    kr = importlib.util.module_from_spec(s)
    s.loader.exec_module(kr)
    built = set(kr.kernel_resources())
    assert set(parent) <= built and sum("scan_deep" in k for k in built) == 8
