"""CPU: the host side of the deep quantised search (``QuantizedIndex.search(path="pq_deep")``: ``mf_pq_scan_deep`` and its allow
twin in csrc/mf_ivf_deep.hip, ``mf_pq_refine_deep`` in csrc/mf_pq.hip) -- the five exports, every refusal and its order (all
decided before any launch: never-dereferenced fake pointers do), the plan over its domain, the kernels' resources from the
code objects' notes, the buffer's constants, ``serving_path`` / ``default_path``, the Python refusals, the config rule on both
sides of 64 rows, the settles the long-cell cases of tests/test_gpu_ivf_pq_deep.py reach, and the digest record.

The kernels are ``pq_deep_scan_kernel``, ``pq_deep_scan_allow_kernel`` and ``pq_refine_deep_kernel``: tests/test_ivf_deep_cpu.py
counts the kernels of the built library whose name holds ``scan_deep`` (the eight of the deep cell scan), so the quantised deep
scans carry the two words the other way round."""
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
from tests import _ivf_pq_deep_spec as pqd
from tests import _ivf_pq_spec as spec

ROOT = pathlib.Path(__file__).resolve().parents[1]
FAKE = ctypes.c_void_p(0x1000)
EXPORTS = {"mf_pq_deep_ws_bytes": "size_t", "mf_pq_deep_plan": "int", "mf_pq_scan_deep": "int", "mf_pq_scan_deep_allow": "int",
           "mf_pq_refine_deep": "int"}
TWINS = {"mf_pq_deep_ws_bytes": "mf_pq_ws_bytes", "mf_pq_deep_plan": "mf_pq_plan", "mf_pq_scan_deep": "mf_pq_scan",
         "mf_pq_scan_deep_allow": "mf_pq_scan_allow", "mf_pq_refine_deep": "mf_pq_refine"}


def test_exports_are_declared_bound_documented_and_present(mf):
    lib = mf._lib.lib()
    header = (ROOT / "include" / "mf_hip.h").read_text()
    guide = (ROOT / "INTEGRATION.md").read_text()
    sig = mf._lib.SIGNATURES
    for name, ret in EXPORTS.items():
        assert hasattr(lib, name) and name in sig and f"{ret} {name}(" in header and name in guide, name
        assert sig[name] == sig[TWINS[name]], name
    assert mf._lib.MF_TOPK_DEEP_MAX_K == pqd.MAX_R and mf._lib.MF_TOPK_MERGE_DEEP_MAX_KEYS == pqd.MERGE_KEYS
    R = mf.retrieval
    assert R.QuantizedIndex.DEEP_MAX_CANDIDATES == 1024 and R.QuantizedIndex.MAX_CANDIDATES == 256 and R.MERGE_DEEP_MAX_KEYS == 16384


# ------------------------------------------------------------------------------------------------------ refusals ----
def _scan(lib, allow, **kw):
    a = dict(q=FAKE, Q=4, codes=FAKE, books=FAKE, dsub=8, cell_blk=FAKE, row_of=FAKE, Npad=1024, N=1000, C=8, d=64, mcb=4, probes=FAKE,
             scores=FAKE, nprobe=3, R=400, S=0, eo=None, ei=None, base=0, words=FAKE, n_masks=1, of=None, ws=FAKE, ws_bytes=1 << 30)
    a.update(kw)
    head = (a["q"], a["Q"], a["codes"], a["books"], a["dsub"], a["cell_blk"], a["row_of"], a["Npad"], a["N"], a["C"], a["d"], a["mcb"],
            a["probes"], a["scores"], a["nprobe"], a["R"], a["S"], a["eo"], a["ei"], a["base"])
    if allow:
        rc = lib.mf_pq_scan_deep_allow(*head, a["words"], a["n_masks"], a["of"], a["ws"], a["ws_bytes"], None)
    else:
        rc = lib.mf_pq_scan_deep(*head, a["ws"], a["ws_bytes"], None)
    return rc, (lib.mf_last_error() if rc else b"")


# (what is wrong, the code, a piece of the text) in mf_pq_scan's order: a fault further up wins over every one below it
FAULTS = (
    (dict(q=None), "MF_EINVAL", b"bad argument"),
    (dict(R=1025), "MF_ENOTSUP", b"R = 1025 outside 1..1024"),
    (dict(nprobe=9), "MF_ENOTSUP", b"nprobe = 9 outside 1..8"),
    (dict(d=48), "MF_EINVAL", b"embedding width 48 not in {32,64,128,256}"),
    (dict(dsub=5), "MF_ENOTSUP", b"sub-vector length 5 not in {4,8,16}"),
    (dict(base=2**32 - 999), "MF_ENOTSUP", b"item indices must fit 32 bits"),
    (dict(S=14, mcb=256, Npad=16384), "MF_ENOTSUP", b"nprobe * S * R too large"),        # 3 * 14 * 400 = 16,800 keys
    (dict(ws_bytes=16), "MF_ENOSPC", b"workspace too small"),
    (dict(eo=FAKE), "MF_EINVAL", b"excl_off/excl_idx mismatch"),
)
ALLOW_FAULTS = ((dict(words=None), "MF_EINVAL", b"bad allow argument"), (dict(n_masks=2**31), "MF_ENOTSUP", b"words exceed 2^31"))


@pytest.mark.parametrize("allow", [False, True])
def test_each_refusal_of_the_scans_has_its_code_and_text(mf, allow):
    lib, E = mf._lib.lib(), mf._lib
    who = b"mf_pq_scan_deep_allow: " if allow else b"mf_pq_scan_deep: "
    for kw, code, text in FAULTS + (ALLOW_FAULTS if allow else ()):
        if "n_masks" in kw:
            kw = {**kw, "of": FAKE}
        rc, msg = _scan(lib, allow, **kw)
        assert rc == getattr(E, code) and msg.startswith(who) and text in msg, (kw, rc, msg)
    for kw in (dict(codes=None), dict(books=None), dict(cell_blk=None), dict(row_of=None), dict(probes=None), dict(scores=None), dict(ws=None),
               dict(Q=0), dict(N=0), dict(C=0), dict(Npad=960), dict(Npad=1000), dict(mcb=0), dict(mcb=17), dict(S=-1)):
        rc, msg = _scan(lib, allow, **kw)
        assert rc == E.MF_EINVAL and who + b"bad argument" in msg, (kw, rc, msg)
    for kw, text in ((dict(R=0), b"R = 0 outside 1..1024"), (dict(nprobe=0), b"nprobe = 0 outside"), (dict(C=100, nprobe=65), b"outside 1..64"),
                     (dict(dsub=32), b"sub-vector length 32"), (dict(dsub=0), b"sub-vector length 0"),
                     (dict(Npad=2**31, N=2**31 - 5, mcb=4), b"32 bits"), (dict(base=-1), b"32 bits"), (dict(S=5), b"too large"),
                     (dict(ei=FAKE), b"mismatch"), (dict(C=64, nprobe=17, R=1024, S=1), b"nprobe * S * R too large"),
                     (dict(C=64, nprobe=64, R=257, S=1), b"nprobe * S * R too large")):
        rc, msg = _scan(lib, allow, **kw)
        assert rc in (E.MF_ENOTSUP, E.MF_EINVAL) and text in msg, (kw, rc, msg)
    if allow:
        for kw in (dict(n_masks=0), dict(n_masks=2, of=None)):
            rc, msg = _scan(lib, True, **kw)
            assert rc == E.MF_EINVAL and b"bad allow argument" in msg, (kw, rc, msg)
    # the shallow scan keeps its limit
    assert lib.mf_pq_scan(FAKE, 4, FAKE, FAKE, 8, FAKE, FAKE, 1024, 1000, 8, 64, 4, FAKE, FAKE, 3, 257, 0, None, None, 0, FAKE, 1 << 30,
                          None) == E.MF_ENOTSUP and b"R = 257 outside 1..256" in lib.mf_last_error()


@pytest.mark.parametrize("allow", [False, True])
def test_which_of_two_faults_wins(mf, allow):
    lib, E = mf._lib.lib(), mf._lib
    faults = FAULTS + (ALLOW_FAULTS[:1] if allow else ())
    for (i, (kw_a, code, text)), (j, (kw_b, _, _)) in itertools.combinations(enumerate(faults), 2):
        if set(kw_a) & set(kw_b):
            continue                                     # (both faults need the same argument: not one call)
        rc, msg = _scan(lib, allow, **kw_a, **kw_b)
        assert rc == getattr(E, code) and text in msg, (i, j, rc, msg)


def _refine(lib, q=FAKE, Q=4, items=FAKE, N=1000, d=64, cand=FAKE, R=400, k=100, base=0, s=FAKE, r=FAKE):
    rc = lib.mf_pq_refine_deep(q, Q, items, N, d, cand, R, k, base, s, r, None)
    return rc, (lib.mf_last_error() if rc else b"")


def test_refusals_of_the_refine_and_their_order(mf):
    lib, E = mf._lib.lib(), mf._lib
    for kw in (dict(q=None), dict(items=None), dict(cand=None), dict(s=None), dict(r=None), dict(Q=0), dict(N=0), dict(Q=2**31)):
        assert _refine(lib, **kw) == (E.MF_EINVAL, b"mf_pq_refine_deep: bad argument"), kw
    order = ((dict(q=None), E.MF_EINVAL, b"bad argument"), (dict(k=1025), E.MF_ENOTSUP, b"k = 1025 outside 1..1024"),
             (dict(R=1025), E.MF_ENOTSUP, b"R = 1025 outside k..1024"), (dict(d=48), E.MF_EINVAL, b"embedding width 48"),
             (dict(base=2**32 - 999), E.MF_ENOTSUP, b"item indices must fit 32 bits"))
    for kw, code, text in order:
        rc, msg = _refine(lib, **kw)
        assert rc == code and msg.startswith(b"mf_pq_refine_deep: ") and text in msg, kw
    for (kw_a, code, text), (kw_b, _, _) in itertools.combinations(order, 2):
        rc, msg = _refine(lib, **kw_a, **kw_b)
        assert rc == code and text in msg, (kw_a, kw_b)
    for kw, text in ((dict(k=0), b"k = 0 outside"), (dict(R=99), b"R = 99 outside k..1024"), (dict(base=-1), b"32 bits"), (dict(N=2**31), b"32 bits")):
        rc, msg = _refine(lib, **kw)
        assert rc == E.MF_ENOTSUP and text in msg, kw
    # the shallow refine keeps its limits
    assert lib.mf_pq_refine(FAKE, 4, FAKE, 1000, 64, FAKE, 400, 100, 0, FAKE, FAKE, None) == E.MF_ENOTSUP
    assert b"k = 100 outside 1..64" in lib.mf_last_error()


def test_the_boundaries_are_accepted(mf):
    """R = 1024 with nprobe = 16 and R = 256 with nprobe = 64 (16,384 keys), every sub-vector length, idx_base + N = 2^32 and an
    exact workspace pass every check: where there is no device the launch itself then fails, past every refusal."""
    lib, E = mf._lib.lib(), mf._lib
    if torch.cuda.is_available():
        return                      # (a launch on fake pointers is only harmless where there is no device: the GPU file runs real ones)
    for allow in (False, True):
        for kw in (dict(C=64, nprobe=16, R=1024, S=1), dict(C=64, nprobe=64, R=256, S=1), dict(base=2**32 - 1000),
                   dict(ws_bytes=3 * 4 * 400 * 8, S=1), dict(S=4), dict(dsub=4), dict(dsub=16), dict(d=256, dsub=4), dict(d=32, dsub=16),
                   dict(R=1), dict(R=257)):
            rc, msg = _scan(lib, allow, **kw)
            assert rc == E.MF_ELAUNCH, (allow, kw, rc, msg)
    for kw in (dict(R=1024, k=1024), dict(R=1, k=1), dict(R=1024, k=1), dict(base=2**32 - 1000), dict(R=257, k=65)):
        assert _refine(lib, **kw)[0] == E.MF_ELAUNCH, kw


# ---------------------------------------------------------------------------------------------------------- plan ----
def test_plan_over_its_domain(mf):
    lib, E = mf._lib.lib(), mf._lib
    out = (ctypes.c_int64 * 4)()
    sliced = beyond = 0
    for nq, nprobe, r, mcb in itertools.product((1, 2, 8, 32, 33, 1024, 100_000), (1, 3, 8, 16, 17, 64), (1, 64, 65, 100, 256, 257, 1000, 1024),
                                                (1, 3, 4, 40, 96, 5000, 200_000)):
        assert lib.mf_pq_deep_plan(nq, nprobe, r, mcb, out) == E.MF_OK
        s, g, wgs, nbytes = out
        assert 1 <= s <= mcb, (nq, nprobe, r, mcb, s)
        if nprobe * r <= pqd.MERGE_KEYS:
            assert nprobe * s * r <= pqd.MERGE_KEYS, (nq, nprobe, r, mcb, s)
        else:
            assert s == 1                                  # (planned with one slice; the scan refuses the shape)
            beyond += 1
        assert s == spec.plan_slices(nq, nprobe, r, mcb) and g == nprobe * s and wgs == nq * g and nbytes == g * nq * r * 8
        assert nbytes <= lib.mf_pq_deep_ws_bytes(nq, nprobe, r, mcb) < nbytes + 256
        if r <= 256:                                       # the shallow plan at the depths both take: the same four words
            shallow = (ctypes.c_int64 * 4)()
            assert lib.mf_pq_plan(nq, nprobe, r, mcb, shallow) == E.MF_OK and list(shallow) == list(out)
        sliced += s > 1
    assert sliced > 100 and beyond > 0
    assert lib.mf_pq_deep_plan(1, 8, 400, 32, out) == E.MF_OK and out[0] == 5             # 16,384 // 3,200
    assert lib.mf_pq_deep_plan(1, 8, 1024, 32, out) == E.MF_OK and out[0] == 2
    assert lib.mf_pq_deep_plan(1, 8, 400, 96, None) == E.MF_EINVAL and lib.mf_last_error() == b"mf_pq_deep_plan: out is NULL"
    for bad in ((0, 8, 400, 96), (1, 0, 400, 96), (1, 65, 400, 96), (1, 8, 0, 96), (1, 8, 1025, 96), (1, 8, 400, 0)):
        assert lib.mf_pq_deep_plan(*bad, out) == E.MF_EINVAL and lib.mf_pq_deep_ws_bytes(*bad) == 0, bad
        assert b"R in 1..1024 and nprobe in 1..64" in lib.mf_last_error()
    assert lib.mf_pq_plan(1, 8, 257, 96, out) == E.MF_EINVAL and lib.mf_pq_ws_bytes(1, 8, 257, 96) == 0       # the shallow plan keeps its limit


def test_the_python_plan_goes_to_the_deep_export(mf):
    R = mf.retrieval
    quant = object.__new__(R.QuantizedIndex)
    quant.num_probes, quant.num_partitions, quant.refine_factor, quant.max_cell_blocks = 8, 64, 4, 96
    for nq, top_k, nprobe, rf in ((1, 100, 8, 4), (33, 256, 3, 4), (1, 1000, 16, 1), (1024, 65, 1, 1), (1, 20, 8, 13)):
        got = quant.plan(nq, top_k, nprobe, rf, path="pq_deep")
        s = spec.plan_slices(nq, nprobe, rf * top_k, 96)
        assert got == {"slices": s, "lists": nprobe * s, "workgroups": nq * nprobe * s, "bytes": nprobe * s * nq * rf * top_k * 8}
    assert quant.plan(1, 100, path="pq_deep") == quant.plan(1, 100, 8, 4, path="pq_deep")
    assert quant.plan(1, 20, 8, 4, path="pq_deep") == quant.plan(1, 20, 8, 4)                # (depths both take: one rule)
    for kw in (dict(top_k=1025), dict(top_k=0), dict(top_k=300), dict(nprobe=0), dict(nprobe=65), dict(top_k=1024, refine_factor=1, nprobe=17),
               dict(num_queries=0), dict(refine_factor=0)):
        with pytest.raises(ValueError):
            quant.plan(**{"num_queries": 1, "top_k": 100, "path": "pq_deep", **kw})
    with pytest.raises(ValueError):
        quant.plan(1, 100)                                                                   # path="pq" keeps its limits


# ----------------------------------------------------------------------------------------------------- resources ----
def test_the_new_kernels_have_no_spill_no_scratch_and_the_lds_they_document():
    s = importlib.util.spec_from_file_location("kernel_resources", ROOT / "tools" / "kernel_resources.py")
    kr = importlib.util.module_from_spec(s)
    s.loader.exec_module(kr)
    table = kr.kernel_resources()
    c = deep.constants()

    def args(name):
        return tuple(int(x) for x in name.split("<")[1].split(">")[0].split(","))

    pairs = sorted((d // dsub, dsub) for d in (32, 64, 128, 256) for dsub in (4, 8, 16))           # (M, dsub)
    for stem in ("pq_deep_scan_kernel<", "pq_deep_scan_allow_kernel<"):
        scan = {args(n): r for n, r in table.items() if stem in n}
        assert sorted(scan) == pairs and len(scan) == 12, (stem, sorted(scan))
        for (m, dsub), r in scan.items():
            assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0 and r["max_flat_workgroup_size"] == 256, (m, dsub, r)
            assert r.get("sgpr_spill_count", 0) == 0 and r["vgpr_count"] + r["agpr_count"] <= 128, (m, dsub, r)
            # the query's tables (M KiB), the deep scan's buffer and the waves' counts: static, one workgroup at least in a CU's 160 KiB
            assert r["group_segment_fixed_size"] == m * 1024 + c["IVFD_BUF"] * 8 + 16 <= 160 * 1024, (m, dsub, r)
        assert scan[(2, 16)]["group_segment_fixed_size"] == 34 * 1024 + 16 and scan[(64, 4)]["group_segment_fixed_size"] == 96 * 1024 + 16
    refine = {args(n): r for n, r in table.items() if "pq_refine_deep_kernel<" in n}
    assert sorted(refine) == [(32,), (64,), (128,), (256,)]
    for d, r in refine.items():
        assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0 and r["max_flat_workgroup_size"] == 256, (d, r)
        assert r["group_segment_fixed_size"] == 1024 * 8 and r["vgpr_count"] + r["agpr_count"] <= 128, (d, r)     # 1,024 keys
    # the names the other tests select by are the parent's kernels alone
    count = lambda stem: sum(stem in n for n in table)  # noqa: E731
    assert count("pq_scan_kernel") == 12 and count("pq_scan_allow_kernel<") == 12 and count("pq_refine_kernel") == 4
    assert count("ivf_scan_deep_kernel<") == 4 and count("ivf_scan_deep_allow_kernel<") == 4 and count("scan_deep") == 8


def test_the_buffer_constants_are_still_the_six():
    c = deep.constants()
    assert c == {"IVFD_PASS": 256, "IVFD_KP_MIN": 128, "IVFD_KP_MAX": 1024, "IVFD_BUF_MIN": 2048, "IVFD_BUF": 4096, "IVFD_SORT_MIN": 512}
    csrc = ROOT / "matrix-factorization-torch_amd" / "csrc"
    # one sort, one kept rule, one capacity rule: the quantised deep scan is text of the unit that defines them
    for word in ("void ivfd_sort_desc(", "int ivfd_kept(", "int ivfd_capacity("):
        assert sum(p.read_text().count(word) for p in csrc.iterdir() if p.is_file()) == 1, word
    assert '#include "mf_pq_deep_scan.inc"' in (csrc / "mf_ivf_deep.hip").read_text()
    shared = (csrc / "mf_pq_tables.h").read_text()
    for unit in ("mf_pq.hip", "mf_ivf_deep.hip"):
        text = (csrc / unit).read_text()
        assert '#include "mf_pq_tables.h"' in text, unit
        for word in ("struct PqScanParams", "float pq_chain(", "void pq_load_sub(", "bool pq_dsub_ok(", "define PQ_DISPATCH(", "int PQ_MAX_M"):
            assert word in shared and word not in text, (unit, word)


# -------------------------------------------------------------------------------------------------------- python ----
def test_serving_path_and_default_path(mf):
    R = mf.retrieval
    exact, cells, quant = (object.__new__(cls) for cls in (R.ItemIndex, R.PartitionedIndex, R.QuantizedIndex))
    depths = (1, 64, 65, 100, 1024)
    assert [exact.serving_path(k) for k in depths] == [exact.default_path(k) for k in depths] == ["auto"] * 5
    assert [cells.serving_path(k) for k in depths] == [cells.default_path(k) for k in depths] == ["cells", "cells", "cells_deep", "cells_deep",
                                                                                                  "cells_deep"]
    assert [quant.serving_path(k) for k in depths] == ["pq", "pq", "pq_deep", "pq_deep", "pq_deep"]
    assert [quant.default_path(k) for k in depths] == ["pq"] * 5                             # left as it is


def test_the_python_refusals_and_their_messages(mf):
    R = mf.retrieval
    quant = object.__new__(R.QuantizedIndex)
    quant.num_probes, quant.num_partitions, quant.refine_factor = 8, 64, 4
    quant._ws, quant._cells = {}, None
    # refused before the queries are looked at: an index that holds nothing but its numbers has nothing to launch with
    for top_k, nprobe, rf, text in ((0, 8, 4, "1..1024 rows per query"), (1025, 8, 1, "1..1024 rows per query"),
                                    (257, 8, 4, "refine_factor \\* top_k must not exceed 1024"), (1024, 1, 2, "must not exceed 1024"),
                                    (20, 1, 52, "must not exceed 1024"), (1024, 17, 1, "must not exceed 16384"),
                                    (100, 64, 4, "must not exceed 16384"), (257, 64, 1, "nprobe \\* refine_factor \\* top_k"),
                                    (100, 65, 4, "nprobe must be in 1..64"), (100, 0, 4, "nprobe must be"), (100, 8, 0, "refine_factor must be at least 1")):
        with pytest.raises(ValueError, match=text):
            quant.search(None, top_k, nprobe=nprobe, refine_factor=rf, path="pq_deep")
    with pytest.raises(ValueError, match="must not exceed 1024"):
        quant.search(None, 300, path="pq_deep")                           # the index's own factor: 4 * 300
    with pytest.raises(NotImplementedError, match="takes no filter"):
        quant.search(None, 100, path="pq_deep", where=R.TagFilter(all_of=1))
    with pytest.raises(ValueError, match="give one of them"):
        quant.search(None, 100, path="pq_deep", allow=object(), where=object())
    with pytest.raises(ValueError, match="it needs one"):
        quant.search(None, 100, path="pq_deep", allow_of=[0])
    with pytest.raises(ValueError, match="no bitmap route"):
        quant.search(None, 100, path="deep", allow=object())
    # path="pq" refuses what it refused
    for top_k, rf in ((100, 4), (65, 1), (64, 5)):
        with pytest.raises(ValueError):
            quant.search(None, top_k, refine_factor=rf, path="pq")
    with pytest.raises(ValueError, match="1..256"):
        quant.candidates(None, 257)
    for r in (0, 1025):
        with pytest.raises(ValueError, match="1..1024"):
            quant.candidates(None, r, path="pq_deep")
    with pytest.raises(ValueError, match="path in"):
        quant.candidates(None, 100, path="cells_deep")
    quant.max_cell_blocks = 40
    for slices in (0, 41, 3):                                               # 8 * 3 * 1000 keys
        with pytest.raises(ValueError, match="slices"):
            quant.candidates(None, 1000, slices=slices, path="pq_deep")
    assert quant._ws == {} and quant._cells is None


def test_the_config_rule_on_both_sides_of_64(mf):
    Config = mf.lightning.MatrixFactorizationLitConfig
    base = dict(num_users=50, num_items=600, hidden_size=64, index_type="quantized")
    # up to 64 rows: the rule of before
    for rf, top_k in ((4, 20), (4, 64), (12, 20), (256, 1), (1, 64)):
        assert Config(**base, refine_factor=rf, top_k=top_k).top_k == top_k
    for rf, top_k in ((13, 20), (5, 64), (129, 2)):
        with pytest.raises(ValueError, match="at most 256 candidates"):
            Config(**base, refine_factor=rf, top_k=top_k)
    # beyond: the deep search's limits, each named
    for rf, top_k, probes in ((4, 100, 8), (4, 256, 16), (1, 1024, 16), (1, 65, 64), (10, 100, 16), (1, 256, 64), (15, 65, 8)):
        cfg = Config(**base, refine_factor=rf, top_k=top_k, num_probes=probes)
        assert (cfg.refine_factor, cfg.top_k, cfg.num_probes) == (rf, top_k, probes)
    for rf, top_k, probes, text in ((1, 1025, 1, "at most 1024 rows"), (4, 257, 1, "at most 1024 candidates"), (11, 100, 1, "at most 1024 candidates"),
                                    (16, 65, 1, "at most 1024 candidates"), (1, 1024, 17, "at most 16384 candidates"),
                                    (4, 100, 41, "num_probes \\* refine_factor \\* top_k = 16400"), (1, 257, 64, "at most 16384")):
        with pytest.raises(ValueError, match=text):
            Config(**base, refine_factor=rf, top_k=top_k, num_probes=probes)
    # the other index types never meet the rule
    assert Config(**{**base, "index_type": "partitioned"}, refine_factor=13, top_k=1024).top_k == 1024
    assert Config(**{**base, "index_type": "exact"}, refine_factor=13, top_k=300).top_k == 300


# ------------------------------------------------------------------------- the long cell: the settles it reaches ----
def test_the_case_set_holds_what_the_gpu_assertions_lean_on():
    cs = pqd.cases()
    widths = {c.base.items.shape[1] for c in cs.values()}
    assert widths >= {32, 48, 64, 128, 256} and {c.dsub for c in cs.values()} == {4, 8, 16}
    assert {c.m for c in cs.values()} >= {2, 4, 8, 16, 32, 64}
    assert cs["pqd_w256_m32_k1024"].m == 32 and cs["pqd_w256_m64_k1024"].m == 64 and cs["pqd_w256_m32_k1024"].r == cs["pqd_w256_m64_k1024"].r == 1024
    assert {c.base.items.shape[0] for c in cs.values()} >= {33, 1000, 2500} and {c.base.q.shape[0] for c in cs.values()} >= {1, 33, 70}
    assert {(c.base.k, c.refine_factor) for c in cs.values()} >= {(65, 1), (100, 4), (256, 4), (1000, 1), (1024, 1)}
    assert {c.base.nprobe for c in cs.values()} >= {1, 3, 8, 16}
    assert all(c.base.k > 64 and c.r <= 1024 and c.base.nprobe * c.r <= pqd.MERGE_KEYS for c in cs.values())
    assert {c.base.nprobe * c.r for c in cs.values()} >= {pqd.MERGE_KEYS}
    assert {len(e) for c in cs.values() if c.base.exclude for e in c.base.exclude} >= {0, 1, 17, 1025}
    assert cs["pqd_idx_base"].base.idx_base == cs["pqd_idx_base_no_lists"].base.idx_base == 1000 and cs["pqd_idx_base_no_lists"].base.exclude is None
    c = cs["pqd_cell_sizes"].base
    assert c.sizes[:5].tolist() == [0, 1, 63, 64, 65] and spec.ivf.probes(c.q, c.centroids, c.nprobe)[0, 0] == 0


@pytest.mark.parametrize("order", pqd.LONG_ORDERS)
def test_the_long_cell_settles_under_a_live_bound(order):
    """A condition on the inputs of the GPU test: another seed or a longer cell if it fails, never a weaker condition.  The
    ascending order fills the buffer again and again -- three settles and more under a live bound at every depth, as one slice
    --; the descending one settles once inside the loop and then turns every key away (no order of the rows can do both); the
    shuffled one meets a live bound that turns most keys away."""
    n = deep.settle_rows()
    c = pqd.long_cell(order)
    approx = pqd.long_approx(order)
    assert c.base.items.shape == (n, 32) and (c.m, c.dsub) == (4, 8) and n == 13288 and -(-n // 64) == pqd.LONG_BLOCKS
    steps = np.diff(approx)
    if order == "ascending":
        assert (steps >= 0).all() and (steps > 0).sum() > n - 200
    elif order == "descending":
        assert (steps <= 0).all() and (steps < 0).sum() > n - 200
    else:
        assert 0.4 < (steps > 0).mean() < 0.6
    rows = np.arange(n)
    for r in pqd.LONG_DEPTHS:
        w = deep.walk(approx, r, np.ones(n, dtype=bool), rows)
        live = [s for s in w["settles"] if s[1]]
        want = rows[np.argsort(spec.keys(approx, rows + pqd.LONG_BASE))[::-1][:r]]
        assert w["rows"] == want.tolist(), (order, r)
        if order == "ascending":
            assert len(live) >= 3 and sum(s[2] for s in live) >= 3, (order, r, w["settles"])
        elif order == "descending":
            assert [s[1:3] for s in w["settles"]] == [(False, True)], (order, r, w["settles"])
        else:
            assert len(live) >= 1 and sum(s[0] for s in w["settles"]) < n - r, (order, r, w["settles"])
        one, planned, most = pqd.long_slices(r)
        assert one == 1 and planned == {100: 52, 1000: 16, 1024: 16}[r] and most == {100: 163, 1000: 16, 1024: 16}[r]
        lists = pqd.long_lists(order, r, most)
        assert lists.shape == (most, r) and (lists[:, : min(r, 64)] != -1).all()
        assert np.array_equal(pqd.long_lists(order, r, 1)[0], pqd.packed(approx[want], want + pqd.LONG_BASE))


# ---------------------------------------------------------------------------------------------------- the record ----
def test_the_digest_record_shows_the_parents_kernels_unchanged():
    """profiles/pq_deep_digest_{parent,branch}.json: ``tools/kernel_resources.py --text-digest`` of the parent's library and of this
    one with one ``--only=`` list, the branch's record cut to the kernels the parent's names (``--names-of=``): every kernel of
    mf_ivf.hip, mf_ivf_deep.hip, mf_pq.hip, mf_filter.hip and the top-k units.  The two records are equal: same kernels, same
    instruction text, same resource figures -- the helpers moved into csrc/mf_pq_tables.h and the scans added to the unit of
    the deep cell scan left every kernel of before as it was."""
    parent = json.loads((ROOT / "profiles" / "pq_deep_digest_parent.json").read_text())
    branch = json.loads((ROOT / "profiles" / "pq_deep_digest_branch.json").read_text())
    assert branch == parent and all(len(v["text_sha256"]) == 64 for v in parent.values())
    count = lambda unit: sum(unit in k for k in parent)  # noqa: E731
    assert count("ivf_scan_kernel<") == 4 and count("ivf_scan_allow_kernel<") == 4 and count("ivf_cell_mean_kernel") == 1
    assert count("ivf_scan_deep_kernel<") == 4 and count("ivf_scan_deep_allow_kernel<") == 4
    assert count("pq_scan_kernel<") == 12 and count("pq_scan_allow_kernel<") == 12 and count("pq_encode_kernel") == 3 and count("pq_refine_kernel") == 4
    for unit in ("filter_mark_kernel", "filter_pack_kernel", "filter_remap_kernel", "filter_unmap_kernel", "filter_lists_count_kernel",
                 "filter_lists_scan_kernel", "filter_lists_write_kernel", "filter_cell_bits", "topk_small_scan_kernel", "topk_small_mfma_scan_kernel",
                 "bf3_scan_kernel", "bf3_final_kernel", "topk_deep_slab_kernel", "topk_deep_select_kernel", "topk_merge_kernel",
                 "topk_merge_deep_kernel", "topk_pack_kernel", "select_kernel", "select_seed_kernel", "target_positions_kernel"):
        assert count(unit) >= 1, unit
    assert not any("pq_deep_scan" in k or "pq_refine_deep" in k for k in parent)
    # the library that is built now has every one of them under the same name, and the new kernels beside them
    s = importlib.util.spec_from_file_location("kernel_resources", ROOT / "tools" / "kernel_resources.py")
    kr = importlib.util.module_from_spec(s)
    s.loader.exec_module(kr)
    built = set(kr.kernel_resources())
    assert set(parent) <= built and sum("pq_deep_scan" in k for k in built) == 24 and sum("pq_refine_deep_kernel" in k for k in built) == 4
