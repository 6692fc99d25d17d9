"""CPU: the host side of the deep cell scan (csrc/mf_ivf_deep.hip, ``PartitionedIndex.search(path="cells_deep")``) -- the four
exports, every refusal of the two scans and of the plan with their order (all decided before any launch: never-dereferenced fake
pointers do), the plan over its domain, the kernels' resources from the code objects' notes, the buffer's constants read from
the source with what the GPU test of several settles leans on, the long cell under masks, lists and ties (what
tests/test_gpu_ivf_deep_settles.py leans on: its inputs reach the settles they are chosen for and tell wrong kernels apart),
``default_path``, the Python refusals, the deep case set, and the digest record."""
from __future__ import annotations

import ctypes
import importlib.util
import itertools
import json
import pathlib

import numpy as np
import pytest
import torch

from oracle import chain
from tests import _cell_mask_spec as cell_mask_spec
from tests import _filter_spec
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


# ------------------------------------------------------- the long cell under masks, lists and ties: the inputs ----
# What tests/test_gpu_ivf_deep_settles.py leans on, from the walk with admission (``deep.walk(scores, k, admitted, rows)``): its
# inputs drive the buffer where they are meant to, and they tell a subtly wrong kernel from the right one.
WIDTHS = (64, 256)
GPU_MASKS = {64: tuple(deep.SETTLE_MASKS), 256: ("half", "every other block")}      # the masks the GPU file runs at each width


def _walk(d, i, k, mask="all", lists=None, lo=0, hi=None, **kw):
    """The walk of query i over positions ``[lo, hi)`` of the long cell of width d."""
    hi = deep.settle_rows() if hi is None else hi
    admitted = deep.settle_admitted(d, mask, lists)[i]
    return deep.walk(deep.long_scores(d)[i][lo:hi], k, admitted[lo:hi], deep.long_rows(d)[lo:hi], **kw)


def _in_loop_live(w):
    return sum(live and inside for _, live, inside, _ in w["settles"])


def test_the_walk_without_admission_is_the_walk_of_before():
    scores = deep.settle_scores("shuffled")
    n = scores.size
    plain = deep.walk(scores, 100)
    assert set(plain) == {"settles", "best"} and all(len(s) == 2 for s in plain["settles"])
    full = deep.walk(scores, 100, np.ones(n, dtype=bool), np.arange(n))
    assert [s[:2] for s in full["settles"]] == plain["settles"] and full["best"] == plain["best"] == full["rows"]
    for waiting, _, inside, length in full["settles"]:
        assert inside == (waiting > deep.room_of(100)) and length >= max(512, 128 + waiting) and (length == 512 or length // 2 < 128 + waiting)
    assert [deep.room_of(k) for k in deep.SETTLE_DEPTHS] == [1664, 1536, 1280, 2816]
    assert [deep.kept(k) for k in deep.SETTLE_DEPTHS] == [128, 256, 512, 1024]


@pytest.mark.parametrize("d", WIDTHS)
def test_the_settle_catalog_is_what_the_gpu_file_takes_it_for(d):
    c = deep.settle_catalog(d)
    n = deep.settle_rows()
    rows, scores = deep.long_rows(d), deep.long_scores(d)
    assert c.sizes.tolist() == [150, n, 70] == list(deep.settle_sizes()) and n == 13288 and -(-n // 64) == 208 and n % 64 == 40
    assert c.idx_base == deep.SETTLE_BASE == 30 and c.max_cell_blocks == 208 and c.items.shape == (13508, d)
    # position is not row: the long cell begins at block 3 of the mask, and its rows are no shifted range
    assert -(-150 // 64) == deep.SETTLE_FIRST_BLOCK == 3
    assert np.unique(rows - np.arange(n)).size > 100 and (np.diff(rows) > 0).all()
    # query 0 ascends along the cell, query 1 is its negation to the bit, query 2 neither ascends nor descends
    assert (np.diff(scores[0]) >= 0).all() and (np.diff(scores[0]) > 0).sum() > n - 50
    assert np.array_equal((-scores[0]).view(np.uint32), scores[1].view(np.uint32)) and not (scores == 0).any()
    up = (np.diff(scores[2]) > 0).mean()
    assert 0.4 < up < 0.6
    # queries 0 and 2 probe the long cell at nprobe = 1; query 1 cannot (its score with centroid 1 is -1)
    probed = spec.probes(c.q, c.centroids, 1)[:, 0].tolist()
    assert probed[0] == probed[2] == deep.SETTLE_CELL != probed[1]
    # the in-cell oracle is the spec at nprobe = 1 for the queries that probe the cell, and numpy's selection is the oracle's
    lists = deep.settle_lists("long and scattered", d, 100, "half")
    every = _filter_spec.extended_lists(lists, 3, deep.settle_ok("half", d), c.idx_base)
    ws, wr = spec.expected(c.q, c.items, c.centroids, c.assign, 100, 1, every, c.idx_base)
    gs, gr = deep.settle_expected(d, 100, "half", lists)
    admitted = deep.settle_admitted(d, "half", lists)
    for i in range(3):
        if i != 1:
            assert np.array_equal(gr[i], wr[i]) and np.array_equal(gs[i].view(np.uint32), ws[i].view(np.uint32)), i
        best = deep.best_first(scores[i], rows, admitted[i], 0, n)[:100]
        assert np.array_equal(rows[best] + c.idx_base, gr[i]) and np.array_equal(scores[i][best].view(np.uint32), gs[i].view(np.uint32)), i
        assert _walk(d, i, 100, "half", lists)["rows"] == rows[best].tolist(), i


def test_the_masks_and_the_lists_are_what_their_names_say():
    n = deep.settle_rows()
    count = {name: int(deep.settle_mask(name).sum()) for name in deep.SETTLE_MASKS}
    assert count["all"] == n and count["none"] == 0 and count["last block only"] == 40 and count["late"] == n - 3000
    assert 0.48 * n < count["half"] < 0.52 * n and count["every other block"] == 104 * 64 and count["one block in five"] == n - 41 * 64
    # tails: the last block alone leaves fewer than k rows at every depth
    assert count["last block only"] < min(deep.SETTLE_DEPTHS)
    # zero words in a pass of four waves: none, one beside three live waves, two, all four
    live_word = {name: np.pad(deep.settle_mask(name), (0, 24)).reshape(52, 4, 64).any(axis=2) for name in deep.SETTLE_MASKS}
    zero_words = {name: set((4 - w.sum(axis=1)).tolist()) for name, w in live_word.items()}
    assert zero_words["one block in five"] == {0, 1} and zero_words["every other block"] == {2} and zero_words["late"] == {4, 2, 0}
    assert zero_words["last block only"] == {4, 3} and zero_words["none"] == {4} and zero_words["all"] == zero_words["half"] == {0}
    ok = deep.settle_ok("half", 64)
    c = deep.settle_catalog(64)
    assert ok[c.assign != deep.SETTLE_CELL].all() and np.array_equal(ok[deep.long_rows(64)], deep.settle_mask("half"))
    for d in WIDTHS:
        c = deep.settle_catalog(d)
        inside = set((deep.long_rows(d) + c.idx_base).tolist())
        for k in (100, 1000):
            for mask in ("all", "half"):
                admitted = deep.settle_mask(mask)
                best, scattered, three = (deep.settle_lists(f, d, k, mask) for f in deep.SETTLE_LISTS)
                for i in range(3):
                    assert len(set(best[i])) == len(best[i]) == 2 * k and set(best[i]) <= inside
                    assert len(scattered[i]) == 1025 + 40 + 2 and c.idx_base - 1 in scattered[i] and c.idx_base + 13508 in scattered[i]
                    assert len(set(scattered[i]) & inside) == 1025 and len(set(scattered[i]) - inside) == 42
                    assert len(three[i]) == int(admitted.sum()) - 3 and int(deep.settle_admitted(d, mask, three)[i].sum()) == 3
                assert list(best[0]) != sorted(best[0]) and best[0] != best[2]


@pytest.mark.parametrize("d", WIDTHS)
def test_the_ascending_query_settles_inside_the_loop_under_a_live_bound(d):
    """A condition on the inputs: another seed or a longer cell if it fails, never a weaker condition."""
    live = []
    for k in deep.SETTLE_DEPTHS:
        w = _walk(d, 0, k)
        live.append(sum(s[1] for s in w["settles"]))
        assert _in_loop_live(w) >= 2, (k, w["settles"])
        for mask, lists in (("half", None), ("every other block", None), ("half", deep.settle_lists("long and scattered", d, k, "half"))):
            w = _walk(d, 0, k, mask, lists)
            assert _in_loop_live(w) >= 1, (k, mask, lists is not None, w["settles"])
        for family in deep.SETTLE_LISTS[:2]:                # the lists meet a live bound in the plain kernel too
            assert _in_loop_live(_walk(d, 0, k, "all", deep.settle_lists(family, d, k))) >= 1, (k, family)
    assert live == [7, 7, 8, 4]                             # every key beats the bound: 13,288 rows in settles of 1792 / 1792 / 1536 / 3072
    # the descending query: one settle inside the loop, then nothing beats the bound; the third: live settles, not all keys
    for k in deep.SETTLE_DEPTHS:
        assert [s[1:3] for s in _walk(d, 1, k)["settles"]] == [(False, True)], k
        w = _walk(d, 2, k)
        assert _in_loop_live(w) >= 1 and sum(s[0] for s in w["settles"]) < deep.settle_rows() - k, (k, w["settles"])


def test_every_sort_length_runs_and_each_under_a_live_bound():
    n = deep.settle_rows()
    lengths, live = set(), set()
    for d in WIDTHS:
        for mask in GPU_MASKS[d]:
            for k in deep.SETTLE_DEPTHS:
                for i in range(3):
                    for slices in (1, 3):
                        for s in range(slices):
                            w = _walk(d, i, k, mask, lo=min(n, 64 * (208 * s // slices)), hi=min(n, 64 * (208 * (s + 1) // slices)))
                            lengths |= {length for _, _, _, length in w["settles"]}
                            live |= {length for _, was_live, _, length in w["settles"] if was_live}
    assert lengths == live == {512, 1024, 2048, 4096}


@pytest.mark.parametrize("d", WIDTHS)
def test_depths_200_and_500_settle_by_their_own_class(d):
    """Class 512 is the boundary of ``ivfd_capacity`` (4 * 512 == IVFD_BUF_MIN): room 1280, where class 256 has 1536.  The cases
    tell the two rules apart: a walk with the other class's room settles at other passes."""
    for k, room, other in ((500, 1280, 1536), (200, 1536, 1280)):
        assert deep.room_of(k) == room
        for i, mask in ((0, "all"), (0, "half"), (2, "all")):
            right, wrong = _walk(d, i, k, mask), _walk(d, i, k, mask, room=other)
            inside = [waiting for waiting, _, begun, _ in right["settles"] if begun]
            assert len(inside) >= 2 and all(room < waiting <= room + 256 for waiting in inside), (k, i, mask, right["settles"])
            assert [s[0] for s in wrong["settles"]] != [s[0] for s in right["settles"]], (k, i, mask)
            assert wrong["best"] == right["best"]          # (the rule decides when the buffer is sorted and whether it overflows, not the list)
    assert 512 + 1536 + 256 > deep.capacity(512)            # class 256's room at kept part 512: a full pass more would not fit


def test_the_slicings_of_the_long_cell(mf):
    """Three queries on one probe: the plan cuts the 208 blocks into 52 / 52 / 32 / 16 slices; the deepest slicing the merge holds
    is a list per 1.3 ... 13 blocks.  Slices of four blocks exactly at k = 100 and 200 -- the slicings of 3 and the deepest have
    the ragged last passes."""
    lib = mf._lib.lib()
    out = (ctypes.c_int64 * 4)()
    planned = []
    for k in deep.SETTLE_DEPTHS:
        assert lib.mf_ivf_deep_plan(3, 1, k, 208, out) == 0
        planned.append(out[0])
    assert planned == [52, 52, 32, 16] and [min(208, deep.MERGE_KEYS // k) for k in deep.SETTLE_DEPTHS] == [163, 81, 32, 16]
    assert [208 * (s + 1) // 3 - 208 * s // 3 for s in range(3)] == [69, 69, 70]


# ---- the inputs tell wrong kernels apart: each restated in a few lines, each differs from the spec on a case of the set
def test_a_mask_applied_by_row_gives_another_list():
    d, k = 64, 100
    c = deep.settle_catalog(d)
    rows, n = deep.long_rows(d), deep.settle_rows()
    cell_blk, row_of = cell_mask_spec.layout(c.assign, 3)
    assert cell_blk.tolist() == [0, 3, 211, 213] and np.array_equal(row_of[192: 192 + n], rows)
    for mask in ("half", "every other block", "late"):
        ok = deep.settle_ok(mask, d)
        bits = (row_of >= 0) & ok[np.clip(row_of, 0, None)]                      # the words, a bit per padded position
        assert np.array_equal(bits[192: 192 + n], deep.settle_mask(mask))
        by_row = bits[rows]                                                      # the wrong kernel: bit number `row`, not `position`
        want = deep.settle_expected(d, k, mask)[1]
        for i in range(3):
            wrong = rows[deep.best_first(deep.long_scores(d)[i], rows, by_row, 0, n)[:k]] + c.idx_base
            assert not np.array_equal(wrong, want[i]), (mask, i)


def test_ties_broken_by_position_give_another_list():
    n, row_of = deep.settle_rows(), deep.tie_row_of()
    c = deep.tie_catalog()
    assert sorted(row_of[:n].tolist()) == list(range(n)) and (row_of[n:] == -1).all() and row_of.size == 208 * 64
    assert 0.2 < (np.diff(row_of[:n]) > 0).mean() < 0.8                     # neither ascending nor descending from one position to the next
    assert (c.items == c.items[0]).all() and np.array_equal(c.q, c.items[:1]) and c.idx_base == 30
    scores = np.full(n, chain.scores(c.q, c.items[:1])[0, 0], dtype=np.float32)
    for mask in ("all", "half"):
        admitted = deep.settle_mask(mask)
        for k in deep.TIE_DEPTHS:
            for slices in (1, 3):
                for s in range(slices):
                    lo, hi = min(n, 64 * (208 * s // slices)), min(n, 64 * (208 * (s + 1) // slices))
                    right = deep.walk(scores[lo:hi], k, admitted[lo:hi], row_of[lo:hi])
                    want = np.sort(row_of[lo:hi][admitted[lo:hi]])[:k].tolist()
                    assert right["rows"] == want, (mask, k, slices, s)
                    # a later pass holds better tied keys: the bound is live and still moves (half a slice of three at k = 1000
                    # is 2,200 keys, fewer than a first settle's 2,816: the whole cell below does it)
                    assert mask == "half" or sum(live for _, live, _, _ in right["settles"]) >= 1, (mask, k, slices, s)
                    by_position = deep.walk(scores[lo:hi], k, admitted[lo:hi])      # the wrong kernel: the key holds the position
                    assert row_of[lo:hi][by_position["best"]].tolist() != want, (mask, k, slices, s)
            assert _in_loop_live(deep.walk(scores, k, admitted, row_of[:n])) >= 1, (mask, k)


def test_excluded_keys_that_enter_the_bound_give_a_short_list():
    d = 64
    c = deep.settle_catalog(d)
    rows, n = deep.long_rows(d), deep.settle_rows()
    for k in (100, 1000):
        for mask in ("all", "half"):
            lists = deep.settle_lists("the best 2k", d, k, mask)
            want = deep.settle_expected(d, k, mask, lists)[1]
            assert (want >= 0).all()                                             # the right kernel fills its list
            for i in range(3):
                # the wrong kernel: a listed key waits and is kept like any other, and is dropped when the list is written
                held = deep.walk(deep.long_scores(d)[i], k, deep.settle_mask(mask), rows)["rows"]
                left = [r + c.idx_base for r in held if r + c.idx_base not in set(lists[i])]
                assert left == [] and left != want[i].tolist(), (k, mask, i)


def test_a_word_read_past_the_slices_end_gives_another_list():
    """A wave past ``b1`` that took its block's word would admit rows of the next slice.  The slices of 3 and of the deepest
    slicing are no multiples of four blocks, so the last pass of a slice has such waves."""
    d, n = 64, deep.settle_rows()
    rows = deep.long_rows(d)
    for k in deep.SETTLE_DEPTHS:
        for slices in (3, min(208, deep.MERGE_KEYS // k)):
            ragged = differs = 0
            for s in range(slices):
                b0, b1 = 208 * s // slices, 208 * (s + 1) // slices
                over = min(208, b0 + -(-(b1 - b0) // 4) * 4)                     # the blocks the slice's last pass covers
                ragged += over > b1
                for i, mask in ((0, "all"), (2, "half")):
                    admitted = deep.settle_mask(mask)
                    right = deep.best_first(deep.long_scores(d)[i], rows, admitted, 64 * b0, min(n, 64 * b1))[:k]
                    wrong = deep.best_first(deep.long_scores(d)[i], rows, admitted, 64 * b0, min(n, 64 * over))[:k]
                    differs += not np.array_equal(right, wrong)
            assert ragged >= 2 and differs >= 2, (k, slices, ragged, differs)


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
