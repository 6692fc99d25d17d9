"""CPU: the host side of the in-place filter of the cell scans (``mf_filter_cell_bits``, ``mf_ivf_scan_allow``,
``mf_pq_scan_allow``; ``retrieval.CellMask``, ``filter_mode``) -- the exports and their argument types, every refusal on calls
that never launch (fake pointers are never dereferenced) and the order of the refusals, the kernels' resources from the code
object's notes, the numpy spec on hand-worked rows, the ``filter_mode`` setting, and the digest record."""
from __future__ import annotations

import ctypes
import importlib.util
import json
import pathlib

import numpy as np
import pytest

from tests import _cell_mask_spec as spec

ROOT = pathlib.Path(__file__).resolve().parents[1]
FAKE = ctypes.c_void_p(0x1000)


def test_exports_are_declared_bound_documented_and_present(mf):
    lib, L = mf._lib.lib(), mf._lib
    header = (ROOT / "include" / "mf_hip.h").read_text()
    guide = (ROOT / "INTEGRATION.md").read_text()
    for name in ("mf_filter_cell_bits", "mf_ivf_scan_allow", "mf_pq_scan_allow"):
        assert hasattr(lib, name) and name in L.SIGNATURES and f"int {name}(" in header and name in guide, name
    vp, i64, u64, sz, i = L.c_vp, L.c_i64, L.c_u64, L.c_sz, L.c_int
    assert L.SIGNATURES["mf_filter_cell_bits"] == (i, [vp, i64, u64, u64, u64, vp, i64, vp, vp])
    # every argument of the scan in its order, and before ws: allow, n_masks, allow_of
    for scan in ("mf_ivf_scan", "mf_pq_scan"):
        ret, args = L.SIGNATURES[scan]
        assert args[-3:] == [vp, sz, vp]
        assert L.SIGNATURES[scan + "_allow"] == (ret, [*args[:-3], vp, i64, vp, *args[-3:]]), scan


# ------------------------------------------------------------------------------------------------------ refusals ----
def _bits(lib, **kw):
    a = dict(tags=FAKE, N=1000, row_of=FAKE, Npad=1024, out=FAKE)
    a.update(kw)
    rc = lib.mf_filter_cell_bits(a["tags"], a["N"], 1, 2, 4, a["row_of"], a["Npad"], a["out"], None)
    return rc, (lib.mf_last_error() if rc else b"")


SCAN = dict(q=FAKE, Q=4, blocked=FAKE, cell_blk=FAKE, row_of=FAKE, Npad=1024, N=1000, C=8, d=64, mcb=4, probes=FAKE, nprobe=2, depth=20,
            S=1, excl_off=None, excl_idx=None, base=0, allow=FAKE, n_masks=1, allow_of=None, ws=FAKE, ws_bytes=1 << 24)


def _ivf(lib, **kw):
    a = {**SCAN, **kw}
    rc = lib.mf_ivf_scan_allow(a["q"], a["Q"], a["blocked"], a["cell_blk"], a["row_of"], a["Npad"], a["N"], a["C"], a["d"], a["mcb"],
                               a["probes"], a["nprobe"], a["depth"], a["S"], a["excl_off"], a["excl_idx"], a["base"], a["allow"],
                               a["n_masks"], a["allow_of"], a["ws"], a["ws_bytes"], None)
    return rc, (lib.mf_last_error() if rc else b"")


def _pq(lib, **kw):
    a = {**SCAN, "codebooks": FAKE, "dsub": 8, "scores": FAKE, **kw}
    rc = lib.mf_pq_scan_allow(a["q"], a["Q"], a["blocked"], a["codebooks"], a["dsub"], a["cell_blk"], a["row_of"], a["Npad"], a["N"], a["C"],
                              a["d"], a["mcb"], a["probes"], a["scores"], a["nprobe"], a["depth"], a["S"], a["excl_off"], a["excl_idx"],
                              a["base"], a["allow"], a["n_masks"], a["allow_of"], a["ws"], a["ws_bytes"], None)
    return rc, (lib.mf_last_error() if rc else b"")


def test_cell_bits_refusals_and_their_order(mf):
    lib, E = mf._lib.lib(), mf._lib
    for kw in (dict(tags=None), dict(row_of=None), dict(out=None), dict(N=0), dict(N=-3), dict(Npad=960), dict(Npad=1000), dict(Npad=1025)):
        rc, msg = _bits(lib, **kw)
        assert rc == E.MF_EINVAL and b"mf_filter_cell_bits: bad argument" in msg, (kw, rc, msg)
    rc, msg = _bits(lib, N=2**31, Npad=2**31)
    assert rc == E.MF_ENOTSUP and b"32 bits" in msg
    assert _bits(lib, N=5, Npad=2**31)[0] == E.MF_ENOTSUP
    assert _bits(lib, tags=None, Npad=2**31)[0] == E.MF_EINVAL                     # a null pointer wins over the range
    assert _bits(lib, N=2**31 + 1, Npad=2**31)[0] == E.MF_EINVAL                  # so does Npad < N


@pytest.mark.parametrize("scan", ["ivf", "pq"])
def test_scan_allow_refusals_and_their_order(mf, scan):
    lib, E = mf._lib.lib(), mf._lib
    call = _ivf if scan == "ivf" else _pq
    name = b"mf_ivf_scan_allow" if scan == "ivf" else b"mf_pq_scan_allow"
    # the scan's own refusals, under the new export's name
    for kw in (dict(q=None), dict(row_of=None), dict(ws=None), dict(Q=0), dict(Npad=1000), dict(mcb=17), dict(S=-1)):
        rc, msg = call(lib, **kw)
        assert rc == E.MF_EINVAL and name + b": bad argument" in msg, (kw, rc, msg)
    assert call(lib, depth=0)[0] == E.MF_ENOTSUP and call(lib, nprobe=9)[0] == E.MF_ENOTSUP and call(lib, d=48)[0] == E.MF_EINVAL
    assert call(lib, base=-1)[0] == E.MF_ENOTSUP and call(lib, S=5)[0] == E.MF_ENOTSUP
    rc, msg = call(lib, ws_bytes=2 * 4 * 20 * 8 - 1)
    assert rc == E.MF_ENOSPC and name + b": workspace too small" in msg
    rc, msg = call(lib, excl_off=FAKE)
    assert rc == E.MF_EINVAL and b"excl_off/excl_idx mismatch" in msg
    if scan == "pq":
        assert call(lib, dsub=5)[0] == E.MF_ENOTSUP
    # the bitmap's, after all of those
    for kw in (dict(allow=None), dict(n_masks=0), dict(n_masks=-1), dict(n_masks=2), dict(n_masks=3, allow_of=None)):
        rc, msg = call(lib, **kw)
        assert rc == E.MF_EINVAL and name + b": bad allow argument" in msg, (kw, rc, msg)
    for kw in (dict(n_masks=2**27, allow_of=FAKE), dict(n_masks=2**31, allow_of=FAKE), dict(n_masks=2**62, allow_of=FAKE)):
        rc, msg = call(lib, **kw)                                                # 16 words per mask: 2^27 masks are 2^31 words
        assert rc == E.MF_ENOTSUP and b"exceed 2^31" in msg, (kw, rc, msg)
    assert call(lib, allow=None, n_masks=2**31, allow_of=FAKE)[0] == E.MF_EINVAL      # bad argument, then the range
    # a fault further up wins: each of the scan's own before the bitmap's
    for kw, want in ((dict(q=None), E.MF_EINVAL), (dict(depth=0), E.MF_ENOTSUP), (dict(base=-1), E.MF_ENOTSUP), (dict(ws_bytes=0), E.MF_ENOSPC)):
        rc, msg = call(lib, allow=None, **kw)
        assert rc == want and b"allow" not in msg.split(b":", 1)[1], (kw, rc, msg)
    rc, msg = call(lib, allow=None, excl_idx=FAKE)
    assert rc == E.MF_EINVAL and b"mismatch" in msg


def test_the_new_kernels_have_no_spill_and_no_scratch():
    s = importlib.util.spec_from_file_location("kernel_resources", ROOT / "tools" / "kernel_resources.py")
    kr = importlib.util.module_from_spec(s)
    s.loader.exec_module(kr)
    res = kr.kernel_resources()
    mine = {n: r for n, r in res.items() if "filter_cell_bits_kernel" in n or "ivf_scan_allow_kernel<" in n or "pq_scan_allow_kernel<" in n}
    assert sum("filter_cell_bits_kernel" in n for n in mine) == 1
    assert sum("ivf_scan_allow_kernel" in n for n in mine) == 4 and sum("pq_scan_allow_kernel" in n for n in mine) == 12, sorted(mine)
    for name, r in mine.items():
        # (scalar registers parked in vector lanes are not memory traffic: the unfiltered ivf_scan_kernel parks the query's too)
        assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, (name, r)
    # the bitmap adds no LDS: an ALLOW kernel has its unfiltered twin's
    for name, r in mine.items():
        if "scan_allow_kernel" in name:
            assert r["group_segment_fixed_size"] == res[name.replace("scan_allow_kernel", "scan_kernel")]["group_segment_fixed_size"], name


# ------------------------------------------------------------------------------------------------------ the spec ----
def test_the_spec_on_hand_worked_rows():
    # eight rows in two cells: cell 0 = rows 1, 2, 5, 6, 7, cell 1 = rows 0, 3, 4; one 64-row block each, 59 and 61 padding places
    assign = [1, 0, 0, 1, 1, 0, 0, 0]
    cell_blk, row_of = spec.layout(assign, 2)
    assert cell_blk.tolist() == [0, 1, 2] and row_of.size == 128
    assert row_of[:6].tolist() == [1, 2, 5, 6, 7, -1] and row_of[64:68].tolist() == [0, 3, 4, -1] and (row_of[5:64] == -1).all() and (row_of[67:] == -1).all()
    tags = np.array([0b0001, 0b0001, 0b0011, 0b0111, 0b1001, 0b0110, -2**63, -2**63 | 0b0001], dtype=np.int64)
    ok = spec.admits(tags, all_of=0b0001)                      # rows 0, 1, 2, 3, 4, 7
    assert ok.tolist() == [True, True, True, True, True, False, False, True]
    # cell 0 holds rows 1, 2, 5, 6, 7 at lanes 0 .. 4: lanes 0, 1, 4 admitted; cell 1 holds rows 0, 3, 4: all three
    assert spec.words(ok, row_of).tolist() == [0b10011, 0b111]
    assert spec.words(spec.admits(tags, any_of=1 << 63), row_of).tolist() == [0b11000, 0]           # rows 6, 7
    assert spec.words(spec.admits(tags, any_of=0b0110, all_of=0b0001, none_of=0b1000), row_of).tolist() == [0b00010, 0b010]     # rows 2, 3
    assert spec.words(np.ones(8, bool), row_of).tolist() == [0b11111, 0b111]                       # padding is never set
    assert spec.words(np.zeros(8, bool), row_of).tolist() == [0, 0]
    # bit 63 of a word is the sign bit of the int64 that carries it
    full = spec.words(np.ones(64, bool), np.arange(64))
    assert full.tolist() == [-1] and spec.words(np.arange(64) == 63, np.arange(64)).tolist() == [-2**63]
    # an empty cell has no block
    cell_blk, row_of = spec.layout([2, 2, 0], 3)
    assert cell_blk.tolist() == [0, 1, 1, 2] and row_of[0] == 2 and row_of[64:66].tolist() == [0, 1]
    assert spec.extended_lists([[5], []], 2, ok, 100) == [[5, 105, 106], [105, 106]]


# ------------------------------------------------------------------------------- the long cell and its strips ----
GEOMETRIES = [(64, 8), (32, 16), (256, 4)]


def _slice_bits(cell_blk, cell, S, i, words):  # noqa: N803
    """The positions of the set bits of ``words`` inside slice ``i`` of ``S`` of ``cell``."""
    c0, nb = int(cell_blk[cell]), int(cell_blk[cell + 1] - cell_blk[cell])
    u = np.asarray(words, dtype=np.int64).view(np.uint64)
    return {blk * 64 + lane for blk in range(c0 + nb * i // S, c0 + nb * (i + 1) // S) for lane in range(64) if int(u[blk]) >> lane & 1}


def test_strip_walk_on_hand_worked_words():
    # one cell of 70 blocks from block 2 on; bits at blocks 2 (first of strip 0), 65 (last of strip 0), 66 (first of strip 1), 71 (the last)
    cell_blk = [0, 2, 72]
    words = np.zeros(72, dtype=np.int64)
    words[[2, 65, 66, 71]] = [0b1, -2**63, 0b110, 0b1000]
    words[0] = -1                                                                   # another cell's: never seen
    t = spec.strip_walk(cell_blk, 1, 1, 0, words)
    assert t["seen"] == {2 * 64, 65 * 64 + 63, 66 * 64 + 1, 66 * 64 + 2, 71 * 64 + 3}
    assert (t["passes"], t["rotations"], t["blocks_read"], t["blocks_skipped"], t["blocks_in_last_strip"]) == (18, 1, 4, 66, 6)
    # passes 0, 15 (block 65), 16 (block 66) and 17 (block 71; two waves past the end) have a reader beside an idle wave
    assert t["mixed_passes"] == 4 and t["passes_without_a_reader"] == 14
    stale = spec.strip_walk(cell_blk, 1, 1, 0, words, rotate=False)                 # blocks 66 .. 71 read lanes 0 .. 5 of the first strip
    assert stale["seen"] == {2 * 64, 65 * 64 + 63, 66 * 64} and stale["rotations"] == 0 and stale["passes"] == 18
    # two slices of 35 blocks: no rotation, a word past b1 reads 0 even where the mask has one
    t = spec.strip_walk(cell_blk, 1, 2, 0, words)
    assert t["seen"] == {2 * 64} and (t["passes"], t["rotations"], t["blocks_in_last_strip"]) == (9, 0, 35)
    t = spec.strip_walk(cell_blk, 1, 2, 1, words)
    assert t["seen"] == {65 * 64 + 63, 66 * 64 + 1, 66 * 64 + 2, 71 * 64 + 3} and t["rotations"] == 0
    full = np.full(72, -1, dtype=np.int64)
    t = spec.strip_walk(cell_blk, 1, 1, 0, full)
    assert len(t["seen"]) == 70 * 64 and min(t["seen"]) == 128 and (t["blocks_read"], t["mixed_passes"]) == (70, 1)


@pytest.mark.parametrize("d,dsub", GEOMETRIES)
def test_the_long_cell_case_is_what_the_gpu_tests_lean_on(d, dsub):
    """tests/test_gpu_cell_mask_strips.py: a cell of 129 blocks that starts at block 1, probed by every query at nprobe = 1."""
    c = spec.long_cell_case(d, dsub)
    b = c.base
    assert (b.items.shape, b.q.shape, b.idx_base, b.nprobe, b.exclude) == ((8440, d), (5, d), 30, 1, None) and c.m == d // dsub
    cell_blk, row_of = spec.long_cell_layout(d)
    assert cell_blk.tolist() == [0, 1, 130, 132, 134] and b.max_cell_blocks == 129
    assert int((row_of[129 * 64: 130 * 64] >= 0).sum()) == 38 and (row_of[64: 129 * 64] >= 0).all()
    assert (spec.ivf.probes(b.q, b.centroids, 1) == 1).all()
    if d == 64:
        many = spec.long_cell_queries(64, 1024)
        assert many.shape == (1024, 64) and (spec.ivf.probes(many, b.centroids, 1) == 1).all()
        assert spec.pq.plan_slices(1024, 1, 80, 129) == 1 and spec.pq.plan_slices(256, 1, 80, 129) == 4
        # the scan itself: 33 passes, settles inside the loop
        t = spec.pq.scan_trace(*c._args(), 80, None, b.idx_base)
        assert t["passes"] == 33 and t["settles_in_loop"] >= 2


def test_the_slicings_reach_the_rotation():
    cell_blk, row_of = spec.long_cell_layout(64)
    full = spec.words(np.ones(8440, bool), row_of)
    t = spec.strip_walk(cell_blk, 1, 1, 0, full)
    assert (t["passes"], t["rotations"], t["blocks_in_last_strip"], t["blocks_read"]) == (33, 2, 1, 129)
    first, second = (spec.strip_walk(cell_blk, 1, 2, i, full) for i in (0, 1))
    assert (first["blocks_read"], first["rotations"], first["blocks_in_last_strip"]) == (64, 0, 64)
    assert (second["blocks_read"], second["rotations"], second["blocks_in_last_strip"]) == (65, 1, 1)
    for i in range(3):
        t = spec.strip_walk(cell_blk, 1, 3, i, full)
        assert t["rotations"] == 0 and t["blocks_read"] == 43
    # the largest slicings the GPU tests force: never more than three blocks a slice, one pass
    for S in (129, 64):  # noqa: N806
        assert all(spec.strip_walk(cell_blk, 1, S, i, full)["passes"] == 1 for i in range(S))


@pytest.mark.parametrize("d", [64, 32, 256])
def test_the_mask_families_reach_what_they_are_chosen_for(d):
    cell_blk, row_of = spec.long_cell_layout(d)
    assert list(spec.MASK_FAMILIES) == ["third_strip", "second_strip", "not_first_strip", "strip_edges", "two_bits", "alternate_blocks",
                                        "sparse_blocks", "half"]
    inside = lambda ok, j0, j1: int(ok[row_of[(1 + j0) * 64: (1 + j1) * 64].clip(0)][row_of[(1 + j0) * 64: (1 + j1) * 64] >= 0].sum())  # noqa: E731
    for name in spec.MASK_FAMILIES:
        ok = spec.family_ok(name, d)
        assert ok.shape == (8440,) and 1 <= int(ok.sum()) <= 8440 - 1, name
        small = np.concatenate([row_of[:64], row_of[130 * 64:]])
        small = small[small >= 0]
        assert 0 < int(ok[small].sum()) < small.size, name                          # about half of the three small cells
        words = spec.words(ok, row_of)
        for S in (1, 2, 3):  # noqa: N806
            for i in range(S):
                t = spec.strip_walk(cell_blk, 1, S, i, words)
                assert t["seen"] == _slice_bits(cell_blk, 1, S, i, words), (name, S, i)
                assert t["blocks_read"] + t["blocks_skipped"] == 129 * (i + 1) // S - 129 * i // S
        one = spec.strip_walk(cell_blk, 1, 1, 0, words)
        assert len(one["seen"]) == inside(ok, 0, 129), name
        if name in ("third_strip", "second_strip", "not_first_strip", "strip_edges", "two_bits"):
            # a kernel that never rotates sees other bits: at one slice, and in the second of two
            assert spec.strip_walk(cell_blk, 1, 1, 0, words, rotate=False)["seen"] != one["seen"], name
            assert spec.strip_walk(cell_blk, 1, 2, 1, words, rotate=False)["seen"] != spec.strip_walk(cell_blk, 1, 2, 1, words)["seen"], name
    ok = {name: spec.family_ok(name, d) for name in spec.MASK_FAMILIES}
    assert inside(ok["third_strip"], 0, 129) == inside(ok["third_strip"], 128, 129) == 38
    assert inside(ok["second_strip"], 0, 129) == inside(ok["second_strip"], 64, 128) == 64 * 64
    assert inside(ok["not_first_strip"], 0, 64) == 0 and inside(ok["not_first_strip"], 64, 129) == 64 * 64 + 38
    assert inside(ok["strip_edges"], 0, 129) == 3 * 64 + 38 and inside(ok["strip_edges"], 63, 65) == 128 and inside(ok["strip_edges"], 127, 129) == 102
    assert inside(ok["two_bits"], 0, 129) == 2
    two = spec.words(ok["two_bits"], row_of)
    assert int(two[1 + 64]) == -2**63 and int(two[1 + 128]) == 1 and int((two[1:130] != 0).sum()) == 2
    alt = spec.strip_walk(cell_blk, 1, 1, 0, spec.words(ok["alternate_blocks"], row_of))
    assert alt["mixed_passes"] == alt["passes"] == 33 and (alt["blocks_read"], alt["blocks_skipped"]) == (65, 64)
    sparse = spec.strip_walk(cell_blk, 1, 1, 0, spec.words(ok["sparse_blocks"], row_of))
    assert sparse["passes_without_a_reader"] >= 1 and sparse["mixed_passes"] >= 1 and sparse["blocks_read"] >= 10
    assert 0.4 * 8230 < inside(ok["half"], 0, 129) < 0.6 * 8230


# --------------------------------------------------------------------------------------------------- filter_mode ----
def test_filter_mode_of_the_processor_and_the_config(mf):
    P = mf.retrieval.ItemProcessor
    assert P().filter_mode == "view" and P.FILTER_MODES == ("view", "mask")
    for index_type in ("partitioned", "quantized"):
        assert P(index_type=index_type, filter_mode="mask").filter_mode == "mask"
        assert P(index_type=index_type).filter_mode == "view"
    with pytest.raises(ValueError, match="index_type must be 'partitioned' or 'quantized'"):
        P(filter_mode="mask")
    with pytest.raises(ValueError, match="index_type must be 'partitioned' or 'quantized'"):
        P(index_type="exact", filter_mode="mask")
    for bad in ("bitmap", "", None, "VIEW"):
        with pytest.raises(ValueError, match="filter_mode must be"):
            P(index_type="partitioned", filter_mode=bad)
    C = mf.lightning.MatrixFactorizationLitConfig
    base = {"num_users": 10, "num_items": 12, "hidden_size": 32}
    assert C(**base).filter_mode == "view"
    cfg = C(**base, index_type="quantized", filter_mode="mask")
    dumped = cfg.model_dump()
    assert dumped["filter_mode"] == "mask" and C(**dumped) == cfg and C(**json.loads(json.dumps(dumped))).filter_mode == "mask"
    with pytest.raises(ValueError, match="index_type must be"):
        C(**base, filter_mode="mask")
    with pytest.raises(ValueError, match="filter_mode must be"):
        C(**base, index_type="partitioned", filter_mode="masks")
    m = mf.lightning.MatrixFactorizationLitModule({**base, "index_type": "partitioned", "filter_mode": "mask"})
    assert m._item_processor().filter_mode == "mask"
    assert mf.lightning.MatrixFactorizationLitModule(base)._item_processor().filter_mode == "view"


# ---------------------------------------------------------------------------------------------------- the record ----
def test_the_digest_record_shows_the_unfiltered_scans_unchanged():
    """profiles/cell_mask_digest_{parent,branch}.json: ``tools/kernel_resources.py --text-digest`` of the parent's library and of
    this one with one ``--only=`` list, the branch's record cut to the kernels the parent's names: every kernel of mf_ivf.hip,
    mf_pq.hip, mf_filter.hip and the four top-k units that the parent has -- the unfiltered forms of the two scan kernels
    (csrc/mf_ivf_scan.inc, csrc/mf_pq_scan.inc with ``MF_SCAN_ALLOW false``) among them, under the names they had.  The two
    records are equal: same kernels, same instruction text, same resource figures."""
    parent = json.loads((ROOT / "profiles" / "cell_mask_digest_parent.json").read_text())
    branch = json.loads((ROOT / "profiles" / "cell_mask_digest_branch.json").read_text())
    assert branch == parent and all(len(v["text_sha256"]) == 64 for v in parent.values())
    count = lambda unit: sum(unit in k for k in parent)  # noqa: E731
    assert count("ivf_scan_kernel<") == 4 and count("pq_scan_kernel<") == 12 and count("ivf_cell_mean_kernel") == 1
    assert count("pq_encode_kernel") == 3 and count("pq_refine_kernel") == 4
    for unit in ("filter_mark_kernel", "filter_pack_kernel", "filter_remap_kernel", "filter_unmap_kernel", "filter_lists_count_kernel",
                 "filter_lists_scan_kernel", "filter_lists_write_kernel", "topk_small_scan_kernel", "topk_small_mfma_scan_kernel",
                 "bf3_scan_kernel", "bf3_final_kernel", "topk_deep_slab_kernel", "topk_deep_select_kernel", "topk_merge_kernel",
                 "topk_merge_deep_kernel", "topk_pack_kernel", "select_kernel", "select_seed_kernel", "target_positions_kernel"):
        assert count(unit) >= 1, unit
    assert not any("scan_allow_kernel" in k or "filter_cell_bits" in k for k in parent)
    # the library that is built now has every one of them under the same name
    s = importlib.util.spec_from_file_location("kernel_resources", ROOT / "tools" / "kernel_resources.py")
    kr = importlib.util.module_from_spec(s)
    s.loader.exec_module(kr)
    assert set(parent) <= set(kr.kernel_resources())
