"""CPU: the host side of the quantised index (csrc/mf_pq.hip, ``retrieval.QuantizedIndex``) -- the exports, every refusal and
their order (all decided before any launch, so never-dereferenced fake pointers do), the plan over its whole domain, the new
kernels' resources from the code object's notes, the config fields -- and the numpy restatement the GPU tests compare with
(tests/_ivf_pq_spec.py): pinned to the oracle of the exact engines on every shared case, worked by hand on four rows, and
checked for the properties the GPU assertions lean on."""
from __future__ import annotations

import ctypes
import importlib.util
import itertools
import pathlib

import numpy as np
import pytest
import torch

from tests import _ivf_pq_spec as spec

ROOT = pathlib.Path(__file__).resolve().parents[1]
FAKE = ctypes.c_void_p(0x1000)
EXPORTS = {"mf_pq_encode": "int", "mf_pq_ws_bytes": "size_t", "mf_pq_plan": "int", "mf_pq_scan": "int", "mf_pq_refine": "int"}


def test_exports_are_declared_bound_documented_and_present(mf):
    lib = mf._lib.lib()
    header = (ROOT / "include" / "mf_hip.h").read_text()
    guide = (ROOT / "INTEGRATION.md").read_text()
    for name, ret in EXPORTS.items():
        assert hasattr(lib, name) and name in mf._lib.SIGNATURES and f"{ret} {name}(" in header and name in guide, name
    assert "mf_pq.hip" in (ROOT / "matrix-factorization-torch_amd" / "csrc" / "Makefile").read_text()
    assert not hasattr(lib, "mf_pq_codebook_mean")                        # the update is mf_ivf_cell_mean without normalisation
    for words in ("xfmr_rec/data/lightning.py:162-165", "[64-row block][M / 4][64]", "mf_pq_encode replaces", "mf_pq_scan replaces",
                  "mf_pq_refine replaces"):
        assert words in header, words


# ------------------------------------------------------------------------------------------------------ refusals ----
def _scan(lib, **kw):
    a = dict(q=FAKE, Q=4, codes=FAKE, books=FAKE, dsub=8, cell_blk=FAKE, row_of=FAKE, Npad=1024, N=1000, C=8, d=64, mcb=4, probes=FAKE,
             scores=FAKE, nprobe=3, R=80, S=0, eo=None, ei=None, base=0, ws=FAKE, ws_bytes=1 << 30)
    a.update(kw)
    rc = lib.mf_pq_scan(a["q"], a["Q"], a["codes"], a["books"], a["dsub"], a["cell_blk"], a["row_of"], a["Npad"], a["N"], a["C"], a["d"], a["mcb"],
                        a["probes"], a["scores"], a["nprobe"], a["R"], a["S"], a["eo"], a["ei"], a["base"], a["ws"], a["ws_bytes"], None)
    return rc, (lib.mf_last_error() if rc else b"")


# (what is wrong, the code, a piece of the text) in the documented order: a fault further up wins over every one below it
FAULTS = (
    (dict(q=None), "MF_EINVAL", b"mf_pq_scan: bad argument"),
    (dict(R=257), "MF_ENOTSUP", b"R = 257 outside 1..256"),
    (dict(nprobe=9), "MF_ENOTSUP", b"nprobe = 9 outside 1..8"),
    (dict(d=48), "MF_EINVAL", b"embedding width 48 not in {32,64,128,256}"),
    (dict(dsub=5), "MF_ENOTSUP", b"sub-vector length 5 not in {4,8,16}"),
    (dict(base=2**32 - 999), "MF_ENOTSUP", b"item indices must fit 32 bits"),
    (dict(S=69, mcb=256, Npad=16384), "MF_ENOTSUP", b"nprobe * S * R too large"),        # 3 * 69 * 80 = 16,560 keys
    (dict(ws_bytes=16), "MF_ENOSPC", b"workspace too small"),
    (dict(eo=FAKE), "MF_EINVAL", b"excl_off/excl_idx mismatch"),
)


def test_each_refusal_of_the_scan_has_its_code_and_text(mf):
    lib, E = mf._lib.lib(), mf._lib
    for kw, code, text in FAULTS:
        rc, msg = _scan(lib, **kw)
        assert rc == getattr(E, code) and text in msg, (kw, rc, msg)
    for kw in (dict(codes=None), dict(books=None), dict(cell_blk=None), dict(row_of=None), dict(probes=None), dict(scores=None), dict(ws=None),
               dict(Q=0), dict(N=0), dict(C=0), dict(Npad=960), dict(Npad=1000), dict(mcb=0), dict(mcb=17), dict(S=-1)):
        rc, msg = _scan(lib, **kw)
        assert rc == E.MF_EINVAL and b"mf_pq_scan: bad argument" in msg, (kw, rc, msg)
    for kw, text in ((dict(R=0), b"R = 0 outside"), (dict(nprobe=0), b"nprobe = 0 outside"), (dict(C=100, nprobe=65), b"outside 1..64"),
                     (dict(dsub=32), b"sub-vector length 32"), (dict(dsub=0), b"sub-vector length 0"),
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
    """R = 256 with nprobe = 64 (16,384 keys), every sub-vector length, idx_base + N = 2^32 and an exact workspace pass every
    check: where there is no device the launch itself then fails, past every refusal."""
    lib, E = mf._lib.lib(), mf._lib
    if torch.cuda.is_available():
        return                      # (a launch on fake pointers is only harmless where there is no device: tests/test_gpu_ivf_pq.py runs real ones)
    for kw in (dict(C=64, nprobe=64, R=256, S=1), dict(base=2**32 - 1000), dict(ws_bytes=3 * 4 * 80 * 8, S=1), dict(S=4), dict(dsub=4),
               dict(dsub=16), dict(d=256, dsub=4), dict(d=32, dsub=16), dict(R=1)):
        rc, msg = _scan(lib, **kw)
        assert rc == E.MF_ELAUNCH, (kw, rc, msg)
    assert lib.mf_pq_refine(FAKE, 4, FAKE, 1000, 64, FAKE, 256, 64, 2**32 - 1000, FAKE, FAKE, None) == E.MF_ELAUNCH
    assert lib.mf_pq_refine(FAKE, 4, FAKE, 1000, 64, FAKE, 1, 1, 0, FAKE, FAKE, None) == E.MF_ELAUNCH
    assert lib.mf_pq_encode(FAKE, 1000, 64, FAKE, FAKE, FAKE, 8, FAKE, 1024, FAKE, None) == E.MF_ELAUNCH
    assert lib.mf_pq_encode(FAKE, 1000, 64, None, None, FAKE, 8, None, 1000, FAKE, None) == E.MF_ELAUNCH


def test_refusals_of_the_encode_and_the_refine(mf):
    lib, E = mf._lib.lib(), mf._lib

    def encode(rows=FAKE, N=1000, d=64, cen=FAKE, assign=FAKE, books=FAKE, dsub=8, row_of=FAKE, Npad=1024, codes=FAKE):
        rc = lib.mf_pq_encode(rows, N, d, cen, assign, books, dsub, row_of, Npad, codes, None)
        return rc, lib.mf_last_error()

    for kw in (dict(rows=None), dict(books=None), dict(codes=None), dict(N=0), dict(Npad=960), dict(Npad=1000), dict(row_of=None),
               dict(row_of=None, Npad=1001)):
        assert encode(**kw) == (E.MF_EINVAL, b"mf_pq_encode: bad argument"), kw
    for kw in (dict(cen=None), dict(assign=None)):
        rc, msg = encode(**kw)
        assert rc == E.MF_EINVAL and b"centroids/assign mismatch" in msg, kw
    rc, msg = encode(d=48, dsub=5)
    assert rc == E.MF_EINVAL and b"embedding width 48" in msg                # the width before the sub-vector length
    rc, msg = encode(dsub=5)
    assert rc == E.MF_ENOTSUP and b"sub-vector length 5 not in {4,8,16}" in msg
    rc, msg = encode(rows=None, cen=None)
    assert rc == E.MF_EINVAL and b"bad argument" in msg                      # pointers and sizes before the pair

    def refine(q=FAKE, Q=4, items=FAKE, N=1000, d=64, cand=FAKE, R=80, k=20, base=0, s=FAKE, r=FAKE):
        rc = lib.mf_pq_refine(q, Q, items, N, d, cand, R, k, base, s, r, None)
        return rc, lib.mf_last_error()

    for kw in (dict(q=None), dict(items=None), dict(cand=None), dict(s=None), dict(r=None), dict(Q=0), dict(N=0)):
        assert refine(**kw) == (E.MF_EINVAL, b"mf_pq_refine: bad argument"), kw
    order = ((dict(k=65), E.MF_ENOTSUP, b"k = 65 outside 1..64"), (dict(R=257), E.MF_ENOTSUP, b"R = 257 outside k..256"),
             (dict(d=48), E.MF_EINVAL, b"embedding width 48"), (dict(base=2**32 - 999), E.MF_ENOTSUP, b"item indices must fit 32 bits"))
    for kw, code, text in order:
        rc, msg = refine(**kw)
        assert rc == code and text in msg, kw
    for (kw_a, code, text), (kw_b, _, _) in itertools.combinations(order, 2):
        rc, msg = refine(**kw_a, **kw_b)
        assert rc == code and text in msg, (kw_a, kw_b)
    for kw, text in ((dict(k=0), b"k = 0 outside"), (dict(R=19), b"R = 19 outside k..256"), (dict(base=-1), b"32 bits"), (dict(N=2**31), b"32 bits")):
        rc, msg = refine(**kw)
        assert rc == E.MF_ENOTSUP and text in msg, kw


# ---------------------------------------------------------------------------------------------------------- plan ----
def test_plan_over_its_domain(mf):
    lib, E = mf._lib.lib(), mf._lib
    out = (ctypes.c_int64 * 4)()
    sliced = 0
    for nq, nprobe, r, mcb in itertools.product((1, 2, 8, 32, 33, 1024, 100_000), (1, 3, 8, 32, 64), (1, 20, 80, 256), (1, 3, 4, 40, 96, 5000, 200_000)):
        assert lib.mf_pq_plan(nq, nprobe, r, mcb, out) == E.MF_OK
        s, g, wgs, nbytes = out
        assert 1 <= s <= mcb and nprobe * s * r <= 16384, (nq, nprobe, r, mcb, s)
        assert s == spec.plan_slices(nq, nprobe, r, mcb) and g == nprobe * s and wgs == nq * g and nbytes == g * nq * r * 8
        assert nbytes <= lib.mf_pq_ws_bytes(nq, nprobe, r, mcb) < nbytes + 256
        sliced += s > 1
    assert sliced > 50
    assert lib.mf_pq_plan(1, 8, 80, 96, out) == E.MF_OK and out[0] == 24                # the serving shape: 192 workgroups of 4 blocks
    assert lib.mf_pq_plan(1, 32, 256, 96, out) == E.MF_OK and out[0] == 2               # the merge's keys bound it: 32 * 2 * 256 = 16,384
    assert lib.mf_pq_plan(1, 8, 80, 96, None) == E.MF_EINVAL and lib.mf_last_error() == b"mf_pq_plan: out is NULL"
    for bad in ((0, 8, 80, 96), (1, 0, 80, 96), (1, 65, 80, 96), (1, 8, 0, 96), (1, 8, 257, 96), (1, 8, 80, 0)):
        assert lib.mf_pq_plan(*bad, out) == E.MF_EINVAL and lib.mf_pq_ws_bytes(*bad) == 0, bad


def test_the_two_plans_are_one_rule(mf):
    """``mf_ivf_plan`` and ``mf_pq_plan`` differ in the merge's key budget (8,192 / 16,384) and the largest depth (64 / 256)
    alone: over the grid above at the depths both take, wherever neither budget binds -- the slices the larger budget gives
    keep ``nprobe * S * depth`` within 8,192 -- they return the same four words.  That is most of the grid."""
    lib, E = mf._lib.lib(), mf._lib
    a, b = (ctypes.c_int64 * 4)(), (ctypes.c_int64 * 4)()
    grid = list(itertools.product((1, 2, 8, 32, 33, 1024, 100_000), (1, 3, 8, 32, 64), (1, 20, 64), (1, 3, 4, 40, 96, 5000, 200_000)))
    free = 0
    for nq, nprobe, depth, mcb in grid:
        assert lib.mf_ivf_plan(nq, nprobe, depth, mcb, a) == E.MF_OK and lib.mf_pq_plan(nq, nprobe, depth, mcb, b) == E.MF_OK
        assert b[0] == spec.ivf.plan_slices(nq, nprobe, depth, mcb, merge_keys=16384) >= a[0]
        if nprobe * b[0] * depth <= 8192:
            assert list(a) == list(b), (nq, nprobe, depth, mcb, list(a), list(b))
            free += 1
    assert 2 * free >= len(grid), (free, len(grid))


# ----------------------------------------------------------------------------------------------------- resources ----
def test_the_new_kernels_have_no_spill_no_scratch_and_the_lds_they_document():
    s = importlib.util.spec_from_file_location("kernel_resources", ROOT / "tools" / "kernel_resources.py")
    kr = importlib.util.module_from_spec(s)
    s.loader.exec_module(kr)
    table = kr.kernel_resources()

    def args(name):
        return tuple(int(x) for x in name.split("<")[1].split(">")[0].split(","))

    scan = {args(n): r for n, r in table.items() if "pq_scan_kernel" in n}
    encode = {args(n): r for n, r in table.items() if "pq_encode_kernel" in n}
    refine = {args(n): r for n, r in table.items() if "pq_refine_kernel" in n}
    assert sorted(scan) == sorted((d // dsub, dsub) for d in (32, 64, 128, 256) for dsub in (4, 8, 16))       # (M, dsub)
    assert sorted(encode) == [(4,), (8,), (16,)] and sorted(refine) == [(32,), (64,), (128,), (256,)]
    for name, r in {**scan, **encode, **refine}.items():
        assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, (name, r)
        assert r.get("sgpr_spill_count", 0) == 0 and r["max_flat_workgroup_size"] == 256, (name, r)
        assert r["vgpr_count"] + r["agpr_count"] <= 128, (name, r)                       # two workgroups per SIMD
    for (m, _), r in scan.items():
        # the query's tables (M KiB), the 1,024 keys of the buffer (8 KiB) and the waves' counts
        assert r["group_segment_fixed_size"] == m * 1024 + 8192 + 16 <= 80 * 1024, (m, r)
    assert all(r["group_segment_fixed_size"] == 4096 for r in encode.values())           # four waves' half norms
    assert all(r["group_segment_fixed_size"] == 3072 for r in refine.values())           # 256 keys and two lists of 64


# -------------------------------------------------------------------------------------------------------- config ----
def test_config_fields_and_round_trip(mf):
    cfg_cls = mf.lightning.MatrixFactorizationLitConfig
    base = dict(num_users=10, num_items=20)
    cfg = cfg_cls(**base)
    assert (cfg.index_type, cfg.num_sub_vectors, cfg.refine_factor) == ("exact", None, 4)
    cfg = cfg_cls(**base, index_type="quantized", num_partitions=4, num_probes=3, index_seed=7, num_sub_vectors=8, refine_factor=2)
    again = cfg_cls.model_validate(cfg.model_dump())
    assert again == cfg and again.model_dump()["index_type"] == "quantized" and (again.num_sub_vectors, again.refine_factor) == (8, 2)
    for bad in (dict(index_type="ivf"), dict(index_type="hnsw"), dict(num_sub_vectors=0), dict(refine_factor=0), dict(refine_factor=257),
                dict(index_type="quantized", refine_factor=13, top_k=20)):
        with pytest.raises(ValueError):
            cfg_cls(**base, **bad)
    assert cfg_cls(**base, index_type="partitioned", refine_factor=13, top_k=20).refine_factor == 13      # (read by "quantized" only)
    proc = mf.lightning.MatrixFactorizationLitModule(cfg)._item_processor()
    assert (proc.index_type, proc.num_partitions, proc.num_probes, proc.index_seed, proc.num_sub_vectors, proc.refine_factor) == ("quantized", 4, 3, 7, 8, 2)
    for kind in ("ivf", "hnsw"):
        with pytest.raises(ValueError, match="index_type"):
            mf.retrieval.ItemProcessor(index_type=kind)
    for bad in (dict(num_sub_vectors=0), dict(refine_factor=0)):
        with pytest.raises(ValueError):
            mf.retrieval.ItemProcessor(index_type="quantized", **bad)
    assert mf.retrieval.ItemProcessor.INDEX_TYPES == ("exact", "partitioned", "quantized")
    assert not hasattr(mf.distributed.ShardedIndex, "codes")                            # the sharded index does not offer it


def test_cpu_tensors_and_bad_geometries_are_refused(mf):
    c = spec.cases()["width32"]
    t = [torch.from_numpy(x) for x in (c.base.items, c.base.centroids, c.base.assign, c.books)]
    with pytest.raises(mf._lib.MfHipError, match="must live on the GPU"):
        mf.retrieval.QuantizedIndex.from_codebooks(*t)
    with pytest.raises(mf._lib.MfHipError, match="must live on the GPU"):
        mf.retrieval.QuantizedIndex.build(t[0], 4)
    with pytest.raises(mf._lib.MfHipError, match="must live on the GPU"):
        mf.retrieval.ItemProcessor(index_type="quantized").set_index(t[0])
    # the geometry and the factor are judged before anything touches the rows
    for m in (0, 1, 3, 16, 5):                                                          # 32 / m outside {4, 8, 16}
        with pytest.raises(ValueError, match="num_sub_vectors"):
            mf.retrieval.QuantizedIndex.build(t[0], 4, num_sub_vectors=m)
    with pytest.raises(ValueError, match="refine_factor"):
        mf.retrieval.QuantizedIndex.build(t[0], 4, refine_factor=0)
    with pytest.raises(ValueError, match="pq_iters"):
        mf.retrieval.QuantizedIndex.build(t[0], 4, pq_iters=-1)
    assert [mf.retrieval.QuantizedIndex._geometry(d, d // 8) for d in (32, 64, 128, 256)] == [(4, 8), (8, 8), (16, 8), (32, 8)]
    assert mf.retrieval.QuantizedIndex._geometry(256, 64) == (64, 4) and mf.retrieval.QuantizedIndex._geometry(32, 2) == (2, 16)


# -------------------------------------------------------------------------------------------- the spec by hand ----
def _hand():
    """Four rows of width 32 in one cell whose centroid is 0 (residual = row, base = 0), two sub-vectors of 16 channels.
    Sub-space 0 has codewords e0 (code 0), e1 (code 1) and e0 again (code 2); sub-space 1 has e0 (0) and e1 (1); every other
    codeword is 100 e15: half norm 5,000, never the best.  All values are small dyadic numbers: every sum is exact."""
    books = np.zeros((2, 256, 16), dtype=np.float32)
    books[:, :, 15] = 100.0
    books[0, 0] = books[0, 2] = books[1, 0] = np.eye(16, dtype=np.float32)[0]
    books[0, 1] = books[1, 1] = np.eye(16, dtype=np.float32)[1]
    items = np.zeros((4, 32), dtype=np.float32)
    items[0, [0, 16]] = 1.0                       # e0 | e0: code 0 ties with code 2 at 1 - 0.5 -- the lowest wins
    items[1] = items[0]                           # its twin: equal approximate scores, the lower row first
    items[2, [0, 1, 16]] = 0.75, 0.5, 1.0         # 0.75 e0 + 0.5 e1 | e0: code 0 (0.25 against 0), so approx as rows 0 and 1 -- exact above them
    items[3, [1, 17]] = 1.0                       # e1 | e1: codes 1, 1
    q = np.zeros((1, 32), dtype=np.float32)
    q[0, [0, 1, 16]] = 1.0                        # exact: 2, 2, 2.25, 1;   lut[0] = 1, 1, 1, ..;  lut[1] = 1, 0, ..
    return q, items, np.zeros((1, 32), dtype=np.float32), np.zeros(4, dtype=np.int64), books


def test_hand_worked_rows():
    q, items, cen, assign, books = _hand()
    res = spec.residuals(items, cen, assign)
    assert np.array_equal(res, items)
    h = spec.half_norms(books)
    assert h[0, :3].tolist() == [0.5, 0.5, 0.5] and h[1, :2].tolist() == [0.5, 0.5] and (h[:, 3:] == 5000.0).all()
    codes = spec.encode(res, books)
    assert codes.tolist() == [[0, 0], [0, 0], [0, 0], [1, 1]]                           # never code 2: the tie goes to the lowest
    lut = spec.tables(q, books)
    assert lut[0, 0, :3].tolist() == [1.0, 1.0, 1.0] and lut[0, 1, :2].tolist() == [1.0, 0.0] and not lut[0, :, 3:].any()
    args = (q, items, cen, assign, books, codes)
    s, r = spec.candidates(*args, 4, 1)
    assert r.tolist() == [[0, 1, 2, 3]] and s.tolist() == [[2.0, 2.0, 2.0, 1.0]]           # equal approx: by row
    s, r = spec.candidates(*args, 2, 1)
    assert r.tolist() == [[0, 1]] and s.tolist() == [[2.0, 2.0]]
    s, r = spec.candidates(*args, 2, 1, [[0]])
    assert r.tolist() == [[1, 2]]                                                       # an excluded row takes no candidate slot
    s, r = spec.candidates(*args, 6, 1, [[3]], idx_base=100)
    assert r.tolist() == [[100, 101, 102, 103, -1, -1]] and np.isneginf(s[0, 4:]).all()  # (nothing excluded: 3 is no global row)
    s, r = spec.candidates(*args, 6, 1, [[103]], idx_base=100)
    assert r.tolist() == [[100, 101, 102, -1, -1, -1]] and np.isneginf(s[0, 3:]).all()
    # refine: row 2 is the exact best (2.25) and the approximate third
    s, r = spec.search(*args, 2, 1, 1)
    assert r.tolist() == [[0, 1]] and s.tolist() == [[2.0, 2.0]]                         # R = 2: it is never looked at
    s, r = spec.search(*args, 3, 1, 1)
    assert r.tolist() == [[2, 0, 1]] and s.tolist() == [[2.25, 2.0, 2.0]]                # R = 3: it moves from third to first
    s, r = spec.search(*args, 2, 2, 1)
    assert r.tolist() == [[2, 0]] and s.tolist() == [[2.25, 2.0]]
    s, r = spec.search(*args, 3, None, 1, [[1]])
    assert r.tolist() == [[2, 0, 3]] and s.tolist() == [[2.25, 2.0, 1.0]]
    # the layout: M = 2 is one 16-bit unit per row, M = 8 two 32-bit units
    cell_blk, row_of = spec.layout(np.array([1, 0, 1, 1]), 3)
    assert cell_blk.tolist() == [0, 1, 2, 2] and row_of[:2].tolist() == [1, -1] and row_of[64:68].tolist() == [0, 2, 3, -1]
    laid = spec.device_codes(codes + np.array([[0, 10]], dtype=np.uint8), row_of)
    assert laid.size == 128 * 2 and laid[:4].tolist() == [0, 10, 0, 0] and laid[128:136].tolist() == [0, 10, 0, 10, 1, 11, 0, 0]
    wide = np.arange(4 * 8, dtype=np.uint8).reshape(4, 8)
    laid = spec.device_codes(wide, row_of)
    assert laid.size == 128 * 8 and laid[:4].tolist() == [8, 9, 10, 11] and laid[256:260].tolist() == [12, 13, 14, 15]     # block 0: row 1
    assert laid[512:520].tolist() == [0, 1, 2, 3, 16, 17, 18, 19] and laid[768:772].tolist() == [4, 5, 6, 7]              # block 1: rows 0, 2


def test_the_seeded_build_by_hand():
    """258 training rows of width 32 as four sub-vectors of 8, all on channel 0 of sub-space 0: row i < 256 is (i + 1) e0 and
    starts as codeword i; row 256 = 1.25 e0 is nearest codeword 0 (0.75 against 0.5 for codeword 1) and row 257 = 1.5 e0 ties
    between codewords 0 and 1 (1.0 each): the lowest.  So codeword 0 becomes ((0 + 1) + 1.25 + 1.5) / 3 = 1.25, every other
    one is the mean of its own row, and a second iteration moves nothing.  The other sub-spaces are all zero: every code 0."""
    res = np.zeros((258, 32), dtype=np.float32)
    res[:256, 0] = np.arange(1, 257)
    res[256:, 0] = 1.25, 1.5
    books = spec.build_codebooks(res, 4, 0)
    assert books.shape == (4, 256, 8) and np.array_equal(books, res[:256].reshape(256, 4, 8).transpose(1, 0, 2))
    codes = spec.encode(res, books)
    assert codes[:, 0].tolist() == list(range(256)) + [0, 0] and not codes[:, 1:].any()
    once, twice = spec.build_codebooks(res, 4, 1), spec.build_codebooks(res, 4, 2)
    assert once[0, 0, 0] == 1.25 and np.array_equal(once[0, 1:], books[0, 1:]) and not once[0, 0, 1:].any() and not once[1:].any()
    assert np.array_equal(twice, once) and np.array_equal(spec.encode(res, once), codes)
    few = spec.build_codebooks(res[:6], 4, 1)                                            # T < 256: codeword j starts as row j mod T
    assert few[0, :, 0].tolist() == [float(j % 6 + 1) for j in range(256)]               # (the copies tie with the first six and stay)


# ------------------------------------------------------------------------------------------------ the case set ----
@pytest.fixture(scope="module")
def results():
    return {name: (c, c.candidates(), c.expected()) for name, c in spec.cases().items()}


def test_with_every_row_refined_the_spec_is_the_oracle_of_the_exact_engines():
    """R at least the admissible rows of the probed cells: the quantiser chooses nothing, and what is left -- probes, exclusions,
    the chain, the order, the tail -- is tests/_ivf_spec.py's ``expected``, which the partitioned and exact engines are held to."""
    for name, c in spec.cases().items():
        s, r = c.expected(None)
        ws, wr = c.base.expected()
        assert np.array_equal(r, wr) and np.array_equal(s.view(np.uint32), ws.view(np.uint32)), name


def test_the_case_set_holds_what_the_gpu_assertions_lean_on(mf, results):
    cs = spec.cases()
    assert {c.r for c in cs.values()} >= {1, 20, 80, 256} and {c.dsub for c in cs.values()} == {4, 8, 16}
    assert {c.m for c in cs.values()} >= {2, 4, 8, 16, 64} and {c.width for c in cs.values()} == {32, 64, 128, 256}
    assert cs["padded_width"].base.items.shape[1] == 48 and cs["padded_width"].width == 64
    differs = ranks_move = 0
    for name, (c, (cs_, cr), (s, r)) in results.items():
        nq = c.base.q.shape[0]
        assert cs_.shape == cr.shape == (nq, c.r) and s.shape == r.shape == (nq, c.base.k), name
        ws, wr = c.base.expected()
        differs += not np.array_equal(r, wr)
        for i in range(nq):
            got = r[i][r[i] >= 0]
            cand = cr[i][cr[i] >= 0]
            assert np.isin(got, cand).all() and got.size == min(c.base.k, cand.size), (name, i)       # results come from the candidates
            if c.base.exclude is not None:
                assert not np.isin(cand, c.base.exclude[i]).any(), (name, i)
            ranks_move += got.tolist() != cand[: got.size].tolist()
            keys = spec.keys(cs_[i][: cand.size], cand)
            assert (keys[:-1] > keys[1:]).all(), (name, i)                                         # ordered, no key twice
    assert differs >= 5 and ranks_move >= 50                               # the approximation is real, and the refine reorders
    # tails: fewer admissible rows than R
    for name in ("all_but_three", "fewer_rows_than_k", "one_cell_one_row_list"):
        assert (results[name][1][1][:, -1] == -1).all() or cs[name].r == 1, name
    assert ((results["all_but_three"][1][1] >= 0).sum(axis=1) == 3).all()
    # approximate ties: the twin rows of one cell share their codes, so their keys differ by the row alone
    c, (a, rows), _ = results["ties_across_cells"]
    bits = a[0].view(np.uint32)
    runs = [rows[0][bits == b] for b in np.unique(bits[rows[0] >= 0])]
    assert max(len(run) for run in runs) >= 20 and all((np.diff(run) > 0).all() for run in runs)
    # the zero query: every table entry and every base is 0
    c, (a, rows), _ = results["zero_query"]
    assert not a[1].any() and (np.diff(rows[1]) > 0).all()
    # an empty cell under the probe, a cell of one row, and the sliced cell
    assert cs["cell_sizes_nprobe3"].base.sizes[:5].tolist() == [0, 1, 63, 64, 65]
    lib = mf._lib.lib()
    out = (ctypes.c_int64 * 4)()
    slices = {}
    for name, c in cs.items():
        assert lib.mf_pq_plan(c.base.q.shape[0], c.base.nprobe, c.r, c.base.max_cell_blocks, out) == 0
        slices[name] = out[0]
    assert slices["big_cell"] == 10 and slices["width64"] == 1 and sum(s > 1 for s in slices.values()) >= 2


def test_the_steady_cases_reach_the_bound_and_every_settle():
    """What tests/test_gpu_ivf_pq.py leans on when it scans a 40-block cell as one slice: at least three passes, a settle
    inside the loop (two at R = 256: the second sorts kept and waiting keys together), keys turned away by the bound, excluded
    rows met under a bound, and both ways out of the loop -- keys still waiting (``steady``) and none (``steady_tail``).  The
    walk's list is the spec's candidate list whatever the path."""
    cs = spec.steady_cases()
    for name in ("steady", "steady_tail"):
        c = cs[name]
        assert c.base.max_cell_blocks == 40 and c.base.q.shape[0] == 1 and len(c.base.exclude[0]) > 64
        _, top = spec.candidates(*c._args(), 60, 1, None, c.base.idx_base)
        assert np.isin(top[0][:60], c.base.exclude[0]).sum() >= 3, name                      # true top candidates are excluded
        for r in (1, 80, 256):
            t = spec.scan_trace(*c._args(), r, c.base.exclude, c.base.idx_base)
            s, rows = c.candidates(r)
            assert np.array_equal(t["keys"], spec.keys(s[0], rows[0])) and (rows >= 0).all(), (name, r)
            assert t["passes"] == 10 and t["settles_in_loop"] >= 1 and t["turned_away_by_the_bound"] > 1000, (name, r, t)
            assert t["excluded_hits_under_a_bound"] > 0 or name == "steady_tail", (name, r, t)
            assert t["settle_after_the_loop"] == (name == "steady"), (name, r, t)
        assert spec.scan_trace(*c._args(), 256, c.base.exclude)["settles_in_loop"] == (2 if name == "steady" else 1), name
    t = spec.scan_trace(*cs["steady_tail"]._args(), 80, cs["steady_tail"].base.exclude)
    assert t["excluded_hits"] == 100 and t["lookups"] == 768                             # before the bound: every row is looked up
    # the shared cases never get there: no slice of theirs has more than eight blocks (two passes)
    for name, c in spec.cases().items():
        s = spec.plan_slices(c.base.q.shape[0], c.base.nprobe, c.r, c.base.max_cell_blocks)
        assert -(-c.base.max_cell_blocks // s) <= 8, name
    many = cs["steady_many"]
    assert many.base.q.shape[0] == 1024 and spec.plan_slices(1024, 1, 80, 40) == 1
    assert (spec.ivf.probes(many.base.q, many.base.centroids, 1) == 0).all()              # every query walks the 40-block cell
    assert {len(e) for e in many.base.exclude} == {0, 1, 100}
