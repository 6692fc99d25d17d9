"""CPU: the deep top-k engine's host side (csrc/mf_topk_deep.hip) -- exports, workspace sizes, the block plan and every
refusal.  All of it is decided before any launch, so never-dereferenced fake pointers do."""
from __future__ import annotations

import ctypes
import importlib.util
import pathlib

import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
SRD_MAX = 0xFFF00000                     # MF_SRD_MAX_BYTES (csrc/mf_stream.h)
CAP = 256 << 20                          # the preferred block's slab is at most this large
QS = (1, 31, 32, 33, 1024, 65_536)
NS = (1, 31, 33, 62_423, 8_400_000)
DS = (32, 64, 128, 256)
KS = (1, 64, 65, 1024)
FAKE = ctypes.c_void_p(0x1000)


def _pad32(x):
    return -(-x // 32) * 32


def test_exports_exist_and_are_bound(mf):
    lib = mf._lib.lib()
    header = (ROOT / "include" / "mf_hip.h").read_text()
    for name in ("mf_topk_deep_ws_bytes", "mf_topk_deep_min_ws_bytes", "mf_topk_deep_plan", "mf_topk_deep"):
        assert hasattr(lib, name) and name in mf._lib.SIGNATURES and name + "(" in header, name
    assert "#define MF_TOPK_DEEP_MAX_K 1024" in header


def test_workspace_sizes(mf):
    lib = mf._lib.lib()
    for q in QS:
        for n in NS:
            for d in DS:
                for k in KS:
                    pref, low = lib.mf_topk_deep_ws_bytes(q, n, d, k), lib.mf_topk_deep_min_ws_bytes(q, n, d, k)
                    assert pref >= low > 0, (q, n, d, k, pref, low)
                    assert low == 32 * _pad32(n) * 4, (q, n, d, k, low)           # one block of 32 queries: the slab is the workspace
    for q, n, d, k in ((0, 10, 64, 100), (-1, 10, 64, 100), (4, 0, 64, 100), (4, 10, 48, 100), (4, 10, 64, 0), (4, 10, 64, 1025),
                       (4, 1 << 31, 64, 100), (4, 40_000_000, 64, 100)):              # (the last: a 32-query slab beyond 4 GiB)
        assert lib.mf_topk_deep_ws_bytes(q, n, d, k) == 0 and lib.mf_topk_deep_min_ws_bytes(q, n, d, k) == 0, (q, n, d, k)


def test_plan_arithmetic(mf):
    lib = mf._lib.lib()
    out = (ctypes.c_int64 * 3)()
    for q in QS:
        for n in NS:
            for d in DS:
                for k in KS:
                    what = (q, n, d, k)
                    row = _pad32(n) * 4
                    pref, low = lib.mf_topk_deep_ws_bytes(q, n, d, k), lib.mf_topk_deep_min_ws_bytes(q, n, d, k)
                    for ws in (low, pref, (low + pref) // 2, pref + 12345, 2**40):
                        assert lib.mf_topk_deep_plan(q, n, d, k, ws, out) == 0, what
                        qb, blocks, slab = out
                        assert qb >= 32 and qb % 32 == 0 and blocks * qb >= q and (blocks - 1) * qb < q, (what, ws, list(out))
                        assert slab == qb * row and slab <= ws and slab < SRD_MAX, (what, ws, list(out))
                    assert lib.mf_topk_deep_plan(q, n, d, k, low, out) == 0
                    assert (out[0], out[1]) == (32, -(-q // 32)), (what, list(out))
                    assert lib.mf_topk_deep_plan(q, n, d, k, pref, out) == 0
                    if _pad32(q) * row <= CAP:
                        assert out[1] == 1 and out[0] == _pad32(q), (what, list(out))
                    else:                                                         # the largest multiple of 32 under the cap (at least 32)
                        assert out[0] == max(32, CAP // row // 32 * 32), (what, list(out))
                    # a larger workspace never gives more than the preferred block
                    assert lib.mf_topk_deep_plan(q, n, d, k, 2**40, out) == 0 and out[0] * row == pref
                    assert lib.mf_topk_deep_plan(q, n, d, k, low - 1, out) == mf._lib.MF_ENOSPC, what
    assert lib.mf_topk_deep_plan(4, 10, 48, 100, 2**30, out) == mf._lib.MF_EINVAL
    assert lib.mf_topk_deep_plan(4, 10, 64, 100, 2**30, None) == mf._lib.MF_EINVAL
    # the shapes the GPU tests reach the multi-block path with (tests/test_gpu_topk_deep.py)
    low = lib.mf_topk_deep_min_ws_bytes(130, 4100, 64, 300)
    assert lib.mf_topk_deep_plan(130, 4100, 64, 300, low, out) == 0 and list(out) == [32, 5, 32 * 4128 * 4]
    assert lib.mf_topk_deep_plan(130, 4100, 64, 300, lib.mf_topk_deep_ws_bytes(130, 4100, 64, 300), out) == 0 and list(out)[:2] == [160, 1]


def test_refusals_come_before_any_launch(mf):
    lib = mf._lib.lib()
    E = mf._lib
    big = ctypes.c_size_t(2**40)

    def call(q=FAKE, Q=4, items=FAKE, N=1000, d=64, k=100, eo=None, ei=None, base=0, ws=FAKE, wsb=big, os_=FAKE, oi=FAKE):
        return lib.mf_topk_deep(q, Q, items, N, d, k, eo, ei, base, ws, wsb, os_, oi, None)

    for kw in (dict(q=None), dict(items=None), dict(ws=None), dict(os_=None), dict(oi=None), dict(Q=0), dict(Q=-3), dict(N=0)):
        assert call(**kw) == E.MF_EINVAL and b"mf_topk_deep: bad argument" in lib.mf_last_error(), kw
    assert call(d=48) == E.MF_EINVAL and b"embedding width 48" in lib.mf_last_error()
    assert call(eo=FAKE) == E.MF_EINVAL and b"excl_off/excl_idx mismatch" in lib.mf_last_error()
    assert call(ei=FAKE) == E.MF_EINVAL and b"excl_off/excl_idx mismatch" in lib.mf_last_error()
    assert call(k=1025) == E.MF_ENOTSUP and b"k = 1025 outside 1..1024" in lib.mf_last_error()
    assert call(k=0) == E.MF_ENOTSUP and b"k = 0 outside 1..1024" in lib.mf_last_error()
    assert call(k=-5) == E.MF_ENOTSUP and b"k = -5 outside 1..1024" in lib.mf_last_error()
    assert call(N=1 << 31) == E.MF_ENOTSUP and b"must fit 32 bits" in lib.mf_last_error()
    assert call(base=-1) == E.MF_ENOTSUP and b"must fit 32 bits" in lib.mf_last_error()
    assert call(N=1000, base=(1 << 32) - 999) == E.MF_ENOTSUP and b"must fit 32 bits" in lib.mf_last_error()
    assert call(N=40_000_000) == E.MF_ENOTSUP and b"descriptor limit" in lib.mf_last_error()
    low = lib.mf_topk_deep_min_ws_bytes(4, 1000, 64, 100)
    assert call(wsb=ctypes.c_size_t(low - 1)) == E.MF_ENOSPC and b"workspace too small" in lib.mf_last_error()
    assert call(wsb=ctypes.c_size_t(0)) == E.MF_ENOSPC
    # metrics: deeper than the deep engine stays refused, and says up to where it goes
    assert lib.mf_retrieval_metrics(FAKE, 4, 1025, FAKE, FAKE, FAKE, FAKE, None) == E.MF_ENOTSUP
    assert b"k = 1025 outside 1..1024" in lib.mf_last_error()
    assert lib.mf_retrieval_metrics(FAKE, 4, 0, FAKE, FAKE, FAKE, FAKE, None) == E.MF_ENOTSUP


def test_python_surface_names_the_engine(mf):
    idx = mf.retrieval.ItemIndex
    assert mf._lib.MF_TOPK_DEEP_MAX_K == idx.DEEP_MAX_K == 1024 and idx.TILE_MAX_K == 64
    assert idx.PATHS == ("auto", "scan", "tiles", "bf16", "deep")
    assert mf.retrieval.RetrievalMetrics(top_k=1024).top_k == 1024


def test_new_kernels_do_not_spill():
    spec = importlib.util.spec_from_file_location("kernel_resources", ROOT / "tools" / "kernel_resources.py")
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    deep_r = 1024 // 64                                          # MF_TOPK_DEEP_MAX_K / 64: ranks per lane of the metrics kernel for k > 64
    table = kr.kernel_resources()
    mine = {n: r for n, r in table.items() if "topk_deep_" in n or f"retrieval_metrics_kernel<{deep_r}>" in n}
    assert sum("topk_deep_slab_kernel" in n for n in mine) == 4 and len(mine) == 7, sorted(mine)
    assert sum("topk_deep_excl_kernel" in n for n in mine) == 1 and sum("topk_deep_select_kernel" in n for n in mine) == 1
    shallow = {n: r for n, r in table.items() if "retrieval_metrics_kernel<1>" in n}
    assert len(shallow) == 1 and sum("retrieval_metrics_kernel" in n for n in table) == 2, sorted(shallow)
    mine.update(shallow)
    for name, r in mine.items():
        assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, (name, r)
        assert r["group_segment_fixed_size"] <= 64 * 1024, (name, r)
