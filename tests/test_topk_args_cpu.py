"""CPU: the argument checks the four exact top-k engines share (csrc/mf_topk_io.h: mf_topk_check_args) and the merge
exports' size refusal.  Every refusal is decided on the host before any launch, so never-dereferenced fake pointers do.
The table is what the exports returned when each still had its own copy of the checks."""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

import pytest

FAKE = ctypes.c_void_p(0x1000)
BIG = ctypes.c_size_t(2**40)


@dataclass(frozen=True)
class Engine:
    export: str
    ws_bytes: str            # the smallest accepted workspace
    max_k: int
    width_code: str          # code of a width outside the engine's set
    widths: bytes
    refused_width: int       # 32 where the engine takes fewer widths than the others (else 0)
    max_n: int               # first refused row count
    suffix: bytes = b""
    index: bool = False      # a second source pointer behind `items`
    k: int = 20              # a k every check accepts


ENGINES = {
    "tiles": Engine("mf_topk", "mf_topk_ws_bytes", 64, "MF_EINVAL", b"{32,64,128,256}", 0, 1 << 31),
    "scan": Engine("mf_topk_small", "mf_topk_small_ws_bytes", 64, "MF_EINVAL", b"{32,64,128,256}", 0, 1 << 31),
    "bf16": Engine("mf_topk_bf3", "mf_topk_bf3_ws_bytes", 64, "MF_ENOTSUP", b"{64,128,256}", 32, 1 << 28,
                   suffix=b" (and a shard 2^28 rows)", index=True),
    "deep": Engine("mf_topk_deep", "mf_topk_deep_min_ws_bytes", 1024, "MF_EINVAL", b"{32,64,128,256}", 0, 1 << 31, k=100),
}


@pytest.fixture(params=sorted(ENGINES))
def engine(request, mf):
    e = ENGINES[request.param]
    lib = mf._lib.lib()

    def call(q=FAKE, Q=4, items=FAKE, index=FAKE, N=1000, d=64, k=e.k, eo=None, ei=None, base=0, ws=FAKE, wsb=BIG, os_=FAKE, oi=FAKE):
        src = (items, index) if e.index else (items,)
        rc = getattr(lib, e.export)(q, Q, *src, N, d, k, eo, ei, base, ws, wsb, os_, oi, None)
        return rc, (lib.mf_last_error() if rc else b"")

    return e, call, lib, mf._lib


def test_each_single_fault_has_its_code_and_message(engine):
    e, call, lib, E = engine
    who = e.export.encode() + b": "

    def refused(code, text, **kw):
        rc, msg = call(**kw)
        assert rc == code and who + text in msg, (e.export, kw, rc, msg)

    nulls = [dict(q=None), dict(items=None), dict(ws=None), dict(os_=None), dict(oi=None), dict(Q=0), dict(Q=-3), dict(N=0), dict(N=-1)]
    for kw in nulls + ([dict(index=None)] if e.index else []):
        refused(E.MF_EINVAL, b"bad argument", **kw)
    for k in (0, -5, e.max_k + 1):
        refused(E.MF_ENOTSUP, b"k = %d outside 1..%d" % (k, e.max_k), k=k)
    refused(getattr(E, e.width_code), b"embedding width 48 not in " + e.widths, d=48)
    if e.refused_width:
        refused(E.MF_ENOTSUP, b"embedding width 32 not in " + e.widths, d=e.refused_width)
    fit = b"item indices must fit 32 bits" + e.suffix
    refused(E.MF_ENOTSUP, fit, N=e.max_n)
    refused(E.MF_ENOTSUP, fit, base=-1)
    refused(E.MF_ENOTSUP, fit, N=1000, base=(1 << 32) - 999)              # idx_base + N = 2^32 + 1
    refused(E.MF_EINVAL, b"excl_off/excl_idx mismatch", eo=FAKE)
    refused(E.MF_EINVAL, b"excl_off/excl_idx mismatch", ei=FAKE)
    low = getattr(lib, e.ws_bytes)(4, 1000, 64, e.k)
    assert low > 0
    refused(E.MF_ENOSPC, b"workspace too small", wsb=ctypes.c_size_t(low - 1))
    refused(E.MF_ENOSPC, b"workspace too small", wsb=ctypes.c_size_t(0))


def test_the_scan_refuses_more_than_32_queries(mf):
    lib, E = mf._lib.lib(), mf._lib

    def call(**kw):
        a = dict(q=FAKE, Q=33, k=20)
        a.update(kw)
        rc = lib.mf_topk_small(a["q"], a["Q"], FAKE, 1000, 64, a["k"], None, None, 0, FAKE, BIG, FAKE, FAKE, None)
        return rc, lib.mf_last_error()

    rc, msg = call()
    assert rc == E.MF_ENOTSUP and b"mf_topk_small: Q = 33 > 32 (use mf_topk)" in msg
    rc, msg = call(k=65)                          # the query count is looked at before k ...
    assert rc == E.MF_ENOTSUP and b"Q = 33 > 32" in msg
    rc, msg = call(q=None)                        # ... and after the pointers
    assert rc == E.MF_EINVAL and b"bad argument" in msg


def test_which_of_two_faults_wins(engine):
    """The order: pointers and sizes, k, width, 32-bit rows, the exclusion pair, then the engine's geometry and workspace."""
    e, call, lib, E = engine
    width = getattr(E, e.width_code)
    for kw, code, text in (
        (dict(q=None, k=0), E.MF_EINVAL, b"bad argument"),
        (dict(N=0, d=48), E.MF_EINVAL, b"bad argument"),
        (dict(k=e.max_k + 1, d=48), E.MF_ENOTSUP, b"outside 1.."),
        (dict(k=0, eo=FAKE), E.MF_ENOTSUP, b"outside 1.."),
        (dict(d=48, N=e.max_n), width, b"embedding width 48"),
        (dict(d=48, ei=FAKE), width, b"embedding width 48"),
        (dict(base=-1, eo=FAKE), E.MF_ENOTSUP, b"must fit 32 bits"),
        (dict(N=e.max_n, wsb=ctypes.c_size_t(0)), E.MF_ENOTSUP, b"must fit 32 bits"),
        (dict(eo=FAKE, wsb=ctypes.c_size_t(0)), E.MF_EINVAL, b"excl_off/excl_idx mismatch"),
    ):
        rc, msg = call(**kw)
        assert rc == code and text in msg, (e.export, kw, rc, msg)
    if e.index:
        rc, msg = call(index=None, k=0)
        assert rc == E.MF_EINVAL and b"bad argument" in msg


@pytest.mark.parametrize("export", ["mf_topk_merge", "mf_topk_merge_packed"])
def test_merge_refuses_more_keys_than_lds_holds(mf, export):
    """G * k * 8 bytes of keys per query: 65,544 is refused (65,536 is accepted: tests/test_gpu_topk_merge.py)."""
    lib, E = mf._lib.lib(), mf._lib
    src = (FAKE, FAKE) if export == "mf_topk_merge" else (FAKE,)
    fn = getattr(lib, export)
    for g, k in ((8193, 1), (1, 8193), (129, 64)):
        assert fn(*src, g, 4, k, FAKE, FAKE, None) == E.MF_ENOTSUP
        assert export.encode() + b": G * k too large" in lib.mf_last_error()
    for kw in (dict(g=0), dict(q=0), dict(k=0), dict(out=None)):
        a = dict(g=2, q=4, k=20, out=FAKE)
        a.update(kw)
        assert fn(*src, a["g"], a["q"], a["k"], a["out"], FAKE, None) == E.MF_EINVAL
        assert export.encode() + b": bad argument" in lib.mf_last_error()
    assert fn(*((None,) * len(src)), 2, 4, 20, FAKE, FAKE, None) == E.MF_EINVAL
