"""CPU: the geometry of the distinct-column sweeps of the dense loss (csrc/mf_loss_cols.h), through the host-only
``mf_loss_cols_plan``.

The three sweeps are launched for the worst case and read their share from words the device derives from N', the number of
distinct columns of the batch.  A tile range of 0 tiles, a stage issued past N' or a partial written beyond its buffer would
be a GPU fault; here every quantity a workgroup derives from those words is recomputed as the kernels do it and checked
against what is launched and allocated, for N' at every tile and X-block edge."""
from __future__ import annotations

import ctypes

import pytest

from tests import _dense_cases as dc

SHAPES = tuple(dc.SHAPES) + ((8192, 16384),)
XB = dc.XB
NAMES = ("ok", "nt", "nsf", "tpsf", "nsu", "tpsu", "nsv", "tpsv", "xbv", "grid_f", "grid_u", "grid_v", "cap_f", "cap_u", "cap_v")


def cols_plan(lib, b, n, d, ncols):
    out = (ctypes.c_int64 * 16)()
    rc = lib.mf_loss_cols_plan(b, n, d, ncols, out)
    assert rc == 0, (rc, lib.mf_last_error())
    return dict(zip(NAMES, list(out)[:15]))


def ncols_of(n):
    return sorted({c for c in (1, 31, 32, 33, 127, 128, 129, n - 1, n) if 1 <= c <= n})


def streamed_ranges(launched, tps, tiles):
    """tile ranges of the launched splits of the forward / dU, as the kernels cut them; () for a split that leaves at once"""
    out = []
    for split in range(launched):
        t0 = split * tps
        t1 = min(tiles, t0 + tps)
        out.append(range(t0, t1) if t0 < t1 else range(0))
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("d", (128,) + tuple(w for w in dc.WIDTHS if w != 128))
def test_device_geometry_covers_every_tile_once_inside_what_is_launched(mf, shape, d):
    lib = mf._lib.lib()
    b, n = shape
    bp, np_ = -(-b // XB) * XB, -(-n // XB) * XB
    bt, nt_all = bp // 32, np_ // 32
    for ncols in ncols_of(n):
        p = cols_plan(lib, b, n, d, ncols)
        what = (shape, d, ncols, p)
        assert p["ok"] == (1 if d == 128 else 0), what
        assert p["xbv"] == -(-ncols // XB) and p["nt"] == 4 * p["xbv"], what
        assert -(-ncols // 32) <= p["nt"] <= nt_all, what                  # every distinct column streamed, none past the padding
        # forward and dU: item tiles [0, NT') in splits of tps; launched splits beyond the last one stream nothing
        for nsplit, tps, grid, cap, rows in ((p["nsf"], p["tpsf"], p["grid_f"], p["cap_f"], bp),
                                             (p["nsu"], p["tpsu"], p["grid_u"], p["cap_u"], bp)):
            assert tps >= 1 and 1 <= nsplit <= grid <= cap, what
            ranges = streamed_ranges(grid, tps, p["nt"])
            seen = [t for r in ranges for t in r]
            assert seen == list(range(p["nt"])), what                      # each tile exactly once, in order
            assert len(ranges[nsplit - 1]) >= 1 and all(len(r) == 0 for r in ranges[nsplit:]), what
            assert all(len(r) >= 1 for r in ranges[:nsplit]), what
            assert (nsplit - 1) * rows + rows - 1 < cap * rows, what      # the last partial row written
        # dV: a linear grid; workgroup id -> (X block, split) by the device words
        nsv, tpsv, xbv = p["nsv"], p["tpsv"], p["xbv"]
        assert tpsv >= 1 and nsv >= 1 and xbv * nsv <= p["grid_v"] <= p["cap_v"], what
        used = {}
        for wg in range(p["grid_v"]):
            xblk, split = wg // nsv, wg % nsv
            if xblk >= xbv:
                continue
            t0 = split * tpsv
            t1 = min(bt, t0 + tpsv)
            assert t0 < t1, what                                           # (the last split included: non-empty)
            assert (xblk, split) not in used, what
            used[(xblk, split)] = range(t0, t1)
            last_row = split * xbv * XB + xblk * XB + XB - 1               # of dpart_v / rpart_v, in rows
            assert last_row < p["cap_v"] * XB, what
        assert len(used) == xbv * nsv, what
        for xblk in range(xbv):
            assert [t for s in range(nsv) for t in used[(xblk, s)]] == list(range(bt)), what
        # the epilogue reads split s of slot k at row s * xbv * XB + k, k < ncols
        assert (nsv - 1) * xbv * XB + ncols - 1 < p["cap_v"] * XB, what


@pytest.mark.parametrize("d", dc.WIDTHS)
def test_no_copies_gives_the_geometry_of_mf_loss_plan(mf, d):
    lib = mf._lib.lib()
    for b, n in SHAPES:
        p, q = cols_plan(lib, b, n, d, n), dc.plan(lib, b, n, d)
        got = (p["nsf"], p["tpsf"], p["nsu"], p["tpsu"], p["nsv"], p["tpsv"])
        assert got == (q["nsplit_f"], q["tps_f"], q["nsplit_u"], q["tps_u"], q["nsplit_v"], q["tps_v"]), (b, n, d, p, q)
        assert p["nt"] == -(-n // XB) * 4 and p["xbv"] == -(-n // XB), (b, n, d, p)
        # the uncompacted launch fits what the distinct-column sweeps launch and allocate
        assert q["nsplit_f"] <= p["grid_f"] and q["nsplit_u"] <= p["grid_u"] and q["nsplit_v"] * p["xbv"] <= p["grid_v"], (b, n, d)


def test_headline_shape_at_the_measured_duplicate_ratio(mf):
    """B = 8192, N = 16384 with ~10,700 distinct ids: 336 tiles instead of 512, and the sweeps keep their workgroup counts"""
    lib = mf._lib.lib()
    p = cols_plan(lib, 8192, 16384, 128, 10700)
    assert (p["nt"], p["xbv"]) == (336, 84)
    assert (p["nsf"], p["tpsf"], p["nsu"], p["tpsu"]) == (8, 42, 8, 42), p
    # dV keeps X blocks of items: the most splits whose workgroups still fit one round of 512 (not 7 x 84 = 588)
    assert (p["nsv"], p["tpsv"]) == (6, 43), p


def test_bad_arguments_are_refused(mf):
    lib = mf._lib.lib()
    out = (ctypes.c_int64 * 16)()
    for b, n, d, c in ((4, 2, 128, 1), (8, 16, 128, 0), (8, 16, 128, 17), (8, 16, 48, 4)):
        assert lib.mf_loss_cols_plan(b, n, d, c, out) == mf._lib.MF_EINVAL and b"mf_loss_cols_plan" in lib.mf_last_error()
    assert lib.mf_loss_cols_plan(8, 16, 128, 4, None) == mf._lib.MF_EINVAL
