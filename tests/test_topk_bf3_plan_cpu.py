"""CPU: the bf16 retrieval prefilter's plan (csrc/mf_topk_bf3.hip), read through the host-only export ``mf_topk_bf3_plan``
-- every case of tests/test_gpu_topk_prefilter_geometry.py lands in the cell its name claims, the plan's invariants over a sweep
of shapes, and (by the CPU oracle) the planted rows of the ``seams`` case do what that case is about."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

from oracle import chain
from tests import _bf3_cases as bc


def test_plan_export_is_bound_and_refuses_what_the_workspace_sizes_as_zero(mf):
    lib = mf._lib.lib()
    assert "mf_topk_bf3_plan" in mf._lib.SIGNATURES
    out = (ctypes.c_int64 * 16)(*([-7] * 16))
    assert lib.mf_topk_bf3_plan(1024, 62_423, 128, None) == mf._lib.MF_EINVAL and b"mf_topk_bf3_plan" in lib.mf_last_error()
    for nq, n, d in ((0, 100, 64), (-1, 100, 64), (8, 0, 64), (8, 100, 48), (8, 100, 0)):
        assert lib.mf_topk_bf3_ws_bytes(nq, n, d, 20) == 0
        assert lib.mf_topk_bf3_plan(nq, n, d, out) == mf._lib.MF_EINVAL, (nq, n, d)
    assert list(out) == [-7] * 16                                   # a refusal writes nothing
    # the bench's shape, by hand: 1951 tiles, 488 blocks of four, one workgroup of 8 waves x 4 query tiles, every second block
    # sampled (244), one block per workgroup in both scans, 244 x 2 lane halves x (8 / 8) maxima, one prep window
    p = bc.plan(lib, 1024, 62_423, 128)
    assert [p[f] for f in bc.PLAN_FIELDS] == [1951, 488, 4, 8, 1024, 1, 2, 244, 1, 244, 2, 244, 488, 1]
    assert bc.plan(lib, 512, 62_423, 256)["XT"] == 2 and bc.plan(lib, 513, 62_423, 256)["gy"] == 2


@pytest.mark.parametrize("name", list(bc.CASES))
def test_every_named_case_lands_in_its_cell(mf, name):
    case = bc.CASES[name]
    bc.check_cell(case, bc.plan(mf._lib.lib(), case.nq, case.n, case.d))


def test_the_cases_together_name_every_cell(mf):
    lib = mf._lib.lib()
    plans = {name: bc.plan(lib, c.nq, c.n, c.d) for name, c in bc.CASES.items()}
    with_lists = {name: p for name, p in plans.items() if bc.CASES[name].lists}
    assert any(p["gy"] >= 2 for p in plans.values()) and any(p["gy"] >= 3 for p in plans.values())
    assert any(p["bpc_seed"] >= 2 for p in with_lists.values()) and any(p["bpc"] >= 3 for p in with_lists.values())
    assert {2, 3} <= {p["windows"] for p in with_lists.values()}
    assert any(p["bs"] == 2 for p in with_lists.values()) and any(p["nvals"] > 1024 for p in plans.values())
    assert any(p["XT"] == 1 and p["xw"] == 2 and p["bpc"] >= 3 for p in plans.values())
    assert any(p["XT"] == 2 and p["gy"] >= 2 and p["bpc"] >= 3 for p in plans.values())              # d = 256
    # the twelve scan instantiations, each of them launched with the geometry of its template arguments
    seen = set()
    for d, nq, lists in bc.INSTANTIATIONS:
        case = bc.instantiation(d, nq, lists)
        p = bc.plan(lib, case.nq, case.n, case.d)
        bc.check_cell(case, p)
        seen.add((d, p["XT"], lists))
    assert seen == {(d, xt, lists) for d in (64, 128) for xt in (1, 4) for lists in (False, True)} | {
        (256, xt, lists) for xt in (1, 2) for lists in (False, True)}
    assert bc.NEVER_LAUNCHED_BEFORE <= set(bc.INSTANTIATIONS)
    # what the older tests of this engine reach (tests/test_gpu_parity.py, test_gpu_configs.py): one query workgroup, at most two
    # blocks per workgroup, one prep window -- the reason for the cases above
    for nq, n, d in ((1024, 62_423, 128), (300, 30_000, 64), (100, 9_000, 256), (200, 20_000, 128), (150, 20_000, 128),
                     (300, 9_000, 256), (50, 5_000, 64), (40, 2_500, 256), (31, 5_003, 64), (64, 4_001, 64)):
        p = bc.plan(lib, nq, n, d)
        assert p["gy"] == 1 and p["bpc_seed"] == 1 and p["bpc"] <= 2 and p["windows"] == 1 and p["nvals"] <= 1024, (nq, n, d, p)


def test_plan_invariants_over_a_sweep(mf):
    lib = mf._lib.lib()
    for d in (64, 128, 256):
        for nq in (1, 32, 33, 64, 65, 128, 129, 256, 257, 1024, 1025, 3000):
            for n in (1, 45, 2048, 32_640, 32_641, 65_408, 65_409, 65_536, 65_537, 140_000, 12_500_000):
                p = bc.plan(lib, nq, n, d)
                what = dict(Q=nq, N=n, d=d, **p)
                assert p["NT"] == -(-n // 32) and p["nblk"] == -(-p["NT"] // 4), what
                per_wg = 32 * p["XT"] * p["xw"]
                assert p["XT"] in (1, 2 if d == 256 else 4) and p["xw"] in (1, 2, 4, 8) and (p["XT"] == 1 or p["xw"] == 8), what
                assert p["Qp"] % per_wg == 0 and nq <= p["Qp"] < nq + per_wg, what
                assert p["gy"] * per_wg == p["Qp"], what
                assert (p["bs"] == 2) == (p["nblk"] >= 256) and p["bs"] in (1, 2), what
                assert p["nvb_seed"] == -(-p["nblk"] // p["bs"]), what
                assert (p["nvb_seed"] - 1) * p["bs"] < p["nblk"], what                     # the last sampled block exists
                assert (p["nwg"] - 1) * p["bpc"] < p["nblk"] <= p["nwg"] * p["bpc"], what             # no empty workgroup, none missing
                assert (p["nwg_seed"] - 1) * p["bpc_seed"] < p["nvb_seed"] <= p["nwg_seed"] * p["bpc_seed"], what
                assert p["nvals"] == p["nvb_seed"] * 2 * (bc.WAVES // p["xw"]), what
                assert p["windows"] == -(-(p["nblk"] + 1) * 4 * 32 // bc.WINDOW_ROWS), what
                arrays = (p["Qp"] * p["nvals"] * 4                                           # seed maxima
                          + 4 * p["Qp"] * 4                                                  # thr, eps, overflow count and flag
                          + p["Qp"] * d * 2                                                  # the queries' bf16 fragments
                          + p["nwg"] * (bc.WAVES // p["xw"]) * p["Qp"] * 2 * 16              # slot records
                          + p["Qp"] * 256 * 4                                                # overflow lists
                          + (p["nblk"] + 1) * p["Qp"] * 16)                                  # exclusion words
                for k in (1, 64):
                    assert lib.mf_topk_bf3_ws_bytes(nq, n, d, k) >= arrays, what


def test_one_row_tail_case_plants_what_it_is_about(mf):
    """Row 65,536 -- the one real row of the tail tile, the one word of the second prep window -- is the best row of queries 0
    and 1; query 1 excludes it."""
    name = "one_row_tail_at_the_window_seam"
    case = bc.CASES[name]
    data = bc.build(name, case, bc.plan(mf._lib.lib(), case.nq, case.n, case.d))
    sel = [0, 1, 6]
    ws, wi = chain.topk(data.q[sel].numpy(), data.items.numpy(), case.k, data.local_lists(case, sel))
    last = case.n - 1
    assert last == bc.WINDOW_ROWS and last not in data.excl[0] and last in data.excl[1]
    assert wi[0][0] == last and last not in wi[1]
    free = chain.topk(data.q[[1]].numpy(), data.items.numpy(), case.k, None)[1][0]
    assert free[0] == last                                                          # (but for its list, query 1's best row too)
    assert list(wi[2][:2]) == list(bc.DUP_ROWS(case.n))


def test_seams_case_plants_what_it_is_about(mf):
    """The specially constructed queries of ``seams``, answered by the CPU oracle alone: the cells the GPU test is about exist
    in the data (a generator that silently stopped planting would leave a test of random rows)."""
    case = bc.CASES["seams"]
    p = bc.plan(mf._lib.lib(), case.nq, case.n, case.d)
    data = bc.build("seams", case, p)
    sel = list(range(7))
    ws, wi = chain.topk(data.q[sel].numpy(), data.items.numpy(), case.k, data.local_lists(case, sel))
    nt = data.notes
    # 0: every winner in an odd block -- outside the seed scan's sample of every second block
    assert set(wi[0]) <= set(nt["rows0"]) and all((r // bc.BLOCK_ROWS) % 2 == 1 for r in wi[0])
    assert len({r // bc.BLOCK_ROWS for r in wi[0]}) >= 3
    # 1: winners in the last tile of one chunk of the full scan and the first tile of the next
    edge, bpc = nt["edge"], p["bpc"]
    assert edge % (bpc * bc.BLOCK_ROWS) == 0 and set(wi[1]) <= set(nt["rows1"])
    assert (wi[1] < edge).sum() >= 8 and (wi[1] >= edge).sum() >= 8
    assert {(r // bc.BLOCK_ROWS) // bpc for r in wi[1]} == {edge // (bpc * bc.BLOCK_ROWS) - 1, edge // (bpc * bc.BLOCK_ROWS)}
    # 2: the ten neighbours of the two excluded rows at the window seam lead
    seam = bc.WINDOW_ROWS
    assert set(wi[2][:10]) == set(nt["rows2"]) - {seam - 1, seam} and set(wi[2][:2]) == {seam - 2, seam + 1}
    # 3: the tail tile's rows, the last one excluded
    assert list(wi[3][:2]) == [case.n - 2, case.n - 3] and case.n - 1 not in wi[3]
    # 4: the zero query -- the lowest rows that are not on its list
    gone = set(data.excl[4])
    assert list(wi[4]) == [r for r in range(40) if r not in gone][: case.k] and (ws[4] == 0).all()
    # 5: more surviving copies than the final kernel rescores; winners on both sides of the window seam, the upper ones
    # decided by exclusions in the second window
    left = [r for r in nt["low"] + nt["high"] if r not in set(nt["gone"])]
    assert len(left) > bc.CAND and list(wi[5]) == left[: case.k] and len(set(ws[5].view(np.uint32))) == 1
    assert (wi[5] < seam).sum() == 5 and any(g > seam and g < wi[5].max() for g in nt["gone"])
    # 6: the duplicate pair, the lower row first
    assert list(wi[6][:2]) == list(bc.DUP_ROWS(case.n)) and ws[6][0] == ws[6][1]
