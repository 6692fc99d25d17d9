"""CPU: the cases of tests/_bwd_split_cases.py are what tests/test_gpu_dense_bwd_split_routes.py takes them for -- the split
geometry and workspace layout each shape is chosen for (through mf_loss_plan and mf_loss_ws_bytes), inputs whose routes see
the masks and logQ values they claim, and the CPU emulation behind the factor of the plan-served precision test."""
from __future__ import annotations

import math

import numpy as np
import pytest
import torch

from oracle import losses as ol
from tests import _bwd_split_cases as sc
from tests import _dense_cases as dc
from tests import test_gpu_dense_dedup as dd


@pytest.fixture(autouse=True)
def _few_threads():
    before = torch.get_num_threads()
    torch.set_num_threads(min(before, 16))
    yield
    torch.set_num_threads(before)


def test_default_switch_shapes_have_the_geometry_they_are_named_for(mf):
    lib = mf._lib.lib()
    for (b, n), (want_u, want_v, own_room, what) in sc.SERVED.items():
        sc.assert_geometry(lib, b, n, want_u, want_v, own_room)
        assert sc.default_serves(n, sc.D, 0) and b <= 300 and n <= 8200, (b, n, what)
    # (24, 8192): three of dV's four user tiles hold padding only; (128, 8192): none does
    assert sc.padded(24) // 32 == 4 and -(-24 // 32) == 1 and sc.padded(128) == 128
    # (300, 8200): tile 256 starts at column 8192 and holds 8 real columns, the X block's other three tiles none
    assert 8200 - 256 * 32 == 8 and sc.padded(8200) // 32 == 260
    for (b, n, d, k), (path, what) in sc.UNSERVED.items():
        assert not sc.default_serves(n, d, k), (b, n, d, k, what)
        p = dc.plan(lib, b, n, d, k)
        assert p["mined"] == (1 if k else 0), (b, n, d, k)
        assert bool(path & sc.PATH_COLS) == (d == 128 and not k and n >= sc.COLS_MIN_N)
    assert {n for (_, n, d, k) in sc.UNSERVED if d == 128 and not k} == {sc.SPLIT_MIN_N - 1}
    assert min(n for _, n in sc.SERVED) == sc.SPLIT_MIN_N


def test_route_shapes_have_the_geometry_they_are_named_for(mf):
    lib = mf._lib.lib()
    for (b, n), (want_u, want_v, own_room) in sc.ROUTE_GEOMETRY.items():
        sc.assert_geometry(lib, b, n, want_u, want_v, own_room)
    assert sc.padded(sc.ROUTE_SHAPE[0]) == 384 and sc.padded(sc.ROUTE_SHAPE[1]) // 32 == 36
    for d in sc.PADDED_WIDTHS:
        assert 64 < d < 128 and mf._lib.padded_width(d) == 128
    # the workspace of a mined call on the mined row's shape exists and differs from the dense one (no stash)
    assert 0 < lib.mf_loss_ws_bytes(64, 8192, 128, 0, 4) != lib.mf_loss_ws_bytes(64, 8192, 128, 0, 0)


def test_csr_lists_of_a_padded_matrix_give_the_same_masks():
    b, n = sc.ROUTE_SHAPE
    t = dc.random_case(b, n, sc.D)
    uid, off, items = sc.csr_of_padded(t["pos_idx"])
    assert (t["pos_idx"] == 0).any()                                        # the padding is there, and stays
    assert uid.tolist() == list(range(b)) and off[-1] == items.numel() == b * dc.P
    lists = torch.stack([items[off[i]: off[i + 1]] for i in uid.tolist()])
    assert torch.equal(lists, t["pos_idx"])
    assert torch.equal(ol.negative_masks(t["item_idx"], lists, b), ol.negative_masks(t["item_idx"], t["pos_idx"], b))


def test_table_case_looks_its_logq_up_by_item_id():
    b, n = sc.ROUTE_SHAPE
    t, table = sc.table_case(b, n)
    base = dc.random_case(b, n, sc.D)
    assert int(t["item_idx"].min()) >= 0 and int(t["item_idx"].max()) < table.numel()
    assert torch.equal(t["logq"], table[t["item_idx"]]) and not torch.equal(t["logq"], base["logq"])
    assert t["target"].dtype == torch.int64                                  # the routes pass the rating as it is
    assert all(torch.equal(t[k], base[k]) for k in ("u", "v", "item_idx", "pos_idx", "target"))


def test_heavy_case_has_real_copies_and_one_heavy_column():
    for b, n in (sc.PRECISION_SHAPE, sc.SMALL_SHAPE, sc.STREAM_SHAPE):
        t = sc.heavy_case("random", b, n)
        kept, weight = sc.copy_weights(t)
        assert len(kept) == dd.distinct_columns(t) < n and int(weight.sum()) == n
        assert 650 <= float(weight.max()) <= 700 + b // 2 and int((weight > 1).sum()) > 1, (b, n, float(weight.max()))


def test_emulated_contraction_separates_six_products_from_five():
    """The factor of test_split_is_no_worse_than_fp32_where_the_plan_weights_g: r6 = E(six products) / E(fp32 matmul) and r5 =
    the smallest E(five products) / E(fp32 matmul) over both kinds, both sides and the three second-order products, on the
    test's own inputs.  Recorded: r6 = 1.10, r5 = 3.52, factor = sqrt(r6 r5) = 1.97.  An fp32 matmul's summation order
    belongs to the BLAS at hand, so the recorded ratios are met to a quarter, and the separation itself is asserted."""
    t = sc.heavy_case("random", *sc.PRECISION_SHAPE)
    r6, r5 = sc.emulation_ratios(t)
    print(f"r6 = {r6:.4g}, r5 = {r5:.4g}, factor = {math.sqrt(r6 * r5):.4g}")
    assert r5 >= 2 * r6, (r6, r5)
    assert abs(r6 / sc.R6 - 1) <= 0.25 and abs(r5 / sc.R5 - 1) <= 0.25, (r6, r5)
    assert abs(sc.FACTOR - math.sqrt(sc.R6 * sc.R5)) <= 0.005
    assert r6 < sc.FACTOR < r5


def test_emulated_pieces_are_the_device_split():
    """three bf16 pieces, each rounding what the earlier ones left: exact subtractions, the sum within 2^-24 of x (2^-26 but
    for the last piece's own rounding), and all nine products reproduce the fp32-input product to fp32 rounding"""
    g = torch.Generator().manual_seed(5)
    x = torch.randn(64, 96, generator=g) * torch.exp2(torch.randint(-30, 10, (64, 96), generator=g).float())
    p = sc._bf16_pieces(x)
    assert all(torch.equal(q, q.to(torch.bfloat16).float()) for q in p)
    assert float(((p[0].double() + p[1].double() + p[2].double() - x.double()).abs() / x.abs().double()).max()) <= 2.0 ** -24
    a, gm = torch.randn(50, 16, generator=g), torch.randn(20, 50, generator=g)
    six = sc._contract(a, gm).double()
    exact = gm.double() @ a.double()
    assert float((six - exact).abs().max()) <= 2e-6 * float(exact.abs().max())
    five = sc._contract(a, gm, dropped=(1, 1)).double()
    assert float((five - exact).abs().max()) > float((six - exact).abs().max())


def test_floor_scale_only_moves_the_absolute_floor():
    want = np.full((4, 8), 1e-9)
    got = want + 5e-6 * 3.0                       # inside the floor 1e-5 * sigma, far outside the relative part
    p = {"tps_u": 1, "tps_v": 1, "nsplit_u": 0, "nsplit_v": 0}
    dc.assert_grads_close_located(got, want, 3.0, "x", "du", p)
    with pytest.raises(AssertionError):
        dc.assert_grads_close_located(got, want, 3.0, "x", "du", p, floor_scale=2.0 ** -20)
    big = np.ones((4, 8))
    dc.assert_grads_close_located(big * (1 + 5e-5), big, 3.0, "x", "dv", p, floor_scale=0.0)     # the relative part is untouched
