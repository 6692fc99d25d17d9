"""CPU: the operand image of the split forward sweep (csrc/mf_bf_split.h), the cases of tests/_fwd_split_cases.py, and the
emulation behind the factor of the GPU precision test.

The split forward stages a 32-row item tile as three bf16 pieces laid out [piece 3][k-step 8][lane 64][8 bf16]: each 16-byte
read at 16 * lane is the A fragment of one v_mfma_f32_32x32x16_bf16 -- lane (c, h) of k-step s holds features
16 s + 8 h .. + 7 of tile row c.  ``mf_fwd_split_image_index`` is the one index function the device code uses."""
from __future__ import annotations

import math

import numpy as np
import torch

from tests import _dense_cases as dc
from tests import _fwd_split_cases as fc

ROWS, FEATURES, PIECES = 32, 128, 3
SLOTS = ROWS * FEATURES * PIECES


def _index_table(lib):
    return np.array([[[lib.mf_fwd_split_image_index(y, m, p) for p in range(PIECES)] for m in range(FEATURES)]
                     for y in range(ROWS)])


def test_image_index_is_a_bijection_onto_the_tile(mf):
    lib = mf._lib.lib()
    idx = _index_table(lib)
    assert SLOTS == 12288
    assert idx.min() == 0 and idx.max() == SLOTS - 1
    assert len(np.unique(idx)) == SLOTS
    for bad in ((-1, 0, 0), (32, 0, 0), (0, 128, 0), (0, -1, 0), (0, 0, 3), (0, 0, -1)):
        assert lib.mf_fwd_split_image_index(*bad) == -1, bad


def test_image_index_gives_every_lane_eight_consecutive_features_of_one_row(mf):
    """slot = (((piece * 8 + s) * 64 + lane) * 8 + j: lane (c, h) holds tile row c, and its element j of k-step s is feature
    16 s + 8 h + j"""
    idx = _index_table(mf._lib.lib())
    seen = 0
    for piece in range(PIECES):
        for s in range(8):
            for lane in range(64):
                c, h = lane & 31, lane >> 5
                for j in range(8):
                    want = (((piece * 8 + s) * 64 + lane) * 8) + j
                    assert idx[c, 16 * s + 8 * h + j, piece] == want, (piece, s, lane, j)
                    seen += 1
    assert seen == SLOTS


def test_the_two_images_of_a_tile_differ_and_have_one_size(mf):
    """the backward's image is laid out for a contraction over the tile's rows: the forward cannot reuse it"""
    lib = mf._lib.lib()
    same = sum(lib.mf_fwd_split_image_index(y, m, 0) == lib.mf_bwd_split_image_index(y, m, 0) for y in range(ROWS) for m in range(FEATURES))
    assert same < ROWS * FEATURES // 8, same


def test_workspace_does_not_grow_for_the_forward_image(mf):
    """the forward's image lives where the backward's image of the item side does -- inside the G' stash, or in the room the
    backward's images already had for shapes too small for that: mf_loss_ws_bytes is what it was before the split forward"""
    lib = mf._lib.lib()
    before = {(24, 40): 34585856, (24, 1030): 39859456, (300, 1030): 46421248, (1020, 4090): 109451008, (2990, 2990): 153582336,
              (8192, 16384): 1212570112}
    assert set(fc.SHAPES) <= set(before)
    for (b, n), size in before.items():
        assert lib.mf_loss_ws_bytes(b, n, 128, 0, 0) == size, (b, n)
        bp, np_ = -(-b // 128) * 128, -(-n // 128) * 128
        assert np_ // 32 * SLOTS * 2 <= max(bp * np_ * 4, size - 2 * bp * np_ * 4), (b, n)       # the image fits where it is put


def test_shapes_have_the_geometry_they_are_chosen_for(mf):
    lib = mf._lib.lib()
    for b, n in fc.SHAPES:
        fc.assert_geometry(lib, b, n)
    # (24, 40): the last real item tile holds 8 columns
    assert 40 - 32 == 8 and 1030 - 32 * 32 == 6
    lo, hi = fc.GATE_SHAPES
    assert lo[0] * lo[1] < fc.FWD_SPLIT_MIN_BN <= hi[0] * hi[1]
    assert not fc.default_serves(*lo, 128, 0) and fc.default_serves(*hi, 128, 0)
    assert not fc.default_serves(8192, 16384, 64, 0) and not fc.default_serves(8192, 16384, 128, 4)


def test_emulated_pieces_sum_to_the_value():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(4096, generator=g) * torch.exp(4 * torch.randn(4096, generator=g))
    p = fc.bf16_pieces(x)
    assert float(((p[0].double() + p[1].double() + p[2].double()) - x.double()).abs().max() / x.abs().max()) <= 2.0 ** -24
    assert all(torch.equal(q, q.to(torch.bfloat16).float()) for q in p)


def test_six_products_are_fp32_grade_and_five_are_not():
    """the forward emulated on the inputs of the GPU precision test: bf16 casts, six products, fp32 accumulation, the logit map
    in fp32, InfoNCE behind it in float64; E against float64 in units of the gradient bar"""
    t = fc.precision_case()
    assert t["sigma"] == fc.PRECISION_SIGMA and tuple(t["u"].shape) == (fc.PRECISION_SHAPE[0], 128)
    r6, r5 = fc.emulation_ratios(t)
    print(f"r6 = {r6:.4g}, r5 = {r5:.4g}, factor = {math.sqrt(r6 * r5):.4g}")
    assert r5 >= 2 * r6, (r6, r5)
    assert abs(r6 / fc.R6 - 1) <= 0.25 and abs(r5 / fc.R5 - 1) <= 0.25, (r6, r5)
    assert abs(fc.FACTOR - math.sqrt(fc.R6 * fc.R5)) <= 0.005
    assert r6 < fc.FACTOR < r5
    # the scores themselves: six products are as close to float64 as an fp32 matmul, five are far off
    exact = t["u"].double() @ t["v"].double().T
    e32 = float((t["u"] @ t["v"].T - exact).abs().max())
    e6 = float((fc.scores(t["u"], t["v"]) - exact).abs().max())
    e5 = min(float((fc.scores(t["u"], t["v"], dropped=d) - exact).abs().max()) for d in ((2, 0), (1, 1), (0, 2)))
    assert e6 <= 2 * e32 and e5 >= 4 * e32, (e32, e6, e5)


def test_precision_case_is_the_dense_case_with_a_sharp_softmax():
    t, base = fc.precision_case(), dc.random_case(*fc.PRECISION_SHAPE, 128)
    assert all(torch.equal(t[k], base[k]) for k in ("u", "v", "target", "item_idx", "pos_idx", "logq"))
    assert base["sigma"] == 3.0 and t["sigma"] == 24.0          # (the shared case is left as it is)
