"""CPU: the operand image of the split backward sweeps (csrc/mf_bf_split.h) and the workspace that holds it.

A split sweep stages a 32-row tile of its streamed operand as three bf16 pieces laid out
[piece 3][accumulator block 4][k-step 2][lane 64][8 bf16]: each 16-byte read at 16 * lane is the A fragment of one
v_mfma_f32_32x32x16_bf16, whose B fragment is the G' tile in accumulator layout.  ``mf_bwd_split_image_index`` is the one
index function the device code uses; here it is checked against that description for every (row, feature, piece).
The piece split itself is device code: its exactness is covered by tests/test_gpu_dense_bwd_split.py."""
from __future__ import annotations

import numpy as np

ROWS, FEATURES, PIECES = 32, 128, 3
SLOTS = ROWS * FEATURES * PIECES
SHAPES = ((256, 512), (1020, 4090), (1990, 3050), (2990, 2990), (3060, 3060), (8192, 16384))


def _index_table(lib):
    return np.array([[[lib.mf_bwd_split_image_index(y, m, p) for p in range(PIECES)] for m in range(FEATURES)]
                     for y in range(ROWS)])


def test_image_index_is_a_bijection_onto_the_tile(mf):
    idx = _index_table(mf._lib.lib())
    assert SLOTS == 12288
    assert idx.min() == 0 and idx.max() == SLOTS - 1
    assert len(np.unique(idx)) == SLOTS
    lib = mf._lib.lib()
    for bad in ((-1, 0, 0), (32, 0, 0), (0, 128, 0), (0, -1, 0), (0, 0, 3), (0, 0, -1)):
        assert lib.mf_bwd_split_image_index(*bad) == -1, bad


def test_image_index_puts_every_lane_on_the_rows_its_stash_registers_hold(mf):
    """slot = (((piece * 4 + block) * 2 + s) * 64 + lane) * 8 + j; lane (r, h) holds feature 4 r + block, and its element j
    of k-step s is row (j & 3) + 8 (2 s + (j >> 2)) + 4 h of the tile -- the row of stash register 8 s + j"""
    idx = _index_table(mf._lib.lib())
    seen = 0
    for piece in range(PIECES):
        for block in range(4):
            for s in range(2):
                for lane in range(64):
                    r, h = lane & 31, lane >> 5
                    for j in range(8):
                        e = 8 * s + j                                  # the stash register
                        row = (e & 3) + 8 * (e >> 2) + 4 * h            # mf_acc_row(e, h)
                        assert row == (j & 3) + 8 * (2 * s + (j >> 2)) + 4 * h
                        want = (((piece * 4 + block) * 2 + s) * 64 + lane) * 8 + j
                        assert idx[row, 4 * r + block, piece] == want, (piece, block, s, lane, j)
                        seen += 1
    assert seen == SLOTS


def test_workspace_has_room_for_the_images_and_grows_with_the_shape(mf):
    lib = mf._lib.lib()
    sizes = [lib.mf_loss_ws_bytes(b, n, 128, 0, 0) for b, n in SHAPES]
    assert all(x > 0 for x in sizes), sizes
    by_area = sorted(zip((b * n for b, n in SHAPES), sizes))
    assert [x for _, x in by_area] == sorted(sizes), by_area       # monotone in the stash area, which dominates
    for (b, n), size in zip(SHAPES, sizes):
        bp, np_ = -(-b // 128) * 128, -(-n // 128) * 128
        images = (bp + np_) // 32 * SLOTS * 2
        # both stashes; the images live in the G' stash, which a split backward leaves unused, unless they do not fit it
        own_room = images if images > bp * np_ * 4 else 0
        assert own_room == (images if (b, n) == (256, 512) else 0), (b, n)
        assert size > 2 * bp * np_ * 4 + own_room, ((b, n), size)
        assert lib.mf_loss_ws_bytes(b, n + 128, 128, 0, 0) > size and lib.mf_loss_ws_bytes(b + 128, n + 128, 128, 0, 0) > size
    # a shape too small for that gets room of its own: 8 tiles of 24 KiB against a 128 x 128 stash
    tiny = lib.mf_loss_ws_bytes(100, 100, 128, 0, 0)
    assert tiny > 2 * 128 * 128 * 4 + 8 * SLOTS * 2, tiny
