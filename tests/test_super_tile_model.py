"""The host model of the two-level grouping's pair counts (super_tile_model.py), on rectangles worked out by hand: each branch of
super_rect_of, rectangles whose corners lie off the 4-tile grid, and the rectangle of more than 64 super-tiles that keeps one block of
its tiles -- where the super level lists MORE pairs than the tile level (Ds_i > D_i), the case the library must not cut short."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import super_tile_model as stm  # noqa: E402


def _rec(rects):
    """geom records (N x 16 float32) holding the given (x0, x1, y0, y1, mask) rectangles."""
    rec = np.zeros((len(rects), 16), np.float32)
    u = rec.view(np.uint32)
    for i, (x0, x1, y0, y1, m) in enumerate(rects):
        u[i, 12], u[i, 13] = x0 | (x1 << 16), y0 | (y1 << 16)
        u[i, 14], u[i, 15] = m & 0xFFFFFFFF, m >> 32
    return rec


# (x0, x1, y0, y1, mask) -> (D_i, Ds_i, listed super-tiles), each worked out by hand in the comment
HAND = [
    # a bit per tile: 6 x 3 tiles from (3, 2); tiles (3, 2) (bit 0) and (8, 4) (bit 2 * 6 + 5) -> super-tiles (0, 0), (2, 1)
    ((3, 9, 2, 5, (1 << 0) | (1 << 17)), 2, [(0, 0), (2, 1)]),
    # a bit per tile: tiles (4, 2), (5, 2) (bits 1, 2) share super-tile (1, 0)
    ((3, 9, 2, 5, 0b110), 2, [(1, 0)]),
    # a bit per tile, one row straddling two super-columns: tiles (6, 7), (7, 7), (8, 7) of a 5 x 1 rectangle from (5, 7)
    ((5, 10, 7, 8, 0b01110), 3, [(1, 1), (2, 1)]),
    # a bit per block (17 x 5 = 85 tiles, blocks 3 x 1): block 2 = tiles x 7..9 of row y 5 -> super-columns 1, 2 of super-row 1
    ((1, 18, 5, 10, 1 << 2), 3, [(1, 1), (2, 1)]),
    # a bit per block: block 5 of the last block column is min(3, 17 - 15) = 2 wide: tiles x 16, 17 -> super-tile (4, 1)
    ((1, 18, 5, 10, 1 << 5), 2, [(4, 1)]),
    # a bit per block: block 8 (block row 1) = tiles x 1..3 of row y 6 -> super-column 0, super-row 1
    ((1, 18, 5, 10, 1 << 8), 3, [(0, 1)]),
]


def test_hand_checked_rectangles():
    for (rect, D, listed) in HAND:
        got_D, got_Ds = stm.pair_counts(*rect)
        assert got_D == D, rect
        assert sorted(stm.super_rect(*rect)[4]) == sorted(listed), rect
        assert got_Ds == len(listed), rect


def test_more_than_64_super_tiles_list_them_all():
    # the whole 1280 x 720 grid (80 x 45 tiles, blocks 10 x 6) with block 0 kept: 60 tiles; 20 x 12 = 240 super-tiles
    x0, x1, y0, y1 = 0, 80, 0, 45
    assert stm.block_grid(80, 45) == (10, 6)
    assert stm.pair_counts(x0, x1, y0, y1, 1) == (60, 240)
    # corners off the 4-tile grid: 67 x 38 tiles from (3, 1), blocks 9 x 5; the last block (63) is min(9, 67 - 63) = 4 wide and
    # min(5, 38 - 35) = 3 high: 12 tiles.  Super-columns 0 .. 69 // 4 = 17, super-rows 0 .. 38 // 4 = 9: 18 x 10 = 180
    sx0, sx1, sy0, sy1, listed = stm.super_rect(3, 70, 1, 39, 1 << 63)
    assert (sx0, sx1, sy0, sy1) == (0, 18, 0, 10) and len(listed) == 180
    assert stm.pair_counts(3, 70, 1, 39, 1 << 63) == (12, 180)
    # two kept blocks, still far fewer tiles than super-tiles
    D, Ds = stm.pair_counts(0, 80, 0, 45, (1 << 0) | (1 << 7))
    assert (D, Ds) == (120, 240) and Ds > D


def test_frame_counts_match_the_per_rectangle_model():
    rng = np.random.default_rng(0)
    rects = [r for r, _, _ in HAND] + [(0, 80, 0, 45, 1), (3, 70, 1, 39, 1 << 63), (0, 0, 0, 0, 0), (2, 4, 2, 4, 0)]
    for _ in range(300):
        x0, y0 = int(rng.integers(0, 79)), int(rng.integers(0, 44))
        x1, y1 = int(rng.integers(x0 + 1, 81)), int(rng.integers(y0 + 1, 46))
        area = (x1 - x0) * (y1 - y0)
        bits = min(area, 64) if area <= 64 else 64
        m = int(rng.integers(0, 1 << 62)) & ((1 << bits) - 1) if rng.random() < 0.7 else 1 << int(rng.integers(0, bits))
        rects.append((x0, x1, y0, y1, m))
    rec = _rec(rects + [(0, 80, 0, 45, (1 << 64) - 1)])   # + a culled Gaussian: its record is not read
    live = np.arange(len(rec)) < len(rects)
    D, Ds, per_super = stm.frame_counts(rec, 1280, 720, live)
    assert D[-1] == Ds[-1] == 0
    D, Ds = D[:-1], Ds[:-1]
    D4, Ds4, per_super4 = stm.frame_counts(np.where(live[:, None], rec.view(np.uint32)[:, 12:16], 0).astype(np.uint32), 1280, 720)
    assert np.array_equal(D4[:-1], D) and np.array_equal(Ds4[:-1], Ds) and np.array_equal(per_super4, per_super)
    want = np.zeros((12, 20), np.int64)
    for i, r in enumerate(rects):
        d, ds = stm.pair_counts(*r)
        assert (D[i], Ds[i]) == (d, ds), r
        for sx, sy in stm.super_rect(*r)[4]:
            want[sy, sx] += 1
        if stm.super_rect(*r)[4] and (r[1] - r[0]) * (r[3] - r[2]) <= 64:
            assert ds <= d, r   # a bit per tile: a listed super-tile holds a listed tile
    assert np.array_equal(per_super, want)
    assert per_super.sum() == Ds.sum()
