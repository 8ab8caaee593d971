"""Host model of how the two-level grouping (LVDGS_FLAG_SUPER_TILES) lists a Gaussian: its (Gaussian, tile) pairs and its
(Gaussian, super-tile) pairs, from the tile rectangle and the 64-bit kept-tile mask of its geom record (include/lvdgs.h, geom_rec).

Tile level (csrc/binning.hpp: for_each_pair_of_rect, RectBlocks): a rectangle of at most 64 tiles has a bit per tile (row-major); a
larger one has a bit per block of its 8 x 8 block grid (blocks ceil(w / 8) x ceil(h / 8) tiles, the last column and row narrower), and
every tile of a kept block is listed.
Super level (csrc/binning.hpp: super_rect_of): the rectangle in 4 x 4-tile super-tiles; a rectangle of more than 64 super-tiles lists
every one of them, otherwise a super-tile is listed when one of its tiles is."""
import numpy as np

MASK_TILES = 64
SUPER = 4


def decode(rec, live=None):
    """geom records (N x 16 float32) -> (x0, x1, y0, y1, mask) arrays (int64, mask uint64).  A record is written only for a Gaussian the
    projection kept (radius > 0): `live` (N bools, radii > 0) empties the others.  rec may also be the geom_state's rectangle array
    (N x 4 uint32, GeomView::rect: the same four words, zero for a culled Gaussian)."""
    rec = np.ascontiguousarray(rec)
    u = rec.view(np.uint32)
    u = u[:, 12:16] if u.shape[1] == 16 else u
    if live is not None:
        u = np.where(np.asarray(live, bool)[:, None], u, 0).astype(np.uint32)
    rx, ry = u[:, 0].astype(np.int64), u[:, 1].astype(np.int64)
    mask = u[:, 2].astype(np.uint64) | (u[:, 3].astype(np.uint64) << np.uint64(32))
    return rx & 0xFFFF, rx >> 16, ry & 0xFFFF, ry >> 16, mask


def _bit(mask, k):
    return (int(mask) >> int(k)) & 1


def block_grid(w, h):
    """-> (bw, bh): the tiles of a block of a rectangle of more than 64 tiles."""
    return (w + 7) // 8, (h + 7) // 8


def kept_tiles(x0, x1, y0, y1, mask):
    """The listed tiles of one rectangle, as (tx, ty) grid coordinates."""
    w, h = x1 - x0, y1 - y0
    if w <= 0 or h <= 0:
        return []
    out = []
    if w * h <= MASK_TILES:
        for ty in range(h):
            for tx in range(w):
                if _bit(mask, ty * w + tx):
                    out.append((x0 + tx, y0 + ty))
        return out
    bw, bh = block_grid(w, h)
    for ty in range(h):
        for tx in range(w):
            if _bit(mask, (ty // bh) * 8 + tx // bw):
                out.append((x0 + tx, y0 + ty))
    return out


def super_rect(x0, x1, y0, y1, mask):
    """super_rect_of: -> (sx0, sx1, sy0, sy1, listed super-tiles as (sx, sy))."""
    w, h = x1 - x0, y1 - y0
    if w <= 0 or h <= 0 or int(mask) == 0:
        return 0, 0, 0, 0, []
    sx0, sx1, sy0, sy1 = x0 // SUPER, (x1 - 1) // SUPER + 1, y0 // SUPER, (y1 - 1) // SUPER + 1
    if (sx1 - sx0) * (sy1 - sy0) > MASK_TILES:
        return sx0, sx1, sy0, sy1, [(sx, sy) for sy in range(sy0, sy1) for sx in range(sx0, sx1)]
    listed = sorted({(tx // SUPER, ty // SUPER) for tx, ty in kept_tiles(x0, x1, y0, y1, mask)}, key=lambda p: (p[1], p[0]))
    return sx0, sx1, sy0, sy1, listed


def pair_counts(x0, x1, y0, y1, mask):
    """-> (D_i, Ds_i) of one rectangle."""
    return len(kept_tiles(x0, x1, y0, y1, mask)), len(super_rect(x0, x1, y0, y1, mask)[4])


def _cdiv(a, b):
    return -(-a // b)


def _tile_count_fast(w, h, mask):
    if w <= 0 or h <= 0:
        return 0
    if w * h <= MASK_TILES:
        return bin(int(mask) & ((1 << (w * h)) - 1)).count("1")
    bw, bh = block_grid(w, h)
    n = 0
    for b in range(64):
        if _bit(mask, b):
            bwid, bhgt = min(bw, w - (b & 7) * bw), min(bh, h - (b >> 3) * bh)
            if bwid > 0 and bhgt > 0:
                n += bwid * bhgt
    return n


def frame_counts(rec, W, H, live=None):
    """-> (D_i, Ds_i, per-super-tile counts (gys x gxs)) of a frame's geom records or rectangles (decode; the hint-off run's are the same)."""
    x0, x1, y0, y1, mask = decode(rec, live)
    gxs, gys = _cdiv(_cdiv(W, 16), SUPER), _cdiv(_cdiv(H, 16), SUPER)
    D = np.zeros(len(x0), np.int64)
    Ds = np.zeros(len(x0), np.int64)
    per_super = np.zeros((gys, gxs), np.int64)
    for i in range(len(x0)):
        a, b, c, d, m = int(x0[i]), int(x1[i]), int(y0[i]), int(y1[i]), int(mask[i])
        if b <= a or d <= c or m == 0:
            continue
        D[i] = _tile_count_fast(b - a, d - c, m)
        sx0, sx1, sy0, sy1 = a // SUPER, (b - 1) // SUPER + 1, c // SUPER, (d - 1) // SUPER + 1
        if (sx1 - sx0) * (sy1 - sy0) > MASK_TILES:
            Ds[i] = (sx1 - sx0) * (sy1 - sy0)
            per_super[sy0:sy1, sx0:sx1] += 1
        else:
            listed = super_rect(a, b, c, d, m)[4]
            for sx, sy in listed:
                per_super[sy, sx] += 1
            Ds[i] = len(listed)
    return D, Ds, per_super
