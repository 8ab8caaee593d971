"""Independent restatement of the frame ingest's arithmetic (include/lvdgs.h: ``lvdgs_undistort_map``, ``lvdgs_ingest_frame``), held
against both the HIP kernels and ``lvdgs.dataset``'s host mode.  Nothing here is shared with either.

Two forms of the same rule:
  * ``map_pixel`` / ``remap_pixel`` / ``unit``: one pixel at a time in Python floats (IEEE float64) and Python integers -- the rule as
    the header writes it, used whole on the small cases;
  * ``undistort_map`` / ``remap`` / ``convert``: the same over flat arrays of pixel indices, for frames too large for a Python loop --
    integer floor division and modulo instead of shifts and masks, a zero frame around the image instead of per-neighbour tests,
    rounding spelled out instead of ``rint``.  tests/test_dataset.py holds the two forms to each other on the small cases.
"""
import math

import numpy as np

OUTSIDE = -2 ** 31
LIMIT = 2.0 ** 20


# ---- one pixel at a time ----
def fixed(m):
    """A float32 map coordinate -> its fixed-point value with 5 fractional bits (ties to even), or OUTSIDE."""
    m = float(m)
    if not math.isfinite(m) or abs(m) >= LIMIT:
        return OUTSIDE
    return round(m * 32.0)          # exact product; Python's round of a float: half to even


def map_pixel(u, v, fx, fy, cx, cy, dist):
    k1, k2, p1, p2, k3 = (float(d) for d in dist)
    with np.errstate(all="ignore"):
        x = (np.float64(u) - cx) / fx
        y = (np.float64(v) - cy) / fy
        r2 = x * x + y * y
        kr = 1 + ((k3 * r2 + k2) * r2 + k1) * r2
        xd = x * kr + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
        yd = y * kr + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
        mapx, mapy = np.float32(fx * xd + cx), np.float32(fy * yd + cy)
    return fixed(mapx), fixed(mapy)


def is_tie(s_float32):
    """Does this float32 coordinate, times 32, lie exactly between two integers?"""
    m = float(s_float32)
    return math.isfinite(m) and abs(m) < LIMIT and (m * 32.0) - math.floor(m * 32.0) == 0.5


def remap_pixel(image, sx, sy):
    """image: (H, W, 3) uint8 -> the three bytes of a destination pixel whose map entry is (sx, sy)."""
    H, W = image.shape[:2]
    if sx == OUTSIDE or sy == OUTSIDE:
        return (0, 0, 0)
    ix, ax, iy, ay = sx // 32, sx % 32, sy // 32, sy % 32      # Python: floor division, a non-negative remainder
    out = []
    for c in range(3):
        total = 0
        for xx, yy, w in ((ix, iy, (32 - ax) * (32 - ay)), (ix + 1, iy, ax * (32 - ay)), (ix, iy + 1, (32 - ax) * ay), (ix + 1, iy + 1, ax * ay)):
            if 0 <= xx < W and 0 <= yy < H:
                total += w * int(image[yy, xx, c])
        out.append((total + 512) // 1024)
    return tuple(out)


def unit(byte):
    return np.float32(int(byte) / 255.0)


def undistort_map_loop(W, H, fx, fy, cx, cy, dist):
    sx, sy = np.empty((H, W), np.int32), np.empty((H, W), np.int32)
    for v in range(H):
        for u in range(W):
            sx[v, u], sy[v, u] = map_pixel(u, v, fx, fy, cx, cy, dist)
    return sx, sy


def remap_loop(image, sx, sy):
    out = np.empty_like(image)
    for v in range(image.shape[0]):
        for u in range(image.shape[1]):
            out[v, u] = remap_pixel(image, int(sx[v, u]), int(sy[v, u]))
    return out


def convert_loop(image):
    H, W = image.shape[:2]
    out = np.empty((3, H, W), np.float32)
    for c in range(3):
        for v in range(H):
            for u in range(W):
                out[c, v, u] = unit(image[v, u, c])
    return out


# ---- over flat arrays ----
def _fixed_array(m32):
    m = m32.astype(np.float64)
    ok = np.isfinite(m) & (np.abs(m) < LIMIT)
    t = np.where(ok, m, 0.0) * 32.0
    lo = np.floor(t)
    frac = t - lo
    up = (frac > 0.5) | ((frac == 0.5) & (np.mod(lo, 2.0) == 1.0))     # half to even
    return np.where(ok, (lo + up).astype(np.int64), OUTSIDE).astype(np.int32)


def undistort_map(W, H, fx, fy, cx, cy, dist):
    k1, k2, p1, p2, k3 = (float(d) for d in dist)
    p = np.arange(W * H, dtype=np.int64)
    u, v = (p % W).astype(np.float64), (p // W).astype(np.float64)
    with np.errstate(all="ignore"):
        x, y = (u - cx) / fx, (v - cy) / fy
        r2 = x * x + y * y
        kr = 1 + ((k3 * r2 + k2) * r2 + k1) * r2
        xd = x * kr + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
        yd = y * kr + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
        mapx, mapy = (fx * xd + cx).astype(np.float32), (fy * yd + cy).astype(np.float32)
    return _fixed_array(mapx).reshape(H, W), _fixed_array(mapy).reshape(H, W)


def remap(image, sx, sy):
    H, W = image.shape[:2]
    framed = np.zeros((H + 2, W + 2, 3), np.int64)           # one zero pixel all round: row iy + 1, column ix + 1
    framed[1:-1, 1:-1] = image
    sx, sy = sx.reshape(-1).astype(np.int64), sy.reshape(-1).astype(np.int64)
    gone = (sx == OUTSIDE) | (sy == OUTSIDE)
    ix, ax, iy, ay = sx // 32, sx % 32, sy // 32, sy % 32
    gone |= (ix < -1) | (ix > W - 1) | (iy < -1) | (iy > H - 1)   # all four neighbours off the image: nothing to add
    ix, iy = np.where(gone, 0, ix), np.where(gone, 0, iy)
    total = ((32 - ax) * (32 - ay))[:, None] * framed[iy + 1, ix + 1] + (ax * (32 - ay))[:, None] * framed[iy + 1, ix + 2] \
        + ((32 - ax) * ay)[:, None] * framed[iy + 2, ix + 1] + (ax * ay)[:, None] * framed[iy + 2, ix + 2]
    out = (total + 512) // 1024
    out[gone] = 0
    return out.astype(np.uint8).reshape(H, W, 3)


def convert(image):
    table = np.array([np.float32(b / 255.0) for b in range(256)], np.float32)
    return np.ascontiguousarray(np.moveaxis(table[image], 2, 0))
