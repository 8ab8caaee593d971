"""NumPy float64 restatement of ``lvdgs_match_depth_scale`` (include/lvdgs.h; the reference's ``find_scale``, utils/depth_utils.py:31-55)
and of the nearest-neighbour rule ``init_pose.get_depth`` resizes with.  Every expression is written as the kernel writes it, so a
sample is the same float64 bits on both sides; only the order of the two sums differs."""
import numpy as np

OK, NO_VALID = 1, 2


def axis(i, n_src, n_dst):
    """-> (s, s + 1 clamped, t) of raster index array ``i``."""
    f = (i.astype(np.float64) + 0.5) * (np.float64(n_src) / np.float64(n_dst)) - 0.5
    fl = np.floor(f)
    s = fl.astype(np.int64)
    t = f - fl
    low, high = s < 0, s >= n_src - 1
    s = np.where(low, 0, np.where(high, n_src - 1, s))
    t = np.where(low | high, 0.0, t)
    return s, np.minimum(s + 1, n_src - 1), t


def sample(depth, x, y, raster):
    """``depth`` (H, W) as if resized bilinearly to ``raster`` = (W1, H1), at the raster pixels (x, y) (inside it) -> float64."""
    H, W = depth.shape
    W1, H1 = raster
    d = depth.astype(np.float64)
    sx, sx1, tx = axis(x, W, W1)
    sy, sy1, ty = axis(y, H, H1)
    a, b, c, e = d[sy, sx], d[sy, sx1], d[sy1, sx], d[sy1, sx1]
    with np.errstate(invalid="ignore"):
        return (1.0 - ty) * ((1.0 - tx) * a + tx * b) + ty * ((1.0 - tx) * c + tx * e)


def match_scale(matches_im1, matches_im2, depth1, depth2, raster, order=None):
    """-> dict(status, matches, valid, scale (np.float32, None without a valid match), sum1, sum2, mask).  ``order``: a permutation of
    the valid matches in which the two sums are taken one term after the other (default: NumPy's pairwise sum)."""
    W1, H1 = raster
    m1 = np.asarray(matches_im1, dtype=np.int32).reshape(-1, 2)
    m2 = np.asarray(matches_im2, dtype=np.float32).reshape(-1, 2)
    M = len(m1)
    x1, y1, u, v = m1[:, 0].astype(np.int64), m1[:, 1].astype(np.int64), m2[:, 0], m2[:, 1]
    with np.errstate(invalid="ignore"):
        inside = (x1 >= 0) & (x1 < W1) & (y1 >= 0) & (y1 < H1) & (u > np.float32(-1)) & (u < np.float32(W1)) & (v > np.float32(-1)) & (v < np.float32(H1))
    idx = np.nonzero(inside)[0]
    x2, y2 = np.trunc(u[idx]).astype(np.int64), np.trunc(v[idx]).astype(np.int64)
    a = sample(np.asarray(depth1, dtype=np.float32), x1[idx], y1[idx], raster)
    b = sample(np.asarray(depth2, dtype=np.float32), x2, y2, raster)
    with np.errstate(invalid="ignore"):
        good = (a > 0) & (a < np.inf) & (b > 0) & (b < np.inf)
    mask = np.zeros(M, dtype=bool)
    mask[idx[good]] = True
    a, b = a[good], b[good]
    n = int(good.sum())
    if order is not None:
        s1 = float(np.cumsum(a[order])[-1]) if n else 0.0
        s2 = float(np.cumsum(b[order])[-1]) if n else 0.0
    else:
        s1, s2 = float(a.sum()), float(b.sum())
    scale = np.float32((s1 / n) / (s2 / n)) if n else None
    return dict(status=OK if n else NO_VALID, matches=M, valid=n, scale=scale, sum1=s1, sum2=s2, mask=mask)


def nearest_resize(z, W, H):
    """``cv2.resize(z, (W, H), interpolation=cv2.INTER_NEAREST)``'s rule: source index min(floor(d * n_src / n_dst), n_src - 1), float64."""
    Hs, Ws = z.shape
    sx = np.minimum(np.floor(np.arange(W, dtype=np.float64) * np.float64(Ws) / np.float64(W)).astype(np.int64), Ws - 1)
    sy = np.minimum(np.floor(np.arange(H, dtype=np.float64) * np.float64(Hs) / np.float64(H)).astype(np.int64), Hs - 1)
    return z[sy][:, sx]
