"""NumPy oracle of the fused seeding (lvdgs_seed_points; include/lvdgs.h): the selection rule restated, and the float32 expressions of a
selected pixel one rounding at a time.

Pixel i = v*W + u is VALID when depth[i] > 0 and depth[i] <= depth_trunc (NaN fails).  n_keep = int(n_valid * inv_downsample) in double.
key(i) = fmix32(fmix32(uint32(i) + seed_lo) ^ seed_hi), uint32 with wrap-around; fmix32, the addition and the xor are bijections, so the
keys of one image are distinct.  Selected: the n_keep valid pixels with the smallest keys, rows in ascending pixel index."""
import numpy as np

MASK64 = (1 << 64) - 1
C0 = np.float32(0.28209479177387814)


def splitmix64(state):
    """One SplitMix64 step from ``state``: -> the output (the new state is state + 0x9E3779B97F4A7C15)."""
    z = (state + 0x9E3779B97F4A7C15) & MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


def fmix32(h):
    h = h.astype(np.uint32, copy=True)
    h ^= h >> np.uint32(16)
    h *= np.uint32(0x85EBCA6B)
    h ^= h >> np.uint32(13)
    h *= np.uint32(0xC2B2AE35)
    h ^= h >> np.uint32(16)
    return h


def keys(n, seed):
    """The keys of pixels 0 .. n - 1 under the 64-bit ``seed``."""
    lo, hi = np.uint32(seed & 0xFFFFFFFF), np.uint32((seed >> 32) & 0xFFFFFFFF)
    with np.errstate(over="ignore"):
        return fmix32(fmix32(np.arange(n, dtype=np.uint32) + lo) ^ hi)


def valid_mask(depth, depth_trunc=100.0):
    d = np.asarray(depth, np.float32).reshape(-1)
    with np.errstate(invalid="ignore"):
        return (d > np.float32(0)) & (d <= np.float32(depth_trunc))


def select(depth, inv_downsample, seed, depth_trunc=100.0):
    """-> dict(n_valid, n_keep, pixel: the selected pixel indices ascending (int64), threshold: the key t, or None when nothing is kept)."""
    valid = valid_mask(depth, depth_trunc)
    idx = np.flatnonzero(valid)
    n_valid = int(idx.size)
    n_keep = int(float(n_valid) * float(inv_downsample))
    if n_keep == 0:
        return dict(n_valid=n_valid, n_keep=0, pixel=np.empty(0, np.int64), threshold=None)
    k = keys(valid.size, seed)
    t = np.partition(k[idx], n_keep - 1)[n_keep - 1]
    pixel = idx[k[idx] <= t]
    return dict(n_valid=n_valid, n_keep=n_keep, pixel=pixel.astype(np.int64), threshold=int(t))


def colours(image, pixel, gain=1.0, offset=0.0):
    """(rgb, f_dc) of the pixels: c = min(max(gain * x + offset, 0), 1), q = uint8(c * 255) truncated, rgb = float(q) * (1 / 255) with the
    reciprocal rounded to float32 (PyTorch's `/ 255.0` on a GPU), f_dc = (rgb - 0.5) / C0."""
    f = np.float32
    x = np.asarray(image, f).reshape(3, -1)[:, pixel].T
    c = np.minimum(np.maximum(f(gain) * x + f(offset), f(0)), f(1))
    q = (c * f(255)).astype(np.uint8)
    rgb = q.astype(f) * (f(1) / f(255))
    return rgb, (rgb - f(0.5)) / C0


def points(depth, pixel, W, intrinsics, R, T):
    """xyz of the pixels: cam = ((u - cx) * z / fx, (v - cy) * z / fy, z); xyz[j] = sum_k (cam[k] - T[k]) * R[k][j], left to right."""
    f = np.float32
    fx, fy, cx, cy = (f(v) for v in intrinsics)
    R, T = np.asarray(R, f).reshape(3, 3), np.asarray(T, f).reshape(3)
    z = np.asarray(depth, f).reshape(-1)[pixel]
    v, u = pixel // W, pixel % W
    cam = [(u.astype(f) - cx) * z / fx, (v.astype(f) - cy) * z / fy, z]
    d = [cam[k] - T[k] for k in range(3)]
    return np.stack([(d[0] * R[0, j] + d[1] * R[1, j]) + d[2] * R[2, j] for j in range(3)], axis=1)


def seed_points(image, depth, intrinsics, R, T, inv_downsample, seed, gain=1.0, offset=0.0, depth_trunc=100.0):
    H, W = np.asarray(depth).shape
    out = select(depth, inv_downsample, seed, depth_trunc)
    out["xyz"] = points(depth, out["pixel"], W, intrinsics, R, T)
    if image is not None:
        out["rgb"], out["f_dc"] = colours(image, out["pixel"], gain, offset)
    return out


def lower_median(values):
    """torch.median of a NaN-free array: the (n - 1) // 2-th smallest."""
    v = np.sort(np.asarray(values, np.float32).reshape(-1))
    return v[(v.size - 1) // 2]
