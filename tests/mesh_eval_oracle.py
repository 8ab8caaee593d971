"""The mesh-scoring rules of include/lvdgs.h ("Mesh scoring") in NumPy, each written twice:

``sample_f32`` / ``nearest_f32``   mirrors of the header, operation for operation: float64 areas, Python-integer weights, prefix and
                                   ``(h64 * total) >> 64``, float32 barycentric arithmetic; a brute-force float32 ``argmin`` with the
                                   lowest-index rule;
``sample_f64`` / ``nearest_f64``   the same rules stated independently in float64 (the integer decisions by other means).

And the meshes and clouds the tests of both files share.
"""
import bisect
import math

import numpy as np

F = np.float32
MASK32 = 0xFFFFFFFF
TWO24 = 1 << 24
NO_AREA, NO_REFERENCE = 1, 1


# ---------------------------------------------------------------- keys ----
def fmix32(h):
    h &= MASK32
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & MASK32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & MASK32
    h ^= h >> 16
    return h


def key(i, seed):
    """key(i) of the header: i a Python integer below 2^64, seed a Python integer (64 bits)."""
    seed_lo, seed_hi = seed & MASK32, (seed >> 32) & MASK32
    return fmix32(fmix32((i + seed_lo) & MASK32) ^ ((seed_hi + (i >> 32)) & MASK32))


def sample_keys(n, seed):
    """(n, 3) Python integers as a uint64 array: vectorised ``key`` (checked against it in the tests)."""
    i = np.arange(3 * n, dtype=np.uint64)
    lo, hi = np.uint64(seed & MASK32), np.uint64((seed >> 32) & MASK32)
    m = np.uint64(MASK32)

    def mix(h):
        h = h & m
        h = h ^ (h >> np.uint64(16))
        h = (h * np.uint64(0x85EBCA6B)) & m
        h = h ^ (h >> np.uint64(13))
        h = (h * np.uint64(0xC2B2AE35)) & m
        return h ^ (h >> np.uint64(16))
    return mix(mix((i + lo) & m) ^ ((hi + (i >> np.uint64(32))) & m)).reshape(n, 3)


# ---------------------------------------------------------------- sampling, the mirror ----
def face_areas(vertices, faces):
    """Step 1: float64 areas from the float32 coordinates, as written; 0 for a face the rule gives no weight."""
    v = np.asarray(vertices, np.float32).astype(np.float64)
    f = np.asarray(faces, np.int64)
    ok = ((f >= 0) & (f < len(v))).all(1)
    g = np.where(ok[:, None], f, 0)
    a, b, c = v[g[:, 0]], v[g[:, 1]], v[g[:, 2]]
    with np.errstate(all="ignore"):
        e1, e2 = b - a, c - a
        nx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        ny = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        nz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        A = 0.5 * np.sqrt((nx * nx + ny * ny) + nz * nz)
        good = ok & np.isfinite(A) & (A > 0)
    return np.where(good, A, 0.0)


def weights(areas):
    """Steps 2 and 3 -> (q, the inclusive prefix, total) as Python integers."""
    amax = float(areas.max()) if len(areas) else 0.0
    q = [int(math.floor(float(A) / amax * 4294967296.0)) if A > 0 else 0 for A in areas]
    prefix, acc = [], 0
    for w in q:
        acc += w
        prefix.append(acc)
    return q, prefix, acc


def draws(n, seed, total):
    """Step 4's integers for samples 0 .. n-1: (t as Python integers, u1, u2 after the fold)."""
    k = sample_keys(n, seed)
    t = [((int(a) << 32 | int(b)) * total) >> 64 for a, b in zip(k[:, 0], k[:, 1])]
    u1, u2 = (k[:, 2] >> np.uint64(8)).astype(np.int64), (k[:, 1] & np.uint64(0xFFFFFF)).astype(np.int64)
    fold = u1 + u2 > TWO24
    return t, np.where(fold, TWO24 - u1, u1), np.where(fold, TWO24 - u2, u2)


def sample_f32(vertices, faces, n, seed, colors=None):
    """-> dict(points (n, 3) float32, face_index (n,) int32, colors or None, flags, n_weighted, total); with no weighted face
    points / face_index / colors are None."""
    vertices = np.asarray(vertices, np.float32)
    areas = face_areas(vertices, faces)
    q, prefix, total = weights(areas)
    out = dict(flags=NO_AREA if total == 0 else 0, n_weighted=int((areas > 0).sum()), total=total, points=None, face_index=None, colors=None)
    if total == 0:
        return out
    t, u1, u2 = draws(n, seed, total)
    pre = np.array(prefix, dtype=np.uint64)
    face = np.searchsorted(pre, np.array(t, dtype=np.uint64), side="right")      # the first f with prefix[f] > t
    r1, r2 = (u1.astype(F) * F(2.0 ** -24))[:, None], (u2.astype(F) * F(2.0 ** -24))[:, None]
    f = np.asarray(faces, np.int64)[face]

    def blend(values):
        a, b, c = values[f[:, 0]], values[f[:, 1]], values[f[:, 2]]
        with np.errstate(all="ignore"):
            return ((a + r1 * (b - a)) + r2 * (c - a)).astype(F)
    out["points"], out["face_index"] = blend(vertices), face.astype(np.int32)
    if colors is not None:
        out["colors"] = blend(np.asarray(colors, np.float32))
    return out


# ---------------------------------------------------------------- sampling, float64 ----
def sample_f64(vertices, faces, n, seed):
    """The rule again: areas by the norm of the cross product, the weights as exact integer floors, the face of a draw by counting
    (``bisect``), the point as the barycentric combination in float64.  -> (points float64, face_index)."""
    v = np.asarray(vertices, np.float32).astype(np.float64)
    faces = np.asarray(faces, np.int64)
    areas = np.zeros(len(faces))
    for i, (a, b, c) in enumerate(faces):
        if min(a, b, c) < 0 or max(a, b, c) >= len(v):
            continue
        with np.errstate(all="ignore"):
            A = 0.5 * math.sqrt(float((np.cross(v[b] - v[a], v[c] - v[a]) ** 2).sum())) if np.isfinite(v[[a, b, c]]).all() else 0.0
        areas[i] = A if (A > 0 and math.isfinite(A)) else 0.0
    amax = areas.max()
    cum, acc = [], 0
    for A in areas:
        acc += int(A / amax * 2.0 ** 32) if A > 0 else 0      # (int truncates: the floor of a positive number)
        cum.append(acc)
    points, chosen = np.zeros((n, 3)), np.zeros(n, np.int64)
    for k in range(n):
        k0, k1, k2 = key(3 * k, seed), key(3 * k + 1, seed), key(3 * k + 2, seed)
        t = ((k0 * 2 ** 32 + k1) * acc) // 2 ** 64
        f = bisect.bisect_right(cum, t)
        u1, u2 = k2 // 256, k1 % TWO24
        if u1 + u2 > TWO24:
            u1, u2 = TWO24 - u1, TWO24 - u2
        a, b, c = v[faces[f]]
        points[k] = a + (u1 / TWO24) * (b - a) + (u2 / TWO24) * (c - a)
        chosen[k] = f
    return points, chosen


# ---------------------------------------------------------------- the search ----
def nearest_f32(query, reference, chunk=256):
    """The result rule by brute force in float32 as written -> (d2 (M,) float32, idx (M,) int32).  ``argmin`` returns the first of
    equal minima: the lowest index."""
    q, r = np.asarray(query, np.float32).reshape(-1, 3), np.asarray(reference, np.float32).reshape(-1, 3)
    usable = np.isfinite(r).all(1)
    d2 = np.full(len(q), np.inf, F)
    idx = np.full(len(q), -1, np.int32)
    finite = np.isfinite(q).all(1)
    if not usable.any():
        return d2, idx
    for first in range(0, len(q), chunk):
        sl = slice(first, first + chunk)
        with np.errstate(all="ignore"):
            dx, dy, dz = (q[sl, None, a] - r[None, :, a] for a in range(3))
            d = ((dx * dx + dy * dy) + dz * dz).astype(F)
        d[:, ~usable] = np.inf
        j = np.argmin(d, axis=1)
        if not usable[0]:      # all-infinite rows: the lowest USABLE index
            j = np.where(np.isinf(d[np.arange(len(j)), j]), np.argmax(usable), j)
        d2[sl], idx[sl] = d[np.arange(len(j)), j], j
    d2[~finite], idx[~finite] = np.inf, -1
    return d2, idx


def nearest_f64(query, reference, chunk=256):
    """min_j |q - r_j|^2 in float64 by the expanded norm of differences (``einsum``) -> d2 (M,) float64; NaN where the rule skips."""
    q, r = np.asarray(query, np.float32).astype(np.float64).reshape(-1, 3), np.asarray(reference, np.float32).astype(np.float64).reshape(-1, 3)
    r = r[np.isfinite(r).all(1)]
    out = np.full(len(q), np.nan)
    if not len(r):
        return out
    for first in range(0, len(q), chunk):
        diff = q[first:first + chunk, None, :] - r[None, :, :]
        with np.errstate(all="ignore"):
            out[first:first + chunk] = np.einsum("mnk,mnk->mn", diff, diff).min(1)
    out[~np.isfinite(q).all(1)] = np.nan
    return out


def row_of(d2, idx, thresholds=(), n_reference=None):
    """The row's counts and maximum from a call's d2 / idx (exact), and its sums by ``math.fsum``."""
    counted = idx >= 0
    d = np.sqrt(d2[counted].astype(F)).astype(F)
    return dict(n_counted=int(counted.sum()), n_skipped=int((~counted).sum()),
                n_below=[int((d < F(t)).sum()) for t in thresholds] + [0] * (4 - len(thresholds)),
                max_distance=float(d.max()) if len(d) else 0.0,
                sum_distance=math.fsum(float(x) for x in d), sum_squared=math.fsum(float(x) for x in d2[counted]),
                flags=NO_REFERENCE if n_reference == 0 else 0)


# ---------------------------------------------------------------- shared inputs ----
def three_triangles():
    """Areas 1 : 2 : 5 (0.5, 1.0, 2.5) in three planes, with vertex colours."""
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0],
                  [2, 0, 1], [4, 0, 1], [2, 0, 2],
                  [0, 3, 0], [0, 5, 0], [0, 3, 2.5]], np.float32)
    f = np.arange(9, dtype=np.int32).reshape(3, 3)
    c = np.random.default_rng(3).random((9, 3)).astype(np.float32)
    return v, f, c


def wavy_wall(nu, nv, seed=0, size=2.0, amplitude=0.15, offset=0.0):
    """A wall z = offset + amplitude * sin(3x) * cos(2y) over [0, size]^2 as 2 * (nu - 1) * (nv - 1) triangles of uneven size."""
    rng = np.random.default_rng(seed)
    u = np.sort(np.concatenate([[0.0, 1.0], rng.random(nu - 2)])) * size
    w = np.sort(np.concatenate([[0.0, 1.0], rng.random(nv - 2)])) * size
    x, y = np.meshgrid(u, w, indexing="xy")
    z = offset + amplitude * np.sin(3 * x) * np.cos(2 * y)
    vertices = np.stack([x, y, z], -1).reshape(-1, 3).astype(np.float32)
    i, j = np.meshgrid(np.arange(nu - 1), np.arange(nv - 1), indexing="xy")
    p = (j * nu + i).reshape(-1)
    faces = np.concatenate([np.stack([p, p + 1, p + nu], 1), np.stack([p + 1, p + nu + 1, p + nu], 1)]).astype(np.int32)
    colors = rng.random((len(vertices), 3)).astype(np.float32)
    return vertices, faces, colors


def unit_square(z=0.0):
    v = np.array([[0, 0, z], [1, 0, z], [1, 1, z], [0, 1, z]], np.float32)
    return v, np.array([[0, 1, 2], [0, 2, 3]], np.int32)


def score_of(d_est, d_gt, threshold):
    """The score from the two directions' float32 distances (counted queries only), in float64."""
    t = F(threshold)
    acc, comp = math.fsum(map(float, d_est)) / len(d_est), math.fsum(map(float, d_gt)) / len(d_gt)
    p, r = float((d_est < t).sum()) / len(d_est), float((d_gt < t).sum()) / len(d_gt)
    return dict(accuracy=acc, completion=comp, completion_ratio=r, precision=p, recall=r, fscore=2 * p * r / (p + r) if p + r > 0 else 0.0,
                chamfer=0.5 * (acc + comp))
