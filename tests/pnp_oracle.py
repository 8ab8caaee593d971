"""Float64 NumPy statement of the pose initialisation by PnP-RANSAC on the rendered depth (the semantics of ``lvdgs_pnp_ransac``,
include/lvdgs.h): the gather with the ten-step Brown undistortion, the counter-based sample hash, the
three-point Gauss-Newton hypotheses, the scoring, the winner and the refinement on the consensus set.

``solve(depth, m1, m2, K, dist, ...)`` returns a dict: status, valid (count), valid_mask, pose (4 x 4; the exact identity on failure),
inlier_mask, inliers (final count), hypothesis (the winner, -1: none), winner_count, counts (per hypothesis, -1: void), samples
(hypotheses x 3, -1: void slot), fragile_counts (per hypothesis: the valid matches whose reprojection error lies within ``tie`` px of
the threshold -- where a computation that rounds otherwise may count the other way), fragile_rounds (the same over the refinement's
re-selections), fragile_final (bool per match, under the final pose).  ``sum_order``: a permutation of the matches in whose order the
refinement's sums are taken (the sums' own sensitivity to their order; the samples keep their indices)."""
import numpy as np

OK, FAILED = 1, 2
FAIL_NONE, FAIL_FEW_VALID, FAIL_ALL_VOID, FAIL_FEW_INLIERS, FAIL_SINGULAR = 0, 1, 2, 3, 4
UNDISTORT_ITERS, SAMPLE_DRAWS, HYP_STEPS, REFINE_ROUNDS, REFINE_STEPS = 10, 32, 8, 3, 5
MIN_VALID = 6
DAMPING = 1e-3
SMALL_ANGLE = 1e-5
_M32 = np.uint64(0xFFFFFFFF)


def mix32(x):
    """The 32-bit finaliser x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16 (mod 2^32)."""
    x = np.asarray(x, dtype=np.uint64) & _M32
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & _M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & _M32
    return x ^ (x >> np.uint64(16))


def draw(seed, h, d):
    """The d-th draw of hypothesis h: mix32(mix32(mix32(seed ^ 0x9e3779b9) + h) + d)."""
    a = mix32(np.uint64(int(seed) & 0xFFFFFFFF) ^ np.uint64(0x9E3779B9))
    b = mix32((a + np.asarray(h, dtype=np.uint64)) & _M32)
    return mix32((b + np.asarray(d, dtype=np.uint64)) & _M32)


def distort(x, y, dist):
    """The Brown model forward: normalised undistorted -> normalised distorted."""
    k1, k2, p1, p2, k3 = (float(c) for c in dist)
    r2 = x * x + y * y
    cd = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2
    return (x * cd + 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x), y * cd + p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y)


def undistort(u, v, K, dist, iters=UNDISTORT_ITERS):
    """Pixels -> normalised undistorted coordinates by ``iters`` fixed-point steps (float64)."""
    fx, fy, cx, cy = (float(c) for c in K)
    k1, k2, p1, p2, k3 = (float(c) for c in dist)
    x0, y0 = (np.asarray(u, np.float64) - cx) / fx, (np.asarray(v, np.float64) - cy) / fy
    x, y = x0, y0
    for _ in range(iters):
        r2 = x * x + y * y
        icd = 1.0 / (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2)
        dx = 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
        dy = p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
        x, y = (x0 - dx) * icd, (y0 - dy) * icd
    return x, y


def gather(depth, m1, m2, K, dist):
    """-> (valid (M,), P (M, 3) object points in the keyframe's camera frame, q (M, 2) normalised frame points)."""
    depth = np.asarray(depth, np.float32)
    H1, W1 = depth.shape
    m1 = np.asarray(m1, np.int32).reshape(-1, 2)
    m2 = np.asarray(m2, np.float32).reshape(-1, 2)
    x, y = m1[:, 0].astype(np.int64), m1[:, 1].astype(np.int64)
    inside = (x >= 0) & (x < W1) & (y >= 0) & (y < H1)
    Z = np.zeros(len(m1), np.float64)
    Z[inside] = depth[y[inside], x[inside]].astype(np.float64)
    with np.errstate(invalid="ignore"):
        valid = inside & np.isfinite(Z) & (Z > 0)
    Z = np.where(valid, Z, 0.0)
    xn, yn = undistort(x.astype(np.float64), y.astype(np.float64), K, dist)
    un, vn = undistort(m2[:, 0].astype(np.float64), m2[:, 1].astype(np.float64), K, dist)
    return valid, np.stack([xn * Z, yn * Z, Z], 1), np.stack([un, vn], 1)


def samples_of(seed, hypotheses, valid):
    """(hypotheses, 3) indices; a slot that finds no valid unused match in SAMPLE_DRAWS draws is -1 (and the ones behind it)."""
    M = len(valid)
    out = np.full((hypotheses, 3), -1, np.int64)
    if M == 0:
        return out
    d = np.arange(3 * SAMPLE_DRAWS, dtype=np.uint64)
    for h in range(hypotheses):
        idx = (draw(seed, h, d) % np.uint64(M)).astype(np.int64)
        for slot in range(3):
            for k in idx[slot * SAMPLE_DRAWS:(slot + 1) * SAMPLE_DRAWS]:
                if valid[k] and k not in out[h, :slot]:
                    out[h, slot] = k
                    break
            if out[h, slot] < 0:
                break
    return out


def _exp(tau):
    """(B, 6) twists [rho, theta] -> (E (B, 3, 3), V rho (B, 3)): pose_utils' SE3_exp."""
    rho, th = tau[:, :3], tau[:, 3:]
    a = np.sqrt((th * th).sum(1))
    small = a < SMALL_ANGLE
    a_ = np.where(small, 1.0, a)
    A = np.where(small, 1.0, np.sin(a_) / a_)
    Bc = np.where(small, 0.5, (1.0 - np.cos(a_)) / (a_ * a_))
    C = np.where(small, 1.0 / 6.0, (a_ - np.sin(a_)) / (a_ * a_ * a_))
    Kx = np.zeros((len(tau), 3, 3))
    Kx[:, 0, 1], Kx[:, 0, 2], Kx[:, 1, 0], Kx[:, 1, 2], Kx[:, 2, 0], Kx[:, 2, 1] = -th[:, 2], th[:, 1], th[:, 2], -th[:, 0], -th[:, 1], th[:, 0]
    K2 = Kx @ Kx
    eye = np.eye(3)[None]
    E = eye + A[:, None, None] * Kx + Bc[:, None, None] * K2
    V = eye + Bc[:, None, None] * Kx + C[:, None, None] * K2
    return E, np.einsum("bij,bj->bi", V, rho)


def _cholesky_solve(A, g):
    """Solve A d = -g for (B, 6, 6), (B, 6) by a Cholesky factorisation written out; ok false where a pivot is not > 0."""
    B = len(A)
    L = np.zeros_like(A)
    ok = np.ones(B, bool)
    with np.errstate(all="ignore"):
        for j in range(6):
            s = A[:, j, j].copy()
            for k in range(j):
                s = s - L[:, j, k] * L[:, j, k]
            ok &= s > 0          # (NaN: false)
            d = np.sqrt(np.where(s > 0, s, 1.0))
            L[:, j, j] = d
            for i in range(j + 1, 6):
                s = A[:, i, j].copy()
                for k in range(j):
                    s = s - L[:, i, k] * L[:, j, k]
                L[:, i, j] = s / d
        y = np.zeros_like(g)
        for i in range(6):
            s = -g[:, i]
            for k in range(i):
                s = s - L[:, i, k] * y[:, k]
            y[:, i] = s / L[:, i, i]
        x = np.zeros_like(g)
        for i in range(5, -1, -1):
            s = y[:, i].copy()
            for k in range(i + 1, 6):
                s = s - L[:, k, i] * x[:, k]
            x[:, i] = s / L[:, i, i]
    return x, ok


def transform(R, t, P):
    """(B, 3, 3), (B, 3), (B, n, 3) or (n, 3) -> (B, n, 3)."""
    if P.ndim == 2:
        P = P[None]
    return np.einsum("bij,bnj->bni", R, P) + t[:, None, :]


def gn_step(R, t, P, q, w, fx, fy):
    """One damped Gauss-Newton step of sum_i w_i |r_i|^2, r = (fx (X/Z - u), fy (Y/Z - v)), X = R P + t, under T <- Exp(tau) T.
    R (B, 3, 3), t (B, 3), P (B, n, 3), q (B, n, 2), w (B, n).  -> (R, t, ok)."""
    with np.errstate(all="ignore"):
        Xc = transform(R, t, P)
        X, Y, Z = Xc[..., 0], Xc[..., 1], Xc[..., 2]
        iz = 1.0 / Z
        rx, ry = fx * (X * iz - q[..., 0]), fy * (Y * iz - q[..., 1])
        a, c = fx * iz, -fx * X * iz * iz
        b, d = fy * iz, -fy * Y * iz * iz
        zero = np.zeros_like(a)
        Jx = np.stack([a, zero, c, c * Y, a * Z - c * X, -a * Y], -1)
        Jy = np.stack([zero, b, d, d * Y - b * Z, -d * X, b * X], -1)
        ww = w[..., None]
        A = ((Jx * ww)[..., :, None] * Jx[..., None, :]).sum(1) + ((Jy * ww)[..., :, None] * Jy[..., None, :]).sum(1)
        g = (Jx * (w * rx)[..., None]).sum(1) + (Jy * (w * ry)[..., None]).sum(1)
        idx = np.arange(6)
        A[:, idx, idx] = A[:, idx, idx] * (1.0 + DAMPING)
        tau, ok = _cholesky_solve(A, g)
        ok &= np.isfinite(tau).all(1)
        tau = np.where(ok[:, None], tau, 0.0)
        E, Vrho = _exp(tau)
        return E @ R, np.einsum("bij,bj->bi", E, t) + Vrho, ok


def errors(R, t, P, q, fx, fy):
    """Reprojection errors in pixels (B, n) and the depth sign test (B, n)."""
    with np.errstate(all="ignore"):
        Xc = transform(R, t, P)
        Z = Xc[..., 2]
        ex, ey = fx * (Xc[..., 0] / Z - q[None, :, 0]), fy * (Xc[..., 1] / Z - q[None, :, 1])
        return ex * ex + ey * ey, Z > 0


def _failed(out, reason):
    out.update(status=FAILED, reason=reason, pose=np.eye(4))
    return out


def solve(depth, m1, m2, K, dist=(0, 0, 0, 0, 0), hypotheses=128, reproj_error=5.0, seed=0, min_inliers=6, tie=1e-6, sum_order=None,
          chunk=32):
    fx, fy = float(K[0]), float(K[1])
    valid, P, q = gather(depth, m1, m2, K, dist)
    M = len(valid)
    thr, thr2 = float(reproj_error), float(reproj_error) * float(reproj_error)
    out = dict(status=FAILED, reason=FAIL_NONE, valid=int(valid.sum()), valid_mask=valid, pose=np.eye(4), inlier_mask=np.zeros(M, bool), inliers=0,
               hypothesis=-1, winner_count=0, counts=np.full(hypotheses, -1, np.int64), fragile_counts=np.zeros(hypotheses, np.int64),
               samples=np.full((hypotheses, 3), -1, np.int64), fragile_rounds=0, fragile_final=np.zeros(M, bool))
    if out["valid"] < MIN_VALID:
        return _failed(out, FAIL_FEW_VALID)
    S = samples_of(seed, hypotheses, valid)
    out["samples"] = S
    live = (S >= 0).all(1)
    R = np.tile(np.eye(3), (hypotheses, 1, 1))
    t = np.zeros((hypotheses, 3))
    Ps, qs = P[np.where(S >= 0, S, 0)], q[np.where(S >= 0, S, 0)]
    w3 = np.ones((hypotheses, 3))
    for _ in range(HYP_STEPS):
        R, t, ok = gn_step(R, t, Ps, qs, w3, fx, fy)
        live &= ok
    with np.errstate(invalid="ignore"):
        live &= (transform(R, t, Ps)[..., 2] > 0).all(1)
    counts = np.full(hypotheses, -1, np.int64)
    for h0 in range(0, hypotheses, chunk):
        sl = slice(h0, min(h0 + chunk, hypotheses))
        e2, front = errors(R[sl], t[sl], P, q, fx, fy)
        with np.errstate(invalid="ignore"):
            inl = valid[None] & front & (e2 < thr2)
            near = valid[None] & front & (np.abs(np.sqrt(e2) - thr) <= tie)
        counts[sl] = np.where(live[sl], inl.sum(1), -1)
        out["fragile_counts"][sl] = np.where(live[sl], near.sum(1), 0)
    out["counts"] = counts
    if not live.any():
        return _failed(out, FAIL_ALL_VOID)
    win = int(np.argmax(counts))          # the first of the maxima: ties go to the lowest h
    out["hypothesis"], out["winner_count"] = win, int(counts[win])
    if counts[win] < min_inliers:
        return _failed(out, FAIL_FEW_INLIERS)
    order = np.arange(M) if sum_order is None else np.asarray(sum_order)
    Po, qo, vo = P[order][None], q[order][None], valid[order]
    Rw, tw = R[win:win + 1], t[win:win + 1]
    for _ in range(REFINE_ROUNDS):
        e2, front = errors(Rw, tw, Po[0], qo[0], fx, fy)
        with np.errstate(invalid="ignore"):
            sel = vo & front[0] & (e2[0] < thr2)
            out["fragile_rounds"] += int((vo & front[0] & (np.abs(np.sqrt(e2[0]) - thr) <= tie)).sum())
        for _ in range(REFINE_STEPS):
            Rw, tw, ok = gn_step(Rw, tw, Po[:, sel], qo[:, sel], np.ones((1, int(sel.sum()))), fx, fy)
            if not ok[0]:
                return _failed(out, FAIL_SINGULAR)
    e2, front = errors(Rw, tw, P, q, fx, fy)
    with np.errstate(invalid="ignore"):
        out["inlier_mask"] = valid & front[0] & (e2[0] < thr2)
        out["fragile_final"] = valid & front[0] & (np.abs(np.sqrt(e2[0]) - thr) <= tie)
    out["inliers"] = int(out["inlier_mask"].sum())
    pose = np.eye(4)
    pose[:3, :3], pose[:3, 3] = Rw[0], tw[0]
    out.update(status=OK, pose=pose)
    return out


def pose_error(pose, R_true, t_true):
    """(rotation error in degrees, translation error) of a 4 x 4 pose against (R, t)."""
    dR = pose[:3, :3] @ np.asarray(R_true).T
    ang = np.degrees(np.arccos(np.clip((np.trace(dR) - 1.0) / 2.0, -1.0, 1.0)))
    return float(ang), float(np.linalg.norm(pose[:3, 3] - np.asarray(t_true)))
