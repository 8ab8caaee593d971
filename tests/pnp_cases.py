"""Seeded inputs of the pose initialisation (``lvdgs_pnp_ransac``; tests/pnp_oracle.py states its semantics): a keyframe that looks
along a ground plane at a far wall on a 512 x 160 raster, a stride-8 grid of its pixels carried into a second frame by a known
motion, with 2 % depth noise, 0.7 px match noise and a seeded share of matches replaced by uniformly random pixels.

``make_case(name)`` -> dict(depth, m1, m2, K, dist, R, t, kw): the solver's inputs, the true keyframe -> frame motion and the
solver's keyword arguments.  ``CASES`` lists the names; ``RECOVERY`` those whose pose the solver must recover, ``FAILURES`` those it
must refuse."""
import numpy as np

import pnp_oracle as orc

W1, H1 = 512, 160
K = (295.3, 295.3, 251.4, 76.5)           # KITTI-07's intrinsics at the matcher's raster (x 512 / 1226, rounded)
# the front camera of waymo segment 152706 (its published calibration: k1 k2 p1 p2 k3 at fx = fy = 2071.39, 1920 x 1280)
WAYMO_DIST = (0.05036108992329593, -0.3486531774617277, 0.0016151730124412522, -0.000933743404202468, 0.0)
WAYMO_K = (2071.3932896281076 * 512 / 1920, 2071.3932896281076 * 336 / 1280, 952.3805527835524 * 512 / 1920, 653.8669872813746 * 336 / 1280)
CAMERA_HEIGHT, WALL = 1.6, 40.0
SEEDS = range(10)
ANGLES = (1, 5, 10, 20)


def rotation(axis, angle):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * (Kx @ Kx)


def scene_depth(W, H, Kc, dist=(0, 0, 0, 0, 0)):
    """True depth per pixel: the ground plane y = CAMERA_HEIGHT (y points down) in front of a wall at z = WALL."""
    u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    xn, yn = orc.undistort(u, v, Kc, dist)
    with np.errstate(divide="ignore"):
        ground = np.where(yn > 1e-9, CAMERA_HEIGHT / np.where(yn > 1e-9, yn, 1.0), np.inf)
    return np.minimum(ground, WALL), xn, yn


def synth(seed, angle_deg, trans, outliers, W=W1, H=H1, Kc=K, dist=(0, 0, 0, 0, 0), stride=8, depth_noise=0.02, px_noise=0.7, holes=0.0,
          count=None):
    """``count``: that many matches at random keyframe pixels instead of the stride grid."""
    rng = np.random.default_rng(1000 * int(angle_deg) + seed)
    Z, xn, yn = scene_depth(W, H, Kc, dist)
    if count is None:
        gy, gx = np.meshgrid(np.arange(stride // 2, H, stride), np.arange(stride // 2, W, stride), indexing="ij")
        gx, gy = gx.ravel(), gy.ravel()
    else:
        gx, gy = rng.integers(0, W, count), rng.integers(0, H, count)
    axis = rng.normal(size=3)
    R = rotation(axis, np.radians(angle_deg))
    tdir = rng.normal(size=3)
    t = trans * rng.uniform(0.3, 1.0) * tdir / np.linalg.norm(tdir)
    Pw = np.stack([xn[gy, gx] * Z[gy, gx], yn[gy, gx] * Z[gy, gx], Z[gy, gx]], 1)
    Xc = Pw @ R.T + t
    with np.errstate(all="ignore"):
        xd, yd = orc.distort(Xc[:, 0] / Xc[:, 2], Xc[:, 1] / Xc[:, 2], dist)
    u2, v2 = Kc[0] * xd + Kc[2], Kc[1] * yd + Kc[3]
    u2, v2 = u2 + px_noise * rng.normal(size=len(u2)), v2 + px_noise * rng.normal(size=len(u2))
    keep = (Xc[:, 2] > 0.1) & (u2 >= 0) & (u2 <= W - 1) & (v2 >= 0) & (v2 <= H - 1)
    gx, gy, u2, v2 = gx[keep], gy[keep], u2[keep], v2[keep]
    M = len(gx)
    bad = rng.random(M) < outliers
    u2 = np.where(bad, rng.uniform(0, W - 1, M), u2)
    v2 = np.where(bad, rng.uniform(0, H - 1, M), v2)
    depth = (Z * (1.0 + depth_noise * rng.normal(size=Z.shape))).astype(np.float32)
    if holes:
        depth[rng.random(Z.shape) < holes] = 0.0
    return dict(depth=depth, m1=np.stack([gx, gy], 1).astype(np.int32), m2=np.stack([u2, v2], 1).astype(np.float32), K=tuple(Kc), dist=tuple(dist),
                R=R, t=t, kw=dict(hypotheses=128, reproj_error=5.0, seed=seed, min_inliers=6), outlier=bad)


def motion_case(angle, seed):
    rng = np.random.default_rng(77 + 13 * angle + seed)
    return synth(seed, angle, 1.5, rng.uniform(0.3, 0.5))


def _five_valid():
    c = synth(3, 5, 1.0, 0.0)
    keep = np.zeros(c["depth"].shape, bool)
    m1 = c["m1"]
    keep[m1[:5, 1], m1[:5, 0]] = True
    c["depth"] = np.where(keep, c["depth"], 0.0).astype(np.float32)
    c["m1"], c["m2"] = m1[:40].copy(), c["m2"][:40].copy()
    return c


def _all_outliers():
    return synth(4, 5, 1.0, 1.0, stride=32)      # (80 matches: by chance six of a thousand random ones would agree within 5 px)


CASES = {f"rot{a}_seed{s}": (lambda a=a, s=s: motion_case(a, s)) for a in ANGLES for s in SEEDS}
RECOVERY = sorted(CASES)
CASES.update(
    waymo_distortion=lambda: synth(1, 5, 1.0, 0.4, W=512, H=336, Kc=WAYMO_K, dist=WAYMO_DIST),
    zero_depth_holes=lambda: synth(2, 5, 1.0, 0.4, holes=0.3),
    many_matches=lambda: synth(5, 5, 1.0, 0.4, count=20_000),
    five_valid=_five_valid,
    all_outliers=_all_outliers,
)
RECOVERY += ["waymo_distortion", "zero_depth_holes", "many_matches"]
FAILURES = ["five_valid", "all_outliers"]
# the cases the GPU suite runs against the oracle (two seeds per angle keep its time down; the CPU suite runs them all)
GPU_CASES = [f"rot{a}_seed{s}" for a in ANGLES for s in (0, 1)] + ["waymo_distortion", "zero_depth_holes", "many_matches"] + FAILURES


def make_case(name):
    return CASES[name]()
