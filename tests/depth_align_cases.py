"""Inputs of the depth-alignment tests, regenerated from seeds (tests/golden/depth_align.npz stores only their SHA-256 and what the
reference computed on them).

A case is a rendered depth r (a road-like depth field: far at the top rows, near at the bottom, with structure across) and a mono
depth m = r / true_scale with multiplicative noise and a few blobs where the two disagree (objects the map does not hold yet).
``remedy`` is the list of scales a deterministic stand-in for ``find_scale`` returns, call after call."""
import hashlib

import numpy as np


def depth_pair(H, W, seed, true_scale, noise=0.03, blobs=6, zeros_r=0.0, nan_m=0.0):
    rng = np.random.default_rng(seed)
    y = np.linspace(0.0, 1.0, H)[:, None]
    x = np.linspace(0.0, 1.0, W)[None, :]
    r = 6.0 + 40.0 * (1.0 - y) ** 2 + 4.0 * np.sin(9.0 * x + 3.0 * y) + 2.0 * np.cos(23.0 * x * (1.0 + y))
    r = r * (1.0 + 0.01 * rng.standard_normal((H, W)))
    m = r / true_scale * (1.0 + noise * rng.standard_normal((H, W)))
    for _ in range(blobs):
        cy, cx = rng.integers(0, H), rng.integers(0, W)
        ry, rx = rng.integers(H // 20 + 1, H // 6 + 2), rng.integers(W // 20 + 1, W // 6 + 2)
        m[max(cy - ry, 0):cy + ry, max(cx - rx, 0):cx + rx] *= rng.uniform(0.4, 0.7)
    r, m = r.astype(np.float32), m.astype(np.float32)
    if zeros_r:
        r[rng.random((H, W)) < zeros_r] = 0.0
        r[: max(H // 8, 1), : max(W // 5, 1)] = 0.0     # a hole in the render: a whole region the map does not cover
    if nan_m:
        m[rng.random((H, W)) < nan_m] = np.nan
    return r, m


# name -> (H, W, seed, true_scale, pair keywords, process_depth keywords, remedy scales)
CASES = {
    "kitti_clipped_edges": (370, 1226, 1, 1.15, {}, dict(patch_size=10), []),
    "odd_size_patch16": (203, 317, 2, 0.9, {}, dict(patch_size=16), []),
    "zeros_in_render": (120, 250, 3, 1.1, dict(zeros_r=0.05), dict(patch_size=10), []),
    "nans_in_mono": (130, 210, 4, 1.1, dict(nan_m=0.002), dict(patch_size=8), []),
    "converges_at_k1": (150, 260, 5, 1.004, {}, dict(patch_size=10), []),
    "remedy_at_k2": (160, 300, 6, 2.5, {}, dict(patch_size=10), [2.47]),
    "remedy_at_k3": (140, 280, 7, 2.5, {}, dict(patch_size=12), [0.55, 2.44]),
    "no_accurate_pixel": (96, 170, 8, 1.0, dict(noise=0.0, blobs=0), dict(patch_size=10, min_accurate_pixels_ratio=0.0), []),
}


def make_case(name):
    """-> (r, m, process_depth keywords, remedy scales)."""
    H, W, seed, scale, pair_kw, kw, remedy = CASES[name]
    r, m = depth_pair(H, W, seed, scale, **pair_kw)
    if name == "no_accurate_pixel":
        m = np.full_like(r, 10.0)          # flat mono depth: every patch's spread disagrees (std 0 vs std r)
    return r, m, dict(kw), list(remedy)


def sha256(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


class RecordedRemedy:
    """A deterministic stand-in for ``find_scale``: returns the recorded scales in turn and counts its calls."""

    def __init__(self, scales):
        self.scales, self.calls = list(scales), 0

    def __call__(self, *args):
        s = self.scales[min(self.calls, len(self.scales) - 1)] if self.scales else 1.0
        self.calls += 1
        return np.float32(s)


def random_case(seed):
    """A seeded case for the GPU sweep: sizes that are not multiples of the patch, patch 4..32, both remedy branches."""
    rng = np.random.default_rng(10_000 + seed)
    p = int(rng.integers(4, 33))
    H = int(rng.integers(2, 9)) * p + int(rng.integers(1, p)) if p > 1 else int(rng.integers(8, 64))
    W = int(rng.integers(3, 14)) * p + int(rng.integers(1, p))
    kind = seed % 4     # 0: converging, 1: remedy at k = 2, 2: remedy at k = 3, 3: zeros / NaNs
    scale = {0: rng.uniform(0.9, 1.12), 1: 2.5, 2: 2.5, 3: rng.uniform(0.92, 1.1)}[kind]
    r, m = depth_pair(H, W, 20_000 + seed, scale, noise=float(rng.uniform(0.005, 0.05)), blobs=int(rng.integers(0, 5)),
                      zeros_r=0.02 if kind == 3 else 0.0, nan_m=0.003 if kind == 3 else 0.0)
    remedy = {1: [scale * rng.uniform(0.98, 1.02)], 2: [0.5, scale * rng.uniform(0.98, 1.02)]}.get(kind, [])
    kw = dict(patch_size=p, mean_threshold=float(rng.uniform(0.2, 0.3)), std_threshold=float(rng.uniform(0.25, 0.35)),
              error_threshold=float(rng.uniform(0.08, 0.15)), final_error_threshold=float(rng.uniform(0.1, 0.2)),
              min_accurate_pixels_ratio=float(rng.choice([0.01, 0.02, 0.05])))
    return r, m, kw, remedy
