"""Inputs shared by tests/test_seeding.py and tests/test_gpu_seeding.py."""
import numpy as np

# 23x37: 851 pixels, not a multiple of a wave; 96x70: several selection workgroups, so the last-workgroup ticket decides; 1100x960:
# 1 056 000 pixels, above one select pass' span of SEL_MAX_BLOCKS * SEL_THREADS * SEL_ITEMS_PER_THREAD = 1 048 576, so its grid-stride
# loop runs (the count and write passes give every workgroup one contiguous span and have no such bound)
SIZES = [(23, 37), (96, 70), (1100, 960)]      # (W, H)
SPECIALS = [100.0, float(np.nextafter(np.float32(100.0), np.float32(np.inf))), float("nan"), float("inf"), -1.0, 0.0]
INTRINSICS = (707.0912, 705.5, 601.8873, 183.1104)      # fx, fy, cx, cy
GAIN, OFFSET = 1.0832871, -0.0234       # exp(0.08)'s float32 neighbourhood, and a b


def depth_map(W, H, valid_share=0.6, seed=0, specials=True):
    """(H, W) float32: about ``valid_share`` of the pixels in (0, 100], the rest zeros, negatives and values beyond the truncation;
    with ``specials`` the six SPECIALS at fixed places (exactly 100 is valid, its successor is not)."""
    rng = np.random.default_rng(seed)
    d = (0.5 + 60.0 * rng.random((H, W))).astype(np.float32)
    kind = rng.random((H, W))
    d[kind > valid_share] = 0.0
    d[kind > valid_share + 0.15] = 150.0
    d[kind > valid_share + 0.3] = -2.0
    if specials:
        flat = d.reshape(-1)
        at = rng.choice(flat.size, size=len(SPECIALS), replace=False)
        flat[at] = np.asarray(SPECIALS, np.float32)
    return d


def marked_depth_map(W, H, seed=5):
    """(H, W) float32 as a mono depth carries it: -1 markers on three pixels in ten, other negatives on a quarter (so the lower median
    of ALL values, what depth.median() is, is a negative value that is no marker), both zeros, a few +inf, the rest in (0, 100].  No NaN."""
    rng = np.random.default_rng(seed)
    d = (0.5 + 60.0 * rng.random((H, W))).astype(np.float32)
    kind = rng.random((H, W))
    d[kind < 0.55] = (-0.1 - 5.0 * rng.random((H, W))).astype(np.float32)[kind < 0.55]
    d[kind < 0.30] = -1.0
    d[kind > 0.97] = np.inf
    flat = d.reshape(-1)
    flat[::97] = 0.0
    flat[5::97] = -0.0
    return d


def image(W, H, seed=1):
    """(3, H, W) float32 with values below 0, exactly 0 and 1, and above 1."""
    rng = np.random.default_rng(seed)
    x = (-0.2 + 1.4 * rng.random((3, H, W))).astype(np.float32)
    flat = x.reshape(-1)
    flat[::7] = 0.0
    flat[3::11] = 1.0
    return x


def pose(seed=2):
    """A rotation (3, 3) float32 that is no axis permutation, and a translation."""
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q.astype(np.float32), np.asarray([0.31, -0.12, 0.77], np.float32)
