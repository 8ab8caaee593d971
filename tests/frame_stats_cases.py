"""Seeded inputs shared by tests/test_frame_stats.py (CPU) and tests/test_gpu_frame_stats.py (GPU)."""
import numpy as np

f32 = np.float32

EDGE_THRESHOLD = 1.1     # tests/golden/config_07.json Training.edge_threshold
MEDIAN_SIZES = ((23, 37), (64, 64), (370, 1226))          # (H, W)
BLOCK_SIZES = ((70, 45), (45, 70), (96, 64))              # 70 x 45: bh = 2, bw = 1 and 45 x 70: bh = 1, bw = 2, rows and columns left outside the grid
SELECT_SIZES = (0, 1, 2, 3, 255, 256, 257, 65537 + 1000)
SELECT_PATTERNS = ("random", "equal", "low_byte", "duplicates", "increasing")
OPACITY_KINDS = ("all", "none", "third")
COVIS_SIZES = (0, 1, 63, 64, 65, 1000)
COVIS_ROWS = (0, 1, 3, 16)


def image(H, W, seed=0, gain=1.0):
    """(3, H, W) float32: a smooth pattern plus noise of sigma 0.02, the top-left corner black (the validity mask is false there)."""
    rng = np.random.default_rng(1000 * H + W + seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    chans = [0.5 + 0.3 * np.sin(x / 7.0 + c) * np.cos(y / 5.0 - c) + 0.1 * np.sin((x + 2 * y) / 23.0) for c in range(3)]
    img = np.stack(chans) + rng.normal(0.0, 0.02, (3, H, W))
    img[:, :H // 3, :W // 4] = 0.0
    return (img * gain).astype(f32)


def depths(pattern, n, seed=0):
    """n float32 depths.  Every pattern but "equal" carries a few non-positive entries, which the selection must pass over."""
    rng = np.random.default_rng(7 * n + seed)
    if pattern == "random":
        d = rng.uniform(0.5, 30.0, n).astype(f32)
    elif pattern == "equal":
        return np.full(n, 7.25, f32)
    elif pattern == "low_byte":      # one value but for the lowest byte of its bit pattern
        bits = np.full(n, np.array([7.25], f32).view(np.uint32)[0], np.uint32) | rng.integers(0, 256, n).astype(np.uint32)
        d = bits.view(f32).copy()
    elif pattern == "duplicates":    # half of the entries are exact copies of one value in the middle of the range
        d = rng.uniform(0.5, 19.5, n).astype(f32)
        d[rng.permutation(n)[:n // 2]] = f32(10.0)
    elif pattern == "increasing":
        d = (f32(1.0) + np.arange(n, dtype=f32) * f32(0.001)).astype(f32)
    else:
        raise ValueError(pattern)
    d[5::11] = 0.0
    d[7::97] = -1.0
    return d


def opacities(kind, n):
    """"all": every pixel opaque; "none": none; "third": every third, the others exactly float32(0.95) (not above the bar) or 0.9."""
    if kind == "all":
        return np.ones(n, f32)
    if kind == "none":
        return np.full(n, 0.5, f32)
    o = np.full(n, 0.9, f32)
    o[0::3] = 1.0
    o[1::3] = f32(0.95)
    return o


def visibility(kind, n, seed=0):
    rng = np.random.default_rng(31 * n + seed)
    if kind == "false":
        return np.zeros(n, bool)
    if kind == "true":
        return np.ones(n, bool)
    return rng.random(n) < 0.4
