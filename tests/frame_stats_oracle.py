"""NumPy float32 restatement of what include/lvdgs.h fixes for lvdgs_edge_mask and lvdgs_frame_summary: every expression in the
header's order, the lower median by a sort, the summary's counts by NumPy's own.  Test infrastructure (tests/test_frame_stats.py on
the CPU, tests/test_gpu_frame_stats.py against the kernels); the product never imports it."""
import numpy as np

f32 = np.float32
GRID = 32


def lower_median(x):
    """torch.median of a flat array: the (n - 1) // 2-th smallest; NaN for n == 0.  float32 in, float32 out."""
    x = np.asarray(x, dtype=f32).ravel()
    if x.size == 0:
        return f32(np.nan)
    return np.sort(x)[(x.size - 1) // 2]


def magnitude(image):
    """(3, H, W) float32 -> (H, W) float32 edge magnitude."""
    image = np.asarray(image, dtype=f32)
    r, g, b = image
    gray = ((r + g) + b) / f32(3)
    H, W = gray.shape
    p = np.pad(gray, 1, mode="reflect")
    t = [[p[i:i + H, j:j + W] for j in range(3)] for i in range(3)]
    scale = f32(1.0) / f32(32.0)
    gv = (((((t[0][0] * f32(3) + t[0][1] * f32(10)) + t[0][2] * f32(3)) + t[2][0] * f32(-3)) + t[2][1] * f32(-10)) + t[2][2] * f32(-3)) * scale
    gh = (((((t[0][0] * f32(3) + t[0][2] * f32(-3)) + t[1][0] * f32(10)) + t[1][2] * f32(-10)) + t[2][0] * f32(3)) + t[2][2] * f32(-3)) * scale
    full = np.ones((H, W), dtype=bool)
    for i in range(3):
        for j in range(3):
            full &= np.abs(t[i][j]) > f32(0.01)
    m = full.astype(f32)
    gv, gh = gv * m, gh * m
    mag = np.sqrt(gv * gv + gh * gh)
    assert mag.dtype == f32
    return mag


def edge_mask_median(image, edge_threshold):
    """-> dict(mag, median, cut, mask (H, W) bool)."""
    mag = magnitude(image)
    median = lower_median(mag)
    cut = median * f32(edge_threshold)
    return dict(mag=mag, median=median, cut=f32(cut), mask=mag > cut)


def edge_mask_blocks(image, edge_threshold):
    """The replica rule -> dict(mag, medians (32, 32), cuts (32, 32), mask (H, W) float32)."""
    mag = magnitude(image)
    H, W = mag.shape
    bh, bw = int(H / GRID), int(W / GRID)
    out = mag.copy()
    medians, cuts = np.zeros((GRID, GRID), f32), np.zeros((GRID, GRID), f32)
    for i in range(GRID):
        for j in range(GRID):
            blk = mag[i * bh:(i + 1) * bh, j * bw:(j + 1) * bw]
            medians[i, j] = lower_median(blk)
            cut = cuts[i, j] = medians[i, j] * f32(edge_threshold)
            v = np.where(blk > cut, f32(1), blk)       # 1 above the cut ...
            v = np.where(v <= cut, f32(0), v)          # ... then 0 at or below it
            out[i * bh:(i + 1) * bh, j * bw:(j + 1) * bw] = v
    return dict(mag=mag, medians=medians, cuts=cuts, mask=out)


def summary(depth, opacity, n_touched, rows, mask=None, count_mask=None, opacity_bar=0.95):
    """-> dict(median (float32), selected, visible, rows [(intersection, union, own)], mask_count)."""
    depth = np.asarray(depth, dtype=f32).ravel()
    valid = depth > 0
    if opacity is not None:
        valid &= np.asarray(opacity, dtype=f32).ravel() > f32(opacity_bar)
    if mask is not None:
        valid &= np.asarray(mask).ravel() != 0
    cur = np.asarray(n_touched).ravel() > 0
    counts = []
    for row in rows:
        b = np.asarray(row).ravel() != 0
        counts.append((int((cur & b).sum()), int((cur | b).sum()), int(b.sum())))
    return dict(median=lower_median(depth[valid]), selected=int(valid.sum()), visible=int(cur.sum()), rows=counts,
                mask_count=0 if count_mask is None else int((np.asarray(count_mask).ravel() != 0).sum()))
