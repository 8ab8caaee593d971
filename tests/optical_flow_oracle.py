"""The specification of ``lvdgs_farneback_flow`` / ``lvdgs_motion_mask`` (include/lvdgs.h) as NumPy statements,
one per sentence of the header's text: the reference the device code and ``lvdgs.optical_flow.farneback_torch`` are compared with.

``dtype`` is the type every image-sized array and every tap has (float64: the reference; float32: the same text in the device's
precision -- the distance between the two is what the GPU tests derive their tolerance from).  Whatever the header computes "on the
host in double" -- the pyramid's sizes, the resize coordinates, the Gaussian taps before their rounding, the moment matrix and its
inverse -- is float64 here for either ``dtype``.  Sums run over their taps in ascending order, one product added at a time.
"""
import numpy as np

DEFAULTS = dict(pyr_scale=0.5, levels=3, winsize=15, iterations=3, poly_n=5, poly_sigma=1.2)     # the reference's call (flags=0)
BORDER = (0.14, 0.14, 0.4472, 0.4472, 0.4472)
MIN_SIZE = 32


def grey_of(image):
    """(3, H, W) float32 in [0, 1] -> (H, W) uint8: the quantisation ``(img * 255).astype(np.uint8)`` and the integer grey."""
    q = np.clip(np.asarray(image, np.float32) * np.float32(255.0), np.float32(0), np.float32(255)).astype(np.uint8).astype(np.int32)
    return ((4899 * q[0] + 9617 * q[1] + 1868 * q[2] + 8192) >> 14).astype(np.uint8)


def pyramid(W, H, pyr_scale, levels):
    """The levels, coarsest first: dicts of k, scale (a product of k factors), w, h, sigma, ksize."""
    k, s = 0, 1.0
    while k < levels:
        s *= pyr_scale
        if W * s < MIN_SIZE or H * s < MIN_SIZE:
            break
        k += 1
    out = []
    for level in range(k, -1, -1):
        scale = 1.0
        for _ in range(level):
            scale *= pyr_scale
        sigma = (1.0 / scale - 1.0) / 2.0
        ksize = max(int(np.rint(5.0 * sigma)) | 1, 3)
        out.append(dict(k=level, scale=scale, w=int(np.rint(W * scale)), h=int(np.rint(H * scale)), sigma=sigma, ksize=ksize))
    return out


def blur_taps(sigma, ksize):
    if sigma == 0:
        return np.array([0.25, 0.5, 0.25])
    x = np.arange(ksize, dtype=np.float64) - ksize // 2
    w = np.exp(-x * x / (2.0 * sigma * sigma))
    return w / w.sum()


def reflect101(i, n):
    if n == 1:
        return np.zeros_like(i)
    p = 2 * (n - 1)
    i = np.mod(i, p)
    return np.where(i >= n, p - i, i)


def replicate(i, n):
    return np.clip(i, 0, n - 1)


def correlate(img, taps, axis, border, dt):
    """sum_j taps[j] * img[.. border(i + j - r) ..] along ``axis``, j ascending."""
    n, r = img.shape[axis], len(taps) // 2
    acc = np.zeros(img.shape, dt)
    for j, t in enumerate(taps):
        acc = acc + dt(t) * np.take(img, border(np.arange(n) + j - r, n), axis=axis)
    return acc


def axis_taps(n_in, n_out, dt):
    s = (np.arange(n_out, dtype=np.float64) + 0.5) * (float(n_in) / float(n_out)) - 0.5
    i0 = np.floor(s)
    f = (s - i0).astype(dt)
    i0 = i0.astype(np.int64)
    return np.clip(i0, 0, n_in - 1), np.clip(i0 + 1, 0, n_in - 1), f


def resize(img, w, h, dt):
    """(H, W) -> (h, w), bilinear, source coordinate (i + 0.5) * n_in / n_out - 0.5, indices clamped."""
    y0, y1, fy = axis_taps(img.shape[0], h, dt)
    x0, x1, fx = axis_taps(img.shape[1], w, dt)
    fy, fx, one = fy[:, None], fx[None, :], dt(1)
    a, b, c, d = img[y0][:, x0], img[y0][:, x1], img[y1][:, x0], img[y1][:, x1]
    return (a * (one - fx) + b * fx) * (one - fy) + (c * (one - fx) + d * fx) * fy


def level_image(grey, lv, dt):
    img = grey.astype(dt)
    taps = blur_taps(lv["sigma"], lv["ksize"])
    img = correlate(correlate(img, taps, 1, reflect101, dt), taps, 0, reflect101, dt)
    return resize(img, lv["w"], lv["h"], dt)


def poly_taps(n, sigma):
    """g, xg, xxg (float64, taps -n .. n) and ig11, ig03, ig33, ig55."""
    x = np.arange(-n, n + 1, dtype=np.float64)
    g = np.exp(-x * x / (2.0 * sigma * sigma)).astype(np.float32).astype(np.float64)
    g = g / g.sum()
    gg = g[:, None] * g[None, :]
    X, Y = x[None, :], x[:, None]
    G = np.zeros((6, 6))
    G[0, 0] = gg.sum()
    G[1, 1] = (gg * X * X).sum()
    G[3, 3] = (gg * X ** 4).sum()
    G[5, 5] = (gg * X * X * Y * Y).sum()
    G[2, 2] = G[0, 3] = G[0, 4] = G[3, 0] = G[4, 0] = G[1, 1]
    G[4, 4] = G[3, 3]
    G[3, 4] = G[4, 3] = G[5, 5]
    inv = np.linalg.inv(G)
    return g, x * g, x * x * g, (inv[1, 1], inv[0, 3], inv[3, 3], inv[5, 5])


def poly_exp(img, n, sigma, dt):
    """(h, w) -> (h, w, 5): the local polynomial's coefficients in the order (y, x, yy, xx, xy)."""
    g, xg, xxg, (ig11, ig03, ig33, ig55) = poly_taps(n, sigma)
    ig11, ig03, ig33, ig55 = dt(ig11), dt(ig03), dt(ig33), dt(ig55)
    v0, v1, v2 = (correlate(img, t, 0, replicate, dt) for t in (g, xg, xxg))
    b1, b2, b4 = (correlate(v0, t, 1, replicate, dt) for t in (g, xg, xxg))
    b3, b5 = correlate(v1, g, 1, replicate, dt), correlate(v1, xg, 1, replicate, dt)
    b6 = correlate(v2, g, 1, replicate, dt)
    return np.stack([b3 * ig11, b2 * ig11, b1 * ig03 + b6 * ig33, b1 * ig03 + b4 * ig33, b5 * ig55], axis=2)


def border_weight(n, dt):
    """The product of the two border weights of every coordinate 0 .. n-1 (both apply when n < 10)."""
    c = np.arange(n)
    wb = np.array(BORDER + (1.0,), dt)
    return wb[np.minimum(c, 5)] * wb[np.minimum(n - 1 - c, 5)]


def matrices(R0, R1, flow, dt):
    h, w = flow.shape[:2]
    x, y = np.arange(w, dtype=dt)[None, :], np.arange(h, dtype=dt)[:, None]
    dx, dy = flow[..., 0], flow[..., 1]
    fx, fy = x + dx, y + dy
    x1f, y1f = np.floor(fx), np.floor(fy)
    inside = (x1f >= 0) & (x1f < w - 1) & (y1f >= 0) & (y1f < h - 1)
    x1, y1 = np.where(inside, x1f, 0).astype(np.int64), np.where(inside, y1f, 0).astype(np.int64)
    x2, y2 = np.minimum(x1 + 1, w - 1), np.minimum(y1 + 1, h - 1)
    fx, fy, one = (fx - x1f)[..., None], (fy - y1f)[..., None], dt(1)
    a00, a01, a10, a11 = (one - fx) * (one - fy), fx * (one - fy), (one - fx) * fy, fx * fy
    r = a00 * R1[y1, x1] + a01 * R1[y1, x2] + a10 * R1[y2, x1] + a11 * R1[y2, x2]
    half, quarter = dt(0.5), dt(0.25)
    r4, r5, r6 = (R0[..., 2] + r[..., 2]) * half, (R0[..., 3] + r[..., 3]) * half, (R0[..., 4] + r[..., 4]) * quarter
    r2 = (R0[..., 0] - r[..., 0]) * half + (r4 * dy + r6 * dx)
    r3 = (R0[..., 1] - r[..., 1]) * half + (r6 * dy + r5 * dx)
    zero = np.zeros((h, w), dt)
    r2, r3 = np.where(inside, r2, zero), np.where(inside, r3, zero)
    r4, r5, r6 = np.where(inside, r4, R0[..., 2]), np.where(inside, r5, R0[..., 3]), np.where(inside, r6, R0[..., 4] * half)
    s = border_weight(w, dt)[None, :] * border_weight(h, dt)[:, None]
    r2, r3, r4, r5, r6 = r2 * s, r3 * s, r4 * s, r5 * s, r6 * s
    return np.stack([r4 * r4 + r6 * r6, (r4 + r5) * r6, r5 * r5 + r6 * r6, r4 * r2 + r6 * r3, r6 * r2 + r5 * r3], axis=2)


def update(M, winsize, dt):
    ones = np.ones(winsize)
    S = np.stack([correlate(correlate(M[..., c], ones, 1, replicate, dt), ones, 0, replicate, dt) for c in range(5)], axis=2)
    S = S * dt(1.0 / (winsize * winsize))
    g11, g12, g22, h1, h2 = (S[..., c] for c in range(5))
    idet = dt(1) / (g11 * g22 - g12 * g12 + dt(1e-3))
    return np.stack([(g11 * h2 - g12 * h1) * idet, (g22 * h1 - g12 * h2) * idet], axis=2)


def farneback(prev_grey, next_grey, dtype=np.float64, return_levels=False, **params):
    """(H, W) uint8 twice -> flow (H, W, 2) of ``dtype``: [..., 0] along x, [..., 1] along y."""
    p = dict(DEFAULTS, **params)
    dt = np.dtype(dtype).type
    prev_grey, next_grey = np.asarray(prev_grey, np.uint8), np.asarray(next_grey, np.uint8)
    H, W = prev_grey.shape
    levels = pyramid(W, H, p["pyr_scale"], p["levels"])
    flow = None
    for lv in levels:
        I0, I1 = level_image(prev_grey, lv, dt), level_image(next_grey, lv, dt)
        if flow is None:
            flow = np.zeros((lv["h"], lv["w"], 2), dt)
        else:
            flow = np.stack([resize(flow[..., c], lv["w"], lv["h"], dt) for c in range(2)], axis=2) * dt(1.0 / p["pyr_scale"])
        R0, R1 = poly_exp(I0, p["poly_n"], p["poly_sigma"], dt), poly_exp(I1, p["poly_n"], p["poly_sigma"], dt)
        M = matrices(R0, R1, flow, dt)
        for i in range(p["iterations"]):
            flow = update(M, p["winsize"], dt)
            if i < p["iterations"] - 1:
                M = matrices(R0, R1, flow, dt)
    return (flow, len(levels)) if return_levels else flow


def dilate(mask, k):
    """A pixel is set when any pixel of its centred k x k window that lies inside the image is set."""
    h, w = mask.shape
    r = k // 2
    padded = np.zeros((h + 2 * r, w + 2 * r), bool)
    padded[r:r + h, r:r + w] = mask != 0
    out = np.zeros((h, w), bool)
    for dy in range(k):
        for dx in range(k):
            out |= padded[dy:dy + h, dx:dx + w]
    return out


def motion_mask(prev_grey, next_grey, motion_threshold=3.0, dilate_kernel=7, dtype=np.float64, **params):
    """-> (mask before the dilation, mask after it, magnitude, flow)."""
    flow = farneback(prev_grey, next_grey, dtype, **params)
    magnitude = np.sqrt(flow[..., 0] * flow[..., 0] + flow[..., 1] * flow[..., 1])
    moving = magnitude > np.float32(motion_threshold)
    return moving, dilate(moving, dilate_kernel), magnitude, flow
