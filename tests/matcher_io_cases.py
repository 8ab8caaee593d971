"""Inputs of the matcher-I/O tests (image formatting, match depth scale), regenerated from seeds.  tests/golden/image_format.npz stores
only what PIL gave on the formatting inputs."""
import numpy as np

# name -> (W, H, size, the raster (W1, H1) it has to give)
FORMAT_CASES = {
    "lanczos_ratio_4p7": (300, 90, 64, (64, 16)),         # windows clipped at both borders
    "lanczos_ratio_1p2": (613, 185, 512, (512, 144)),     # the half-size KITTI frame
    "bicubic_upsizing": (97, 61, 128, (128, 80)),
    "square_rule": (50, 50, 64, (64, 48)),
    "both_passes_skipped": (512, 160, 512, (512, 160)),
    "one_pixel_of_growth": (511, 300, 512, (512, 288)),
    "odd_crop_offset": (200, 75, 90, (80, 32)),           # resized to 90 x 34: the crop starts at column 5, row 1
}
KINDS = ("noise", "smooth")


def image(name, kind):
    """(3, H, W) float32 in [0, 1]; the noise image carries a few values outside it and a NaN (the quantiser's clamps)."""
    W, H, _, _ = FORMAT_CASES[name]
    rng = np.random.default_rng(sorted(FORMAT_CASES).index(name) * 2 + KINDS.index(kind) + 500)
    if kind == "noise":
        img = rng.random((3, H, W)).astype(np.float32)
        img[0, 0, 0], img[1, H // 2, W // 3], img[2, H - 1, W - 1], img[0, H // 3, W // 2] = -0.3, 1.7, np.nan, 300.0
        return img
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    ph = rng.uniform(0, 6.28, size=(3, 3))
    chans = [0.5 + 0.25 * np.sin(x / (7.0 + 3 * c) + ph[c, 0]) * np.cos(y / (5.0 + 2 * c) + ph[c, 1]) + 0.2 * np.sin((x + 2 * y) / 31.0 + ph[c, 2])
             for c in range(3)]
    return np.stack(chans).astype(np.float32)


# ----------------------------------------------------------------------------------------------- match depth scale
RASTER = (512, 144)


def depth_map(H, W, seed):
    """A positive depth field with structure and 1 % noise, float32."""
    rng = np.random.default_rng(seed)
    y = np.linspace(0.0, 1.0, H)[:, None]
    x = np.linspace(0.0, 1.0, W)[None, :]
    d = 5.0 + 30.0 * (1.0 - y) ** 2 + 3.0 * np.sin(8.0 * x + 2.0 * y) + 1.5 * np.cos(19.0 * x * (1.0 + y))
    return (d * (1.0 + 0.01 * rng.standard_normal((H, W)))).astype(np.float32)


def grid_matches(raster=RASTER, stride=8, seed=0, jitter=0.0):
    """The seeds' grid of ``reciprocal_matches`` as matches: map-1 pixels on the stride grid, map-2 pixels the same, moved by up to
    ``jitter`` pixels (float32, kept inside the raster)."""
    W1, H1 = raster
    gy, gx = np.mgrid[stride // 2:H1:stride, stride // 2:W1:stride]
    m1 = np.stack([gx.ravel(), gy.ravel()], 1).astype(np.int32)
    m2 = m1.astype(np.float32)
    if jitter:
        rng = np.random.default_rng(seed)
        m2 = m2 + rng.uniform(-jitter, jitter, size=m2.shape).astype(np.float32)
        m2[:, 0] = np.clip(m2[:, 0], 0, W1 - 1)
        m2[:, 1] = np.clip(m2[:, 1], 0, H1 - 1)
    return m1, m2.astype(np.float32)


def random_matches(M, raster=RASTER, seed=0):
    rng = np.random.default_rng(seed)
    W1, H1 = raster
    m1 = np.stack([rng.integers(0, W1, M), rng.integers(0, H1, M)], 1).astype(np.int32)
    m2 = np.stack([rng.uniform(0, W1 - 1, M), rng.uniform(0, H1 - 1, M)], 1).astype(np.float32)
    return m1.reshape(-1, 2), m2.reshape(-1, 2)


def holes(d1, d2, seed):
    """30 % zeros in the first map, 5 % NaNs in the second."""
    rng = np.random.default_rng(seed)
    d1, d2 = d1.copy(), d2.copy()
    d1[rng.random(d1.shape) < 0.30] = 0.0
    d2[rng.random(d2.shape) < 0.05] = np.nan
    return d1, d2


def scaled_pair(H, W, s, seed=3):
    """depth2 = depth1 / s (the same size): the scale between them is s wherever both are sampled at the same place."""
    d1 = depth_map(H, W, seed)
    return d1, (d1.astype(np.float64) / s).astype(np.float32)


M_SWEEP = (0, 1, 63, 64, 65, 1137, 8192)


def sweep_case(M, with_holes):
    """Random matches over RASTER, a 185 x 613 first map and a 90 x 300 second one (both resized, by different factors)."""
    m1, m2 = random_matches(M, seed=40 + M)
    d1, d2 = depth_map(185, 613, 7), depth_map(90, 300, 8)
    if with_holes:
        d1, d2 = holes(d1, d2, 9)
    return m1, m2, d1, d2


def border_matches(raster=RASTER):
    """Corners (the clamped branch), then matches outside the raster: -1, W1 and H1 in either map (dropped).  -> (m1, m2, inside (bool))."""
    W1, H1 = raster
    rows = [((0, 0), (0.0, 0.0), True), ((W1 - 1, H1 - 1), (W1 - 1.0, H1 - 1.0), True), ((0, H1 - 1), (W1 - 0.25, 3.0), True),
            ((5, 5), (-0.75, 7.5), True),                       # truncated toward zero: column 0
            ((-1, 3), (4.0, 4.0), False), ((W1, 3), (4.0, 4.0), False), ((3, H1), (4.0, 4.0), False), ((3, -1), (4.0, 4.0), False),
            ((3, 3), (-1.0, 4.0), False), ((3, 3), (float(W1), 4.0), False), ((3, 3), (4.0, float(H1)), False), ((3, 3), (4.0, -1.0), False),
            ((3, 3), (np.nan, 4.0), False)]
    m1 = np.array([r[0] for r in rows], dtype=np.int32)
    m2 = np.array([r[1] for r in rows], dtype=np.float32)
    return m1, m2, np.array([r[2] for r in rows])


def format_refusals(make_args):
    """(what, args, word of the error text) for every condition ``lvdgs_format_image`` refuses with LVDGS_E_INVALID.  ``make_args(**over)``
    builds a valid ``_lib.FormatImageArgs`` (a 200 x 75 image, size 90) with fields replaced."""
    out = [("args NULL", None, b"NULL")]
    for f in ("image", "table_x", "table_y", "out", "scratch"):
        out.append((f + " NULL", make_args(**{f: None}), b"NULL"))
    out += [("width = 0", make_args(width=0), b"image size"), ("height < 0", make_args(height=-4), b"image size"),
            ("size 224", make_args(size=224), b"224"), ("size 8", make_args(size=8), b"size 8"), ("size too large", make_args(size=5000), b"outside"),
            ("edge too long", make_args(width=20000), b"edge"), ("empty raster", make_args(width=4000, height=20, size=512), b"empty raster"),
            ("scratch too small", make_args(scratch_bytes=255), b"scratch")]
    return out


def scale_refusals(make_args):
    """Likewise for ``lvdgs_match_depth_scale`` (64 matches at RASTER, a 185 x 613 and a 90 x 300 map)."""
    out = [("args NULL", None, b"NULL")]
    for f in ("matches_im1", "matches_im2", "depth1", "depth2", "host_state"):
        out.append((f + " NULL", make_args(**{f: None}), b"NULL"))
    out.append(("num_matches < 0", make_args(num_matches=-1), b"num_matches"))
    for f in ("raster_width", "raster_height"):
        out.append((f + " = 0", make_args(**{f: 0}), b"raster size"))
    for f in ("width1", "height1", "width2", "height2"):
        out.append((f + " = 0", make_args(**{f: 0}), b"map size"))
        out.append((f + " < 0", make_args(**{f: -3}), b"map size"))
    return out
