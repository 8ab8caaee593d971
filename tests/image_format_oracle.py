"""NumPy restatement of the matcher's image formatting (``lvdgs_format_image``, include/lvdgs.h; the reference's
``torch_images_to_dust3r_format``, utils/init_pose.py:35-75): quantise, PIL's 8-bit resampling with integer coefficients, centre crop,
normalise.  tests/test_matcher_io.py holds it to PIL byte for byte (tests/golden/image_format.npz, and live PIL where it imports)."""
import math

import numpy as np

PRECISION_BITS = 22
LANCZOS, BICUBIC = "lanczos", "bicubic"


def sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def lanczos(x):
    return sinc(x) * sinc(x / 3) if -3.0 <= x < 3.0 else 0.0


def bicubic(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


FILTERS = {LANCZOS: (lanczos, 3.0), BICUBIC: (bicubic, 2.0)}


def coefficients(n_in, n_out, filt):
    """-> [(xmin, integer coefficients (n,))] per output sample of a pass from ``n_in`` to ``n_out`` samples."""
    f, fsupport = FILTERS[filt]
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = fsupport * fs
    ss = 1.0 / fs
    out = []
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        n = min(int(center + support + 0.5), n_in) - xmin
        w = [f((x + xmin - center + 0.5) * ss) for x in range(n)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        k = [int(v * (1 << PRECISION_BITS) + 0.5) if v >= 0 else int(v * (1 << PRECISION_BITS) - 0.5) for v in w]
        out.append((xmin, np.asarray(k, dtype=np.int64)))
    return out


def resample_axis0(img, n_out, filt):
    """One pass along axis 0 of a uint8 array (the other axes ride along) -> uint8."""
    n_in = img.shape[0]
    res = np.empty((n_out,) + img.shape[1:], dtype=np.uint8)
    src = img.astype(np.int64)
    for xx, (xmin, k) in enumerate(coefficients(n_in, n_out, filt)):
        acc = (1 << (PRECISION_BITS - 1)) + np.tensordot(k, src[xmin:xmin + len(k)], axes=(0, 0))
        assert np.abs(acc).max() < 2 ** 31         # the sums fit int32, as PIL and the kernels take them
        res[xx] = np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return res


def resize(img, w, h, filt):
    """``PIL.Image.resize((w, h), filt)`` of an (H, W, 3) uint8 image: horizontal pass, then vertical; an unchanged edge is skipped."""
    H, W = img.shape[:2]
    if w != W:
        img = resample_axis0(img.transpose(1, 0, 2), w, filt).transpose(1, 0, 2)
    if h != H:
        img = resample_axis0(img, h, filt)
    return np.ascontiguousarray(img)


def plan(W, H, size):
    """-> (w, h, filter, crop_x, crop_y, W1, H1)."""
    if size == 224:
        raise ValueError("size 224 takes the reference's other crop rule")
    S = max(W, H)
    w, h = int(round(W * size / S)), int(round(H * size / S))
    cx, cy = w // 2, h // 2
    halfw, halfh = ((2 * cx) // 16) * 8, ((2 * cy) // 16) * 8
    if w == h:
        halfh = 3 * halfw // 4
    return w, h, (LANCZOS if S > size else BICUBIC), cx - halfw, cy - halfh, 2 * halfw, 2 * halfh


def quantise(image):
    """(3, H, W) float32 -> (H, W, 3) uint8: trunc(x * 255) in float32, clamped to [0, 255], NaN -> 0."""
    v = np.asarray(image, dtype=np.float32) * np.float32(255.0)
    v = np.where(np.isnan(v), np.float32(0.0), np.clip(v, np.float32(0.0), np.float32(255.0)))
    return np.ascontiguousarray(np.trunc(v).astype(np.uint8).transpose(1, 2, 0))


def format_bytes(q, size):
    """The cropped resize of an (H, W, 3) uint8 image -> (H1, W1, 3) uint8."""
    H, W = q.shape[:2]
    w, h, filt, x0, y0, W1, H1 = plan(W, H, size)
    return np.ascontiguousarray(resize(q, w, h, filt)[y0:y0 + H1, x0:x0 + W1])


def normalise(q):
    """uint8 -> float32 (q / 255 - 0.5) / 0.5, every step rounded to float32."""
    return ((q.astype(np.float32) / np.float32(255.0)) - np.float32(0.5)) / np.float32(0.5)


def format_image(image, size=512):
    """(3, H, W) float32 -> (quantised (H1, W1, 3) uint8, img (1, 3, H1, W1) float32)."""
    q = format_bytes(quantise(image), size)
    return q, np.ascontiguousarray(normalise(q).transpose(2, 0, 1))[None]
