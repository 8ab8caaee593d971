"""The frame-ingest cases shared by tests/test_dataset.py (host mode against the oracle) and tests/test_gpu_dataset.py (the HIP entry
points against the oracle): the smallest shapes at which the kernel can go wrong, and one full Waymo frame.

A case: width, height, the intrinsics, the five coefficients (k1, k2, p1, p2, k3) and ``pad`` -- bytes between the rows of the source
beyond 3 W (0: contiguous rows).  References are computed once per process (``reference``) and never modified."""
import functools
import os

import numpy as np

import ingest_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WAYMO_YAML = os.path.join(ROOT, "tests", "golden", "configs", "mono", "waymo", "405841.yaml")


def _case(W, H, fx=None, fy=None, cx=None, cy=None, dist=(0.05, -0.1, 0.002, -0.001, 0.01), pad=0):
    fx = 0.8 * W if fx is None else fx
    return dict(W=W, H=H, fx=float(fx), fy=float(fx if fy is None else fy), cx=float((W - 1) / 2 + 0.3 if cx is None else cx),
                cy=float((H - 1) / 2 - 0.2 if cy is None else cy), dist=tuple(float(d) for d in dist), pad=pad)


def _waymo():
    from lvdgs.config_utils import load_config
    cal = load_config(WAYMO_YAML)["Dataset"]["Calibration"]
    return dict(W=cal["width"], H=cal["height"], fx=float(cal["fx"]), fy=float(cal["fy"]), cx=float(cal["cx"]), cy=float(cal["cy"]),
                dist=tuple(float(cal[k]) for k in ("k1", "k2", "p1", "p2", "k3")), pad=0)


SMALL = {
    "1x1": _case(1, 1, fx=1.5, cx=0.25, cy=-0.25),
    "67x35": _case(67, 35),                     # 3 W odd, rows not dword aligned, a short last group, partial waves
    "131x3": _case(131, 3),
    "64x64": _case(64, 64),
    "row_pitch": _case(67, 35, pad=7),          # src_row_bytes = 3 W + 7
    # fx = W / 2: |x| reaches 1 at the left and right edges; k1 = 1.5 pushes the sources of the outer destinations off the image on every
    # side (negative coordinates on the left and at the top)
    "outside": _case(67, 35, fx=33.5, dist=(1.5, 0.3, 0.01, -0.02, 0.0)),
    # exact arithmetic: fx = fy = 1, cx = cy = 0, k1 = 2^-10 -> mapx * 32 = 32 u + u (u^2 + v^2) / 32, a tie wherever u (u^2 + v^2) = 16 mod 32
    "ties": _case(64, 64, fx=1.0, cx=0.0, cy=0.0, dist=(2.0 ** -10, 0.0, 0.0, 0.0, 0.0)),
    "past_2^20": _case(67, 35, fx=33.5, dist=(1.0e6, 0.0, 0.0, 0.0, 0.0)),        # coordinates of magnitude >= 2^20: the sentinel
    # float64 overflow: 1e308 r2^3 is infinite away from the principal point, and NaN where infinities meet (0 * inf, inf - inf); the
    # principal point's column and row lie on pixels here and keep a finite coordinate each
    "not_finite": _case(67, 35, fx=8.0, cx=33.0, cy=17.0, dist=(0.0, 1.0e200, 0.0, 0.0, -1.0e308)),
}
KINDS = ("noise", "white")
FULL = "waymo_1920x1280"


def case(name):
    return _waymo() if name == FULL else SMALL[name]


@functools.lru_cache(maxsize=None)
def source(name, kind):
    """The source frame as the device receives it: (H, 3 W + pad) uint8 rows; the pad bytes are 255 (a kernel that reads them shows)."""
    c = case(name)
    W, H = c["W"], c["H"]
    rows = np.full((H, 3 * W + c["pad"]), 255, np.uint8)
    if kind == "noise":
        rows[:, :3 * W] = np.random.default_rng(len(name) * 1000 + W).integers(0, 256, size=(H, 3 * W), dtype=np.uint8)
    rows.setflags(write=False)
    return rows


def pixels(name, kind):
    c = case(name)
    return source(name, kind)[:, :3 * c["W"]].reshape(c["H"], c["W"], 3)


@functools.lru_cache(maxsize=None)
def reference_map(name):
    c = case(name)
    sx, sy = orc.undistort_map(c["W"], c["H"], c["fx"], c["fy"], c["cx"], c["cy"], c["dist"])
    sx.setflags(write=False)
    sy.setflags(write=False)
    return sx, sy


@functools.lru_cache(maxsize=None)
def reference(name, kind, remap):
    """(image_u8 (H, W, 3), image (3, H, W) float32) by the oracle's array form."""
    u8 = pixels(name, kind)
    if remap:
        u8 = orc.remap(u8, *reference_map(name))
    image = orc.convert(u8)
    u8 = np.ascontiguousarray(u8)
    u8.setflags(write=False)
    image.setflags(write=False)
    return u8, image
