"""Seeded cases of multi-scale deformable attention (tests/test_ms_deform_attn.py, tests/test_gpu_ms_deform_attn.py and
tests/golden/make_ms_deform_attn_golden.py share them): the smallest shapes at which each path of the kernels can go wrong.

Every array is float32 (what the operator takes), made once per case and read-only.  Two location sets per case:

* ``loc_snapped``: uniform over [-0.3, 1.3]^2, and half of the samples moved exactly onto multiples of half a pixel from -1 to w
  (and -1 to h) -- pixel centres, pixel edges and both validity limits.  For the forward only: the location gradient is
  discontinuous where x or y is an integer.
* ``loc_generic``: the cell index uniform in [-2, w + 1] (and [-2, h + 1]), the fractional part uniform in [1/64, 63/64].  For the
  gradients: with that margin no float32 rounding moves a sample to another cell at these widths, so no element needs to be
  excluded from any comparison.
"""
import functools
import types

import numpy as np

KITTI_LEVELS = ((24, 77), (12, 39), (6, 20), (3, 10))          # S = 2466

CASES = {
    # name: B, H, D, Q, levels (h, w), P                          why
    "tiny": (1, 1, 6, 5, ((2, 3),), 1),                           # scalar path, one of everything
    "odd": (2, 3, 20, 7, ((1, 9), (4, 1)), 3),                    # 5 lanes per head, one-pixel-wide levels
    "dino_small": (2, 8, 32, 6, ((3, 5), (2, 3), (1, 2), (1, 1)), 4),   # the product's head layout, S = 24, level_start non-trivial
    "dino_rows": (1, 8, 32, 300, KITTI_LEVELS, 4),                # decoder-like, Q not a multiple of anything
    "dino_encoder": (1, 8, 32, 2466, KITTI_LEVELS, 4),            # encoder-like, Q = S
}
SMALL = ("tiny", "odd", "dino_small")                             # the cases whose float64 results are in the golden file
LOCATION_SETS = ("snapped", "generic")


def _locked(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def case(name):
    B, H, D, Q, levels, P = CASES[name]
    rng = np.random.default_rng(20261 + sorted(CASES).index(name))   # (a seed at which `tiny`'s five generic samples are not all outside)
    L = len(levels)
    shapes = np.asarray(levels, np.int64).reshape(L, 2)
    areas = shapes[:, 0] * shapes[:, 1]
    starts = np.cumsum(areas) - areas
    S = int(areas.sum())
    value = rng.standard_normal((B, S, H, D)).astype(np.float32)
    weights = rng.random((B, Q, H, L, P)) + 0.05
    weights = (weights / weights.sum(axis=(3, 4), keepdims=True)).astype(np.float32)      # like the module's softmax over L * P
    grad_out = rng.standard_normal((B, Q, H * D)).astype(np.float32)
    snapped = np.empty((B, Q, H, L, P, 2), np.float64)
    generic = np.empty((B, Q, H, L, P, 2), np.float64)
    for l, (h, w) in enumerate(levels):
        shape = (B, Q, H, P)
        moved = rng.random(shape) < 0.5                                                    # half of the samples, both coordinates
        for axis, n in ((0, w), (1, h)):                                                  # (x, y): x runs over the width
            free = rng.uniform(-0.3, 1.3, shape)
            half_pixels = rng.integers(-2, 2 * n + 1, shape) / 2.0                          # -1, -0.5, ..., n
            snapped[:, :, :, l, :, axis] = np.where(moved, (half_pixels + 0.5) / n, free)
            cell = rng.integers(-2, n + 2, shape)                                          # -2 .. n + 1
            generic[:, :, :, l, :, axis] = (cell + rng.uniform(1.0 / 64.0, 63.0 / 64.0, shape) + 0.5) / n
    return types.SimpleNamespace(name=name, B=B, S=S, H=H, D=D, Q=Q, L=L, P=P, levels=levels, shapes=_locked(shapes), starts=_locked(starts),
                                 value=_locked(value), weights=_locked(weights), grad_out=_locked(grad_out),
                                 loc_snapped=_locked(snapped.astype(np.float32)), loc_generic=_locked(generic.astype(np.float32)))


def locations(c, which):
    return {"snapped": c.loc_snapped, "generic": c.loc_generic}[which]
