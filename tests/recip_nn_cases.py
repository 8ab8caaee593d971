"""The seeded descriptor-map pairs the reciprocal nearest-neighbour tests run on, and their oracle results (computed once per process).

Map 1: random Fourier features of the pixel position plus noise, unit-normalised.  Map 2: the same field sampled under a similarity
warp -- a pixel p1 of map 1 shows up at p2 = SCALE * R(ROT) p1 + SHIFT of map 2 -- with noise of its own.  The map sizes are no
multiples of 64, 32 or 16 (the raster's 144 x 512 aside) and most seed counts no multiples of a wave.
"""
import functools
import math
from types import SimpleNamespace

import numpy as np

import recip_nn_oracle as oracle

ROT, SCALE, SHIFT = 0.03, 1.04, (1.37, -0.71)
FREQ, NOISE = 0.35, 0.02     # rad / pixel of the features' frequencies (standard deviation); noise per component before normalisation

# name: (H1, W1, H2, W2, D, S, max_iter)
CASES = {
    "small_d24_s4": (37, 53, 41, 67, 24, 4, 10),
    "small_d16_s3": (33, 47, 29, 61, 16, 3, 10),
    "small_d16_s3_one_round": (33, 47, 29, 61, 16, 3, 1),
    "shrunk_map2": (33, 47, 20, 30, 24, 2, 10),
    "wide_s8": (48, 160, 48, 160, 24, 8, 10),
    "dense_s1": (64, 96, 64, 96, 24, 1, 10),
    "dense_s1_two_rounds": (64, 96, 64, 96, 24, 1, 2),
    "odd_dim7": (35, 45, 38, 50, 7, 3, 10),
    "odd_dim23": (31, 44, 34, 49, 23, 5, 10),       # an odd size on the 24-float build of the search (its last component is padding)
    "dim64": (20, 30, 22, 33, 64, 3, 10),           # the largest descriptor
    "duplicate_rows": (37, 53, 41, 67, 24, 4, 10),
    "raster_144x512": (144, 512, 144, 512, 24, 8, 10),
}
SMALL = [n for n in CASES if n != "raster_144x512"]
PRIMITIVE = ("small_d24_s4", "odd_dim7", "odd_dim23", "dim64")      # the cases whose every pixel is a query of the half-round test


def warp(p1):
    """Where pixels (..., 2) (x, y) of map 1 show up in map 2."""
    c, s = math.cos(ROT), math.sin(ROT)
    p1 = np.asarray(p1, dtype=np.float64)
    return SCALE * np.stack([c * p1[..., 0] - s * p1[..., 1], s * p1[..., 0] + c * p1[..., 1]], -1) + np.asarray(SHIFT)


def unwarp(p2):
    c, s = math.cos(ROT), math.sin(ROT)
    q = (np.asarray(p2, dtype=np.float64) - np.asarray(SHIFT)) / SCALE
    return np.stack([c * q[..., 0] + s * q[..., 1], -s * q[..., 0] + c * q[..., 1]], -1)


def _features(pos, freq, phase, rng):
    f = np.cos(pos @ freq + phase) + NOISE * rng.standard_normal(pos.shape[:-1] + (freq.shape[1],))
    return (f / np.linalg.norm(f, axis=-1, keepdims=True)).astype(np.float32)


def _maps(H1, W1, H2, W2, D, seed):
    rng = np.random.default_rng(seed)
    freq, phase = FREQ * rng.standard_normal((2, D)), rng.uniform(0, 2 * math.pi, D)
    g1 = np.stack(np.meshgrid(np.arange(W1), np.arange(H1), indexing="xy"), -1).astype(np.float64)
    g2 = np.stack(np.meshgrid(np.arange(W2), np.arange(H2), indexing="xy"), -1).astype(np.float64)
    return _features(g1, freq, phase, rng), _features(unwarp(g2), freq, phase, rng)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> namespace: ``desc1`` (H1, W1, D), ``desc2`` (H2, W2, D) float32 C-contiguous (read-only), ``S``, ``max_iter``, ``oracle``
    (``recip_nn_oracle.reciprocal_nn`` on them); the duplicate-row case also ``duplicates`` (copy index -> original index)."""
    H1, W1, H2, W2, D, S, max_iter = CASES[name]
    d1, d2 = _maps(H1, W1, H2, W2, D, seed=[H1, W1, H2, W2, D])
    duplicates = None
    if name == "duplicate_rows":
        # bit-identical copies of the descriptors that win, at HIGHER flat indices: the last rows of map 2 are overwritten, winners there left out
        flat = d2.reshape(-1, D)
        winners = np.unique(oracle.reciprocal_nn(d1, d2, S, max_iter).pairs[:, 1])
        winners = winners[winners < len(flat) - 2 * len(winners)]
        copies = len(flat) - 1 - np.arange(len(winners))
        flat[copies] = flat[winners]
        duplicates = dict(zip(copies.tolist(), winners.tolist()))
    d1, d2 = np.ascontiguousarray(d1), np.ascontiguousarray(d2)
    d1.setflags(write=False); d2.setflags(write=False)
    return SimpleNamespace(name=name, desc1=d1, desc2=d2, S=S, max_iter=max_iter, duplicates=duplicates,
                           oracle=oracle.reciprocal_nn(d1, d2, S, max_iter))


@functools.lru_cache(maxsize=None)
def half_round(name):
    """Every pixel of map 1 as a query against map 2, and the way back from those winners: -> (idx2, margin2, idx1, margin1)."""
    c = case(name)
    D = c.desc1.shape[-1]
    A, B = c.desc1.reshape(-1, D), c.desc2.reshape(-1, D)
    j, mj = oracle.nearest(A, B)
    i, mi = oracle.nearest(B[j], A)
    return j, mj, i, mi


def refusals(make_args):
    """(what, args, word of the error text) for every condition ``lvdgs_reciprocal_nn`` refuses with LVDGS_E_INVALID.  ``make_args(**over)``
    builds a valid ``_lib.RecipNnArgs`` (a 37 x 53 and a 41 x 67 map of 24 floats, subsample 4: 117 seeds) with fields replaced."""
    out = [("args NULL", None, b"NULL")]
    for f in ("desc1", "desc2", "matches_im1", "matches_im2", "host_state", "scratch"):
        out.append((f + " NULL", make_args(**{f: None}), b"NULL"))
    for f in ("width1", "height1", "width2", "height2"):
        out.append((f + " = 0", make_args(**{f: 0}), b"map size"))
        out.append((f + " < 0", make_args(**{f: -3}), b"map size"))
    out += [("dim = 0", make_args(dim=0), b"dim"), ("dim = 65", make_args(dim=65), b"dim"), ("dim < 0", make_args(dim=-1), b"dim"),
            ("subsample = 0", make_args(subsample=0), b"subsample"), ("max_iter = 0", make_args(max_iter=0), b"max_iter"),
            ("too many seeds", make_args(width1=128, height1=128, subsample=1, capacity=16384), b"seeds"),
            ("capacity below the seed count", make_args(capacity=116), b"capacity"),
            ("scratch too small", make_args(scratch_bytes=255), b"scratch"),
            ("map too large", make_args(width1=40000, height1=40000, subsample=4000), b"2^31")]
    return out
