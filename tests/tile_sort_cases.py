"""Scenes whose per-tile list lengths are PRESCRIBED, for the tile depth sort (csrc/tilesort.hip): which code sorts a segment depends
on its length, on the grid and on a per-thread hint, and a random scene puts no segment on the boundaries between them (test
infrastructure: tests/test_tile_sort_cases.py checks the scenes and the reference on the CPU, tests/test_gpu_tile_sort.py runs them
through the kernels).

``ladder(lengths, W, H, seed)`` puts, for every requested length L, L Gaussians into a tile of its own, each of which touches that
tile alone: centres within 2 px of the tile's centre, footprints of 0.8 px (3-sigma radii of at most 5 px, so the rectangle stays
inside the 16 x 16 tile), opacity 0.02 (every Gaussian reaches 1/255 on its own tile, so tile culling keeps the lists as they are).
View depths: a third from 7 values, a third from 300 values, the rest uniform -- long lists hold many equal depths, whose order the id
decides, beside different ones (tests/test_tile_sort_cases.py asserts both of every segment of 64 or more entries).  The Gaussians
are randomly permuted: id order says nothing about tile or depth.
"""
import functools
import os
import sys

import numpy as np
import torch

import edge_scenes

TILE = 16
SUPER = 4             # tiles per super-tile side (LVDGS_FLAG_SUPER_TILES: 64 x 64 pixels)
WAVE_LIMIT = 1024     # longest segment one wave sorts; longer ones are queued
GROUP_LIMIT = 2048    # longest segment a workgroup of the tile sort's own launch sorts in LDS / in registers
LDS_LIMIT = 16384     # longest segment the 1024-thread kernel sorts in LDS

FULL = [0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 16383, 16384, 16385,
        20000]
MID = [n for n in FULL if n <= GROUP_LIMIT]       # the longest queued segment is 2048
SHORT = [n for n in FULL if n <= WAVE_LIMIT]      # nothing is queued
MANY_MID = [1025 + (k * 1023) // 79 for k in range(80)]      # 80 segments of 1025..2048: more than the 64 head workgroups
MANY_TAIL = [1025 + k % 60 for k in range(260)]              # 260 segments of 1025..1084: more than the 256 last workgroups
MANY_LONG = [2049 + k % 60 for k in range(260)]              # 260 segments of 2049..2108: more than the long kernel's 256 workgroups
assert sum(FULL) == 93_158 and MANY_MID[0] == 1025 and MANY_MID[-1] == 2048

POSE_SEED = 3         # the camera: edge_scenes._camera(W, H, "centred", POSE_SEED)
# size classes of a segment: a band or a view "has every class" when it holds a segment of each
CLASSES = ((1, 256), (257, 512), (513, WAVE_LIMIT), (WAVE_LIMIT + 1, GROUP_LIMIT), (GROUP_LIMIT + 1, LDS_LIMIT), (LDS_LIMIT + 1, 1 << 30))


def ladder(lengths, W, H, seed, stride=1):
    """(g, cam): for every entry L of ``lengths`` a distinct tile of the W x H frame (whole tiles only; ``stride=4``: tiles whose
    coordinates are multiples of 4, one per 64 x 64 super-tile) with exactly L Gaussians, each touching that tile alone."""
    rng = np.random.default_rng(seed)
    cam = edge_scenes._camera(W, H, "centred", POSE_SEED)
    gx, gy = W // TILE, H // TILE
    xs, ys = np.meshgrid(np.arange(0, gx, stride), np.arange(0, gy, stride))
    cand = np.stack([xs.ravel(), ys.ravel()], 1)
    assert len(lengths) <= len(cand), "more segments than tiles"
    tiles = cand[rng.choice(len(cand), size=len(lengths), replace=False)]
    n = int(sum(lengths))
    tx = np.repeat(tiles[:, 0], lengths)
    ty = np.repeat(tiles[:, 1], lengths)
    px = TILE * tx + 7.5 + rng.uniform(-2.0, 2.0, n)
    py = TILE * ty + 7.5 + rng.uniform(-2.0, 2.0, n)
    few = np.linspace(1.5, 7.5, 7)[rng.integers(0, 7, n)]
    some = np.linspace(1.0, 9.0, 300)[rng.integers(0, 300, n)]
    kind = rng.integers(0, 3, n)
    z = np.where(kind == 0, few, np.where(kind == 1, some, rng.uniform(1.0, 9.0, n)))
    g = edge_scenes._assemble(cam, px, py, z, 0.8 * np.ones(n), 0.02 * np.ones(n), rng)
    perm = torch.from_numpy(rng.permutation(n))
    return {k: v[perm].contiguous() for k, v in g.items()}, cam


def shifted_camera(cam, W, H, columns):
    """``cam`` with its principal point ``columns`` tiles to the right: every centre moves by that many whole tiles, a ladder's
    segments with it, and those that leave the frame are culled -- another view of the same map with another ladder."""
    from lvdgs import synthetic
    return synthetic.make_camera(W, H, pose_seed=POSE_SEED, cx=cam.cx + TILE * columns)


# ---- the cases the GPU file runs: name -> (lengths, W, H, seed, stride) ----
SMALL = (160, 160)     # 100 tiles: tile order and solo workgroups; >= 64 tiles, so two-level grouping applies
LARGE = (1040, 1040)   # 4225 tiles: the counting path without them
RADIX = (2064, 2064)   # 16641 tiles: the radix path
QUEUE = (320, 320)     # 400 tiles: room for 260 long segments
CASES = {
    "full_small": (FULL, *SMALL, 1, 1), "mid_small": (MID, *SMALL, 2, 1), "short_small": (SHORT, *SMALL, 3, 1),
    "full_large": (FULL, *LARGE, 4, 1), "mid_large": (MID, *LARGE, 5, 1), "short_large": (SHORT, *LARGE, 6, 1),
    "full_radix": (FULL, *RADIX, 7, 1),
    "many_mid": (MANY_MID, *QUEUE, 8, 1), "many_tail": (MANY_TAIL, *QUEUE, 9, 1), "many_long": (MANY_LONG, *QUEUE, 10, 1),
    "full_super4": (FULL, 384, 384, 11, 4), "short_super4": (SHORT, 384, 384, 12, 4),
    "full_super1": (FULL, 128, 128, 13, 1), "short_super1": (SHORT, 128, 128, 14, 1),
}
BATCH_SHIFTS = (0, 1, -2)          # lvdgs_forward_batch: "full_small" under three cameras, shifted by whole tile columns
BAND_ROWS = (2, 8)                 # the band case: tile rows [2, 8) of "full_small"


@functools.lru_cache(maxsize=None)
def scene(name):
    lengths, W, H, seed, stride = CASES[name]
    return ladder(lengths, W, H, seed, stride)


def _oracle():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
    import oracle as orc
    return orc


@functools.lru_cache(maxsize=None)
def reference(name, shift=0):
    """The float32 oracle's forward of a case (under the camera shifted by ``shift`` tile columns): computed once, shared by every
    test that needs it, never modified."""
    import hip_runner
    lengths, W, H, seed, stride = CASES[name]
    g, cam = scene(name)
    if shift:
        cam = shifted_camera(cam, W, H, shift)
    f, _ = hip_runner.run_oracle(_oracle(), g, cam, W, H, torch.zeros(3))
    for v in f.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return f


def list_lengths(f):
    r = f["ranges"].astype(np.int64)
    return r[:, 1] - r[:, 0]


def numpy_sorted_ids(f, gx):
    """Every tile's list stated once more, in NumPy, from the oracle's own per-Gaussian results (not from its C sort): a Gaussian is
    listed on the one tile its rectangle covers (``tiles_touched`` is 1 or 0 in these scenes), the entries ordered by (tile, depth
    bits, id).  Returns (ids, their tiles)."""
    assert (f["tiles_touched"] <= 1).all()
    listed = np.nonzero(f["tiles_touched"] == 1)[0]
    rect = f["rect"].astype(np.int64)           # x0, y0, x1, y1 in tiles (x1 / y1 exclusive)
    tile = rect[listed, 1] * gx + rect[listed, 0]
    depth_bits = np.ascontiguousarray(f["depths"], dtype=np.float32).view(np.uint32)[listed]
    order = np.lexsort((listed, depth_bits, tile))
    return listed[order].astype(np.uint32), tile[order]


def super_list_lengths(lengths_per_tile, W, H):
    """Lengths of the 64 x 64-pixel super-tiles' lists when every Gaussian touches one tile: the sums over each super-tile's tiles."""
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    gxs, gys = (gx + SUPER - 1) // SUPER, (gy + SUPER - 1) // SUPER
    out = np.zeros(gxs * gys, np.int64)
    t = np.arange(gx * gy)
    np.add.at(out, (t // gx // SUPER) * gxs + (t % gx) // SUPER, lengths_per_tile)
    return out
