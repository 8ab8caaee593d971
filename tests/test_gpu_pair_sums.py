"""The pair-sum stage of the per-Gaussian backward (csrc/preprocess_bwd.hip: PairSums) through every branch, at the smallest scene
that reaches them -- 400 Gaussians at 320 x 240, concatenated in this id order:

    waves 0-3   256 small blobs: no Gaussian over BIG_RUN = 64 pairs, regions of more than two chunks of WAVE_CHUNK = 192 slots: streamed;
    waves 4-5   128 surface Gaussians of 16-64 px: tens of them over 64 pairs, regions of more than twelve 512-slot segments, one run
                across the two-part split: the compacted sweep, part after part or with helper waves, the whole-wave sum of the pass;
    wave  6     16 blobs: a wave of 16 lanes, N no multiple of 64.

With and without tile culling (without it the pair lists are the reference's).  The premise is checked on the forward's own
tiles_touched / slot_base; then every gradient against the float32 oracle, helper waves against part-after-part, and the two views of
one lvdgs_gaussian_backward_batch against the view-after-view passes, the last two bit for bit."""
import os
import sys
from functools import lru_cache

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
pytestmark = pytest.mark.gpu

W, H = 320, 240
WAVE_CHUNK, BIG_RUN, SEG = 192, 64, 512   # csrc/preprocess_bwd.hip
NAMES = ["means3D", "means2D", "opacities", "scales", "rotations", "colors", "tau"]


@lru_cache(maxsize=None)
def _scene():
    from lvdgs import synthetic
    parts = [synthetic.make_gaussians(256, W, H, seed=5, r_min=2.0, r_max=12.0),
             synthetic.make_surface_gaussians(128, W, H, seed=5, r_min=16.0, r_max=64.0),
             synthetic.make_gaussians(16, W, H, seed=6)]
    return {k: torch.cat([p[k] for p in parts]).contiguous() for k in parts[0]}


@lru_cache(maxsize=None)
def _hip(tile_cull, super_tiles):
    import hip_runner
    from lvdgs import synthetic
    return hip_runner.run_hip(_scene(), synthetic.make_camera(W, H), W, H, torch.zeros(3), grads=synthetic.make_image_grads(W, H, 1),
                              tile_cull=tile_cull, super_tiles=super_tiles)


@lru_cache(maxsize=None)
def _oracle():
    import hip_runner
    import oracle as orc
    from lvdgs import synthetic
    return hip_runner.run_oracle(orc, _scene(), synthetic.make_camera(W, H), W, H, torch.zeros(3), grads=synthetic.make_image_grads(W, H, 1))


def _waves(f):
    """Per wave of 64 ids: (region in slots, pairs of its largest run, whether a run holds the two-part split) -- the kernel's
    arithmetic on the forward's own tiles_touched and slot_base."""
    tiles, slot = f["tiles_touched"].astype(np.int64), f["slot_base"].astype(np.int64)
    run = np.where(f["radii"] > 0, tiles, 0)
    out = []
    for w0 in range(0, len(tiles), 64):
        w1 = min(w0 + 64, len(tiles))
        lo, hi = int(slot[w0]), int(slot[w1 - 1] + tiles[w1 - 1])
        split = min(hi, lo + -(-((hi - lo) // 2) // SEG) * SEG)
        first = slot[w0:w1][run[w0:w1] > 0]
        last = first + run[w0:w1][run[w0:w1] > 0]
        out.append((hi - lo, int(run[w0:w1].max()), bool(((first < split) & (split < last)).any())))
    return out


@pytest.mark.parametrize("tile_cull", [True, False])
def test_the_scene_reaches_every_branch_of_the_pair_sums(tile_cull):
    f, _ = _hip(tile_cull, False)
    N = len(f["radii"])
    waves = _waves(f)
    print(f"tile_cull={tile_cull}: pairs {f['num_rendered']}, waves (region, largest run, run across the split): {waves}")
    assert N % 64 != 0
    assert any(big <= BIG_RUN and region > 2 * WAVE_CHUNK for region, big, _ in waves), "no streamed wave of more than two chunks"
    assert any(big > BIG_RUN and region > 2 * SEG and across for region, big, across in waves), "no large-footprint wave with a run across the split"


@pytest.mark.parametrize("tile_cull", [True, False])
def test_every_gradient_matches_the_oracle(tile_cull):
    from test_gpu_parity import _check_backward
    _, b_hip = _hip(tile_cull, False)
    f_ora, b_ora = _oracle()
    _check_backward(b_hip, b_ora, NAMES, f_ora, W, H)


@pytest.mark.parametrize("tile_cull", [True, False])
def test_helper_waves_add_the_same_bits(tile_cull):
    """(Without tile culling the library ignores the hint -- rasterizer.super_tiles_flag -- and both runs take the part-after-part kernels.)"""
    from lvdgs import _lib
    (f0, b0), (f1, b1) = _hip(tile_cull, False), _hip(tile_cull, True)
    assert not f0["flags"] & _lib.FLAG_SUPER_TILES
    assert bool(f1["flags"] & _lib.FLAG_SUPER_TILES) == tile_cull
    for k, v in b0.items():
        assert np.array_equal(b1[k], v), k


def _two_views(batch, list_all_tiles):
    """The parameter and pose gradients of the scene's two views -- make_camera(W, H) and make_camera(W, H, pose_seed=1) -- through one
    lvdgs_gaussian_backward_batch (MapWindowBatch) or view after view, the second adding to the first (MapViewPass).  SH colours of
    one coefficient, which that entry point asks for: the same colours as the precomputed ones of the other tests."""
    import bench
    from lvdgs import rasterizer, synthetic
    from lvdgs.fast_mapping import MapViewPass, MapWindowBatch
    from lvdgs.gaussian_model import GaussianModel
    dev = torch.device("cuda", 0)
    g = _scene()
    synthetic.CONFIGS.setdefault("tmp_pair_sums", dict(N=g["means3D"].shape[0], W=W, H=H))
    before = rasterizer.LIST_ALL_TILES
    rasterizer.LIST_ALL_TILES = list_all_tiles
    try:
        torch.manual_seed(0)
        model = GaussianModel.from_activated(g["means3D"], g["scales"], g["rotations"], g["opacities"], shs=g["shs"], sh_degree=0, device=dev)
        backend, _ = bench.build_window("tmp_pair_sums", 2, dev, model)   # (keyframe k + 1: the pose of make_camera(pose_seed=k))
        views = [backend.viewpoints[1], backend.viewpoints[2]]
        views[0].update_RT(torch.eye(3), torch.zeros(3))                  # make_camera(W, H): the identity
        for p_ in model.parameters():
            p_.grad = None
        if batch:
            MapWindowBatch(MapViewPass(dev)).run(backend, views)
        else:
            vpass = MapViewPass(dev)
            for vp in views:
                vpass.run(backend, vp)
        torch.cuda.synchronize()
        return ([p_.grad.clone() for p_ in model.parameters() if p_.grad is not None],
                [p_.grad.clone() for vp in views for p_ in (vp.cam_rot_delta, vp.cam_trans_delta)])
    finally:
        rasterizer.LIST_ALL_TILES = before


@pytest.mark.parametrize("tile_cull", [True, False])
def test_two_views_in_one_launch_are_the_views_one_after_the_other(tile_cull):
    params_b, poses_b = _two_views(True, not tile_cull)
    params_s, poses_s = _two_views(False, not tile_cull)
    assert len(params_b) >= 5 and all(float(t.abs().sum()) > 0 for t in params_b)
    assert len(params_b) == len(params_s) and len(poses_b) == len(poses_s) == 4
    for a, b in zip(params_b + poses_b, params_s + poses_s):
        assert torch.equal(a, b)
