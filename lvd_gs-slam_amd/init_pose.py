"""The initial pose estimate of a tracked frame: PnP-RANSAC of 2D-2D matches against the last keyframe's rendered depth, on the GPU.

The reference starts every frame's pose optimisation from ``get_pose`` (utils/init_pose.py:123-186, called from ``FrontEnd.tracking``,
utils/slam_frontend.py:1448): it renders the last keyframe's depth at the matcher's raster, copies it to the host, back-projects every
pixel (``depth_to_3d`` with ``cv2.undistortPoints``), and solves ``cv2.solvePnPRansac`` against the matched pixels of the new frame.
Here the depth stays on its device and the gather, the hypotheses, the consensus and the refinement are one ``lvdgs_pnp_ransac``
call (include/lvdgs.h states the semantics): two launches, one host wait.

The matcher that produces the matches (MASt3R descriptors + ``fast_reciprocal_NNs``) is out of scope: it is injectable as
``matcher(img1, img2, model, (W1, H1)) -> (matches_im1, matches_im2)`` -- (M, 2) pixel coordinates (x, y) at the raster ``(W1, H1)``,
integers in the keyframe and floats in the new frame, NumPy arrays or tensors.
"""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import torch

from . import _lib
from .gaussian_renderer import render_with_custom_resolution

# The record of the most recent call: status (_lib.PNP_OK / PNP_FAILED), reason (_lib.PNP_FAIL_*), valid_matches, inliers (under the final
# pose), hypothesis (the winner, -1: none), winner_count (its score), matches (M), inlier_mask (bool tensor (M,) on the device).
last_call = SimpleNamespace(status=None, reason=None, valid_matches=0, inliers=0, hypothesis=-1, winner_count=0, matches=0, inlier_mask=None)

_resources = {}   # device index -> (pinned host block, its words as int32, its pose as float64, scratch tensor)


def matcher_raster(W, H, size=512):
    """(W1, H1): the raster ``torch_images_to_dust3r_format`` (utils/init_pose.py:35-75) gives a W x H image -- the long edge resized
    to ``size`` (both edges rounded), then the centre crop to multiples of 16 (a square result is cropped to 4:3)."""
    S = max(W, H)
    w, h = int(round(W * size / S)), int(round(H * size / S))
    cx, cy = w // 2, h // 2
    halfw, halfh = ((2 * cx) // 16) * 8, ((2 * cy) // 16) * 8
    if w == h:
        halfh = 3 * halfw // 4
    return 2 * halfw, 2 * halfh


def _host_block(device, nbytes):
    key = device.index
    block, scratch = _resources.get(key, (None, None))
    if block is None:
        block = torch.zeros(_lib.PNP_HOST_BYTES, dtype=torch.uint8).pin_memory()
    if scratch is None or scratch.numel() < nbytes:
        scratch = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)
    _resources[key] = (block, scratch)
    return block, scratch


def pnp_ransac(depth, matches_im1, matches_im2, K, dist_coeffs=None, hypotheses=128, reproj_error=5.0, seed=0, min_inliers=6):
    """One ``lvdgs_pnp_ransac`` call.  ``depth``: (H1, W1) or (1, H1, W1) float32 CUDA tensor; the matches: (M, 2) arrays or tensors;
    ``K`` = (fx, fy, cx, cy) at that raster.  -> ``(pose (4, 4) float64 NumPy, exactly the identity on failure, inlier mask (M,) bool
    tensor on the device)``; the state words go to ``last_call``."""
    if not torch.is_tensor(depth) or not depth.is_cuda:
        raise _lib.LvdgsError("pnp_ransac: depth must be a tensor on a GPU (there is no CPU path)")
    device = depth.device
    d = _lib.f32(depth[0] if depth.ndim == 3 and depth.shape[0] == 1 else depth, device)
    if d.ndim != 2:
        raise ValueError(f"pnp_ransac: depth must be (H, W) or (1, H, W), got {tuple(depth.shape)}")
    H1, W1 = d.shape
    m1 = torch.as_tensor(np.asarray(matches_im1) if not torch.is_tensor(matches_im1) else matches_im1).reshape(-1, 2)
    m2 = torch.as_tensor(np.asarray(matches_im2) if not torch.is_tensor(matches_im2) else matches_im2).reshape(-1, 2)
    if m1.shape != m2.shape:
        raise ValueError(f"pnp_ransac: matches_im1 {tuple(m1.shape)} and matches_im2 {tuple(m2.shape)} differ")
    m1 = m1.to(device=device, dtype=torch.int32).contiguous()
    m2 = m2.to(device=device, dtype=torch.float32).contiguous()
    M = int(m1.shape[0])
    dist = np.zeros(5) if dist_coeffs is None else np.asarray(dist_coeffs, dtype=np.float64).reshape(-1)
    if dist.size != 5:
        raise ValueError("pnp_ransac: dist_coeffs must be the five coefficients k1 k2 p1 p2 k3")
    L = _lib.lib()
    mask = torch.empty(max(M, 1), dtype=torch.uint8, device=device)
    block, scratch = _host_block(device, L.lvdgs_pnp_scratch_bytes(M, max(int(hypotheses), 0)))
    a = _lib.PnpArgs(width=W1, height=H1, num_matches=M, hypotheses=int(hypotheses), min_inliers=int(min_inliers), seed=int(seed) & 0xFFFFFFFF,
                     fx=float(K[0]), fy=float(K[1]), cx=float(K[2]), cy=float(K[3]), dist=(C.c_double * 5)(*dist.tolist()),
                     reproj_error=float(reproj_error), depth=d.data_ptr(), matches_im1=m1.data_ptr(), matches_im2=m2.data_ptr(),
                     inlier_mask=mask.data_ptr(), host_state=block.data_ptr(), scratch=scratch.data_ptr(), scratch_bytes=scratch.numel())
    with _lib.on_device(device):
        _lib.check(L.lvdgs_pnp_ransac(C.byref(a), _lib.raw_stream(device)), "lvdgs_pnp_ransac")
        torch.cuda.current_stream(device).synchronize()      # the one wait of the call
    raw = block.numpy()
    w = raw[:4 * _lib.PNP_STATE_WORDS].view(np.int32).copy()
    rt = raw[4 * _lib.PNP_STATE_WORDS:].view(np.float64).copy().reshape(3, 4)
    last_call.status, last_call.valid_matches, last_call.inliers, last_call.hypothesis = int(w[0]), int(w[1]), int(w[2]), int(w[3])
    last_call.winner_count, last_call.reason, last_call.matches = int(w[4]), int(w[5]), M
    last_call.inlier_mask = mask[:M].bool()
    pose = np.eye(4)
    if last_call.status == _lib.PNP_OK:
        pose[:3, :] = rt
    elif last_call.status != _lib.PNP_FAILED:
        raise _lib.LvdgsError(f"lvdgs_pnp_ransac left no state (status word {last_call.status})")
    return pose, last_call.inlier_mask


def get_pose(img1, img2, model, dist_coeffs, viewpoint, gaussians, pipeline_params, background, *, matcher=None, hypotheses=128,
             reproj_error=5.0, seed=0, min_inliers=6, size=512):
    """The reference's ``get_pose`` (same positional signature) -> ``(pose_w2c, render_depth)``: the keyframe -> frame motion as a
    (4, 4) float64 NumPy array -- exactly ``np.eye(4)`` when the estimate fails, which is what the caller's
    ``allclose(rel_pose, identity)`` test looks for -- and the keyframe's depth rendered at the matcher's raster.

    Deviation: ``render_depth`` is the detached (1, H1, W1) tensor on its device; the map does not go to the host.
    ``viewpoint`` is the last keyframe (its pose, intrinsics and size); ``matcher(img1, img2, model, (W1, H1))`` supplies the matches."""
    if matcher is None:
        raise TypeError("get_pose: the `matcher` argument is required (the MASt3R matcher is out of scope: pass a callable "
                        "matcher(img1, img2, model, (W1, H1)) -> (matches_im1, matches_im2))")
    W, H = viewpoint.image_width, viewpoint.image_height
    W1, H1 = matcher_raster(W, H, size)
    matches_im1, matches_im2 = matcher(img1, img2, model, (W1, H1))
    with torch.no_grad():
        render_pkg = render_with_custom_resolution(viewpoint, gaussians, pipeline_params, background, target_width=W1, target_height=H1)
    render_depth = render_pkg["depth"].detach()
    scale_W, scale_H = W1 / W, H1 / H
    K = (viewpoint.fx * scale_W, viewpoint.fy * scale_H, viewpoint.cx * scale_W, viewpoint.cy * scale_H)
    pose_w2c, _ = pnp_ransac(render_depth, matches_im1, matches_im2, K, dist_coeffs, hypotheses=hypotheses, reproj_error=reproj_error, seed=seed,
                             min_inliers=min_inliers)
    return pose_w2c, render_depth
