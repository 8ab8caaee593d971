"""The initial pose estimate of a tracked frame: PnP-RANSAC of 2D-2D matches against the last keyframe's rendered depth, on the GPU.

The reference starts every frame's pose optimisation from ``get_pose`` (utils/init_pose.py:123-186, called from ``FrontEnd.tracking``,
utils/slam_frontend.py:1448): it renders the last keyframe's depth at the matcher's raster, copies it to the host, back-projects every
pixel (``depth_to_3d`` with ``cv2.undistortPoints``), and solves ``cv2.solvePnPRansac`` against the matched pixels of the new frame.
Here the depth stays on its device and the gather, the hypotheses, the consensus and the refinement are one ``lvdgs_pnp_ransac``
call (include/lvdgs.h states the semantics): two launches, one host wait.

The matches come from ``matcher(img1, img2, model, (W1, H1)) -> (matches_im1, matches_im2)`` -- (M, 2) pixel coordinates (x, y) at
the raster ``(W1, H1)``, integers in the keyframe and floats in the new frame, NumPy arrays or tensors.  The reference's matcher is
MASt3R descriptors + ``fast_reciprocal_NNs(desc1, desc2, subsample_or_initxy1=8, dist='dot')``.  Only the network that makes the
descriptors is out of scope; the matching is ``reciprocal_matches`` (one ``lvdgs_reciprocal_nn`` call: include/lvdgs.h, DESIGN.md
section 4d), and ``DescriptorMatcher(describe)`` is the matcher built on it -- ``describe`` is the network's seat.  With it everything
between two descriptor maps and the initial pose runs on the device, and the matches never visit the host.

What the reference does around the network is here too: ``torch_images_to_dust3r_format`` / ``format_image``
(one ``lvdgs_format_image`` call per frame: PIL's 8-bit resize, crop and normalisation bit for bit, without the frame's trip to the
host), ``get_depth`` (the pointmap's z resized by nearest neighbour, on the device), and ``NetworkDescribe(infer)``, the ``describe``
whose seat is exactly the reference's ``inference(model)``: formatted views in, ``desc`` / ``pts3d`` out.
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

# The record of the most recent ``reciprocal_matches`` call: seeds, matches (M), unconverged (seeds still active after max_iter rounds,
# dropped), rounds (those that began with an active seed), seed_state ((seeds, 3) int32 device tensor of every seed's final flat xy1, xy2
# and converged flag when the call asked for it, else None).
last_match = SimpleNamespace(seeds=0, matches=0, unconverged=0, rounds=0, seed_state=None)

_pnp = _lib.HostCall("lvdgs_pnp_ransac", statuses=(_lib.PNP_OK, _lib.PNP_FAILED))
_match = _lib.HostCall("lvdgs_reciprocal_nn", statuses=(_lib.RNN_OK,))
_format_tables = {}     # (device index, W, H, size) -> (plan, table_x, table_y device tensors): made once per image size and device
_format_scratch = _lib.DeviceScratch()


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
    block, scratch = _pnp.resources(device, _lib.PNP_HOST_BYTES, L.lvdgs_pnp_scratch_bytes(M, max(int(hypotheses), 0)))
    a = _lib.PnpArgs(width=W1, height=H1, num_matches=M, hypotheses=int(hypotheses), min_inliers=int(min_inliers), seed=int(seed) & 0xFFFFFFFF,
                     fx=float(K[0]), fy=float(K[1]), cx=float(K[2]), cy=float(K[3]), dist=(C.c_double * 5)(*dist.tolist()),
                     reproj_error=float(reproj_error), depth=d.data_ptr(), matches_im1=m1.data_ptr(), matches_im2=m2.data_ptr(),
                     inlier_mask=mask.data_ptr(), host_state=block.data_ptr(), scratch=scratch.data_ptr(), scratch_bytes=scratch.numel())
    w = _pnp.run(device, a).copy()      # the one wait of the call
    rt = w[_lib.PNP_STATE_WORDS:_lib.PNP_STATE_WORDS + 24].view(np.float64).reshape(3, 4)
    last_call.status, last_call.valid_matches, last_call.inliers, last_call.hypothesis = int(w[0]), int(w[1]), int(w[2]), int(w[3])
    last_call.winner_count, last_call.reason, last_call.matches = int(w[4]), int(w[5]), M
    last_call.inlier_mask = mask[:M].bool()
    pose = np.eye(4)
    if last_call.status == _lib.PNP_OK:
        pose[:3, :] = rt
    return pose, last_call.inlier_mask


def reciprocal_matches(desc1, desc2, subsample=8, max_iter=10, seed_state=False):
    """Reciprocal nearest neighbours of two descriptor maps under the dot product (``fast_reciprocal_NNs(desc1, desc2,
    subsample_or_initxy1=subsample, dist='dot')`` as include/lvdgs.h restates it), one ``lvdgs_reciprocal_nn`` call.  ``desc1``: (H1, W1, D),
    ``desc2``: (H2, W2, D) tensors on a GPU.  -> ``(matches_im1 (M, 2) int32, matches_im2 (M, 2) float32)``, pixel coordinates (x, y), on
    that device, sorted by map-1 pixel (row-major), distinct -- what ``pnp_ransac`` takes.  One host wait, to learn M; the counts go to
    ``last_match``."""
    if not torch.is_tensor(desc1) or not torch.is_tensor(desc2):
        raise _lib.LvdgsError("reciprocal_matches: the descriptor maps must be tensors on a GPU (there is no CPU path)")
    if desc1.ndim != 3 or desc2.ndim != 3:
        raise ValueError(f"reciprocal_matches: the maps must be (H, W, D), got {tuple(desc1.shape)} and {tuple(desc2.shape)}")
    if desc1.shape[2] != desc2.shape[2]:
        raise ValueError(f"reciprocal_matches: the maps differ in descriptor size ({desc1.shape[2]} and {desc2.shape[2]})")
    if min(desc1.shape) < 1 or min(desc2.shape) < 1:
        raise ValueError(f"reciprocal_matches: an empty map ({tuple(desc1.shape)} and {tuple(desc2.shape)})")
    if not desc1.is_cuda or not desc2.is_cuda:
        raise _lib.LvdgsError("reciprocal_matches: the descriptor maps must be tensors on a GPU (there is no CPU path)")
    device = desc1.device
    if desc2.device != device:
        raise ValueError(f"reciprocal_matches: the maps are on different devices ({device} and {desc2.device})")
    d1, d2 = _lib.f32(desc1, device), _lib.f32(desc2, device)
    (H1, W1, D), (H2, W2, _) = d1.shape, d2.shape
    S = int(subsample)
    seeds = len(range(S // 2, H1, S)) * len(range(S // 2, W1, S)) if S >= 1 else 0
    L = _lib.lib()
    need = L.lvdgs_recip_nn_scratch_bytes(W1, H1, S) if S >= 1 else 0
    block, scratch = _match.resources(device, 4 * _lib.RNN_STATE_WORDS, need)
    cap = max(seeds, 1)
    m1 = torch.empty((cap, 2), dtype=torch.int32, device=device)
    m2 = torch.empty((cap, 2), dtype=torch.float32, device=device)
    state = torch.empty((cap, 3), dtype=torch.int32, device=device) if seed_state else None
    a = _lib.RecipNnArgs(width1=W1, height1=H1, width2=W2, height2=H2, dim=D, subsample=S, max_iter=int(max_iter), capacity=cap,
                         desc1=d1.data_ptr(), desc2=d2.data_ptr(), matches_im1=m1.data_ptr(), matches_im2=m2.data_ptr(),
                         seed_state=None if state is None else state.data_ptr(), host_state=block.data_ptr(), scratch=scratch.data_ptr(),
                         scratch_bytes=scratch.numel())
    w = _match.run(device, a).copy()      # the one wait of the call
    last_match.seeds, last_match.matches, last_match.unconverged, last_match.rounds = int(w[1]), int(w[2]), int(w[3]), int(w[4])
    last_match.seed_state = None if state is None else state[:last_match.seeds]
    return m1[:last_match.matches], m2[:last_match.matches]


def _format_plan(device, W, H, size):
    key = (device.index, W, H, size)
    hit = _format_tables.get(key)
    if hit is None:
        L = _lib.lib()
        p = _lib.FormatPlan()
        _lib.check(L.lvdgs_format_plan_query(W, H, size, C.byref(p)), "lvdgs_format_plan_query")
        tables = []
        for n_in, n_out, first, count, taps in ((W, p.resized_width, p.crop_x, p.out_width, p.taps_x),
                                                (H, p.resized_height, p.crop_y, p.out_height, p.taps_y)):
            t = np.zeros((count, 2 + taps), dtype=np.int32)
            _lib.check(L.lvdgs_format_table(n_in, n_out, p.filter, first, count, t.ctypes.data), "lvdgs_format_table")
            tables.append(torch.from_numpy(t).to(device))
        hit = _format_tables[key] = (p, tables[0], tables[1])
    return hit


def format_image(img, size=512, *, quantised=False):
    """The matcher's formatting of one frame (``torch_images_to_dust3r_format``'s loop body, utils/init_pose.py:49-72), one
    ``lvdgs_format_image`` call: ``img`` (3, H, W) float tensor on a GPU -> (1, 3, H1, W1) float32, contiguous, on that device, with
    (W1, H1) = ``matcher_raster(W, H, size)`` -- the bits PIL and torchvision give.  ``quantised=True``: the cropped uint8 image
    (H1, W1, 3) before the normalisation instead.  No host wait and no device-to-host copy (the coefficient tables of an image size are
    made on the host and uploaded once per device)."""
    if not torch.is_tensor(img) or not img.is_cuda:
        raise _lib.LvdgsError("format_image: the image must be a tensor on a GPU (there is no CPU path)")
    if img.ndim != 3 or img.shape[0] != 3:
        raise ValueError(f"format_image: the image must be (3, H, W), got {tuple(img.shape)}")
    device = img.device
    x = _lib.f32(img, device)
    H, W = int(x.shape[1]), int(x.shape[2])
    p, table_x, table_y = _format_plan(device, W, H, int(size))
    L = _lib.lib()
    scratch = _format_scratch.get(device, L.lvdgs_format_scratch_bytes(W, H, int(size)))
    out = torch.empty((1, 3, p.out_height, p.out_width), dtype=torch.float32, device=device)
    q = torch.empty((p.out_height, p.out_width, 3), dtype=torch.uint8, device=device) if quantised else None
    a = _lib.FormatImageArgs(width=W, height=H, size=int(size), image=x.data_ptr(), table_x=table_x.data_ptr(), table_y=table_y.data_ptr(),
                             out=out.data_ptr(), quantised=None if q is None else q.data_ptr(), scratch=scratch.data_ptr(),
                             scratch_bytes=scratch.numel())
    with _lib.on_device(device):
        _lib.check(L.lvdgs_format_image(C.byref(a), _lib.raw_stream(device)), "lvdgs_format_image")
    return q if quantised else out


def torch_images_to_dust3r_format(tensor_images, size, square_ok=False, verbose=False):
    """The reference's function (same signature; utils/init_pose.py:35-75) -> its list of dicts ``img`` (1, 3, H1, W1), ``true_shape`` =
    ``np.int32([[H1, W1]])``, ``idx``, ``instance``.  Deviation: ``img`` is a tensor on the images' device -- the frames never visit the
    host.  ``square_ok=True`` (a square image kept square) is not supported: the reference never passes it."""
    if square_ok:
        raise ValueError("torch_images_to_dust3r_format: square_ok=True is not supported")
    imgs = []
    for idx, image in enumerate(tensor_images):
        img = format_image(image, size)
        imgs.append(dict(img=img, true_shape=np.int32([[img.shape[2], img.shape[3]]]), idx=idx, instance=str(idx)))
    assert imgs, "no images found"
    return imgs


class NetworkDescribe:
    """A ``describe`` for ``DescriptorMatcher`` whose seat is the network alone: both images are formatted on the device
    (``torch_images_to_dust3r_format``), ``infer(view1, view2, model) -> (pred1, pred2)`` is the reference's ``inference`` -- dicts with
    ``desc`` (1, H1, W1, D) (and ``pts3d`` (1, H1, W1, 3)) -- and the two (H1, W1, D) descriptor maps come back, checked against the
    raster the matcher was given."""

    def __init__(self, infer, size=512):
        self.infer, self.size = infer, int(size)

    def set_frames(self, keyframe_idx, frame_idx):
        if hasattr(self.infer, "set_frames"):
            self.infer.set_frames(keyframe_idx, frame_idx)

    def __call__(self, img1, img2, model, raster):
        view1, view2 = torch_images_to_dust3r_format([img1, img2], size=self.size)
        pred1, pred2 = self.infer(view1, view2, model)
        W1, H1 = raster
        maps = []
        for pred in (pred1, pred2):
            desc = pred["desc"]
            if desc.ndim != 4 or desc.shape[0] != 1 or tuple(desc.shape[1:3]) != (H1, W1):
                raise ValueError(f"NetworkDescribe: the network's descriptors are {tuple(desc.shape)}, not (1, {H1}, {W1}, D)")
            maps.append(desc[0].detach())
        return maps[0], maps[1]


def get_depth(img1, img2, model, *, infer=None, size=512):
    """The reference's ``get_depth`` (same positional signature; utils/init_pose.py:189-208): the z of the network's pointmap of ``img1``,
    resized to the frame's (H, W) by ``cv2.INTER_NEAREST``'s rule -- source index ``min(floor(d * n_src / n_dst), n_src - 1)`` -- as plain
    device indexing.  ``infer`` as in ``NetworkDescribe``.  Deviation: the result is a float32 tensor on the images' device, not NumPy."""
    if infer is None:
        raise TypeError("get_depth: the `infer` argument is required (the network is out of scope: infer(view1, view2, model) -> (pred1, pred2))")
    H, W = int(img1.shape[1]), int(img1.shape[2])
    view1, view2 = torch_images_to_dust3r_format([img1, img2], size=size)
    pred1, _ = infer(view1, view2, model)
    z = pred1["pts3d"][0][..., 2].detach()
    Hs, Ws = int(z.shape[0]), int(z.shape[1])
    # (integer arithmetic: floor(d * n_src / n_dst) of the float64 rule, exactly)
    sx = torch.clamp(torch.arange(W, device=z.device, dtype=torch.int64) * Ws // W, max=Ws - 1)
    sy = torch.clamp(torch.arange(H, device=z.device, dtype=torch.int64) * Hs // H, max=Hs - 1)
    return z.index_select(0, sy).index_select(1, sx).to(torch.float32).contiguous()


class DescriptorMatcher:
    """The matcher of ``get_pose`` on descriptor maps: ``describe(img1, img2, model, (W1, H1)) -> (desc1, desc2)`` -- the network's seat
    (``NetworkDescribe(infer)`` narrows it to the network alone -- MASt3R in the reference, out of scope; ``synthetic.WorldDescriptors``
    is the stand-in), (H1, W1, D) tensors on a GPU at the matcher's raster -- followed by ``reciprocal_matches``.  ``set_frames`` goes on to a ``describe`` that has it."""

    def __init__(self, describe, subsample=8, max_iter=10):
        self.describe, self.subsample, self.max_iter = describe, int(subsample), int(max_iter)

    def set_frames(self, keyframe_idx, frame_idx):
        if hasattr(self.describe, "set_frames"):
            self.describe.set_frames(keyframe_idx, frame_idx)

    def __call__(self, img1, img2, model, raster):
        desc1, desc2 = self.describe(img1, img2, model, raster)
        return reciprocal_matches(desc1, desc2, subsample=self.subsample, max_iter=self.max_iter)


def get_pose(img1, img2, model, dist_coeffs, viewpoint, gaussians, pipeline_params, background, *, matcher=None, hypotheses=128,
             reproj_error=5.0, seed=0, min_inliers=6, size=512):
    """The reference's ``get_pose`` (same positional signature) -> ``(pose_w2c, render_depth)``: the keyframe -> frame motion as a
    (4, 4) float64 NumPy array -- exactly ``np.eye(4)`` when the estimate fails, which is what the caller's
    ``allclose(rel_pose, identity)`` test looks for -- and the keyframe's depth rendered at the matcher's raster.

    Deviation: ``render_depth`` is the detached (1, H1, W1) tensor on its device; the map does not go to the host.
    ``viewpoint`` is the last keyframe (its pose, intrinsics and size); ``matcher(img1, img2, model, (W1, H1))`` supplies the matches:
    ``DescriptorMatcher(describe)`` is the supplied one (descriptor maps -> ``reciprocal_matches``, on the device)."""
    if matcher is None:
        raise TypeError("get_pose: the `matcher` argument is required (only the descriptor network is out of scope: pass "
                        "DescriptorMatcher(describe), or any callable matcher(img1, img2, model, (W1, H1)) -> (matches_im1, matches_im2))")
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
