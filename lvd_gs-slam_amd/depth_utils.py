"""Patch-based pointmap scale alignment of a keyframe's mono depth (LVD-GS Algorithm 1) on the GPU: ``process_depth``.

The reference scales every keyframe's monocular depth after the first to the map with ``utils/depth_utils.py::process_depth``
(called from ``add_new_keyframe``, utils/slam_frontend.py:1380-1405): the patches whose mean and spread agree between the rendered
depth and the scaled mono depth vote, pixel by pixel, for the scale; the result is the depth map the keyframe's Gaussians are seeded
from, and ``viewpoint.mono_depth *= scale_factor`` feeds the masked depth term of the mapping loss (utils/slam_backend.py:218-233).
Here every iteration is one HIP launch (``lvdgs_depth_align``, include/lvdgs.h): all of them and the fill are enqueued at once and
the host waits once per call.

The algorithm's fall-back, the scale remedy, is injectable as ``scale_remedy(im1, im2, last_depth, mono_depth, model) -> scale``.
The reference's is ``find_scale`` (utils/depth_utils.py:16-57: correspondences to the previous keyframe, both depth maps resized to
the matcher's raster, a ratio of means at the matches); here it is ``find_scale`` / ``MatchScaleRemedy(matcher)`` on
``scale_from_matches`` (one ``lvdgs_match_depth_scale`` call, include/lvdgs.h) -- only the descriptor network
behind the matcher is out of scope.  Without a remedy (or when it returns None), the current scale is kept (the documented
stand-in).  Whether the remedy branch was reached, and what it did, is recorded in ``last_call`` (and logged at INFO level).
"""
import logging
from types import SimpleNamespace

import numpy as np
import torch

from . import _lib

log = logging.getLogger(__name__)

# The record of the most recent call: patch_num (passing patches of the last iteration run, what the reference prints), status
# (_lib.DEPTH_ALIGN_*), iteration (the last iteration run), remedies ([(k, scale the remedy gave or None when there was no remedy
# and the scale was kept)], at most two: k = 2 and k = 3), remedy_fired (bool(remedies)).
last_call = SimpleNamespace(patch_num=0, status=None, iteration=None, remedies=[], remedy_fired=False)

# The record of the most recent ``scale_from_matches`` call: status (_lib.MATCH_SCALE_*), matches (M), valid (n), scale (float or None),
# sum1 / sum2 (the float64 sums of the two maps' samples over the valid matches).
last_scale = SimpleNamespace(status=None, matches=0, valid=0, scale=None, sum1=0.0, sum2=0.0)

# lvdgs_depth_align's block is a state that lvdgs_depth_align_resume reads on the host: no tag, never cleared; its scratch is zero-filled
# once and every call leaves it so
_align = _lib.HostCall("lvdgs_depth_align", tag=None, zeroed=True)
_scale = _lib.HostCall("lvdgs_match_depth_scale", statuses=(_lib.MATCH_SCALE_OK, _lib.MATCH_SCALE_NO_VALID))


def _read_state(words):
    w = words.copy()
    return SimpleNamespace(s=w[0:1].view(np.float32)[0], s_prev=w[1:2].view(np.float32)[0], status=int(w[2]), k=int(w[3]),
                           num_accurate=int(w[4]), patch_num=int(w[5]), count=int(w[6]), filled=int(w[7]))


def _as_map(x, name):
    """(H, W) or (1, H, W) -> (H, W)."""
    if x.ndim == 3 and x.shape[0] == 1:
        x = x[0]
    if x.ndim != 2:
        raise ValueError(f"process_depth: {name} must be (H, W) or (1, H, W), got {tuple(x.shape)}")
    return x


def process_depth(render_depth, mono_depth, last_depth=None, im1=None, im2=None, model=None, patch_size=10, mean_threshold=0.25,
                  std_threshold=0.3, error_threshold=0.1, final_error_threshold=0.15, max_iter=4, epsilon=0.01,
                  min_accurate_pixels_ratio=0.01, *, scale_remedy=None):
    """The reference's ``process_depth`` (same call signature) -> ``(final_depth, scale_factor, error_mask, num_accurate_pixels)``.

    NumPy maps in: NumPy out (float32 depth, bool mask, ``np.float32`` scale, int count), computed on the current GPU.  CUDA
    tensors in: tensors out on their device (float32 depth, bool mask), no host copy of a map; the scale is a Python float.
    ``last_depth``, ``im1``, ``im2``, ``model`` are handed to ``scale_remedy`` only."""
    numpy_io = not torch.is_tensor(render_depth)
    if numpy_io:
        device = torch.device("cuda", torch.cuda.current_device())
        r = torch.from_numpy(np.ascontiguousarray(_as_map(np.asarray(render_depth), "render_depth"), dtype=np.float32)).to(device)
        m = torch.from_numpy(np.ascontiguousarray(_as_map(np.asarray(mono_depth), "mono_depth"), dtype=np.float32)).to(device)
    else:
        if not render_depth.is_cuda:
            raise _lib.LvdgsError("process_depth: tensors must be on a GPU (there is no CPU path); NumPy arrays are accepted")
        device = render_depth.device
        r = _lib.f32(_as_map(render_depth, "render_depth"), device)
        m = _lib.f32(_as_map(torch.as_tensor(mono_depth), "mono_depth"), device)
    if r.shape != m.shape:
        raise ValueError(f"process_depth: render_depth {tuple(r.shape)} and mono_depth {tuple(m.shape)} differ")
    H, W = r.shape
    L = _lib.lib()
    final = torch.empty((H, W), dtype=torch.float32, device=device)
    mask = torch.empty((H, W), dtype=torch.uint8, device=device)
    need = L.lvdgs_depth_align_scratch_bytes(W, H, max(int(patch_size), 1))
    hs, scratch = _align.resources(device, 4 * _lib.DEPTH_ALIGN_STATE_WORDS, need)
    a = _lib.DepthAlignArgs(width=W, height=H, patch_size=int(patch_size), max_iter=int(max_iter), mean_threshold=float(mean_threshold),
                            std_threshold=float(std_threshold), error_threshold=float(error_threshold),
                            final_error_threshold=float(final_error_threshold), epsilon=float(epsilon),
                            min_accurate_pixels_ratio=float(min_accurate_pixels_ratio),
                            render_depth=r.data_ptr(), mono_depth=m.data_ptr(), final_depth=final.data_ptr(), error_mask=mask.data_ptr(),
                            host_state=hs.data_ptr(), scratch=scratch.data_ptr(), scratch_bytes=scratch.numel())
    with _lib.on_device(device):
        st = _read_state(_align.run(device, a))      # the one wait of a call without the remedy
        remedies = []     # (k, scale given by the remedy or None)
        while st.status == _lib.DEPTH_ALIGN_REMEDY and len(remedies) < 2:
            given = None if scale_remedy is None else scale_remedy(im1, im2, last_depth, mono_depth, model)
            if given is not None:
                given = float(given)
                scale = np.float32(given)
            else:
                scale = st.s      # stand-in: keep the current scale
            remedies.append((st.k, given))
            log.info("process_depth: %d accurate pixels at iteration %d (< %d): scale remedy %s", st.count, st.k,
                     int(min_accurate_pixels_ratio * H * W), "applied" if given is not None else "absent, scale kept")
            st = _read_state(_align.run(device, a, lambda args, stream: L.lvdgs_depth_align_resume(args, float(scale), stream)))
        if not st.filled:
            raise _lib.LvdgsError(f"lvdgs_depth_align ended without its fill (status {st.status})")
    last_call.patch_num, last_call.status, last_call.iteration = st.patch_num, st.status, (st.k if max_iter > 0 else None)
    last_call.remedies, last_call.remedy_fired = remedies, bool(remedies)
    error_mask = mask.bool()
    if numpy_io:
        return final.cpu().numpy(), np.float32(st.s), error_mask.cpu().numpy(), int(st.num_accurate)
    return final, float(st.s), error_mask, int(st.num_accurate)


def _device_map(x, device, name):
    """A depth map, NumPy or tensor, (H, W) or (1, H, W) -> contiguous float32 (H, W) on ``device``."""
    if not torch.is_tensor(x):
        x = torch.from_numpy(np.ascontiguousarray(np.asarray(x), dtype=np.float32))
    if x.ndim == 3 and x.shape[0] == 1:
        x = x[0]
    if x.ndim != 2 or min(x.shape) < 1:
        raise ValueError(f"scale_from_matches: {name} must be a non-empty (H, W) or (1, H, W) map, got {tuple(x.shape)}")
    return _lib.f32(x, device)


def scale_from_matches(matches_im1, matches_im2, depth1, depth2, raster):
    """``find_scale``'s arithmetic (utils/depth_utils.py:31-55), one ``lvdgs_match_depth_scale`` call: the ratio of the mean of ``depth1``
    at the map-1 pixels to the mean of ``depth2`` at the map-2 pixels of the matches, each map sampled as if resized bilinearly to
    ``raster`` = (W1, H1), over the matches where both samples are finite and > 0 -> float, or None when no match is valid.  The matches
    are what ``reciprocal_matches`` returns, tensors on a GPU ((M, 2), (x, y); NumPy arrays are uploaded); the depth maps NumPy or
    tensors.  One launch, one host wait; the counts go to ``last_scale``."""
    if torch.is_tensor(matches_im1) and matches_im1.is_cuda:
        device = matches_im1.device
    elif torch.is_tensor(depth1) and depth1.is_cuda:
        device = depth1.device
    else:
        device = torch.device("cuda", torch.cuda.current_device())
    m1 = torch.as_tensor(np.asarray(matches_im1) if not torch.is_tensor(matches_im1) else matches_im1).reshape(-1, 2)
    m2 = torch.as_tensor(np.asarray(matches_im2) if not torch.is_tensor(matches_im2) else matches_im2).reshape(-1, 2)
    if m1.shape != m2.shape:
        raise ValueError(f"scale_from_matches: matches_im1 {tuple(m1.shape)} and matches_im2 {tuple(m2.shape)} differ")
    m1 = m1.to(device=device, dtype=torch.int32).contiguous()
    m2 = m2.to(device=device, dtype=torch.float32).contiguous()
    d1, d2 = _device_map(depth1, device, "depth1"), _device_map(depth2, device, "depth2")
    W1, H1 = int(raster[0]), int(raster[1])
    block, _ = _scale.resources(device, _lib.MATCH_SCALE_HOST_BYTES)
    M = int(m1.shape[0])
    a = _lib.MatchScaleArgs(num_matches=M, raster_width=W1, raster_height=H1, width1=d1.shape[1], height1=d1.shape[0], width2=d2.shape[1],
                            height2=d2.shape[0], matches_im1=m1.data_ptr() if M else None, matches_im2=m2.data_ptr() if M else None,
                            depth1=d1.data_ptr(), depth2=d2.data_ptr(), host_state=block.data_ptr())
    w = _scale.run(device, a).copy()      # the one wait of the call
    sums = w[_lib.MATCH_SCALE_STATE_WORDS:_lib.MATCH_SCALE_STATE_WORDS + 4].view(np.float64)
    status = int(w[0])
    scale = float(w[3:4].view(np.float32)[0]) if status == _lib.MATCH_SCALE_OK else None
    last_scale.status, last_scale.matches, last_scale.valid, last_scale.scale = status, int(w[1]), int(w[2]), scale
    last_scale.sum1, last_scale.sum2 = float(sums[0]), float(sums[1])
    return scale


def find_scale(im1, im2, depth1, depth2, model, *, matcher=None):
    """The reference's ``find_scale`` (same positional signature; utils/depth_utils.py:16-57) -> the scale between ``depth1`` (the
    previous keyframe's) and ``depth2`` (this keyframe's), or None when no match is valid.  ``matcher(im1, im2, model, (W1, H1)) ->
    (matches_im1, matches_im2)`` at the matcher's raster of ``im1`` -- ``init_pose.DescriptorMatcher(describe)``; then
    ``scale_from_matches``."""
    if matcher is None:
        raise TypeError("find_scale: the `matcher` argument is required (only the descriptor network is out of scope: pass "
                        "init_pose.DescriptorMatcher(describe), or any callable matcher(im1, im2, model, (W1, H1)) -> (matches_im1, matches_im2))")
    from .init_pose import matcher_raster
    raster = matcher_raster(int(im1.shape[2]), int(im1.shape[1]))
    matches_im1, matches_im2 = matcher(im1, im2, model, raster)
    return scale_from_matches(matches_im1, matches_im2, depth1, depth2, raster)


class MatchScaleRemedy:
    """``process_depth``'s ``scale_remedy(im1, im2, last_depth, mono_depth, model)`` as the reference has it: ``find_scale`` on the
    matches of ``matcher``.  ``set_frames`` goes on to a matcher that has it.  ``calls`` (None: nothing is kept; ``record`` or an
    assigned list: kept) gets a dict per call: matches_im1, matches_im2 (on their device), raster, depth1, depth2 (as given), scale."""

    def __init__(self, matcher, record=False):
        self.matcher, self.calls = matcher, ([] if record else None)

    def set_frames(self, keyframe_idx, frame_idx):
        if hasattr(self.matcher, "set_frames"):
            self.matcher.set_frames(keyframe_idx, frame_idx)

    def _matcher(self, im1, im2, model, raster):
        m1, m2 = self.matcher(im1, im2, model, raster)
        self._last = dict(matches_im1=m1, matches_im2=m2, raster=raster)
        return m1, m2

    def __call__(self, im1, im2, last_depth, mono_depth, model):
        scale = find_scale(im1, im2, last_depth, mono_depth, model, matcher=self._matcher)
        if self.calls is not None:
            self.calls.append(dict(self._last, depth1=last_depth, depth2=mono_depth, scale=scale))
        return scale
