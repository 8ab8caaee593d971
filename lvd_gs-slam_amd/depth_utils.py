"""Patch-based pointmap scale alignment of a keyframe's mono depth (LVD-GS Algorithm 1) on the GPU: ``process_depth``.

The reference scales every keyframe's monocular depth after the first to the map with ``utils/depth_utils.py::process_depth``
(called from ``add_new_keyframe``, utils/slam_frontend.py:1380-1405): the patches whose mean and spread agree between the rendered
depth and the scaled mono depth vote, pixel by pixel, for the scale; the result is the depth map the keyframe's Gaussians are seeded
from, and ``viewpoint.mono_depth *= scale_factor`` feeds the masked depth term of the mapping loss (utils/slam_backend.py:218-233).
Here every iteration is one HIP launch (``lvdgs_depth_align``, include/lvdgs.h): all of them and the fill are enqueued at once and
the host waits once per call.

The algorithm's fall-back ``find_scale`` (MASt3R correspondences to the previous keyframe) is out of scope: it is injectable as
``scale_remedy(im1, im2, last_depth, mono_depth, model) -> scale``.  Without one (or when it returns None), the remedy keeps the
current scale (the documented stand-in).  Whether the remedy branch was reached, and what it did, is recorded in ``last_call`` (and logged at INFO level).
"""
import ctypes as C
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

_resources = {}   # device index -> (pinned state words, scratch tensor)


def _state_and_scratch(device, nbytes):
    key = device.index
    hs, scratch = _resources.get(key, (None, None))
    if hs is None:
        hs = torch.zeros(_lib.DEPTH_ALIGN_STATE_WORDS, dtype=torch.int32).pin_memory()
    if scratch is None or scratch.numel() < nbytes:
        scratch = torch.zeros(max(int(nbytes), 256), dtype=torch.uint8, device=device)   # zero-filled once; every call leaves it so
    _resources[key] = (hs, scratch)
    return hs, scratch


def _read_state(hs):
    w = hs.numpy().copy()
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
    hs, scratch = _state_and_scratch(device, need)
    a = _lib.DepthAlignArgs(width=W, height=H, patch_size=int(patch_size), max_iter=int(max_iter), mean_threshold=float(mean_threshold),
                            std_threshold=float(std_threshold), error_threshold=float(error_threshold),
                            final_error_threshold=float(final_error_threshold), epsilon=float(epsilon),
                            min_accurate_pixels_ratio=float(min_accurate_pixels_ratio),
                            render_depth=r.data_ptr(), mono_depth=m.data_ptr(), final_depth=final.data_ptr(), error_mask=mask.data_ptr(),
                            host_state=hs.data_ptr(), scratch=scratch.data_ptr(), scratch_bytes=scratch.numel())
    with _lib.on_device(device):
        stream = _lib.raw_stream(device)
        _lib.check(L.lvdgs_depth_align(C.byref(a), stream), "lvdgs_depth_align")
        torch.cuda.current_stream(device).synchronize()      # the one wait of a call without the remedy
        st = _read_state(hs)
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
            _lib.check(L.lvdgs_depth_align_resume(C.byref(a), float(scale), stream), "lvdgs_depth_align_resume")
            torch.cuda.current_stream(device).synchronize()
            st = _read_state(hs)
        if not st.filled:
            raise _lib.LvdgsError(f"lvdgs_depth_align ended without its fill (status {st.status})")
    last_call.patch_num, last_call.status, last_call.iteration = st.patch_num, st.status, (st.k if max_iter > 0 else None)
    last_call.remedies, last_call.remedy_fired = remedies, bool(remedies)
    error_mask = mask.bool()
    if numpy_io:
        return final.cpu().numpy(), np.float32(st.s), error_mask.cpu().numpy(), int(st.num_accurate)
    return final, float(st.s), error_mask, int(st.num_accurate)
