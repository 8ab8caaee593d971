"""Seeding a keyframe's Gaussians as one library call (HIP, ``csrc/seeding.hip``; semantics: ``include/lvdgs.h``, DESIGN.md
section "Seeding").

``seed_points``  what ``GaussianModel.create_pcd_from_image_and_depth`` does between ``valid = ...`` and ``colors = ...`` -- the
                 validity test, the subsample, the back-projection into the world and the colours through 8 bits -- and the
                 ``depth.median()`` of ``adaptive_pointsize``, in one call that ends in ONE wait on a block of pinned host memory.
``call_seed``    the per-call seed: a SplitMix64 step of ``seed_base + calls``.

The subsample is a pure function of (seed, pixel index, validity): the pixels whose 32-bit hash keys are the
``int(n_valid * (1.0 / downsample))`` smallest among the valid pixels.  No generator state: every replica that makes the same calls
selects the same pixels.  It is NOT the subset ``numpy.random.Generator.choice`` draws, hence ``GaussianModel.seeding = "fused"`` is
opt-in.
"""
import numpy as np
import torch

from . import _lib

_call = _lib.HostCall("lvdgs_seed_points", tag=_lib.SEED_SEQ)
_MASK64 = (1 << 64) - 1


def call_seed(seed_base, calls):
    """SplitMix64's output for the state ``seed_base + calls`` (mod 2^64): the seed of a model's ``calls``-th fused seeding call."""
    z = (int(seed_base) + int(calls) + 0x9E3779B97F4A7C15) & _MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _MASK64
    return z ^ (z >> 31)


class SeedPoints:
    """What one ``lvdgs_seed_points`` call leaves.  ``xyz``, ``rgb``, ``f_dc`` (n, 3) float32 and ``pixel`` (n,) int32 -- views of
    buffers sized for the call's capacity, rows in ascending pixel index; ``rgb`` / ``f_dc`` are None without an image --, ``n`` (rows),
    ``n_valid`` (valid depth pixels), ``median_depth`` / ``median_bits`` (the lower median of all depth values; NaN / the quiet NaN's
    bits when not asked for)."""
    __slots__ = ("xyz", "rgb", "f_dc", "pixel", "n", "n_valid", "median_depth", "median_bits", "threshold")


def _scalar(value, device, name):
    """``gain`` / ``offset`` as one float32 on ``device`` (None stays None: the library's 1 and 0)."""
    if value is None:
        return None
    if not torch.is_tensor(value):
        return torch.tensor([float(value)], dtype=torch.float32, device=device)
    if value.numel() != 1:
        raise _lib.LvdgsError(f"seed_points: {name} must hold one value")
    return _lib.f32(value, device).reshape(1)


def seed_points(image, depth, intrinsics, R, T, downsample, seed, *, gain=None, offset=None, depth_trunc=100.0, want_median=False) -> SeedPoints:
    """One ``lvdgs_seed_points`` call and one wait.

    ``image``: (3, H, W) float32 on the depth's GPU, or None (no colours); ``depth``: (H, W) float32 on a GPU; ``intrinsics``:
    (fx, fy, cx, cy); ``R`` (3, 3), ``T`` (3,): the camera's ``p_cam = R p_world + T``; ``downsample``: one seed per this many valid
    pixels (>= 1); ``seed``: 64 bits (``call_seed``); ``gain`` / ``offset``: the exposure's ``exp(a)`` and ``b``, tensors of one
    element or numbers."""
    if not _lib.is_f32(depth) or depth.ndim != 2:
        raise _lib.LvdgsError("seed_points: depth must be a contiguous (H, W) float32 tensor on a GPU (there is no CPU path)")
    device = depth.device
    H, W = depth.shape
    if image is not None and (not _lib.is_f32(image, device) or tuple(image.shape) != (3, H, W)):
        raise _lib.LvdgsError("seed_points: image must be a contiguous (3, H, W) float32 tensor of the depth's size on its device")
    inv = 1.0 / downsample
    R = _lib.f32(R, device)
    T = _lib.f32(T, device)
    if R.numel() != 9 or T.numel() != 3:
        raise _lib.LvdgsError("seed_points: R must be (3, 3) and T (3,)")
    gain, offset = _scalar(gain, device, "gain"), _scalar(offset, device, "offset")
    fx, fy, cx, cy = (float(v) for v in intrinsics)
    capacity = max(int(H * W * inv), 0)

    L = _lib.lib()
    block, scratch = _call.resources(device, _lib.SEED_HOST_BYTES, L.lvdgs_seed_scratch_bytes(W, H))
    out = SeedPoints()
    rows = max(capacity, 1)
    xyz = torch.empty((rows, 3), dtype=torch.float32, device=device)
    rgb = torch.empty((rows, 3), dtype=torch.float32, device=device) if image is not None else None
    f_dc = torch.empty((rows, 3), dtype=torch.float32, device=device) if image is not None else None
    pixel = torch.empty(rows, dtype=torch.int32, device=device)
    a = _lib.SeedArgs(width=W, height=H, fx=fx, fy=fy, cx=cx, cy=cy, depth_trunc=float(depth_trunc), want_median=int(bool(want_median)),
                      inv_downsample=inv, seed=int(seed) & _MASK64, capacity=capacity,
                      image=None if image is None else image.data_ptr(), gain=None if gain is None else gain.data_ptr(),
                      offset=None if offset is None else offset.data_ptr(), depth=depth.data_ptr(), R=R.data_ptr(), T=T.data_ptr(),
                      xyz=xyz.data_ptr(), rgb=None if rgb is None else rgb.data_ptr(), f_dc=None if f_dc is None else f_dc.data_ptr(),
                      pixel=pixel.data_ptr(), host_state=block.data_ptr(), scratch=scratch.data_ptr(), scratch_bytes=scratch.numel())
    w = _call.run(device, a).copy()      # the one wait of the call
    out.n_valid, out.n = int(w[_lib.SEED_N_VALID]), int(w[_lib.SEED_N_KEEP])
    out.median_bits = int(w[_lib.SEED_MEDIAN]) & 0xFFFFFFFF
    out.median_depth = float(w[_lib.SEED_MEDIAN:_lib.SEED_MEDIAN + 1].view(np.float32)[0])
    out.threshold = int(w[_lib.SEED_THRESHOLD]) & 0xFFFFFFFF
    n = out.n
    out.xyz, out.pixel = xyz[:n], pixel[:n]
    out.rgb = None if rgb is None else rgb[:n]
    out.f_dc = None if f_dc is None else f_dc[:n]
    return out
