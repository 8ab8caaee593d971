"""Test helper: the argument block of a forward call of the raw C ABI (include/lvdgs.h) with buffers of its own, for the tests that
drive ``lvdgs_forward`` / ``lvdgs_forward_batch`` / ``lvdgs_forward_prepare`` + ``lvdgs_forward_render`` through ctypes."""
import ctypes as C

import numpy as np
import torch

from lvdgs import _lib


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def forward_view(L, t, cam, W, H, bgd, cap):
    """(lvdgs_args, st) of one view of the map ``t`` (dict of contiguous float32 device tensors: means3D, opacities, scales, rotations,
    colors) seen by ``cam``, with a pair capacity of ``cap``.  ``st`` holds the view's buffers -- radii, n_touched, color, depth, opacity,
    geom, image, binning, scratch, ALL ZERO-FILLED, and the camera's matrices under "mats" -- and must outlive the calls."""
    dev = t["means3D"].device
    N = t["means3D"].shape[0]
    buf = lambda n: torch.zeros(max(int(n), 256), dtype=torch.uint8, device=dev)
    mats = {n: getattr(cam, n).to(dev).contiguous() for n in ("world_view_transform", "full_proj_transform", "projection_matrix", "camera_center")}
    a = _lib.Args()
    a.image_height, a.image_width, a.tanfovx, a.tanfovy = H, W, cam.tanfovx, cam.tanfovy
    a.scale_modifier, a.sh_degree = 1.0, 0
    a.bg, a.viewmatrix, a.projmatrix = _p(bgd), _p(mats["world_view_transform"]), _p(mats["full_proj_transform"])
    a.projmatrix_raw, a.campos = _p(mats["projection_matrix"]), _p(mats["camera_center"])
    a.num_gaussians, a.sh_coeffs = N, 0
    a.means3D, a.opacities, a.scales, a.rotations, a.colors_precomp = _p(t["means3D"]), _p(t["opacities"]), _p(t["scales"]), _p(t["rotations"]), _p(t["colors"])
    st = dict(radii=torch.zeros(N, dtype=torch.int32, device=dev), n_touched=torch.zeros(N, dtype=torch.int32, device=dev),
              color=torch.zeros(3, H, W, device=dev), depth=torch.zeros(1, H, W, device=dev), opacity=torch.zeros(1, H, W, device=dev),
              geom=buf(L.lvdgs_geom_bytes(N)), image=buf(L.lvdgs_image_bytes(W, H)), binning=buf(L.lvdgs_binning_bytes(cap)),
              scratch=buf(max(L.lvdgs_prepare_scratch_bytes(N), L.lvdgs_render_scratch_bytes(N, cap, W, H))), mats=mats)
    a.radii, a.n_touched, a.out_color, a.out_depth, a.out_opacity = _p(st["radii"]), _p(st["n_touched"]), _p(st["color"]), _p(st["depth"]), _p(st["opacity"])
    a.geom_state, a.geom_bytes, a.image_state, a.image_bytes = _p(st["geom"]), st["geom"].numel(), _p(st["image"]), st["image"].numel()
    a.binning_state, a.binning_bytes, a.scratch, a.scratch_bytes = _p(st["binning"]), st["binning"].numel(), _p(st["scratch"]), st["scratch"].numel()
    a.pair_capacity = cap
    return a, st


def read_lists(L, st, N, cap, W, H, D):
    """(tiles_touched (N,), ranges (T, 2), point_list[:D]) of a view's state buffers, as NumPy arrays; ``cap``: what binning_state was
    sized for (its layout goes by its size)."""
    lay = _lib.StateLayout()
    _lib.check(L.lvdgs_state_layout_query(N, cap, W, H, C.byref(lay)), "lvdgs_state_layout_query")
    T = ((W + 15) // 16) * ((H + 15) // 16)
    view = lambda b, off, n, dt: b[off:off + n * np.dtype(dt).itemsize].cpu().numpy().view(dt).copy()
    return (view(st["geom"], lay.geom_tiles_touched, N, np.uint32), view(st["image"], lay.img_ranges, 2 * T, np.uint32).reshape(T, 2),
            view(st["binning"], lay.bin_point_list, D, np.uint32))
