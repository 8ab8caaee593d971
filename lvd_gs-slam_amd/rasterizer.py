"""Autograd boundary of the rasterizer: ``GaussianRasterizationSettings`` / ``GaussianRasterizer``.

Same names, argument lists and return values as the ``diff_gaussian_rasterization`` module the
reference's ``gaussian_splatting.gaussian_renderer.render`` is written against (reference
README.md:43; the module itself is absent from the reference checkout, so the signature is the
published MonoGS one -- SURVEY.md section 8(b)):

    GaussianRasterizer(raster_settings)(means3D, means2D, opacities, shs=None, colors_precomp=None,
                                        scales=None, rotations=None, cov3D_precomp=None,
                                        theta=None, rho=None)
        -> color (3,H,W), radii (N,) int32, depth (1,H,W), opacity (1,H,W), n_touched (N,) int32

Gradients flow to means3D, means2D (the "viewspace points": d/d NDC xy), shs or colors_precomp,
opacities, scales, rotations or cov3D_precomp, and to ``theta`` / ``rho`` -- the camera's
``cam_rot_delta`` / ``cam_trans_delta`` (reference utils/camera_utils.py:51-56), i.e. the left
SE(3) perturbation that ``utils/pose_utils.py:70-87`` later folds into the pose.

All compute happens in ``lib/liblvdgs.so`` (HIP, gfx950) through the C ABI in
``include/lvdgs.h``; this file only allocates tensors and passes pointers.
"""
import ctypes as C
import math
import os
from typing import NamedTuple

import torch
from torch import nn

from . import _lib
from ._lib import ptr as _P

# d(loss)/d(opacity image) is NOT propagated by default: the backward binding this module mirrors
# (`rasterize_gaussians_backward(..., dL_dout_color, dL_dout_depth, ...)`) takes the gradients of
# the colour and depth images only, so the opacity image acts as a detached weight in the tracking loss
# (reference utils/slam_utils.py:60 multiplies the residual by it).  The kernels do implement the path
# (opacity = 1 - final transmittance; checked against the oracle); set this to True to use it.
PROPAGATE_OPACITY_GRAD = False

# True: list every tile of a Gaussian's 3-sigma rectangle (lvdgs_args.flags |= LVDGS_FLAG_LIST_ALL_TILES) -- the reference's
# (Gaussian, tile) pair list, num_rendered and n_contrib bit for bit -- instead of only the tiles the Gaussian can reach with
# alpha >= 1/255.  Images, radii, n_touched are the same either way (a dropped pair contributes to no pixel).
LIST_ALL_TILES = False

# Parity tests set this to read intermediates (state buffers) of the most recent forward.
KEEP_DEBUG_STATE = False
_DEBUG_LAST = {}

# pairs the binning buffers are sized for, per device index (see _RasterizeGaussians.forward)
_PAIR_CAPACITY = {}
_MIN_PAIR_CAPACITY = 1 << 20      # floor of the capacity guess
_PAIRS_PER_GAUSSIAN_GUESS = 8     # first guess before any frame has been seen


class GaussianRasterizationSettings(NamedTuple):
    image_height: int
    image_width: int
    tanfovx: float
    tanfovy: float
    bg: torch.Tensor
    scale_modifier: float
    viewmatrix: torch.Tensor
    projmatrix: torch.Tensor
    projmatrix_raw: torch.Tensor
    sh_degree: int
    campos: torch.Tensor
    prefiltered: bool = False
    debug: bool = False


def _f32(t, device):
    if t is None:
        return None
    if not torch.is_tensor(t):
        t = torch.as_tensor(t)
    return None if t.numel() == 0 else _lib.f32(t, device)


def _fill_settings(a, rs, device, keep):
    a.image_height, a.image_width = int(rs.image_height), int(rs.image_width)
    a.tanfovx, a.tanfovy = float(rs.tanfovx), float(rs.tanfovy)
    a.scale_modifier = float(rs.scale_modifier)
    a.sh_degree, a.prefiltered, a.debug = int(rs.sh_degree), int(bool(rs.prefiltered)), int(bool(rs.debug))
    for name in ("bg", "viewmatrix", "projmatrix", "projmatrix_raw", "campos"):
        t = _f32(getattr(rs, name), device)
        keep.append(t)
        setattr(a, name, _P(t))


def fill_camera(a, viewpoint, sh_degree, bg, view, proj, proj_raw, campos):
    """The camera fields of ``a`` for ``viewpoint`` (a ``Camera``: field of view) with the background and camera matrices given as
    contiguous float32 tensors on the device, which the caller keeps alive -- what ``render()`` puts into the settings."""
    a.tanfovx, a.tanfovy = math.tan(viewpoint.FoVx * 0.5), math.tan(viewpoint.FoVy * 0.5)
    a.scale_modifier, a.sh_degree, a.prefiltered, a.debug = 1.0, int(sh_degree), 0, 0
    a.bg, a.viewmatrix, a.projmatrix, a.projmatrix_raw, a.campos = _P(bg), _P(view), _P(proj), _P(proj_raw), _P(campos)


# ---- the pair capacity: every caller sizes its binning state for a number of (Gaussian, tile) pairs before the forward knows the
# frame's count; a frame with more makes the forward return LVDGS_E_CAPACITY, and the caller grows its buffers and re-runs the
# binning + blend stage (lvdgs_forward_render).  The knobs above are read at every call (tests shrink them to force that path).

def first_pair_capacity(num_gaussians, remembered=0):
    """Pairs to size the buffers of a frame of ``num_gaussians`` for: what the caller remembers, or a guess from the map's size."""
    return max(int(remembered), _MIN_PAIR_CAPACITY, _PAIRS_PER_GAUSSIAN_GUESS * num_gaussians, 1)


def pair_state_bytes(N, pairs, W, H, backward=True):
    """-> (binning state, scratch) bytes for ``pairs`` pairs of a frame of N Gaussians, W x H: the scratch serves the prepare and
    render stages and, with ``backward``, the backward's."""
    L = _lib.lib()
    scratch = max(L.lvdgs_prepare_scratch_bytes(N), L.lvdgs_render_scratch_bytes(N, pairs, W, H),
                  L.lvdgs_backward_scratch_bytes(N, pairs) if backward else 0)
    return L.lvdgs_binning_bytes(pairs), scratch


def pair_buffers(a, pairs, device, backward=True):
    """Binning state and scratch for ``pairs`` pairs of the frame ``a`` describes (its N, W, H), pointed at by ``a``; -> the two
    buffers (the caller keeps them alive)."""
    binning_bytes, scratch_bytes = pair_state_bytes(a.num_gaussians, pairs, a.image_width, a.image_height, backward)
    binning, scratch = _lib.device_bytes(binning_bytes, device), _lib.device_bytes(scratch_bytes, device)
    a.pair_capacity = pairs
    a.binning_state, a.binning_bytes = _P(binning), binning.numel()
    a.scratch, a.scratch_bytes = _P(scratch), scratch.numel()
    return binning, scratch


def run_forward(a, stream, resize, la=None, opacity_grad=0, exact=False):
    """``lvdgs_forward`` on ``a`` -- with the loss block ``la``: ``lvdgs_forward_backward_fused_loss``, the backward evaluating the
    loss per pixel -- and the overflow path behind it (``rerender``).  Sets and returns ``a.num_rendered``."""
    L, num = _lib.lib(), C.c_int64(0)
    if la is None:
        status, what = L.lvdgs_forward(C.byref(a), C.byref(num), stream), "lvdgs_forward"
    else:
        status = L.lvdgs_forward_backward_fused_loss(C.byref(a), C.byref(la), opacity_grad, C.byref(num), stream)
        what = "lvdgs_forward_backward_fused_loss"
    D = int(num.value)
    if status == _lib.E_CAPACITY:
        rerender(a, D, stream, resize, la, opacity_grad, exact)
    else:
        _lib.check(status, what)
    a.num_rendered = D
    return D


def rerender(a, D, stream, resize, la=None, opacity_grad=0, exact=False):
    """A frame of ``D`` pairs, more than its buffers hold: ``resize(pairs)`` grows them -- to D (``exact``) or D + D/2 -- and the
    binning + blend stage runs again, then (with ``la``) the fused backward."""
    L = _lib.lib()
    resize(D if exact else D + D // 2)
    a.num_rendered = D
    _lib.check(L.lvdgs_forward_render(C.byref(a), stream), "lvdgs_forward_render")
    if la is not None:
        _lib.check(L.lvdgs_backward_fused_loss(C.byref(a), C.byref(la), opacity_grad, stream), "lvdgs_backward_fused_loss")


# Two-level grouping (include/lvdgs.h: LVDGS_FLAG_SUPER_TILES): worth it when a Gaussian is listed on many tiles -- the opaque surfaces of
# large flat Gaussians SLAM maps are made of (70-80 tiles each) -- and a loss on scenes of small blobs (3 tiles each), so the hint is set
# from what the PREVIOUS frame of the same caller looked like: pairs per Gaussian at or above SUPER_TILES_MIN_PAIRS_PER_GAUSSIAN.  Outputs
# are the same bits either way.  LVDGS_SUPER_TILES=0 / 1 in the environment: never / always (A/B measurements, tests).
SUPER_TILES_MIN_PAIRS_PER_GAUSSIAN = 16.0
_SUPER_TILES_ENV = os.environ.get("LVDGS_SUPER_TILES", "auto")


def super_tiles_flag(num_gaussians, last_num_rendered):
    """The flag bit for a frame of ``num_gaussians`` whose predecessor listed ``last_num_rendered`` pairs (None / 0: unknown)."""
    if _SUPER_TILES_ENV == "0" or LIST_ALL_TILES:
        return 0
    if _SUPER_TILES_ENV == "1":
        return _lib.FLAG_SUPER_TILES
    if not last_num_rendered or num_gaussians <= 0:
        return 0
    return _lib.FLAG_SUPER_TILES if last_num_rendered >= SUPER_TILES_MIN_PAIRS_PER_GAUSSIAN * num_gaussians else 0


_LAST_PAIRS = {}   # device index -> (N, D) of the last frame through the autograd API on that device


class _RasterizeGaussians(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, theta, rho,
                raster_settings, activations=0):
        L = _lib.lib()
        rs = raster_settings
        dev = means3D.device
        if dev.type != "cuda":
            raise _lib.LvdgsError("GaussianRasterizer needs tensors on the GPU (there is no CPU path)")
        N = int(means3D.shape[0])
        H, W = int(rs.image_height), int(rs.image_width)
        keep = []
        a = _lib.Args()
        _fill_settings(a, rs, dev, keep)
        m3 = _f32(means3D, dev)
        op = _f32(opacities, dev)
        shs, col = _f32(sh, dev), _f32(colors_precomp, dev)
        sc, rot, cov = _f32(scales, dev), _f32(rotations, dev), _f32(cov3Ds_precomp, dev)
        if N > 0:
            if (shs is None) == (col is None):
                raise ValueError("Please provide exactly one of either SHs or precomputed colors!")
            if ((sc is None or rot is None) and cov is None) or ((sc is not None or rot is not None) and cov is not None):
                raise ValueError("Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!")
        a.num_gaussians = N
        a.activations = int(activations)
        a.flags = _lib.FLAG_LIST_ALL_TILES if LIST_ALL_TILES else 0
        key = dev.index if dev.index is not None else torch.cuda.current_device()
        _last = _LAST_PAIRS.get(key)
        a.flags |= super_tiles_flag(N, _last[1] if (_last is not None and _last[0] == N) else None)
        a.sh_coeffs = int(shs.shape[1]) if shs is not None else 0
        a.means3D, a.opacities, a.scales, a.rotations = _P(m3), _P(op), _P(sc), _P(rot)
        a.cov3D_precomp, a.shs, a.colors_precomp = _P(cov), _P(shs), _P(col)

        radii = torch.empty(N, dtype=torch.int32, device=dev)
        n_touched = torch.empty(N, dtype=torch.int32, device=dev)
        color = torch.empty(3, H, W, dtype=torch.float32, device=dev)
        depth = torch.empty(1, H, W, dtype=torch.float32, device=dev)
        opac = torch.empty(1, H, W, dtype=torch.float32, device=dev)
        geom = _lib.device_bytes(L.lvdgs_geom_bytes(N), dev)
        image = _lib.device_bytes(L.lvdgs_image_bytes(W, H), dev)
        a.radii, a.n_touched = _P(radii), _P(n_touched)
        a.out_color, a.out_depth, a.out_opacity = _P(color), _P(depth), _P(opac)
        a.geom_state, a.geom_bytes = _P(geom), geom.numel()
        a.image_state, a.image_bytes = _P(image), image.numel()

        # Single-call forward: buffers are sized for a pair capacity remembered per device (grown when a
        # frame gets within 25 % of it), every kernel is enqueued before the host waits for the pair
        # count, and an overflow (rare) re-runs only the binning + blend stage with exact sizes.
        cap = first_pair_capacity(N, _PAIR_CAPACITY.get(key, 0)) if N > 0 else 0
        bufs = pair_buffers(a, cap, dev, backward=False)

        def resize(pairs):
            nonlocal bufs
            bufs = pair_buffers(a, pairs, dev, backward=False)

        D = run_forward(a, _lib.raw_stream(dev), resize, exact=True)
        binning = bufs[0]
        binning_pairs = int(a.pair_capacity)
        _LAST_PAIRS[key] = (N, D)
        if N > 0 and 4 * D > 3 * cap:
            _PAIR_CAPACITY[key] = max(cap, D + D // 2)
        else:
            _PAIR_CAPACITY[key] = cap

        if KEEP_DEBUG_STATE:
            _DEBUG_LAST.clear()
            _DEBUG_LAST.update(geom=geom, binning=binning, image=image, num_rendered=D, N=N, W=W, H=H,
                               binning_pairs=binning_pairs, overflowed=binning_pairs != cap, capacity=cap, flags=int(a.flags))
        ctx.raster_settings = rs
        ctx.num_rendered = D
        ctx.activations = int(activations)
        ctx.flags = int(a.flags)
        ctx.pose = (torch.is_tensor(theta) and theta.numel() == 3, torch.is_tensor(rho) and rho.numel() == 3)
        ctx.save_for_backward(m3, op, sc, rot, cov, shs, col, radii, geom, binning, image)
        ctx.mark_non_differentiable(radii, n_touched)
        return color, radii, depth, opac, n_touched

    @staticmethod
    def backward(ctx, grad_color, grad_radii, grad_depth, grad_opacity, grad_n_touched):
        L = _lib.lib()
        rs = ctx.raster_settings
        m3, op, sc, rot, cov, shs, col, radii, geom, binning, image = ctx.saved_tensors
        dev = m3.device
        N = int(m3.shape[0])
        H, W = int(rs.image_height), int(rs.image_width)
        D = ctx.num_rendered
        keep = []
        a = _lib.Args()
        _fill_settings(a, rs, dev, keep)
        a.num_gaussians = N
        a.sh_coeffs = int(shs.shape[1]) if shs is not None else 0
        a.means3D, a.opacities, a.scales, a.rotations = _P(m3), _P(op), _P(sc), _P(rot)
        a.cov3D_precomp, a.shs, a.colors_precomp = _P(cov), _P(shs), _P(col)
        a.radii = _P(radii)
        a.activations = ctx.activations
        a.flags = ctx.flags
        a.num_rendered = D
        a.geom_state, a.geom_bytes = _P(geom), geom.numel()
        a.binning_state, a.binning_bytes = _P(binning), binning.numel()
        a.image_state, a.image_bytes = _P(image), image.numel()
        scratch = _lib.device_bytes(L.lvdgs_backward_scratch_bytes(N, D), dev)
        a.scratch, a.scratch_bytes = _P(scratch), scratch.numel()

        g_color = _f32(grad_color, dev) if grad_color is not None else torch.zeros(3, H, W, device=dev)
        g_depth = _f32(grad_depth, dev) if grad_depth is not None else None
        g_opac = _f32(grad_opacity, dev) if (grad_opacity is not None and PROPAGATE_OPACITY_GRAD) else None
        a.dL_dout_color, a.dL_dout_depth, a.dL_dout_opacity = _P(g_color), _P(g_depth), _P(g_opac)

        e = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
        d_m3, d_m2, d_op = e(N, 3), e(N, 3), e(*op.shape) if op is not None else e(N, 1)
        d_sc = e(N, 3) if sc is not None else None
        d_rot = e(N, 4) if rot is not None else None
        d_cov = e(N, 6) if cov is not None else None
        d_sh = e(*shs.shape) if shs is not None else None
        d_col = e(N, 3) if col is not None else None
        d_tau = e(6)
        a.dL_dmeans3D, a.dL_dmeans2D, a.dL_dopacities = _P(d_m3), _P(d_m2), _P(d_op)
        a.dL_dscales, a.dL_drotations, a.dL_dcov3D = _P(d_sc), _P(d_rot), _P(d_cov)
        a.dL_dshs, a.dL_dcolors, a.dL_dtau = _P(d_sh), _P(d_col), _P(d_tau)
        _lib.check(L.lvdgs_backward(C.byref(a), _lib.raw_stream(dev)), "lvdgs_backward")
        # (means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, theta, rho, settings)
        d_theta = d_tau[3:] if ctx.pose[0] else None
        d_rho = d_tau[:3] if ctx.pose[1] else None
        return d_m3, d_m2, d_sh, d_col, d_op, d_sc, d_rot, d_cov, d_theta, d_rho, None, None


def rasterize_gaussians(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, theta, rho,
                        raster_settings, activations=0):
    return _RasterizeGaussians.apply(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                                     theta, rho, raster_settings, activations)


# `activations` bits (include/lvdgs.h): the rasterizer applies the model's activations itself
ACT_EXP_SCALES, ACT_NORMALIZE_ROTATIONS, ACT_SIGMOID_OPACITIES = 1, 2, 4


class GaussianRasterizer(nn.Module):
    def __init__(self, raster_settings):
        super().__init__()
        self.raster_settings = raster_settings

    def markVisible(self, positions):
        """Boolean mask of Gaussians in front of the view's near plane."""
        with torch.no_grad():
            rs = self.raster_settings
            pos = _f32(positions, positions.device)
            N = int(positions.shape[0])
            out = torch.empty(N, dtype=torch.uint8, device=positions.device)
            view, proj = _f32(rs.viewmatrix, positions.device), _f32(rs.projmatrix, positions.device)
            _lib.check(_lib.lib().lvdgs_mark_visible(N, _P(pos), _P(view), _P(proj), _P(out), _lib.raw_stream(positions.device)),
                       "lvdgs_mark_visible")
            return out.bool()

    def forward(self, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None,
                cov3D_precomp=None, theta=None, rho=None, activations=0):
        """`activations` (lvdgs extension, default 0 = upstream behaviour): bit mask saying that `scales` are
        log-scales, `rotations` un-normalised quaternions, `opacities` logits; the kernels then apply
        exp / normalise / sigmoid and return gradients w.r.t. those raw values."""
        if (shs is None and colors_precomp is None) or (shs is not None and colors_precomp is not None):
            raise Exception("Please provide excatly one of either SHs or precomputed colors!")
        if ((scales is None or rotations is None) and cov3D_precomp is None) or (
                (scales is not None or rotations is not None) and cov3D_precomp is not None):
            raise Exception("Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!")
        empty = torch.Tensor([])
        shs = empty if shs is None else shs
        colors_precomp = empty if colors_precomp is None else colors_precomp
        scales = empty if scales is None else scales
        rotations = empty if rotations is None else rotations
        cov3D_precomp = empty if cov3D_precomp is None else cov3D_precomp
        theta = empty if theta is None else theta
        rho = empty if rho is None else rho
        return rasterize_gaussians(means3D, means2D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp,
                                   theta, rho, self.raster_settings, activations)
