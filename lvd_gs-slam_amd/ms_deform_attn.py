"""Multi-scale deformable attention: the ``groundingdino._C`` extension of GroundingDINO's encoder and decoder layers.

Counterpart of ``_C.ms_deform_attn_forward`` / ``_C.ms_deform_attn_backward``, which the reference's
``MultiScaleDeformableAttention`` calls unconditionally on a GPU tensor (GroundingDINO-main/groundingdino/models/GroundingDINO/
ms_deform_attn.py:53, :80, :330-345; the extension is CUDA and absent from the checkout).  The semantics are the published ones of
Deformable-DETR's operator, i.e. those of the reference's ``multi_scale_deformable_attn_pytorch``
(``grid_sample(bilinear, zeros, align_corners=False)``); see ``include/lvdgs.h``.

``install()`` makes ``from groundingdino import _C`` of an installed GroundingDINO resolve to this module.  There is no shim
directory for it under ``dropin/``: a ``groundingdino`` directory on ``sys.path`` would shadow the user's own package.
"""
import ctypes as C
import importlib
import sys

import torch
from torch.autograd.function import once_differentiable

from . import _lib


def _inputs(what, value, spatial_shapes, level_start_index, sampling_locations, attention_weights, grad_output=None):
    tensors = [value, sampling_locations, attention_weights] + ([] if grad_output is None else [grad_output])
    for t in tensors:
        if t.dtype is not torch.float32:
            raise TypeError(f"{what}: float32 tensors, got {t.dtype} (the caller up-casts half precision, as the reference's module does)")
    if any(t.device.type != "cuda" for t in tensors):
        raise _lib.LvdgsError(f"{what} needs GPU tensors (there is no CPU path)")
    dev = value.device
    if value.dim() != 4 or sampling_locations.dim() != 6 or attention_weights.dim() != 5:
        raise ValueError(f"{what}: value (B, S, H, D), sampling_locations (B, Q, H, L, P, 2), attention_weights (B, Q, H, L, P)")
    B, S, H, D = value.shape
    _, Q, _, L, P, _ = sampling_locations.shape
    if tuple(sampling_locations.shape) != (B, Q, H, L, P, 2) or tuple(attention_weights.shape) != (B, Q, H, L, P):
        raise ValueError(f"{what}: shapes disagree: value {tuple(value.shape)}, sampling_locations {tuple(sampling_locations.shape)}, "
                         f"attention_weights {tuple(attention_weights.shape)}")
    shapes = spatial_shapes.detach().to(device=dev, dtype=torch.int64).contiguous()
    if tuple(shapes.shape) != (L, 2):
        raise ValueError(f"{what}: spatial_shapes must be ({L}, 2), got {tuple(shapes.shape)}")
    if level_start_index is None:   # on the device: no host wait
        areas = shapes[:, 0] * shapes[:, 1]
        starts = torch.cumsum(areas, 0) - areas
    else:
        starts = level_start_index.detach().to(device=dev, dtype=torch.int64).contiguous()
        if tuple(starts.shape) != (L,):
            raise ValueError(f"{what}: level_start_index must be ({L},), got {tuple(starts.shape)}")
    if grad_output is not None and grad_output.numel() != B * Q * H * D:
        raise ValueError(f"{what}: grad_output must be ({B}, {Q}, {H * D}), got {tuple(grad_output.shape)}")
    cont = [t.detach().contiguous() for t in tensors]
    return dev, (B, S, H, D, Q, L, P), shapes, starts, cont


def ms_deform_attn_forward(value, spatial_shapes, level_start_index, sampling_locations, attention_weights, im2col_step=64):
    """-> (B, Q, H * D).  ``value`` (B, S, H, D), ``spatial_shapes`` (L, 2) = (h, w) and ``level_start_index`` (L,) integer tensors
    (``None``: computed from the shapes on the device), ``sampling_locations`` (B, Q, H, L, P, 2) = (x, y) in [0, 1],
    ``attention_weights`` (B, Q, H, L, P); float32 on the GPU.  ``im2col_step`` is accepted and ignored: one launch covers the
    batch.  Runs on the current stream, allocates only its output and never waits for the device."""
    dev, (B, S, H, D, Q, L, P), shapes, starts, (v, loc, w) = _inputs("ms_deform_attn_forward", value, spatial_shapes, level_start_index,
                                                                      sampling_locations, attention_weights)
    out = torch.empty((B, Q, H * D), dtype=torch.float32, device=dev)
    with _lib.on_device(dev):
        st = _lib.lib().lvdgs_ms_deform_attn_forward(_lib.ptr(v), _lib.ptr(shapes), _lib.ptr(starts), _lib.ptr(loc), _lib.ptr(w),
                                                     B, S, H, D, Q, L, P, _lib.ptr(out), _lib.raw_stream(dev))
    _lib.check(st, "lvdgs_ms_deform_attn_forward")
    return out


def ms_deform_attn_backward(value, spatial_shapes, level_start_index, sampling_locations, attention_weights, grad_output, im2col_step=64):
    """-> (grad_value, grad_sampling_loc, grad_attn_weight), shaped as their tensors.  Arguments as ``ms_deform_attn_forward``, with
    ``grad_output`` (B, Q, H * D); ``im2col_step`` is accepted and ignored.  The location and weight gradients are bitwise
    reproducible; ``grad_value`` is summed by float atomics, so its last bits may differ from run to run."""
    dev, (B, S, H, D, Q, L, P), shapes, starts, (v, loc, w, go) = _inputs("ms_deform_attn_backward", value, spatial_shapes, level_start_index,
                                                                          sampling_locations, attention_weights, grad_output)
    grad_value = torch.empty((B, S, H, D), dtype=torch.float32, device=dev)   # zeroed by the call
    grad_loc = torch.empty((B, Q, H, L, P, 2), dtype=torch.float32, device=dev)
    grad_w = torch.empty((B, Q, H, L, P), dtype=torch.float32, device=dev)
    with _lib.on_device(dev):
        st = _lib.lib().lvdgs_ms_deform_attn_backward(_lib.ptr(v), _lib.ptr(shapes), _lib.ptr(starts), _lib.ptr(loc), _lib.ptr(w),
                                                      B, S, H, D, Q, L, P, _lib.ptr(go), _lib.ptr(grad_value), _lib.ptr(grad_loc),
                                                      _lib.ptr(grad_w), _lib.raw_stream(dev))
    _lib.check(st, "lvdgs_ms_deform_attn_backward")
    return grad_value, grad_loc, grad_w


class MultiScaleDeformableAttnFunction(torch.autograd.Function):
    """The reference's autograd function (ms_deform_attn.py:41-90), same ``apply`` signature."""

    @staticmethod
    def forward(ctx, value, value_spatial_shapes, value_level_start_index, sampling_locations, attention_weights, im2col_step):
        ctx.im2col_step = im2col_step
        ctx.no_starts = value_level_start_index is None
        out = ms_deform_attn_forward(value, value_spatial_shapes, value_level_start_index, sampling_locations, attention_weights, im2col_step)
        saved = [value, value_spatial_shapes, sampling_locations, attention_weights] + ([] if ctx.no_starts else [value_level_start_index])
        ctx.save_for_backward(*saved)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        value, shapes, loc, w = ctx.saved_tensors[:4]
        starts = None if ctx.no_starts else ctx.saved_tensors[4]
        grad_value, grad_loc, grad_w = ms_deform_attn_backward(value, shapes, starts, loc, w, grad_output, ctx.im2col_step)
        return grad_value, None, None, grad_loc, grad_w, None


def install(force=False):
    """Make ``from groundingdino import _C`` resolve to this module: call it before building the detector.

    Imports the user's own ``groundingdino`` package, sets its ``_C`` attribute and ``sys.modules["groundingdino._C"]``, and sets
    ``_C`` on every already imported ``groundingdino.<...>.ms_deform_attn`` module whose own guarded import of ``_C`` failed (the
    reference swallows that failure with a warning and then raises ``NameError`` in the first encoder layer).  Idempotent.  A real
    ``_C`` that imports successfully is left in place unless ``force``.  -> the module now serving as ``groundingdino._C``."""
    me = sys.modules[__name__]
    pkg = importlib.import_module("groundingdino")
    have = sys.modules.get("groundingdino._C") or getattr(pkg, "_C", None)
    if have is None:
        try:
            have = importlib.import_module("groundingdino._C")
        except Exception:   # not built, or built for another platform
            have = None
    if have is not None and have is not me and not force:
        return have
    pkg._C = me
    sys.modules["groundingdino._C"] = me
    for name, mod in list(sys.modules.items()):
        if mod is not None and name.startswith("groundingdino.") and name.endswith(".ms_deform_attn") and (force or not hasattr(mod, "_C")):
            mod._C = me
    return me
