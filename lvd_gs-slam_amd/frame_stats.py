"""The two statements that bracket a tracked frame's loop, each as one library call (HIP, ``csrc/frame_stats.hip``;
semantics: ``include/lvdgs.h``, DESIGN.md section "Frame statistics").

``edge_mask``       ``Camera.compute_grad_mask`` (reference utils/camera_utils.py:126-155) without its two dozen elementwise kernels
                    and the full sort behind ``mag.median()``: no host wait, no copy.
``frame_summary``   what ``SlamSequence.step`` reads after the last tracking iteration -- ``get_median_depth`` (a boolean gather, whose
                    count the host waits for, and a sort) and every count ``covisibility`` reads one ``int(...)`` at a time for
                    ``is_keyframe`` / ``add_to_window`` -- in one call that ends in ONE wait on a block of pinned host memory.

Both medians are exact order statistics (radix selection on the bit patterns): the bits ``torch.median`` gives.
"""
import ctypes as C
import numpy as np
import torch

from . import _lib

_edge_scratch = _lib.DeviceScratch()
_summary = _lib.HostCall("lvdgs_frame_summary", tag=_lib.FRAME_SUMMARY_SEQ)


class EdgeMask:
    """What one ``lvdgs_edge_mask`` call leaves: ``mask`` (1, H, W) -- torch.bool, or float32 under the replica rule --, and
    whichever of ``loss_mask`` (H*W bytes, the fused loss' grad_mask), ``magnitude`` (H, W) and ``stats`` were asked for."""
    __slots__ = ("mask", "loss_mask", "magnitude", "stats")


def edge_mask_call(image, edge_threshold, dataset_type=None, *, loss_mask=False, magnitude=False, stats=False) -> EdgeMask:
    if not _lib.is_f32(image) or image.ndim != 3 or image.shape[0] != 3:
        raise _lib.LvdgsError("edge_mask: image must be a contiguous (3, H, W) float32 tensor on a GPU (there is no CPU path)")
    device = image.device
    _, H, W = image.shape
    blocks = dataset_type == "replica"
    L = _lib.lib()
    scratch = _edge_scratch.get(device, L.lvdgs_edge_mask_scratch_bytes(W, H))
    out = EdgeMask()
    out.mask = torch.empty((1, H, W), dtype=torch.float32 if blocks else torch.bool, device=device)
    out.loss_mask = torch.empty(H * W, dtype=torch.uint8, device=device) if loss_mask else None
    out.magnitude = torch.empty((H, W), dtype=torch.float32, device=device) if magnitude else None
    out.stats = torch.empty((1024, 2) if blocks else (2,), dtype=torch.float32, device=device) if stats else None
    a = _lib.EdgeMaskArgs(width=W, height=H, mode=_lib.EDGE_MASK_BLOCKS if blocks else _lib.EDGE_MASK_MEDIAN,
                          edge_threshold=float(edge_threshold), image=image.data_ptr(), mask=out.mask.data_ptr(),
                          loss_mask=None if out.loss_mask is None else out.loss_mask.data_ptr(),
                          magnitude=None if out.magnitude is None else out.magnitude.data_ptr(),
                          stats=None if out.stats is None else out.stats.data_ptr(), scratch=scratch.data_ptr(), scratch_bytes=scratch.numel())
    with _lib.on_device(device):
        _lib.check(L.lvdgs_edge_mask(C.byref(a), _lib.raw_stream(device)), "lvdgs_edge_mask")
    return out


def edge_mask(image, edge_threshold, dataset_type=None):
    """``Camera.grad_mask`` of a (3, H, W) float32 image on the GPU: (1, H, W) torch.bool, ``mag > median(mag) * edge_threshold`` --
    its storage is what the fused tracking loss takes as it is --, or with ``dataset_type == "replica"`` the reference's float32
    image of per-block cuts.  The arithmetic is the one ``include/lvdgs.h`` fixes (the grey image is a sum divided by three)."""
    return edge_mask_call(image, edge_threshold, dataset_type).mask


class FrameSummary:
    """``median_depth`` (float; NaN when no pixel is selected), ``selected`` (pixels behind it), ``visible`` (Gaussians with
    ``n_touched > 0``), ``covis`` ({row key: (intersection, union, count of the frame, count of the row)} -- ``covisibility``'s
    tuple), ``mask_count`` / ``mask_share`` (set pixels of ``count_mask``; None without one)."""
    __slots__ = ("median_depth", "median_bits", "selected", "visible", "covis", "mask_count", "mask_share")


def _as_bytes(t, device, n):
    """A visibility row or mask as ``n`` bytes on ``device`` (nonzero = set), or None when it is not ``n`` elements there."""
    if not torch.is_tensor(t) or t.device != device or t.numel() != n:
        return None
    if t.dtype in (torch.bool, torch.uint8) and t.is_contiguous():
        return t.view(torch.uint8).reshape(-1)
    # (the loops store int64 rows: the bytes stay with the row for as long as it is not written to -- rows change when the back end
    # maps, not per frame)
    hit = getattr(t, "_lvdgs_bytes", None)
    if hit is not None and hit[0] == t._version:
        return hit[1]
    b = t.reshape(-1).ne(0).view(torch.uint8)
    try:
        t._lvdgs_bytes = (t._version, b)
    except Exception:
        pass
    return b


def mean_of_mask(count, numel):
    """``float(mask.float().mean())`` of a mask of ``numel`` elements on the GPU with ``count`` of them set: a float32 sum (exact
    below 2^24) times the float32 reciprocal of the element count, which is how the device reduction forms a mean."""
    if numel == 0:
        return float("nan")
    return float(np.float32(count) * (np.float32(1.0) / np.float32(numel)))


def frame_summary(render_pkg, visibility_rows, mask=None, count_mask=None, opacity_bar=0.95) -> FrameSummary:
    """One ``lvdgs_frame_summary`` call on a render package (``depth``, ``opacity``, ``n_touched`` on one GPU) and one wait.

    ``visibility_rows``: {key: row} (or a sequence: keys 0, 1, ...), each row a per-Gaussian visibility vector of any integer or
    bool dtype.  Rows on another device or of another length than ``n_touched`` take ``keyframe_utils.covisibility`` -- the
    PyTorch path, with its host waits --; more than 16 rows on the device go in several calls.  ``mask``: ``get_median_depth``'s
    optional pixel mask.  ``count_mask``: a pixel mask whose set pixels are counted (``is_keyframe``'s ``expanded_static_mask``)."""
    depth, opacity, n_touched = render_pkg["depth"], render_pkg.get("opacity"), render_pkg["n_touched"]
    if not _lib.is_f32(depth):
        raise _lib.LvdgsError("frame_summary: depth must be a contiguous float32 tensor on a GPU (there is no CPU path)")
    device = depth.device
    P, N = depth.numel(), n_touched.numel()
    if n_touched.device != device or n_touched.dtype is not torch.int32 or not n_touched.is_contiguous():
        raise _lib.LvdgsError("frame_summary: n_touched must be a contiguous int32 tensor on the depth's device")
    if opacity is not None and (not _lib.is_f32(opacity, device) or opacity.numel() != P):
        raise _lib.LvdgsError("frame_summary: opacity must be a contiguous float32 tensor of the depth's size on its device")
    items = list(visibility_rows.items()) if isinstance(visibility_rows, dict) else list(enumerate(visibility_rows))
    on_device, elsewhere = [], []
    for key, row in items:
        b = _as_bytes(row, device, N)
        (elsewhere if b is None else on_device).append((key, row if b is None else b))
    pixel_masks = []
    for name, m in (("mask", mask), ("count_mask", count_mask)):
        b = None if m is None else _as_bytes(m, device, P)
        if m is not None and b is None:
            raise _lib.LvdgsError(f"frame_summary: {name} must have the depth's size and device")
        pixel_masks.append(b)
    mask_b, count_b = pixel_masks

    L = _lib.lib()
    block, scratch = _summary.resources(device, _lib.FRAME_SUMMARY_HOST_BYTES, L.lvdgs_frame_summary_scratch_bytes())
    out = FrameSummary()
    out.covis = {}
    R = _lib.FRAME_SUMMARY_MAX_ROWS
    chunks = [on_device[i:i + R] for i in range(0, len(on_device), R)] or [[]]
    for chunk in chunks:
        a = _lib.FrameSummaryArgs(num_pixels=P, num_gaussians=N, num_rows=len(chunk), opacity_bar=float(opacity_bar),
                                  depth=depth.data_ptr(), opacity=None if opacity is None else opacity.data_ptr(),
                                  mask=None if mask_b is None else mask_b.data_ptr(), n_touched=n_touched.data_ptr(),
                                  count_mask=None if count_b is None else count_b.data_ptr(), host_state=block.data_ptr(),
                                  scratch=scratch.data_ptr(), scratch_bytes=scratch.numel())
        for r, (_, b) in enumerate(chunk):
            a.rows[r] = b.data_ptr()
        w = _summary.run(device, a).copy()      # the one wait of the call
        out.median_bits = int(w[_lib.FRAME_SUMMARY_MEDIAN]) & 0xFFFFFFFF
        out.median_depth = float(w[_lib.FRAME_SUMMARY_MEDIAN:_lib.FRAME_SUMMARY_MEDIAN + 1].view(np.float32)[0])
        out.selected, out.visible = int(w[_lib.FRAME_SUMMARY_SELECTED]), int(w[_lib.FRAME_SUMMARY_VISIBLE])
        out.mask_count = int(w[_lib.FRAME_SUMMARY_MASK_COUNT]) if count_b is not None else None
        for r, (key, _) in enumerate(chunk):
            inter, union, own = (int(v) for v in w[_lib.FRAME_SUMMARY_ROWS + 3 * r:_lib.FRAME_SUMMARY_ROWS + 3 * r + 3])
            out.covis[key] = (inter, union, out.visible, own)
    out.mask_share = None if out.mask_count is None else mean_of_mask(out.mask_count, P)
    if elsewhere:
        from .keyframe_utils import covisibility
        cur = n_touched > 0
        for key, row in elsewhere:
            out.covis[key] = covisibility(cur.to(row.device) if torch.is_tensor(row) else cur, row)
    out.covis = {key: out.covis[key] for key, _ in items}      # the caller's order
    return out
