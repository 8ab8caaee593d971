"""From the detector's boxes and the segmenter's masks to the masks the loops consume, on the device (HIP,
``csrc/dynamic_mask.hip``; semantics: ``include/lvdgs.h``).

The reference runs ``EnhancedDynamicObjectMasker.detect_and_segment`` (utils/slam_frontend.py:832-1104) on every tracked frame and
on every keyframe a second time: after its two networks a chain of host statements -- the frame copied to the host and quantised,
NumPy rectangle fills, an OR over the SAM masks, ``np.median`` over a five-frame history, ``cv2.dilate`` there and once more in
``FrontEnd._expand_dynamic_mask``, two uploads and two waited-for means.  Here that chain is ONE library call with a fixed number
of launches and no host wait: ``assemble``.  The two networks stay out of scope and are injectable seats of ``DynamicMasker``, as
MASt3R is for the matcher.

``assemble``        the functional form: device tensors in, a ``DynamicMasks`` out.
``MaskHistory``     the persistent temporal-consistency history of the fused path (a device block the library owns the layout of).
``DynamicMasker``   the reference's class state (``first_frame_processed``, the history) around the seats ``detect`` / ``segment`` /
                    ``fallback``; ``fused=False`` is the same chain as PyTorch statements on whatever device the inputs live on.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib

VEHICLE_KEYWORDS = ("car", "truck", "bus", "vehicle", "van", "suv", "motorcycle", "bike")   # utils/slam_frontend.py:926
BOX_FORMATS = {"xyxy": _lib.DYNAMIC_MASK_BOXES_XYXY, "cxcywh": _lib.DYNAMIC_MASK_BOXES_CXCYWH}
OUTPUTS = ("static_mask", "dynamic_mask", "expanded_dynamic_mask", "expanded_static_mask", "valid_rgb")

_scratch = _lib.DeviceScratch()


def is_vehicle(label):
    """The reference's keyword test on a detection's label (:926-927)."""
    return any(k in label.lower() for k in VEHICLE_KEYWORDS)


class DynamicMasks:
    """What one call leaves: (H, W) torch.bool tensors ``static_mask``, ``dynamic_mask`` and -- on a keyframe --
    ``expanded_dynamic_mask``, ``expanded_static_mask``, ``valid_rgb``; ``depth`` (H, W) float32 when a depth map went in; ``info``:
    16 int32 on the masks' device (``_lib.DYNAMIC_MASK_INFO`` names them; nobody has to read them).  Outputs not asked for are None."""
    __slots__ = OUTPUTS + ("depth", "info")

    def __init__(self):
        for name in self.__slots__:
            setattr(self, name, None)

    def info_dict(self):
        """``info`` by name, on the host (a device-to-host copy and a wait: for tests and logs)."""
        return dict(zip(_lib.DYNAMIC_MASK_INFO, (int(v) for v in self.info.cpu().tolist())))


class MaskHistory:
    """The temporal-consistency history of ``lvdgs_dynamic_mask`` for one frame size: a zeroed block is an empty history."""

    def __init__(self, width, height, history_length=5, device="cuda"):
        self.width, self.height, self.history_length = int(width), int(height), int(history_length)
        nbytes = int(_lib.lib().lvdgs_dynamic_mask_state_bytes(self.width, self.height, self.history_length))
        if nbytes == 0:
            raise _lib.LvdgsError(f"dynamic mask: no history for a {width}x{height} frame and {history_length} entries "
                                  "(at least 1x1, at most 2^31 - 1 pixels, 1..8 entries)")
        self.block = torch.zeros(nbytes, dtype=torch.uint8, device=device)

    def reset(self):
        self.block.zero_()

    def entries(self):
        """The history as a list of (H, W) uint8 NumPy arrays, oldest first (a device-to-host copy: for tests)."""
        raw = self.block.cpu().numpy()
        w, h, n, length, head = (int(v) for v in raw[:20].view(np.int32))
        if (w, h, n) != (self.width, self.height, self.history_length):
            return []
        wpr = (w + 63) // 64
        planes = raw[256:256 + n * h * wpr * 8].view(np.uint64).reshape(n, h, wpr)
        bits = np.unpackbits(planes.view(np.uint8).reshape(n, h, wpr * 8), axis=2, bitorder="little")[:, :, :w]
        return [bits[(head + j) % n].copy() for j in range(length)]


def _bytes_of(t, device, shape, what):
    if t is None:
        return None
    if not torch.is_tensor(t) or t.device != device or t.dtype not in (torch.bool, torch.uint8) or tuple(t.shape) != shape:
        raise _lib.LvdgsError(f"dynamic mask: {what} must be a bool or uint8 tensor of shape {shape} on {device}")
    return t.contiguous().view(torch.uint8)


def assemble(width, height, boxes, vehicle=None, sam_masks=None, *, first_frame, history, box_format="xyxy",
             vehicle_kernels=(7, 5), expand_kernel=0, image=None, rgb_boundary_threshold=0.0, depth=None, outputs=OUTPUTS) -> DynamicMasks:
    """One ``lvdgs_dynamic_mask`` call: steps 1-6 of the specification in ``include/lvdgs.h``.

    ``boxes``: (K, 4) float32 on the GPU (None or K = 0: no boxes), in ``box_format``; ``vehicle``: K bytes on the same device, nonzero
    where the label names a vehicle (``is_vehicle``), or a host sequence of K booleans (uploaded), or None.  ``sam_masks``: (K', H, W) bool
    / uint8 on the device, or None.  ``history``: the ``MaskHistory`` the call reads and advances.  ``expand_kernel``: 0, or the
    keyframe's dilation (9 for frame 0, else 7) -- then ``image`` (3, H, W) float32 is needed and ``depth`` (H, W) float32 may be
    given.  ``outputs``: which masks to store.  No host wait, no device-to-host copy."""
    W, H = int(width), int(height)
    if not isinstance(history, MaskHistory) or (history.width, history.height) != (W, H):
        raise _lib.LvdgsError(f"dynamic mask: history must be a MaskHistory of the frame's size {W}x{H}")
    device = history.block.device
    if box_format not in BOX_FORMATS:
        raise ValueError(f"box_format: 'xyxy' or 'cxcywh', not {box_format!r}")
    K = 0 if boxes is None else int(boxes.shape[0])
    if K:
        if not _lib.is_f32(boxes, device) or tuple(boxes.shape) != (K, 4):
            raise _lib.LvdgsError("dynamic mask: boxes must be a contiguous (K, 4) float32 tensor on the history's GPU (there is no CPU path)")
        if vehicle is not None and not torch.is_tensor(vehicle):
            vehicle = torch.tensor([1 if v else 0 for v in vehicle], dtype=torch.uint8).to(device, non_blocking=True)
        vehicle = _bytes_of(vehicle, device, (K,), "vehicle")
    Ks = 0 if sam_masks is None else int(sam_masks.shape[0])
    sam = _bytes_of(sam_masks, device, (Ks, H, W), "sam_masks") if Ks else None
    if expand_kernel:
        if not _lib.is_f32(image, device) or tuple(image.shape) != (3, H, W):
            raise _lib.LvdgsError("dynamic mask: image must be a contiguous (3, H, W) float32 tensor on the history's GPU")
        if depth is not None and (not _lib.is_f32(depth, device) or depth.numel() != H * W):
            raise _lib.LvdgsError("dynamic mask: depth must be a contiguous float32 tensor of H*W elements on the history's GPU")
    else:
        image = depth = None
    L = _lib.lib()
    scratch = _scratch.get(device, L.lvdgs_dynamic_mask_scratch_bytes(W, H))
    out = DynamicMasks()
    keyframe_only = OUTPUTS[2:]
    for name in outputs:
        if name not in OUTPUTS:
            raise ValueError(f"outputs: names from {OUTPUTS}, not {name!r}")
        if expand_kernel or name not in keyframe_only:
            setattr(out, name, torch.empty((H, W), dtype=torch.bool, device=device))
    out.depth = None if depth is None else torch.empty((H, W), dtype=torch.float32, device=device)
    out.info = torch.empty(_lib.DYNAMIC_MASK_INFO_WORDS, dtype=torch.int32, device=device)
    a = _lib.DynamicMaskArgs(width=W, height=H, first_frame=1 if first_frame else 0, box_format=BOX_FORMATS[box_format], num_boxes=K,
                             boxes=_lib.ptr(boxes) if K else None, vehicle=_lib.ptr(vehicle) if K else None,
                             num_sam_masks=Ks, sam_masks=_lib.ptr(sam), history_length=history.history_length,
                             vehicle_kernel_first=int(vehicle_kernels[0]), vehicle_kernel=int(vehicle_kernels[1]), expand_kernel=int(expand_kernel),
                             image=_lib.ptr(image), rgb_boundary_threshold=float(rgb_boundary_threshold), depth_in=_lib.ptr(depth),
                             depth_out=_lib.ptr(out.depth), static_mask=_lib.ptr(out.static_mask), dynamic_mask=_lib.ptr(out.dynamic_mask),
                             expanded_dynamic=_lib.ptr(out.expanded_dynamic_mask), expanded_static=_lib.ptr(out.expanded_static_mask),
                             valid_rgb=_lib.ptr(out.valid_rgb), info=_lib.ptr(out.info), state=_lib.ptr(history.block),
                             state_bytes=history.block.numel(), scratch=_lib.ptr(scratch), scratch_bytes=scratch.numel())
    with _lib.on_device(device):
        _lib.check(L.lvdgs_dynamic_mask(C.byref(a), _lib.raw_stream(device)), "lvdgs_dynamic_mask")
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# The same chain as PyTorch statements (``DynamicMasker(fused=False)``): the restatement the CPU tests and the A/B runs use
# ------------------------------------------------------------------------------------------------------------------------------
def _dilate(mask, k):
    from .slam_sequence import expand_dynamic_mask
    return expand_dynamic_mask(mask, k)


def _boxes_xyxy(boxes, box_format, W, H):
    """(K, 4) float32 pixel boxes on the host: ``GroundingDINODetector.detect``'s float32 statements for the normalised format."""
    b = torch.as_tensor(boxes).detach().to("cpu", torch.float32).reshape(-1, 4).numpy()
    if box_format == "cxcywh":
        fw, fh, two = np.float32(W), np.float32(H), np.float32(2)
        cx, cy, bw, bh = b[:, 0] * fw, b[:, 1] * fh, b[:, 2] * fw, b[:, 3] * fh
        b = np.stack([np.clip(cx - bw / two, 0, fw), np.clip(cy - bh / two, 0, fh), np.clip(cx + bw / two, 0, fw),
                      np.clip(cy + bh / two, 0, fh)], axis=1).astype(np.float32)
    return b


def assemble_torch(width, height, boxes, vehicle=None, sam_masks=None, *, first_frame, history, history_length=5, box_format="xyxy",
                   vehicle_kernels=(7, 5), expand_kernel=0, image=None, rgb_boundary_threshold=0.0, depth=None, device=None) -> DynamicMasks:
    """``assemble`` as the reference's statements in PyTorch, on ``device`` (default: the image's, the masks' or the boxes').
    ``history``: a Python list of (H, W) bool tensors, changed in place.  The boxes are read on the host, as the reference reads them."""
    W, H = int(width), int(height)
    if device is None:
        device = next((t.device for t in (image, sam_masks, boxes) if torch.is_tensor(t)), torch.device("cpu"))
    K = 0 if boxes is None else int(len(boxes))
    box_mask = torch.zeros((H, W), dtype=torch.bool, device=device)
    kept, vehicle_detected = 0, False
    if K:
        flags = [False] * K if vehicle is None else [bool(v) for v in (vehicle.cpu().tolist() if torch.is_tensor(vehicle) else vehicle)]
        for box, veh in zip(_boxes_xyxy(boxes, box_format, W, H), flags):
            x1, y1, x2, y2 = (int(v) for v in box.astype(np.int64))
            x1, x2 = max(0, min(x1, W - 1)), max(0, min(x2, W - 1))
            y1, y2 = max(0, min(y1, H - 1)), max(0, min(y2, H - 1))
            if x2 <= x1 or y2 <= y1:
                continue
            kept += 1
            if veh:
                vehicle_detected = True
                r = 0.15 if first_frame else 0.1
                ew, eh = int((x2 - x1) * r), int((y2 - y1) * r)
                x1, y1, x2, y2 = max(0, x1 - ew), max(0, y1 - eh), min(W, x2 + ew), min(H, y2 + eh)
            box_mask[y1:y2, x1:x2] = True
    union = torch.zeros((H, W), dtype=torch.bool, device=device)
    if sam_masks is not None and len(sam_masks):
        union = (sam_masks.to(device) != 0).any(dim=0)
    use_sam = bool(union.any())
    final = union if use_sam else box_mask
    filtered = not first_frame and not use_sam
    if filtered:
        history.append(final.clone())
        if len(history) > history_length:
            history.pop(0)
        n = len(history)
        if n >= 3:
            final = torch.stack(history).sum(dim=0) * 2 > n
    if vehicle_detected:
        final = _dilate(final, vehicle_kernels[0] if first_frame else vehicle_kernels[1])
    out = DynamicMasks()
    out.dynamic_mask, out.static_mask = final, ~final
    counts = dict(boxes=kept, vehicle_detected=int(vehicle_detected), use_sam_result=int(use_sam), filtered=int(filtered), history=len(history),
                  box_pixels=int(box_mask.sum()), sam_pixels=int(union.sum()), dynamic_pixels=int(final.sum()), static_pixels=int((~final).sum()))
    if expand_kernel:
        image = image.to(device)
        out.expanded_dynamic_mask = _dilate(final, expand_kernel)
        out.expanded_static_mask = ~out.expanded_dynamic_mask
        thr = torch.tensor(rgb_boundary_threshold, dtype=torch.float32)
        out.valid_rgb = (((image[0] + image[1]) + image[2]) > thr.to(device)) & out.expanded_static_mask
        counts.update(expanded_pixels=int(out.expanded_dynamic_mask.sum()), valid_pixels=int(out.valid_rgb.sum()))
        if depth is not None:
            d = depth.to(device).reshape(H, W)
            out.depth = torch.where(out.valid_rgb, d, torch.zeros_like(d))
            counts["depth_pixels"] = int((out.depth > 0).sum())
    info = [counts.get(k, 0) for k in _lib.DYNAMIC_MASK_INFO]
    out.info = torch.tensor(info + [0] * (_lib.DYNAMIC_MASK_INFO_WORDS - len(info)), dtype=torch.int32, device=device)
    return out


class DynamicMasker:
    """``EnhancedDynamicObjectMasker``'s state and methods around injectable networks (utils/slam_frontend.py:832-1182).

    ``detect(image, frame_idx) -> (boxes, labels)``: the GroundingDINO seat.  ``image`` is the frame, (3, H, W) float32 on its device;
    ``boxes`` (K, 4) float32 in ``box_format`` ("xyxy" pixels as ``GroundingDINODetector.detect`` returns them, or the model's
    normalised "cxcywh"), ``labels`` K host strings -- the vehicle keyword test is done here.
    ``segment(image, boxes) -> (K', H, W)`` bool masks on the device: the SAM seat (None: no SAM).
    ``fallback(image, frame_idx) -> (H, W) bool mask or None``: the reference's ``_fallback_detection`` for a frame without boxes; None
    (the seat or its result) is its last resort, the empty mask.  Such a frame leaves the history untouched.  A seat with an
    ``observe(image)`` method -- ``optical_flow.MotionFallback``, the reference's dense-flow fallback -- is shown every frame WITH
    boxes that is not a first frame: where the reference sets its ``prev_frame``.
    ``fused=True``: ``assemble`` (HIP; the frames must be on a GPU).  ``fused=False``: ``assemble_torch`` on the image's device."""

    def __init__(self, detect, segment=None, fallback=None, history_length=5, fused=True, box_format="xyxy", vehicle_kernels=(7, 5)):
        if box_format not in BOX_FORMATS:
            raise ValueError(f"box_format: 'xyxy' or 'cxcywh', not {box_format!r}")
        if not 1 <= int(history_length) <= 8:
            raise ValueError(f"history_length: 1..8, not {history_length!r}")
        self.detect, self.segment, self.fallback = detect, segment, fallback
        self.history_length, self.fused, self.box_format, self.vehicle_kernels = int(history_length), bool(fused), box_format, tuple(vehicle_kernels)
        self.first_frame_processed = False
        self.mask_history = []          # fused=False: the reference's list
        self._history = None            # fused=True: the MaskHistory of the frames' size and device
        self.last = None                # the last call's DynamicMasks

    def reset(self):
        self.first_frame_processed = False
        self.mask_history = []
        if self._history is not None:
            self._history.reset()
        if hasattr(self.fallback, "reset"):      # a seat with state of its own (MotionFallback's stored frame)
            self.fallback.reset()

    def _device_history(self, W, H, device):
        h = self._history
        if h is None or (h.width, h.height) != (W, H) or h.block.device != device:
            h = self._history = MaskHistory(W, H, self.history_length, device)
        return h

    def detect_and_segment(self, image, frame_idx=None, *, expand_kernel=0, rgb_boundary_threshold=0.0, depth=None) -> DynamicMasks:
        """One frame through both seats and steps 1-5 (with ``expand_kernel``: step 6 too)."""
        _, H, W = image.shape
        first = frame_idx == 0 or not self.first_frame_processed
        boxes, labels = self.detect(image, frame_idx)
        K = 0 if boxes is None else len(boxes)
        if K == 0:      # the fallback branch (:887-904): its mask as it is, no history
            mask = None if self.fallback is None else self.fallback(image, frame_idx)
            mask = torch.zeros((1, H, W), dtype=torch.bool, device=image.device) if mask is None else mask.to(image.device).reshape(1, H, W)
            boxes, vehicle, sam, first_flag = None, None, mask, True
        else:
            vehicle = [is_vehicle(s) for s in labels]
            sam = None if self.segment is None else self.segment(image, boxes)
            first_flag = first
            if not first and hasattr(self.fallback, "observe"):      # where the reference sets prev_frame (_refine_with_motion, :1109, :1139)
                self.fallback.observe(image)
        kw = dict(first_frame=first_flag, box_format=self.box_format, vehicle_kernels=self.vehicle_kernels, expand_kernel=expand_kernel,
                  image=image, rgb_boundary_threshold=rgb_boundary_threshold, depth=depth)
        if self.fused:
            if not image.is_cuda:
                raise _lib.LvdgsError("DynamicMasker(fused=True) needs the frames on a GPU (there is no CPU path; fused=False is the PyTorch chain)")
            if K and (not torch.is_tensor(boxes) or boxes.device != image.device):
                boxes = torch.as_tensor(boxes, dtype=torch.float32).to(image.device)
            out = assemble(W, H, boxes, vehicle, sam, history=self._device_history(W, H, image.device), **kw)
        else:
            out = assemble_torch(W, H, boxes, vehicle, sam, history=self.mask_history, history_length=self.history_length,
                                 device=image.device, **kw)
        self.first_frame_processed = True
        self.last = out
        return out

    def get_static_mask_for_gaussian_init(self, image, frame_idx=None):
        """-> the static mask, (H, W) torch.bool on the image's device (:1151-1166)."""
        return self.detect_and_segment(image, frame_idx).static_mask

    def keyframe_masks(self, viewpoint, frame_idx, threshold, depth=None) -> DynamicMasks:
        """``add_new_keyframe``'s statements from the detector's call to ``valid_rgb`` (:1296-1329): the five masks stored on the
        viewpoint; ``depth`` (H, W) float32 on the device comes back zero where ``valid_rgb`` is not set (:1367-1369)."""
        out = self.detect_and_segment(viewpoint.original_image, frame_idx, expand_kernel=9 if frame_idx == 0 else 7,
                                      rgb_boundary_threshold=threshold, depth=depth)
        viewpoint.static_mask, viewpoint.dynamic_mask = out.static_mask, out.dynamic_mask
        viewpoint.expanded_dynamic_mask, viewpoint.expanded_static_mask = out.expanded_dynamic_mask, out.expanded_static_mask
        return out
