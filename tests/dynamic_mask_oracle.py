"""The specification of lvdgs_dynamic_mask (include/lvdgs.h) as plain NumPy statements on byte masks: no bit planes, no package
imports.  ``Masker`` carries the state of the reference's EnhancedDynamicObjectMasker (utils/slam_frontend.py): the history list
and ``first_frame_processed``; ``assemble`` is one call of the library on explicit state."""
import numpy as np

INFO = ("boxes", "vehicle_detected", "use_sam_result", "filtered", "history", "box_pixels", "sam_pixels", "dynamic_pixels",
        "static_pixels", "expanded_pixels", "valid_pixels", "depth_pixels")
VEHICLE_KEYWORDS = ("car", "truck", "bus", "vehicle", "van", "suv", "motorcycle", "bike")


def is_vehicle(label):
    return any(k in label.lower() for k in VEHICLE_KEYWORDS)


def dilate(mask, k):
    """A pixel is set when any pixel of its centred k x k window that lies inside the image is set (the window is a square of
    ones: the columns first, then the rows)."""
    r = k // 2
    cols = mask.copy()
    for d in range(1, r + 1):
        cols[:, d:] |= mask[:, :-d]
        cols[:, :-d] |= mask[:, d:]
    out = cols.copy()
    for d in range(1, r + 1):
        out[d:, :] |= cols[:-d, :]
        out[:-d, :] |= cols[d:, :]
    return out


def cxcywh_to_xyxy(boxes, w, h):
    """GroundingDINODetector.detect's float32 statements (:364-382)."""
    b = np.asarray(boxes, dtype=np.float32).reshape(-1, 4)
    fw, fh = np.float32(w), np.float32(h)
    cx, cy, bw, bh = b[:, 0] * fw, b[:, 1] * fh, b[:, 2] * fw, b[:, 3] * fh
    x1, y1, x2, y2 = cx - bw / np.float32(2), cy - bh / np.float32(2), cx + bw / np.float32(2), cy + bh / np.float32(2)
    out = np.stack([x1, y1, x2, y2], axis=1).astype(np.float32)
    out[:, 0] = np.clip(out[:, 0], 0, fw)
    out[:, 1] = np.clip(out[:, 1], 0, fh)
    out[:, 2] = np.clip(out[:, 2], 0, fw)
    out[:, 3] = np.clip(out[:, 3], 0, fh)
    return out


def box_mask(boxes, vehicle, w, h, first):
    """-> (mask (h, w) uint8, surviving boxes, vehicle_detected)."""
    m = np.zeros((h, w), np.uint8)
    kept, vehicle_detected = 0, False
    for i, box in enumerate(np.asarray(boxes, dtype=np.float32).reshape(-1, 4)):
        x1, y1, x2, y2 = (int(v) for v in np.trunc(box.astype(np.float64)))
        x1, x2 = max(0, min(x1, w - 1)), max(0, min(x2, w - 1))
        y1, y2 = max(0, min(y1, h - 1)), max(0, min(y2, h - 1))
        if x2 <= x1 or y2 <= y1:
            continue
        kept += 1
        if vehicle is not None and vehicle[i]:
            vehicle_detected = True
            r = 0.15 if first else 0.1
            ew, eh = int((x2 - x1) * r), int((y2 - y1) * r)
            x1, y1, x2, y2 = max(0, x1 - ew), max(0, y1 - eh), min(w, x2 + ew), min(h, y2 + eh)
        m[y1:y2, x1:x2] = 1
    return m, kept, vehicle_detected


def assemble(w, h, first, boxes, vehicle, sam_masks, history, *, box_format="xyxy", history_length=5, vehicle_kernels=(7, 5),
             expand_kernel=0, image=None, threshold=0.0, depth=None):
    """One call.  ``history``: the list of (h, w) uint8 entries, oldest first, CHANGED IN PLACE as the call changes the state.
    -> dict of the byte masks (``expanded_*`` / ``valid_rgb`` / ``depth`` None without step 6) and ``info`` (12 integers, INFO's order)."""
    boxes = np.zeros((0, 4), np.float32) if boxes is None else np.asarray(boxes, np.float32).reshape(-1, 4)
    if box_format == "cxcywh":
        boxes = cxcywh_to_xyxy(boxes, w, h)
    bm, kept, vehicle_detected = box_mask(boxes, vehicle, w, h, first)
    union = np.zeros((h, w), np.uint8)
    for m in ([] if sam_masks is None else sam_masks):
        union |= (np.asarray(m).reshape(h, w) != 0).astype(np.uint8)
    use_sam = bool(union.any())
    final = union if use_sam else bm
    filtered = (not first) and (not use_sam)
    if filtered:
        history.append(final.copy())
        if len(history) > history_length:
            history.pop(0)
        n = len(history)
        if n >= 3:
            final = (2 * np.sum(np.stack(history).astype(np.int64), axis=0) > n).astype(np.uint8)
    if vehicle_detected:
        final = dilate(final, vehicle_kernels[0] if first else vehicle_kernels[1])
    out = dict(dynamic=final, static=(1 - final).astype(np.uint8), expanded_dynamic=None, expanded_static=None, valid_rgb=None, depth=None)
    info = dict.fromkeys(INFO, 0)
    info.update(boxes=kept, vehicle_detected=int(vehicle_detected), use_sam_result=int(use_sam), filtered=int(filtered), history=len(history),
                box_pixels=int(bm.sum()), sam_pixels=int(union.sum()), dynamic_pixels=int(final.sum()), static_pixels=int(h * w - final.sum()))
    if expand_kernel:
        e = dilate(final, expand_kernel)
        img = np.asarray(image, np.float32).reshape(3, h, w)
        valid = (((img[0] + img[1]) + img[2]) > np.float32(threshold)) & (e == 0)
        out.update(expanded_dynamic=e, expanded_static=(1 - e).astype(np.uint8), valid_rgb=valid.astype(np.uint8))
        info.update(expanded_pixels=int(e.sum()), valid_pixels=int(valid.sum()))
        if depth is not None:
            d = np.where(valid, np.asarray(depth, np.float32).reshape(h, w), np.float32(0)).astype(np.float32)
            out["depth"] = d
            info["depth_pixels"] = int((d > 0).sum())
    out["info"] = [info[k] for k in INFO]
    return out


class Masker:
    """detect_and_segment's host state around ``assemble``: ``first_frame_processed`` and the history; the fallback branch
    (:887-904) for a frame without boxes: the fallback mask (None: empty) as it is, history untouched."""

    def __init__(self, history_length=5):
        self.history_length = history_length
        self.reset()

    def reset(self):
        self.first_frame_processed, self.history = False, []

    def frame(self, w, h, frame_idx, boxes, labels, sam_masks, fallback=None, **kw):
        first = frame_idx == 0 or not self.first_frame_processed
        self.first_frame_processed = True
        if boxes is None or len(boxes) == 0:
            m = np.zeros((h, w), np.uint8) if fallback is None else (np.asarray(fallback).reshape(h, w) != 0).astype(np.uint8)
            out = assemble(w, h, True, None, None, [m], [], history_length=self.history_length, **kw)
            out["info"][INFO.index("history")] = len(self.history)
            return out
        vehicle = np.array([is_vehicle(s) for s in labels], np.uint8)
        return assemble(w, h, first, boxes, vehicle, sam_masks, self.history, history_length=self.history_length, **kw)
