#!/usr/bin/env python3
"""Run the reference's OWN ``EnhancedDynamicObjectMasker.detect_and_segment`` with its ``_fallback_detection`` (utils/slam_frontend.py
:635-678, :887-904) and ``_refine_with_motion`` (:1106-1149) over scripted sequences in which the detector returns no boxes on some
frames, and store the frames and the masks that came out: the fixture ``MotionFallback`` in the ``fallback`` seat of ``DynamicMasker``
is replayed against.  What is pinned is the reference's handling AROUND the flow: which frames take the early-frame branch, which the
motion branch, which the last resort; where ``prev_frame`` is set (on frames with boxes that are not first) and that the fallback
branch never advances it; the threshold and the dilation of the flow's magnitude.

Run in the authoring container only (needs the reference checkout; never on the GPU box):

    python -B tests/golden/make_motion_fallback_golden.py

How the reference code is made to run here (CPU, no weights, no cv2): as tests/golden/make_dynamic_mask_golden.py does it -- the masker
made WITHOUT ``__init__``, a scripted detector, and a stand-in ``cv2`` in the module's namespace: ``calcOpticalFlowFarneback`` = the
float64 statement of include/lvdgs.h (tests/optical_flow_oracle.py) rounded to float32 as cv2 returns it, ``cvtColor`` = the header's
integer grey, ``dilate`` = scipy.ndimage.maximum_filter(mode="constant", cval=0), once per iteration.  Parity with the real cv2 is
UNPINNED: OpenCV is not installed.  ``_create_conservative_first_frame_mask`` -- a chain of OpenCV calls -- is replaced by a scripted
rectangle; the reference's own two 9 x 9 dilations of it are kept.
No pixel of a motion-branch frame may lie within 1e-4 px of the threshold (asserted; the float32 text is within 1e-5 px of the float64
one on such scenes), so the float32 text gives the same masks.
Nothing of the reference's text is stored: only the scripted inputs and the masks the calls produced.

Fixture: tests/golden/motion_fallback.npz.
"""
import contextlib
import io
import os
import sys
import types

import numpy as np
import scipy.ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_loop_golden import load_reference  # noqa: E402  (puts the shims and the reference on sys.path)
import optical_flow_cases as cases  # noqa: E402
import optical_flow_oracle as oracle  # noqa: E402

W, H = 96, 70
FLOW_KW = dict(oracle.DEFAULTS, flags=0)
# per sequence: (frame_idx, has boxes) -- A: early fallbacks, two CONSECUTIVE motion fallbacks against the last frame with boxes, one
# more after new boxes; B: starts late with fallbacks that have no stored frame, then boxes, then motion
SCRIPTS = (
    [(0, True), (1, False), (2, True), (3, True), (4, False), (5, False), (6, False), (7, True), (8, False)],
    [(7, False), (8, False), (9, True), (10, True), (11, False), (12, False)],
)
CONSERVATIVE = (60, 40, 80, 60)      # x0, y0, x1, y1 of the scripted early-frame mask


def cv2_stand_in(margins):
    def dilate(src, kernel, iterations=1):
        assert kernel.shape[0] == kernel.shape[1] and kernel.all()
        for _ in range(iterations):
            src = scipy.ndimage.maximum_filter(src, size=kernel.shape, mode="constant", cval=0)
        return src

    def grey(img, code):
        q = img.astype(np.int32)
        return ((4899 * q[..., 0] + 9617 * q[..., 1] + 1868 * q[..., 2] + 8192) >> 14).astype(np.uint8)

    def flow(prev, cur, init, **kw):
        assert init is None and kw == FLOW_KW, kw
        f = oracle.farneback(prev, cur, np.float64, **oracle.DEFAULTS)
        margins.append(float(np.abs(np.sqrt((f ** 2).sum(-1)) - 3.0).min()))
        return f.astype(np.float32)

    return types.SimpleNamespace(dilate=dilate, cvtColor=grey, COLOR_RGB2GRAY=7, calcOpticalFlowFarneback=flow)


def frames_of(n, seed):
    """n RGB frames (H, W, 3) uint8: three textures per layer, the background drifting by (0.4, -0.2) px a frame, a rectangle of other
    textures moving by (4.5, 2) px a frame."""
    bg, fg = [cases.texture(seed + c) for c in range(3)], [cases.texture(seed + 10 + c) for c in range(3)]
    x, y = cases.grid(W, H)
    x0, y0, x1, y1 = 14, 18, 44, 44
    out = []
    for i in range(n):
        sx, sy = 4.5 * i, 2.0 * i
        inside = (x - sx >= x0) & (x - sx < x1) & (y - sy >= y0) & (y - sy < y1)
        out.append(np.stack([cases.to_bytes(np.where(inside, f(x - sx, y - sy), b(x - 0.4 * i, y + 0.2 * i))) for b, f in zip(bg, fg)], axis=2))
    return out


def boxes_of(i):
    return np.array([[8.5 + 3 * i, 10.2, 30.9 + 3 * i, 41.7], [50.0, 30.5 + i, 61.3, 55.1 + i]], np.float32), ["car", "person"]


def run_sequence(frontend, script, seed):
    margins = []
    frontend.cv2 = cv2_stand_in(margins)
    cls = frontend.EnhancedDynamicObjectMasker
    m = cls.__new__(cls)
    frame = {}
    m.device, m.initialization_success, m.first_frame_processed = "cpu", True, False
    m.prompt_manager = types.SimpleNamespace(get_current_prompt=lambda: ("car. person.", 0.3), current_scene="scripted")
    m.grounding_detector = types.SimpleNamespace(detect=lambda image, prompt, thr: (frame["boxes"], np.full(len(frame["boxes"]), 0.5), list(frame["labels"])))
    m.use_sam, m.sam_predictor = False, None
    m.prev_frame = m.prev_mask = None
    m.motion_threshold, m.mask_history, m.history_length = 3.0, [], 5
    m.save_images, m.save_dir = False, None
    conservative = np.zeros((H, W), np.uint8)
    conservative[CONSERVATIVE[1]:CONSERVATIVE[3], CONSERVATIVE[0]:CONSERVATIVE[2]] = 1
    m._create_conservative_first_frame_mask = lambda image: conservative.copy()
    rows, closest = [], np.inf
    for i, ((frame_idx, has_boxes), image) in enumerate(zip(script, frames_of(len(script), seed))):
        boxes, labels = boxes_of(i) if has_boxes else (np.zeros((0, 4), np.float32), [])
        frame.update(boxes=boxes, labels=labels)
        prev = None if m.prev_frame is None else m.prev_frame.copy()
        flows = len(margins)
        log = io.StringIO()
        with contextlib.redirect_stdout(log):
            final, _, _ = m.detect_and_segment(image, frame_idx)
        text = log.getvalue()
        assert "❌" not in text, text      # the reference swallows exceptions and prints them: none may have happened
        kind = ("boxes" if has_boxes else "early" if "Applying conservative detection" in text else
                "motion" if "Motion-based fallback detection" in text else "none")
        assert kind != "none" or "WARNING: No dynamic object detection" in text
        stored = m.prev_frame is not None and (prev is None or not np.array_equal(prev, m.prev_frame))
        final = np.asarray(final)
        assert final.shape == (H, W) and set(np.unique(final)) <= {0, 1}
        assert len(margins) - flows == (kind == "motion" or (has_boxes and prev is not None)), (kind, len(margins) - flows)
        if kind == "motion":
            assert margins[-1] > 1e-4, margins[-1]
            closest = min(closest, margins[-1])
        rows.append(dict(frame_idx=frame_idx, has_boxes=has_boxes, image=image, boxes=boxes, labels=labels, kind=kind, stored=stored,
                         dynamic=final.astype(np.uint8)))
    return rows, closest


def main():
    _, frontend = load_reference()
    out = {"size": np.array([W, H]), "sequences": np.array(len(SCRIPTS)), "conservative": np.array(CONSERVATIVE)}
    for s, script in enumerate(SCRIPTS):
        rows, margin = run_sequence(frontend, script, 40 + 100 * s)
        kinds = [r["kind"] for r in rows]
        out[f"s{s}_frame_idx"] = np.array([r["frame_idx"] for r in rows])
        out[f"s{s}_has_boxes"] = np.array([int(r["has_boxes"]) for r in rows])
        out[f"s{s}_stored"] = np.array([int(r["stored"]) for r in rows])      # the call replaced prev_frame
        out[f"s{s}_kind"] = np.array(kinds, dtype=np.str_)
        out[f"s{s}_images"] = np.stack([r["image"] for r in rows])
        for f, r in enumerate(rows):
            out[f"s{s}_f{f}_boxes"] = r["boxes"]
            out[f"s{s}_f{f}_labels"] = np.array(r["labels"], dtype=np.str_)
            out[f"s{s}_f{f}_dynamic"] = np.packbits(r["dynamic"].reshape(-1))
        print(f"sequence {s}: kinds={kinds} stored={out[f's{s}_stored'].tolist()} pixels={[int(r['dynamic'].sum()) for r in rows]} "
              f"closest |magnitude - 3| = {margin:.4f}")
    # the script shows what it is meant to show
    k0, k1 = list(out["s0_kind"]), list(out["s1_kind"])
    assert k0 == ["boxes", "early", "boxes", "boxes", "early", "motion", "motion", "boxes", "motion"], k0
    assert k1 == ["none", "none", "boxes", "boxes", "motion", "motion"], k1
    assert out["s0_stored"].tolist() == [0, 0, 1, 1, 0, 0, 0, 1, 0] and out["s1_stored"].tolist() == [0, 0, 1, 1, 0, 0]
    path = os.path.join(HERE, "motion_fallback.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
