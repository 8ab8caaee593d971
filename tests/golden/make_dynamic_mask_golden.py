#!/usr/bin/env python3
"""Run the reference's OWN ``EnhancedDynamicObjectMasker.detect_and_segment`` (utils/slam_frontend.py:832-1104, with
``_refine_with_motion`` and ``_temporal_consistency``) and ``FrontEnd._expand_dynamic_mask`` (:1260-1266) on scripted detections and
store what went in and what came out, frame by frame, as the fixture lvdgs_dynamic_mask is replayed against.

Run in the authoring container only (needs the reference checkout; never on the GPU box):

    python -B tests/golden/make_dynamic_mask_golden.py

How the reference code is made to run here (CPU, no weights, no cv2):
  * the module is imported as tests/golden/make_loop_golden.py imports it (drop-in shims, empty stand-in modules);
  * the masker is made WITHOUT ``__init__`` (no weights are loaded) and given the attributes ``__init__`` sets; its detector and its
    SAM predictor are scripted objects that hand out the frame's boxes / labels and one mask per ``predict`` call;
  * ``cv2`` in the module's namespace is a stand-in: ``dilate`` = scipy.ndimage.maximum_filter(mode="constant", cval=0) with the
    kernel's size (the documented behaviour of cv2.dilate's default border for a centred kernel of ones; parity with the real
    cv2.dilate is UNPINNED: OpenCV is not installed), ``cvtColor`` = a channel mean, ``calcOpticalFlowFarneback`` = a scripted flow.
Every sequence is generated TWICE, with a zero flow and with a large random one, and the outputs are asserted equal: the reference's
motion refinement is an identity (``~`` of a uint8 array is 254 / 255, true everywhere, :1134).
Nothing of the reference's text is stored: only the scripted inputs and the masks, flags and history lengths the calls produced.

Fixture: tests/golden/dynamic_mask.npz (masks bit-packed, np.packbits of the row-major bytes).
"""
import contextlib
import io
import os
import sys
import types

import numpy as np
import scipy.ndimage
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
from make_loop_golden import load_reference  # noqa: E402  (puts the shims and the reference on sys.path)

W, H, FRAMES = 96, 70, 8


def cv2_stand_in(flow_kind, calls):
    rng = np.random.default_rng(77)

    def dilate(src, kernel, iterations=1):
        calls.append(kernel.shape)
        assert iterations == 1 and kernel.shape[0] == kernel.shape[1] and kernel.all()
        return scipy.ndimage.maximum_filter(src, size=kernel.shape, mode="constant", cval=0)

    def flow(prev, cur, *a, **k):
        return np.zeros(cur.shape + (2,), np.float32) if flow_kind == 0 else (40.0 * rng.standard_normal(cur.shape + (2,))).astype(np.float32)

    return types.SimpleNamespace(dilate=dilate, cvtColor=lambda img, code: img.mean(axis=2).astype(np.uint8), COLOR_RGB2GRAY=7,
                                 calcOpticalFlowFarneback=flow)


def blob(rng, x0, y0, x1, y1):
    """A ragged object inside a rectangle: what a segmenter returns for a box."""
    m = np.zeros((H, W), bool)
    x0, y0, x1, y1 = (int(round(v)) for v in (x0, y0, x1, y1))
    x0, x1, y0, y1 = max(x0, 0), min(x1, W), max(y0, 0), min(y1, H)
    if x1 > x0 and y1 > y0:
        m[y0:y1, x0:x1] = rng.random((y1 - y0, x1 - x0)) < 0.8
    return m


def scripts():
    """Four sequences of FRAMES frames: per frame (frame_idx, boxes (K, 4) float32 xyxy, labels, per-box masks or None = no SAM)."""
    rng = np.random.default_rng(2024)
    f32 = lambda rows: np.array(rows, np.float32).reshape(-1, 4)
    seqs = []
    # A: boxes only; the history passes through lengths 1, 2, 3, 4, 5 and then drops its oldest entry; a car drifts right, a person flickers
    a = []
    for i in range(FRAMES):
        rows, labels = [[10.6 + 4 * i, 30.2, 34.9 + 4 * i, 52.7]], ["car"]
        if i % 3 != 1:
            rows.append([60.0, 12.5 + i, 70.3, 40.1 + i]); labels.append("person")
        a.append((i, f32(rows), labels, None))
    seqs.append(a)
    # B: SAM on most frames; an EMPTY union on frames 2 and 5 (falls back to the boxes and filters); non-vehicle-only frames 3, 4
    b = []
    for i in range(FRAMES):
        if i in (3, 4):
            rows, labels = [[20.2, 8.8, 50.5, 30.1 + i], [5.0, 40.0, 18.9, 66.0]], ["person", "a dog"]
        else:
            rows, labels = [[30.3 - 2 * i, 20.0, 71.9 - 2 * i, 55.5], [70.1, 5.5, 93.8, 33.3]], ["white truck", "cyclist"]
        masks = [np.zeros((H, W), bool) for _ in rows] if i in (2, 5) else [blob(rng, *r) for r in rows]
        b.append((i, f32(rows), labels, masks))
    seqs.append(b)
    # C: starts at frame 3 (first by the flag, not by the index); dropped boxes (zero area, inverted, outside), boxes on every border,
    # vehicle boxes that clamp to the last column / row and are widened onto them; no SAM
    c = []
    for i in range(FRAMES):
        rows = [[0.0, 0.0, 12.9, 9.9], [80.2, 0.0, 96.0, 15.0], [0.0, 55.5, 20.0, 70.0], [70.7, 50.1, 96.0, 70.0],
                [40.0, 30.0, 40.9, 50.0], [50.0, 40.0, 45.0, 60.0], [120.0, 90.0, 150.0, 95.0], [-30.5, -20.5, 8.2 + i, 6.6 + i],
                [33.3, 0.0, 60.0 + i, 3.9]]
        labels = ["bus", "van" if i % 2 else "pole", "bike", "SUV parked", "car", "truck", "car", "person", "motorcycle" if i > 4 else "sign"]
        c.append((i + 3, f32(rows), labels, None))
    seqs.append(c)
    # D: random boxes, SAM on alternating pairs of frames, a frame where SAM answers for some boxes with empty masks only
    d = []
    words = ["car", "person", "Bus stop", "tree", "minivan", "rider", "vehicle", "bicycle"]
    for i in range(FRAMES):
        k = int(rng.integers(1, 6))
        xy = rng.uniform(-10, [W + 10, H + 10], (k, 2))
        wh = rng.uniform(-4, 40, (k, 2))
        rows = np.concatenate([xy, xy + wh], axis=1)
        labels = [words[int(j)] for j in rng.integers(0, len(words), k)]
        masks = None
        if (i // 2) % 2 == 1:
            masks = [blob(rng, *r) if rng.random() < 0.7 else np.zeros((H, W), bool) for r in rows]
        d.append((i, f32(rows), labels, masks))
    seqs.append(d)
    return seqs


def run_sequence(frontend, script, flow_kind):
    calls = []
    frontend.cv2 = cv2_stand_in(flow_kind, calls)
    cls = frontend.EnhancedDynamicObjectMasker
    m = cls.__new__(cls)
    frame = {}
    m.device, m.initialization_success, m.first_frame_processed = "cpu", True, False
    m.prompt_manager = types.SimpleNamespace(get_current_prompt=lambda: ("car. person.", 0.3), current_scene="scripted")
    m.grounding_detector = types.SimpleNamespace(detect=lambda image, prompt, thr: (frame["boxes"], np.full(len(frame["boxes"]), 0.5), list(frame["labels"])))

    def predict(point_coords=None, point_labels=None, box=None, multimask_output=False):
        frame["used"].append(frame["masks"][len(frame["used"])])
        return frame["used"][-1][None], np.ones(1), None

    m.sam_predictor = types.SimpleNamespace(set_image=lambda image: None, predict=predict)
    m.prev_frame = m.prev_mask = None
    m.motion_threshold, m.mask_history, m.history_length = 3.0, [], 5
    m.save_images, m.save_dir = False, None
    rng = np.random.default_rng(5)
    rows = []
    for frame_idx, boxes, labels, masks in script:
        frame.update(boxes=boxes, labels=labels, masks=masks, used=[])
        m.use_sam = masks is not None
        first = frame_idx == 0 or not m.first_frame_processed
        n_hist, n_dil = len(m.mask_history), len(calls)
        appended = []
        real = cls._temporal_consistency
        m._temporal_consistency = lambda cur, _m=m: (appended.append(1), real(_m, cur))[1]
        image = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
        log = io.StringIO()
        with contextlib.redirect_stdout(log):
            final, _, _ = m.detect_and_segment(image, frame_idx)
            k = 9 if frame_idx == 0 else 7
            expanded = frontend.FrontEnd._expand_dynamic_mask(None, torch.from_numpy(np.asarray(final)).bool(), kernel_size=k)
        final = np.asarray(final)
        # the reference swallows exceptions and prints them: none may have happened, and the scripted flow was consumed
        assert "\u274c" not in log.getvalue() and ("Motion refinement" in log.getvalue()) == (not first and len(rows) >= 2), log.getvalue()
        assert final.shape == (H, W) and set(np.unique(final)) <= {0, 1}
        rows.append(dict(frame_idx=frame_idx, boxes=boxes, labels=labels, sam=np.array(frame["used"], bool).reshape(-1, H, W), first=first,
                         dynamic=final.astype(np.uint8), expanded=expanded.numpy().astype(np.uint8), expand_kernel=k,
                         filtered=bool(appended), history=len(m.mask_history), dilated=len(calls) - n_dil - 1))
        assert len(m.mask_history) - n_hist in (0, 1)
    return rows


def main():
    _, frontend = load_reference()
    out = {"size": np.array([W, H]), "sequences": np.array(4), "frames": np.array(FRAMES)}
    for s, script in enumerate(scripts()):
        a, b = run_sequence(frontend, script, 0), run_sequence(frontend, script, 1)
        for ra, rb in zip(a, b):      # the motion refinement is an identity: the flow never shows
            assert np.array_equal(ra["dynamic"], rb["dynamic"]) and np.array_equal(ra["expanded"], rb["expanded"])
            assert (ra["filtered"], ra["history"], ra["dilated"]) == (rb["filtered"], rb["history"], rb["dilated"])
        for key in ("frame_idx", "first", "filtered", "history", "dilated", "expand_kernel"):
            out[f"s{s}_{key}"] = np.array([int(r[key]) for r in a])
        for f, r in enumerate(a):
            out[f"s{s}_f{f}_boxes"] = r["boxes"]
            out[f"s{s}_f{f}_labels"] = np.array(r["labels"], dtype=np.str_)
            out[f"s{s}_f{f}_sam"] = np.packbits(r["sam"].reshape(len(r["sam"]), H * W), axis=1)
            out[f"s{s}_f{f}_dynamic"] = np.packbits(r["dynamic"].reshape(-1))
            out[f"s{s}_f{f}_expanded"] = np.packbits(r["expanded"].reshape(-1))
        print(f"sequence {s}: first={out[f's{s}_first'].tolist()} filtered={out[f's{s}_filtered'].tolist()} history={out[f's{s}_history'].tolist()} "
              f"dilated={out[f's{s}_dilated'].tolist()} pixels={[int(r['dynamic'].sum()) for r in a]}")
    path = os.path.join(HERE, "dynamic_mask.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
