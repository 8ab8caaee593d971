"""Shared inputs of the dynamic-mask tests (tests/test_dynamic_mask.py on the CPU, tests/test_gpu_dynamic_mask.py on the GPU): the
recorded reference sequences of tests/golden/dynamic_mask.npz and seeded random frames.  NumPy only."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LABELS = ("car", "person", "Bus stop", "tree", "minivan", "rider", "a Truck", "bicycle", "dog", "motorcycle")
SHAPE_WIDTHS, SHAPE_HEIGHTS = (1, 7, 63, 64, 65, 127, 129, 200), (1, 2, 9, 37)

_golden = None


def golden():
    """-> (W, H, sequences): per sequence a list of frames, each a dict of the scripted inputs (``frame_idx``, ``boxes``, ``labels``,
    ``sam`` (K', H, W) uint8) and what the reference's calls gave (``first``, ``filtered``, ``history``, ``dilated``, ``dynamic``,
    ``expanded`` under ``expand_kernel``)."""
    global _golden
    if _golden is None:
        z = np.load(os.path.join(HERE, "golden", "dynamic_mask.npz"))
        W, H = (int(v) for v in z["size"])
        bits = lambda a, lead: np.unpackbits(a, axis=-1)[..., :H * W].reshape(lead + (H, W))
        seqs = []
        for s in range(int(z["sequences"])):
            frames = []
            for f in range(int(z["frames"])):
                row = {k: int(z[f"s{s}_{k}"][f]) for k in ("frame_idx", "first", "filtered", "history", "dilated", "expand_kernel")}
                sam = z[f"s{s}_f{f}_sam"]
                row.update(boxes=z[f"s{s}_f{f}_boxes"], labels=[str(v) for v in z[f"s{s}_f{f}_labels"]], sam=bits(sam, (len(sam),)),
                           dynamic=bits(z[f"s{s}_f{f}_dynamic"], ()), expanded=bits(z[f"s{s}_f{f}_expanded"], ()))
                frames.append(row)
            seqs.append(frames)
        _golden = (W, H, seqs)
    return _golden


def random_boxes(rng, W, H, n, box_format="xyxy"):
    """``n`` boxes: ordinary ones, zero-area and inverted ones, boxes outside the frame, boxes that clamp to the last column / row."""
    xy = rng.uniform(-0.2, 1.1, (n, 2)) * [W, H]
    wh = rng.uniform(-0.1, 0.5, (n, 2)) * [W, H]
    b = np.concatenate([xy, xy + wh], axis=1)
    kind = rng.integers(0, 8, n)
    b[kind == 0, 2] = b[kind == 0, 0]                      # zero area
    b[kind == 1] = b[kind == 1][:, [2, 3, 0, 1]]           # (possibly) inverted
    b[kind == 2] += [2.0 * W, 0, 2.0 * W, 0]               # outside
    b[kind == 3, 2] = W + rng.uniform(0, 3, (kind == 3).sum())   # clamps to the last column
    b[kind == 4, 3] = H
    b[kind == 5, :2] = np.floor(b[kind == 5, :2])          # integers: truncation has nothing to do
    if box_format == "cxcywh":
        b = np.stack([(b[:, 0] + b[:, 2]) / 2 / W, (b[:, 1] + b[:, 3]) / 2 / H, (b[:, 2] - b[:, 0]) / W, (b[:, 3] - b[:, 1]) / H], axis=1)
    return b.astype(np.float32)


def random_frame(seed, W, H, num_boxes, num_sam, box_format="xyxy", empty_sam=False):
    """A frame's inputs: boxes, labels, SAM masks (``empty_sam``: all zero), an image whose values are multiples of 1 / 256 (its channel
    sums are exact in any order) with a dark border region, a depth map with non-positive entries."""
    rng = np.random.default_rng([seed, W, H, num_boxes, num_sam])
    boxes = random_boxes(rng, W, H, num_boxes, box_format)
    labels = [LABELS[int(j)] for j in rng.integers(0, len(LABELS), num_boxes)]
    sam = np.zeros((num_sam, H, W), np.uint8)
    if not empty_sam:
        for m in sam:
            x0, y0 = int(rng.integers(0, W)), int(rng.integers(0, H))
            x1, y1 = x0 + 1 + int(rng.integers(0, max(W // 3, 1))), y0 + 1 + int(rng.integers(0, max(H // 3, 1)))
            m[y0:y1, x0:x1] = (rng.random(m[y0:y1, x0:x1].shape) < 0.8) * rng.integers(1, 256)     # nonzero, not only 1
    image = (rng.integers(0, 256, (3, H, W)) / 256.0).astype(np.float32)
    image[:, :, : W // 5] *= (rng.random((H, W // 5)) < 0.5)
    depth = rng.uniform(-0.5, 20.0, (H, W)).astype(np.float32)
    return dict(boxes=boxes, labels=labels, sam=sam, image=image, depth=depth)
