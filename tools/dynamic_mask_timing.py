"""Times the assembly of a keyframe's dynamic-object masks -- one ``lvdgs_dynamic_mask`` call (``lvdgs.dynamic_mask.assemble``) --
against two baselines, in one process and on the same inputs:

* ``torch_chain``: ``dynamic_mask.assemble_torch`` on the device tensors (what ``DynamicMasker(fused=False)`` runs): the boxes are read
  on the host, the rest are PyTorch kernels, every count is waited for;
* ``host_chain``: what the reference does around its two networks (utils/slam_frontend.py:906-1056, :1260-1266, :1290-1333), restated
  with NumPy and ``scipy.ndimage`` in place of ``cv2``: the frame copied to the host and quantised, rectangle fills, the OR over the SAM
  masks (downloaded: the reference's SAM predictor returns host arrays), ``np.median`` over the history, two maximum filters, the
  uploads of the masks and the two waited-for means.

Sizes: KITTI-07's frame (1226 x 370) and a Waymo frame (1920 x 1280); six boxes, and either no SAM masks (the temporal filter runs
over a full five-entry history) or six of them.  Wall time per call with a device synchronisation on either side, the sides
alternating inside one loop after a warm-up; medians, quartiles and extremes.  One JSON line per measurement on stdout.  The three
sides are checked to give the same masks before anything is timed.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import scipy.ndimage  # noqa: E402
import torch  # noqa: E402

import lvdgs  # noqa: E402,F401
from lvdgs import dynamic_mask as dm  # noqa: E402

SIZES = {"kitti07": (370, 1226), "waymo": (1280, 1920)}


def wall_ms(fns, calls, warmup, dev):
    for _ in range(warmup):
        for f in fns.values():
            f()
    ms = {k: [] for k in fns}
    for _ in range(calls):
        for k, f in fns.items():
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize(dev)
            ms[k].append(1e3 * (time.perf_counter() - t0))
    out = {}
    for k, v in ms.items():
        q = statistics.quantiles(v, n=4)
        out[k] = dict(median_ms=round(statistics.median(v), 4), q1_ms=round(q[0], 4), q3_ms=round(q[2], 4), min_ms=round(min(v), 4),
                      max_ms=round(max(v), 4), calls=len(v))
    return out


def host_chain(image, boxes, vehicle, sam, history, k2, thr, dev):
    """The reference's statements for a keyframe that is not a first frame; ``history``: the list of host masks (not changed: every
    timed call sees the same state).  -> (static, expanded_static, valid_rgb on the device, the two ratios)."""
    _, H, W = image.shape
    img_np = (image.permute(1, 2, 0).cpu().numpy() * 255).astype(np.uint8)      # the detector's input (:1300-1301)
    box_mask = np.zeros((H, W), np.uint8)
    vehicle_detected = False
    for box, veh in zip(boxes.cpu().numpy(), vehicle):
        x1, y1, x2, y2 = box.astype(int)
        x1, x2 = max(0, min(x1, W - 1)), max(0, min(x2, W - 1))
        y1, y2 = max(0, min(y1, H - 1)), max(0, min(y2, H - 1))
        if x2 <= x1 or y2 <= y1:
            continue
        if veh:
            vehicle_detected = True
            ew, eh = int((x2 - x1) * 0.1), int((y2 - y1) * 0.1)
            x1, y1, x2, y2 = max(0, x1 - ew), max(0, y1 - eh), min(W, x2 + ew), min(H, y2 + eh)
        box_mask[y1:y2, x1:x2] = 1
    final = box_mask.copy()
    use_sam = False
    if sam is not None:
        union = np.zeros((H, W), np.uint8)
        for m in sam.cpu().numpy():
            union = np.logical_or(union, m.astype(np.uint8)).astype(np.uint8)
        if union.sum() > 0:
            final, use_sam = union, True
    if not use_sam:
        stack = np.stack((history + [final.copy()])[-5:], axis=0)
        if len(stack) >= 3:
            final = np.median(stack, axis=0).astype(np.uint8)
    if vehicle_detected and final.sum() > 0:
        final = scipy.ndimage.maximum_filter(final, size=(5, 5), mode="constant", cval=0)
    static_np = (1 - final).astype(np.uint8)
    dynamic = torch.from_numpy(1 - static_np).to(dev).bool()
    static = torch.from_numpy(static_np).to(dev).bool()
    grown_np = scipy.ndimage.maximum_filter(dynamic.cpu().numpy().astype(np.uint8), size=(k2, k2), mode="constant", cval=0)
    expanded_static = ~torch.from_numpy(grown_np).to(dev).bool()
    valid_rgb = (image.sum(dim=0) > thr) & expanded_static
    return static, expanded_static, valid_rgb, static.float().mean().item(), expanded_static.float().mean().item(), img_np.shape


def measure(name, H, W, with_sam, dev, calls, warmup):
    rng = np.random.default_rng(0)
    K, k2, thr = 6, 7, 0.01
    xy = rng.uniform(0.05, 0.7, (K, 2)) * [W, H]
    wh = rng.uniform(0.05, 0.25, (K, 2)) * [W, H]
    boxes = torch.from_numpy(np.concatenate([xy, xy + wh], axis=1).astype(np.float32)).to(dev)
    vehicle = [True, False, True, True, False, True]
    vehicle_dev = torch.tensor(vehicle, dtype=torch.uint8, device=dev)
    image = torch.from_numpy((rng.integers(0, 256, (3, H, W)) / 256.0).astype(np.float32)).to(dev)
    sam = None
    if with_sam:
        sam = torch.zeros((K, H, W), dtype=torch.bool, device=dev)
        for m, b in zip(sam, boxes.cpu().numpy().astype(int)):
            m[b[1]:b[3], b[0]:b[2]] = torch.rand((b[3] - b[1], b[2] - b[0]), device=dev) < 0.8
    # a full history: five earlier box masks, slightly shifted
    full = dm.MaskHistory(W, H, 5, dev)
    torch_history, host_history = [], []
    for j in range(5):
        shifted = boxes + float(3 * (j + 1))
        dm.assemble(W, H, shifted, vehicle_dev, None, first_frame=False, history=full)
        dm.assemble_torch(W, H, shifted, vehicle, None, first_frame=False, history=torch_history)
    host_history = [h.cpu().numpy().astype(np.uint8) for h in torch_history]
    work = dm.MaskHistory(W, H, 5, dev)

    def fused():
        work.block.copy_(full.block)      # every timed call sees the same state (a device-to-device copy of 37 / 123 kB, in the timing)
        return dm.assemble(W, H, boxes, vehicle_dev, sam, first_frame=False, history=work, expand_kernel=k2, image=image, rgb_boundary_threshold=thr)

    def torch_chain():
        return dm.assemble_torch(W, H, boxes, vehicle, sam, first_frame=False, history=list(torch_history), expand_kernel=k2, image=image,
                                 rgb_boundary_threshold=thr)

    def host():
        return host_chain(image, boxes, vehicle, sam, host_history, k2, thr, dev)

    a, b, c = fused(), torch_chain(), host()
    same = all(torch.equal(getattr(a, n), getattr(b, n)) for n in dm.OUTPUTS) and torch.equal(a.static_mask, c[0]) \
        and torch.equal(a.expanded_static_mask, c[1]) and torch.equal(a.valid_rgb, c[2])
    print(json.dumps(dict(what="dynamic_mask", size=name, height=H, width=W, boxes=K, sam_masks=K if with_sam else 0, history=5,
                          same_masks=bool(same), info=a.info_dict(),
                          **wall_ms({"lvdgs_dynamic_mask": fused, "torch_chain": torch_chain, "host_chain": host}, calls, warmup, dev))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    for name, (H, W) in SIZES.items():
        for with_sam in (False, True):
            measure(name, H, W, with_sam, dev, a.calls, a.warmup)


if __name__ == "__main__":
    main()
