"""Times the two statements that bracket a tracked frame's loop against their fused forms (``lvdgs.frame_stats``), in one process and
on the same inputs, and the drive's wall time with the two switches off and on.

1. ``Camera.compute_grad_mask`` as ``SlamSequence.new_viewpoint`` calls it against ``frame_stats.edge_mask``: wall time per frame with a
   stream synchronisation on either side.
2. Today's epilogue of a tracked frame -- ``get_median_depth``, ``is_keyframe``, the covisibility ``SlamSequence.step`` reads, and
   ``add_to_window`` with a full window -- against ``frame_summary`` (its one wait) followed by the same functions with ``covis=``.
   Both end with every value on the host, so the wall time is the whole cost.
3. ``--drive``: ``tools/sequence.py``'s 60-frame drive (no colour refinement), frames per second of wall time, with ``frame_stats`` /
   ``edge_mask`` both "torch", the first "fused", and both "fused", in turn, ``--repeats`` times in one process.  The first drive of a
   process also pays the one-off costs (kernel loading, allocator growth): read repeat 0 of the first mode as the cold figure a
   single ``tools/sequence.py`` run reports, the later repeats as the warm ones.

Sizes: KITTI-07's frame (1226 x 370) with 200 k Gaussians, and 1920 x 1080 with 500 k.  The inputs are synthetic (an image of
``tests/frame_stats_cases.py``'s kind, random depths, opacities and visibility rows): none of the statements' cost depends on what
the values are, except the sorts', which random data does not favour.  The sides alternate inside one loop after a warm-up; medians,
extremes and quartiles are reported.  One JSON line per measurement on stdout.
"""
import argparse
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import lvdgs  # noqa: E402,F401
from lvdgs import frame_stats  # noqa: E402
from lvdgs.camera_utils import Camera  # noqa: E402
from lvdgs.keyframe_utils import add_to_window, covisibility, is_keyframe  # noqa: E402
from lvdgs.slam_utils import get_median_depth  # noqa: E402

SIZES = {"kitti07_200k": (370, 1226, 200_000), "1080p_500k": (1080, 1920, 500_000)}


def wall_ms(fns, calls, warmup, dev):
    """Wall milliseconds of each callable with a device synchronisation on either side, the callables alternating."""
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


def test_image(H, W, dev):
    rng = np.random.default_rng(0)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    img = np.stack([0.5 + 0.3 * np.sin(x / 7.0 + c) * np.cos(y / 5.0 - c) for c in range(3)]) + rng.normal(0.0, 0.02, (3, H, W))
    img[:, :H // 3, :W // 4] = 0.0
    return torch.from_numpy(img.astype(np.float32)).to(dev)


def measure_edge_mask(name, H, W, dev, cfg, calls, warmup):
    cam = SimpleNamespace(original_image=test_image(H, W, dev), grad_mask=None)
    fns = {"compute_grad_mask": lambda: Camera.compute_grad_mask(cam, cfg), "edge_mask": lambda: Camera.compute_grad_mask(cam, cfg, fused=True)}
    fns["compute_grad_mask"]()
    a = cam.grad_mask
    fns["edge_mask"]()
    differ = int((a != cam.grad_mask).sum())
    print(json.dumps(dict(what="edge_mask", size=name, height=H, width=W, pixels_that_differ=differ, set_share=round(float(a.float().mean()), 4),
                          **wall_ms(fns, calls, warmup, dev))))


def measure_epilogue(name, H, W, N, dev, cfg, calls, warmup):
    g = torch.Generator(device=dev).manual_seed(1)
    window_size = cfg["Training"]["window_size"]
    depth = torch.rand((1, H, W), device=dev, generator=g) * 60 + 0.5
    depth[torch.rand((1, H, W), device=dev, generator=g) < 0.2] = 0.0
    opacity = torch.where(torch.rand((1, H, W), device=dev, generator=g) < 0.8, 0.99, 0.5)
    n_touched = (torch.rand(N, device=dev, generator=g) < 0.3).int() * 3
    pkg = dict(depth=depth, opacity=opacity, n_touched=n_touched)
    window = list(range(window_size, 0, -1))          # a full window, newest first; the tracked frame is window_size + 1
    occ = {k: (torch.rand(N, device=dev, generator=g) < 0.3).long() for k in window}
    cameras = {k: SimpleNamespace(R=torch.eye(3, device=dev), T=torch.tensor([0.0, 0.0, 0.3 * k], device=dev)) for k in window + [window_size + 1]}
    cur_idx, last = window_size + 1, window[0]

    def today():
        md = get_median_depth(pkg["depth"], pkg["opacity"])
        vis = (pkg["n_touched"] > 0).long()
        kf = is_keyframe(cfg, cameras, cur_idx, last, vis, occ, md)
        inter, union, _, _ = covisibility(vis, occ[last])
        visible = int(vis.count_nonzero())
        return float(md), kf, inter, union, visible, add_to_window(cfg, cameras, cur_idx, vis, occ, window)

    def fused():
        fs = frame_stats.frame_summary(pkg, occ)
        kf = is_keyframe(cfg, cameras, cur_idx, last, None, None, fs.median_depth, covis=fs.covis)
        inter, union, _, _ = fs.covis[last]
        return fs.median_depth, kf, inter, union, fs.visible, add_to_window(cfg, cameras, cur_idx, None, None, window, covis=fs.covis)

    same = today() == fused()
    print(json.dumps(dict(what="epilogue", size=name, height=H, width=W, gaussians=N, window=window_size, same_results=bool(same),
                          **wall_ms({"today": today, "frame_summary": fused}, calls, warmup, dev))))


def measure_drive(dev, frames, repeats):
    import sequence as tool
    for r in range(repeats):
        for stats, edge in (("torch", "torch"), ("fused", "torch"), ("fused", "fused")):
            rec, seq = tool.run_sequence(dev, frames=frames, refine=0, frame_stats=stats, edge_mask=edge)
            print(json.dumps(dict(what="drive", frames=frames, frame_stats=stats, edge_mask=edge, repeat=r, frames_per_s=rec["frames_per_s"],
                                  keyframes=rec["keyframes"], tracking_iterations=rec["tracking_iterations"], seconds=rec["seconds"],
                                  kf_indices=[int(k) for k in seq.kf_indices])), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--drive", action="store_true", help="only measurement 3: the 60-frame drive with the switches off, frame_stats on, and both on")
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    if a.drive:
        measure_drive(dev, a.frames, a.repeats)
        return
    cfg = json.load(open(os.path.join(ROOT, "tests", "golden", "config_07.json")))
    cfg.setdefault("Dataset", {}).setdefault("type", "kitti")
    for name, (H, W, N) in SIZES.items():
        measure_edge_mask(name, H, W, dev, cfg, a.calls, a.warmup)
        measure_epilogue(name, H, W, N, dev, cfg, a.calls, a.warmup)


if __name__ == "__main__":
    main()
