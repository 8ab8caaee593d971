"""Times the motion mask of the masker's fallback branch -- one ``lvdgs_motion_mask`` call (``lvdgs.optical_flow.motion_mask``: grey,
the four-level Farneback flow, threshold, dilation) -- against ``optical_flow.motion_mask_torch`` on the same device tensors (what
``MotionFallback(fused=False)`` runs: the same text as PyTorch statements, some two thousand small kernels), in one process.

Sizes: KITTI-07's frame (1226 x 370) and a Waymo frame (1920 x 1280); a band-limited texture whose middle third moves by (5, 2) px.
Wall time per call with a device synchronisation on either side, the sides alternating inside one loop after a warm-up; medians,
quartiles and extremes; the library's own per-kernel times (HIP events) from a separate profiled pass.  Per pyramid level the bytes
the call must move -- each launch's inputs read once and outputs written once -- and the launch count.  A ``cv2`` column
(``cv2.calcOpticalFlowFarneback`` on the host with the download and upload around it, as the reference runs it) appears only where
OpenCV imports.  One JSON line per size on stdout.  The two sides' masks are compared before anything is timed; no time is asserted.
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
import torch  # noqa: E402

import lvdgs  # noqa: E402,F401
from lvdgs import _lib  # noqa: E402
from lvdgs import optical_flow as of  # noqa: E402

try:
    import cv2  # noqa: E402
except ImportError:
    cv2 = None

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


def frames(H, W, dev):
    """Two (3, H, W) float32 frames: 24 sinusoids below 0.35 rad/px, the middle third of the second one moved by (5, 2) px."""
    rng = np.random.default_rng(0)
    y, x = torch.meshgrid(torch.arange(H, dtype=torch.float64, device=dev), torch.arange(W, dtype=torch.float64, device=dev), indexing="ij")
    freq, angle, phase = 0.35 * np.sqrt(rng.uniform(0.05, 1, 24)), rng.uniform(0, 2 * np.pi, 24), rng.uniform(0, 2 * np.pi, 24)

    def texture(xs, ys):
        v = sum(torch.sin(f * np.cos(a) * xs + f * np.sin(a) * ys + p) for f, a, p in zip(freq, angle, phase)) / 24
        return (0.5 + 1.1 * v).clamp(0, 1).to(torch.float32)

    inside = (x >= W // 3) & (x < W - W // 3) & (y >= H // 3) & (y < H - H // 3)
    first = texture(x, y)
    second = torch.where(inside, texture(x - 5.0, y - 2.0), texture(x - 0.5, y + 0.25))
    return first.expand(3, H, W).contiguous(), second.expand(3, H, W).contiguous()


def level_traffic(W, H, params):
    """Per level: its size, the launches, and the bytes they must move (inputs once, outputs once)."""
    rows = []
    for lv in of.pyramid(W, H, params["pyr_scale"], params["levels"]):
        px, it = lv["w"] * lv["h"], params["iterations"]
        level = 2 * W * H + 2 * 4 * px                      # both grey planes in, both level images out
        polyexp = 2 * 4 * px + 2 * 20 * px                  # level images in, five channels out, twice
        matrices = 2 * 20 * px + 8 * px + 20 * px           # R0, R1 in (+ a quarter-size flow), flow and M out
        update = it * (20 * px + 8 * px) + (it - 1) * (2 * 20 * px + 20 * px)      # M in, flow out; but for the last: R0, R1 in, M out
        rows.append(dict(level=lv["k"], width=lv["w"], height=lv["h"], blur_taps=lv["ksize"], launches=3 + it,
                         bytes=level + polyexp + matrices + update))
    return rows


def measure(name, H, W, dev, calls, warmup):
    first, second = frames(H, W, dev)
    state = of.MotionState(W, H, dev)
    of.motion_mask(first, state, _lib.MOTION_OBSERVE)
    prev_grey = of.grey_torch(first)
    assert np.array_equal(state.stored(), prev_grey.cpu().numpy())

    def fused():
        return of.motion_mask(second, state)[0]

    def torch_chain():
        return of.motion_mask_torch(prev_grey, second)[0]

    sides = {"lvdgs_motion_mask": fused, "torch_chain": torch_chain}
    if cv2 is not None:
        def host():
            cur = cv2.cvtColor((second.permute(1, 2, 0).cpu().numpy() * 255).astype(np.uint8), cv2.COLOR_RGB2GRAY)
            flow = cv2.calcOpticalFlowFarneback(prev_grey.cpu().numpy(), cur, None, flags=0, **of.DEFAULTS)
            moving = (np.sqrt(flow[..., 0] ** 2 + flow[..., 1] ** 2) > 3.0).astype(np.uint8)
            return torch.from_numpy(cv2.dilate(moving, np.ones((7, 7), np.uint8), iterations=1)).to(dev)
        sides["cv2_host_chain"] = host
    a, b = fused(), torch_chain()
    differing = int((a != b).sum())
    levels = level_traffic(W, H, of.DEFAULTS)
    _lib.profile_enable(True)
    _lib.profile_reset()
    for _ in range(10):
        fused()
    torch.cuda.synchronize(dev)
    kernels = {k: dict(launches_per_call=n // 10, us_per_call=round(1e3 * ms / 10, 2)) for k, (n, ms) in _lib.profile_read().items() if k.startswith("of_")}
    _lib.profile_enable(False)
    print(json.dumps(dict(what="motion_mask", size=name, height=H, width=W, mask_pixels=int(a.sum()), pixels_differing_from_torch=differing,
                          launches=2 + sum(r["launches"] for r in levels) + 2, levels=levels, bytes_all_levels=sum(r["bytes"] for r in levels),
                          kernels=kernels, cv2=cv2 is not None, **wall_ms(sides, calls, warmup, dev))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    for name, (H, W) in SIZES.items():
        measure(name, H, W, dev, a.calls, a.warmup)


if __name__ == "__main__":
    main()
