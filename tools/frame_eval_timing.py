#!/usr/bin/env python3
"""Times the per-frame block of ``eval_rendering`` (reference utils/eval_utils_0806.py:216-312) on the device:

    python tools/frame_eval_timing.py [--repeats 30] [--out profiles/frame_eval_timing.json]

 (a) today's path: ``eval_utils.frame_metrics`` (boolean gathers, two ``lvdgs_ssim_l1`` calls, five ``float()`` reads) plus the
     reference's quantisation and depth statements written in torch on the device, with the copy of the three byte images and the
     depth image to the host that its ``Image.fromarray`` calls need;
 (b) one ``FrameEvaluator.add`` without and with the byte outputs (no wait in the call; the timed region ends with a stream wait), and
     with the four byte images copied to the host as well -- the like-for-like partner of (a) with its copies.
At 1226 x 370 and 1920 x 1280, static mask and depth map present.  Per variant: the median device time between two events recorded
around the call on the stream (for (a) that span includes the host waits inside it -- the device idles while the host reads) and the
median wall time, after warm-up calls; for (b) also the three launches by the library's own events and the algorithmic bytes per
pixel against the HBM rate.  No time is asserted anywhere."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import lvdgs  # noqa: E402,F401
from lvdgs import _lib  # noqa: E402
from lvdgs.eval_utils import FrameEvaluator, frame_metrics  # noqa: E402

HBM_TB_PER_S = 8.0      # MI355X peak


def torch_quantisation(rendering, gt_image, depth):
    """The reference's :221-225 and :309-312 as torch statements on the device, and the host copies its PIL calls take."""
    image = torch.clamp(rendering, 0.0, 1.0)
    gt = (gt_image.permute(1, 2, 0) * 255).to(torch.uint8)
    pred = (image.permute(1, 2, 0) * 255).to(torch.uint8)
    residual = (pred.float() - gt.float()).abs().clamp(0, 255).to(torch.uint8)
    d = depth.squeeze()
    depth_max, depth_min = d.max(), d.min()
    depth8 = (((d - depth_min) / (depth_max - depth_min)) * 255).to(torch.uint8)
    return pred.cpu(), gt.cpu(), residual.cpu(), depth8.cpu()


def timed(fn, repeats, warmup, dev):
    """-> medians of (device ms between two events around ``fn``, wall ms up to the end of the stream's work)."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize(dev)
    device_ms, wall_ms = [], []
    for _ in range(repeats):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        start.record()
        fn()
        stop.record()
        stop.synchronize()
        wall_ms.append(1e3 * (time.perf_counter() - t0))
        device_ms.append(start.elapsed_time(stop))
    return dict(device_ms=round(statistics.median(device_ms), 4), wall_ms=round(statistics.median(wall_ms), 4),
                device_ms_best=round(min(device_ms), 4))


def size_record(W, H, dev, repeats, warmup):
    g = torch.Generator().manual_seed(W)
    gt = torch.rand(3, H, W, generator=g)
    gt[:, : H // 16] = 0.0
    render = ((gt + 0.1 * torch.randn(3, H, W, generator=g)) * 1.2 - 0.1).to(dev)
    gt = gt.to(dev)
    mask = (torch.rand(H, W, generator=g) > 0.3).to(dev)
    depth = (torch.rand(1, H, W, generator=g) * 40 + 0.5).to(dev)
    bg = torch.zeros(3, device=dev)
    rec = dict(frame=f"{W}x{H}")
    rec["a_frame_metrics"] = timed(lambda: frame_metrics(render, gt, mask, bg), repeats, warmup, dev)
    rec["a_frame_metrics_plus_quantisation"] = timed(lambda: (frame_metrics(render, gt, mask, bg), torch_quantisation(render, gt, depth)), repeats, warmup, dev)
    for name, images in (("b_add", False), ("b_add_with_bytes", True)):
        ev = FrameEvaluator(H, W, dev, 1, want_images=images)
        rec[name] = timed(lambda: (ev.reset(), ev.add(render, gt, mask, bg, depth)), repeats, warmup, dev)      # (reset: a host counter)
        if images:      # like for like with (a): the four byte images copied to the host, as saving them takes
            rec[name + "_copied"] = timed(lambda: (ev.reset(), [v.cpu() for v in ev.images(ev.add(render, gt, mask, bg, depth)).values()]),
                                          repeats, warmup, dev)
        ev.reset()
        _lib.profile_enable(True)
        _lib.profile_reset()
        for _ in range(repeats):
            ev.add(render, gt, mask, bg, depth)
            ev.reset()
        torch.cuda.synchronize(dev)
        prof = _lib.profile_read()
        _lib.profile_enable(False)
        rec[name]["launch_us"] = {k: round(1e3 * ms / n, 2) for k, (n, ms) in prof.items() if k.startswith("frame_eval")}
    # algorithmic bytes per pixel, each read once: render 12 + gt 12 + mask 1 + depth 4 = 29; with the byte outputs 9 + 1 written
    # and the depth read again by the third launch
    us = rec["b_add"]["launch_us"].get("frame_eval", 0.0)
    rec["b_add"]["bytes_per_pixel"] = 29
    rec["b_add"]["fraction_of_hbm_rate"] = round(29 * W * H / (us * 1e-6) / (HBM_TB_PER_S * 1e12), 4) if us else None
    us = sum(rec["b_add_with_bytes"]["launch_us"].values())
    rec["b_add_with_bytes"]["bytes_per_pixel"] = 29 + 10 + 4
    rec["b_add_with_bytes"]["fraction_of_hbm_rate"] = round(43 * W * H / (us * 1e-6) / (HBM_TB_PER_S * 1e12), 4) if us else None
    rec["speedup_wall_with_bytes_copied"] = round(rec["a_frame_metrics_plus_quantisation"]["wall_ms"] / rec["b_add_with_bytes_copied"]["wall_ms"], 2)
    rec["speedup_wall_metrics_only"] = round(rec["a_frame_metrics"]["wall_ms"] / rec["b_add"]["wall_ms"], 2)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frame_eval_timing.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    out = dict(device=torch.cuda.get_device_name(dev), repeats=a.repeats, warmup=a.warmup, hbm_tb_per_s_assumed=HBM_TB_PER_S,
               note="(a) = frame_metrics + the reference's quantisation in torch with its host copies; (b) = one FrameEvaluator.add; "
                    "device_ms is the span between two stream events around the call, which for (a) includes its host waits",
               frames=[size_record(1226, 370, dev, a.repeats, a.warmup), size_record(1920, 1280, dev, a.repeats, a.warmup)])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
