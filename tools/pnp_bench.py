#!/usr/bin/env python3
"""Wall time per call of the pose initialisation (``lvdgs.init_pose.pnp_ransac`` on a device depth map: two launches and one host
wait) at a KITTI raster (512 x 160, the stride-8 grid: M ~ 1 150) and at M = 20 000, with 128 and 512 hypotheses, measured with device
events around the whole call -- the uploads of the matches and the wait included; the kernels' own time from the library's per-launch
event timing.  ``--get-pose``: also ``init_pose.get_pose`` on a rendered map (the render at the raster + the call).  One JSON line per
figure.

    python tools/pnp_bench.py [--calls 200] [--get-pose]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import lvdgs  # noqa: E402,F401
from lvdgs import _lib, init_pose, synthetic  # noqa: E402
import pnp_cases as pc  # noqa: E402

CASES = {"kitti_raster": lambda: pc.synth(0, 5, 1.0, 0.4), "many_matches": lambda: pc.synth(5, 5, 1.0, 0.4, count=24_500)}


def timed(fn, calls):
    for _ in range(10):
        fn()
    times = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return dict(calls=calls, ms_median=round(float(np.median(times)), 4), ms_min=round(float(np.min(times)), 4), ms_max=round(float(np.max(times)), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--get-pose", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    for name, make in CASES.items():
        c = make()
        depth = torch.from_numpy(c["depth"]).to(dev)
        m1, m2 = torch.from_numpy(c["m1"]).to(dev), torch.from_numpy(c["m2"]).to(dev)      # a matcher on the GPU hands over device tensors
        for hyp in (128, 512):
            kw = {**c["kw"], "hypotheses": hyp}
            fn = lambda: init_pose.pnp_ransac(depth, m1, m2, c["K"], c["dist"], **kw)
            fn()
            _lib.profile_reset()
            _lib.profile_enable(True)
            fn()
            kernels = _lib.profile_read()
            _lib.profile_enable(False)
            line = dict(case=name, matches=len(c["m1"]), hypotheses=hyp, **timed(fn, a.calls))
            lc = init_pose.last_call
            line.update(status=lc.status, inliers=lc.inliers, hypothesis=lc.hypothesis,
                        kernels_us={k: dict(launches=n, us_per_launch=round(1e3 * t / max(n, 1), 2)) for k, (n, t) in kernels.items() if k.startswith("pnp")})
            print(json.dumps(line), flush=True)
    if a.get_pose:
        import sequence as tool
        from lvdgs.camera_utils import Camera
        from lvdgs.graphics_utils import getProjectionMatrix2
        cfg, ds, truth = tool.kitti_sequence(dev, frames=3, scale=1.0, cadence="short", masks=False)
        proj = getProjectionMatrix2(znear=0.01, zfar=100.0, fx=ds.fx, fy=ds.fy, cx=ds.cx, cy=ds.cy, W=ds.width, H=ds.height).transpose(0, 1).to(dev)
        vp = Camera.init_from_dataset(ds, 0, proj)
        vp.update_RT(vp.R_gt, vp.T_gt)
        matcher = synthetic.GroundTruthMatcher(ds, seed=0)
        matcher.set_frames(0, 2)
        matches = matcher(None, None, None, init_pose.matcher_raster(ds.width, ds.height))
        held = tuple(torch.from_numpy(m).to(dev) for m in matches)
        bg = torch.zeros(3, device=dev)
        fn = lambda: init_pose.get_pose(ds.images[0], ds.images[2], None, None, vp, truth, tool.PIPE, bg, matcher=lambda *args: held)
        line = dict(case="get_pose_kitti07", gaussians=int(truth.get_xyz.shape[0]), raster=init_pose.matcher_raster(ds.width, ds.height), matches=len(matches[0]),
                    hypotheses=128, **timed(fn, a.calls))
        line.update(status=init_pose.last_call.status, inliers=init_pose.last_call.inliers)
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    main()
