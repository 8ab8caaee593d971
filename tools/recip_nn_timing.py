"""Times ``init_pose.reciprocal_matches`` (one ``lvdgs_reciprocal_nn`` call) at the matcher's raster against a PyTorch restatement of the
reference's own method on the same GPU and inputs, and the matcher's share of one tracked frame's pose initialisation.

Inputs: ``synthetic.WorldDescriptors`` of frames 0 and 3 of the default KITTI-geometry drive at 160 x 512 and at 144 x 512 (what
``init_pose.matcher_raster`` gives a KITTI frame), 24 floats per pixel, subsample 8.

The baseline is the method of ``fast_reciprocal_NNs(..., dist='dot')`` as the reference runs it: per half round, blocks of
``Q @ DB.T`` with ``max`` over each block and a running maximum across blocks, then the active set updated with boolean masks --
which is a device-to-host wait after every half round.  It is the yardstick, not the code under test.

Every call is timed with device events on the current stream after a warm-up; the two sides alternate in one loop; the medians are
reported.  ``--only hip --calls N`` just makes N calls (for a kernel trace: ``rocprofv3 --kernel-trace --stats -d DIR -- python
tools/recip_nn_timing.py --only hip --calls 20``).  One JSON line per measurement on stdout.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import lvdgs  # noqa: E402,F401
from lvdgs import init_pose, synthetic  # noqa: E402


def torch_reciprocal_matches(desc1, desc2, subsample=8, max_iter=10, block=2 ** 13):
    """The reference's method in PyTorch: -> (matches_im1 (M, 2) int32, matches_im2 (M, 2) float32), sorted and distinct as
    ``reciprocal_matches`` returns them."""
    (H1, W1, D), (H2, W2, _) = desc1.shape, desc2.shape
    A, B = desc1.reshape(-1, D), desc2.reshape(-1, D)
    dev = desc1.device

    def nearest(Q, DB):
        best = torch.full((len(Q),), -float("inf"), device=dev)
        idx = torch.zeros(len(Q), dtype=torch.long, device=dev)
        for lo in range(0, len(DB), block):
            v, i = (Q @ DB[lo:lo + block].T).max(dim=1)
            better = v > best
            best = torch.where(better, v, best)
            idx = torch.where(better, i + lo, idx)
        return idx
    ys, xs = torch.arange(subsample // 2, H1, subsample, device=dev), torch.arange(subsample // 2, W1, subsample, device=dev)
    xy1 = (xs[None, :] + W1 * ys[:, None]).reshape(-1)
    xy2 = torch.full_like(xy1, -1)
    old1, old2 = xy1.clone(), xy2.clone()
    notyet = torch.ones(len(xy1), dtype=torch.bool, device=dev)
    for _ in range(max_iter):
        if not bool(notyet.any()):                       # (host wait)
            break
        xy2[notyet] = nearest(A[xy1[notyet]], B)         # (boolean indexing: a host wait for the count)
        notyet &= xy2 != old2
        if bool(notyet.any()):
            xy1[notyet] = nearest(B[xy2[notyet]], A)
            notyet &= xy1 != old1
        old1, old2 = xy1.clone(), xy2.clone()
    conv = ~notyet
    keys = torch.unique(xy1[conv] * (H2 * W2) + xy2[conv])      # sorted, distinct
    a, b = keys // (H2 * W2), keys % (H2 * W2)
    return torch.stack([a % W1, a // W1], 1).int(), torch.stack([b % W2, b // W2], 1).float()


def time_calls(fns, calls, warmup, dev):
    """Median / min / max milliseconds of each callable, alternating them, by device events."""
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize(dev)
    ms = {k: [] for k in fns}
    for _ in range(calls):
        for k, f in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    return {k: dict(median_ms=round(statistics.median(v), 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4), calls=len(v)) for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", choices=["hip"], default=None, help="hip: only make --calls calls of reciprocal_matches at both rasters (for a kernel trace)")
    ap.add_argument("--scale", type=float, default=1.0, help="frame size of the drive (1.0: KITTI's 1226 x 370)")
    a = ap.parse_args()
    import sequence as tool
    from lvdgs.camera_utils import Camera
    from lvdgs.graphics_utils import getProjectionMatrix2
    dev = torch.device("cuda", 0)
    cfg, ds, truth = tool.kitti_sequence(dev, frames=4, scale=a.scale, cadence="short", masks=True)
    wd = synthetic.WorldDescriptors(ds)
    kf, cur = 0, 3
    for raster in ((512, 160), (512, 144)):
        d1, d2 = wd.describe(kf, raster), wd.describe(cur, raster)
        hip = lambda: init_pose.reciprocal_matches(d1, d2, subsample=8, max_iter=10)
        if a.only == "hip":
            for _ in range(a.calls):
                hip()
            torch.cuda.synchronize(dev)
            continue
        m1, m2 = hip()
        lm = init_pose.last_match
        t1, t2 = torch_reciprocal_matches(d1, d2, 8, 10)
        mine = set(map(tuple, torch.cat([m1, m2.int()], 1).cpu().tolist()))
        theirs = set(map(tuple, torch.cat([t1, t2.int()], 1).cpu().tolist()))
        out = time_calls({"hip": hip, "torch_baseline": lambda: torch_reciprocal_matches(d1, d2, 8, 10)}, a.calls, a.warmup, dev)
        print(json.dumps(dict(what="reciprocal_matches", raster=f"{raster[1]}x{raster[0]}", dim=24, subsample=8, seeds=lm.seeds, matches=lm.matches,
                              unconverged=lm.unconverged, rounds=lm.rounds, baseline_matches=len(theirs), pairs_not_shared=len(mine ^ theirs), **out)))
    if a.only == "hip":
        return
    # the share of one tracked frame's pose initialisation: get_pose = matcher + the keyframe's depth render + PnP-RANSAC (the
    # descriptor network's stand-in is left out of both: its maps are made beforehand)
    proj = getProjectionMatrix2(znear=0.01, zfar=100.0, fx=ds.fx, fy=ds.fy, cx=ds.cx, cy=ds.cy, W=ds.width, H=ds.height).transpose(0, 1).to(dev)
    vp = Camera.init_from_dataset(ds, kf, proj)
    vp.update_RT(vp.R_gt, vp.T_gt)
    bg = torch.zeros(3, device=dev)
    raster = init_pose.matcher_raster(ds.width, ds.height)
    maps = (wd.describe(kf, raster), wd.describe(cur, raster))
    matcher = init_pose.DescriptorMatcher(lambda *args: maps)
    out = time_calls({"get_pose": lambda: init_pose.get_pose(ds.images[kf], ds.images[cur], None, None, vp, truth, tool.PIPE, bg, matcher=matcher),
                      "matcher": lambda: matcher(None, None, None, raster)}, a.calls, a.warmup, dev)
    lc = init_pose.last_call
    rel = ds.poses[cur].double().numpy() @ np.linalg.inv(ds.poses[kf].double().numpy())
    pose, _ = init_pose.get_pose(ds.images[kf], ds.images[cur], None, None, vp, truth, tool.PIPE, bg, matcher=matcher)
    print(json.dumps(dict(what="pose_init", raster=f"{raster[1]}x{raster[0]}", inliers=lc.inliers, matches=lc.matches,
                          translation_error=float(np.linalg.norm(pose[:3, 3] - rel[:3, 3])), motion=float(np.linalg.norm(rel[:3, 3])),
                          matcher_share=round(out["matcher"]["median_ms"] / out["get_pose"]["median_ms"], 4), **out)))


if __name__ == "__main__":
    main()
