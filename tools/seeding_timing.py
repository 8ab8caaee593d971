"""Times the seeding of a keyframe's Gaussians, ``GaussianModel.seeding = "host"`` (the PyTorch statements and the host draw) against
``"fused"`` (one ``lvdgs_seed_points`` call and one wait), in one process and on the same inputs:

* ``create_pcd_from_image``: the back-projection, the subsample, the colours, the kNN scales -- everything but the append;
* ``extend_from_pcd_seq``: the same and the append to a map of a fixed size (a fresh copy of it for every call, made outside the clock);
* for the fused path the stages on their own: the library call with its wait, the kNN and scale statements after the wait, the append.

Sizes: KITTI-07's frame (1226 x 370) with one seed per 32 and per 64 valid pixels (the first frame's and the later keyframes'
``pcd_downsample``), and a Waymo frame (1920 x 1280) with 64; about 80 % of the depth map valid; ``adaptive_pointsize`` on, as in the
reference's configurations.  Wall time per call with a device synchronisation on either side, the two modes alternating inside one loop
after a warm-up; medians and minima.  One JSON line on stdout and in ``profiles/seeding_timing.json``.  Needs a GPU.
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
from lvdgs.camera_utils import Camera  # noqa: E402
from lvdgs.gaussian_model import GaussianModel  # noqa: E402
from lvdgs.graphics_utils import focal2fov, getProjectionMatrix2  # noqa: E402

CASES = [("kitti07_ds32", 1226, 370, 707.0912, 601.8873, 183.1104, 32), ("kitti07_ds64", 1226, 370, 707.0912, 601.8873, 183.1104, 64),
         ("waymo_ds64", 1920, 1280, 2066.697564417299, 950.5512774150723, 641.1870541472169, 64)]
OPT = dict(position_lr_init=0.0016, position_lr_final=0.00016, position_lr_delay_mult=0.01, position_lr_max_steps=30000,
           feature_lr=0.0025, opacity_lr=0.05, scaling_lr=0.001, rotation_lr=0.001, percent_dense=0.01,
           densify_grad_threshold=0.0002, lambda_dssim=0.2)
BASE_MAP = 60_000      # Gaussians in the map a keyframe is appended to


def wall_ms(fns, calls, warmup, dev, before=None):
    """{name: [ms per call]}; ``before(name)``: preparation outside the clock, its result passed to the timed function."""
    ms = {k: [] for k in fns}
    for it in range(warmup + calls):
        for k, f in fns.items():
            arg = before(k) if before else None
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            f(arg) if before else f()
            torch.cuda.synchronize(dev)
            if it >= warmup:
                ms[k].append(1e3 * (time.perf_counter() - t0))
    return ms


def stats(v):
    return dict(median_ms=round(statistics.median(v), 4), min_ms=round(min(v), 4), calls=len(v))


def camera(W, H, fx, cx, cy, dev, rng):
    image = torch.from_numpy(rng.random((3, H, W)).astype(np.float32)).to(dev)
    proj = getProjectionMatrix2(znear=0.01, zfar=100.0, fx=fx, fy=fx, cx=cx, cy=cy, W=W, H=H).transpose(0, 1)
    cam = Camera(0, image, None, None, torch.eye(4), proj.to(dev), fx, fx, cx, cy, focal2fov(fx, W), focal2fov(fx, H), H, W, device=str(dev))
    with torch.no_grad():
        cam.exposure_a.fill_(0.05)
        cam.exposure_b.fill_(-0.01)
    return cam


def model(mode, ds, dev, base=None):
    cfg = {"Dataset": {"sensor_type": "depth", "pcd_downsample": ds, "pcd_downsample_init": ds, "point_size": 0.01, "adaptive_pointsize": True}}
    m = GaussianModel(0, config=cfg, device=str(dev))
    m.seeding = mode
    m.init_lr(6.0)
    m.training_setup(OPT)
    if base is not None:
        m.extend_from_pcd(*[t.clone() for t in base], kf_id=0)
    return m


def measure(name, W, H, fx, cx, cy, ds, dev, calls, warmup):
    rng = np.random.default_rng(0)
    cam = camera(W, H, fx, cx, cy, dev, rng)
    d = (2.0 + 40.0 * rng.random((H, W))).astype(np.float32)
    d[rng.random((H, W)) > 0.8] = 0.0
    depth = torch.from_numpy(d).to(dev)
    n = BASE_MAP
    base = (torch.from_numpy(rng.standard_normal((n, 3)).astype(np.float32)).to(dev) * 20, torch.zeros(n, 3, 1, device=dev), torch.zeros(n, 3, device=dev),
            torch.zeros(n, 4, device=dev), torch.zeros(n, 1, device=dev))
    seeders = {mode: model(mode, ds, dev) for mode in ("host", "fused")}
    pcd = wall_ms({mode: (lambda m=m: m.create_pcd_from_image(cam, init=False, depthmap=depth)) for mode, m in seeders.items()}, calls, warmup, dev)
    ext = wall_ms({mode: (lambda m: m.extend_from_pcd_seq(cam, kf_id=1, init=False, depthmap=depth)) for mode in seeders}, calls, warmup, dev,
                  before=lambda mode: model(mode, ds, dev, base))
    # the fused path's stages
    m = seeders["fused"]
    held = {}

    def call(_):
        held["pts"] = m._seed_fused(cam, depth, ds, 0.01)

    def after(_):
        xyz, colors, f_dc, point_size = held["pts"]
        held["seeds"] = m._seeds_from_points(xyz, colors, f_dc, point_size)

    def append(target):
        target.extend_from_pcd(*held["seeds"], kf_id=1)

    stages = wall_ms({"call": call, "after_wait": after, "append": append}, calls, warmup, dev,
                     before=lambda k: model("fused", ds, dev, base) if k == "append" else None)
    med = {k: statistics.median(v) for k, v in stages.items()}
    out = dict(size=name, width=W, height=H, downsample=ds, valid_share=round(float((d > 0).mean()), 4), seeds=int(held["seeds"][0].shape[0]),
               base_map=BASE_MAP,
               create_pcd_from_image={k: stats(v) for k, v in pcd.items()}, extend_from_pcd_seq={k: stats(v) for k, v in ext.items()},
               fused_stages={k: stats(v) for k, v in stages.items()},
               fused_share_after_wait=round((med["after_wait"] + med["append"]) / (med["call"] + med["after_wait"] + med["append"]), 4))
    print(f"  {name}: create_pcd host {out['create_pcd_from_image']['host']['median_ms']} ms, fused {out['create_pcd_from_image']['fused']['median_ms']} ms; "
          f"extend host {out['extend_from_pcd_seq']['host']['median_ms']} ms, fused {out['extend_from_pcd_seq']['fused']['median_ms']} ms", file=sys.stderr)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seeding_timing.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("seeding_timing needs a GPU")
    dev = torch.device("cuda", 0)
    out = dict(what="seeding", device=torch.cuda.get_device_name(dev), calls=a.calls, warmup=a.warmup,
               cases=[measure(*case, dev, a.calls, a.warmup) for case in CASES])
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
