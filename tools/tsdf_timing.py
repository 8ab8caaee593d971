#!/usr/bin/env python3
"""Times TSDF fusion and mesh extraction on the device (``lvdgs.tsdf``: ``lvdgs_tsdf_integrate``, ``lvdgs_tsdf_mesh``):

    python tools/tsdf_timing.py [--repeats 10] [--out profiles/tsdf_timing.json]

For a 256^3 volume with frames of 1226 x 370 and a 512 x 512 x 256 volume with frames of 1920 x 1280 (colour planes, 16 views of a wavy
wall that crosses the volume, seen from in front of it):
 (a) ``integrate_views`` with 1 view per call and with 16 views per call -- device time between two stream events around the calls,
     after warm-up, on a volume that already holds state (so every touched row is read and written);
 (b) the same voxel-major rule restated in PyTorch on the same device (one pass of elementwise kernels over the whole volume per
     view), for 1 and for 16 views;
 (c) ``extract_mesh`` (its one wait inside the timed span), and the six launches by the library's own events;
 (d) the bytes each must move at the least, against the HBM rate: integrate reads and writes the five planes of the bricks some view
     can touch once per CALL (40 bytes per voxel of those bricks; the share of such voxels is reported) plus the frames; the mesh
     passes read tsdf and weight once (8), write and read the class byte and the edge byte (4) and read the class byte again for the
     vertices (1): 13 bytes per sample, plus the outputs.
No time is asserted anywhere."""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import lvdgs  # noqa: E402,F401
from lvdgs import _lib  # noqa: E402
from lvdgs.tsdf import TsdfVolume  # noqa: E402

HBM_TB_PER_S = 8.0      # MI355X peak


def events_ms(fn, repeats, warmup, dev):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize(dev)
    times = []
    for _ in range(repeats):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        stop.record()
        stop.synchronize()
        times.append(start.elapsed_time(stop))
    return dict(ms=round(statistics.median(times), 4), ms_best=round(min(times), 4))


def make_views(dims, voxel, W, H, dev, count=16):
    """Cameras in front of the volume's -z face that look into it at a wavy wall two thirds of the way through."""
    nx, ny, nz = dims
    ext = [voxel * (n - 1) for n in dims]
    fx = fy = 0.9 * W
    views = []
    g = torch.Generator().manual_seed(1)
    vi, ui = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    for n in range(count):
        a = 0.12 * math.sin(0.7 * n)      # yaw about y
        R = torch.tensor([[math.cos(a), 0.0, -math.sin(a)], [0.0, 1.0, 0.0], [math.sin(a), 0.0, math.cos(a)]])
        C = torch.tensor([ext[0] * (0.5 + 0.02 * n - 0.15), ext[1] * 0.5 + 0.01 * n, -0.6 * ext[2]])
        T = -R @ C
        wall = 0.6 * ext[2] + 0.66 * ext[2]      # camera depth of the wall along the axis
        depth = wall * (1.0 + 0.04 * torch.sin(ui / 37.0 + n) * torch.cos(vi / 29.0))
        image = torch.rand(3, H, W, generator=g)
        views.append(dict(depth=depth.to(dev).contiguous(), R=R.to(dev), T=T.to(dev), intrinsics=(fx, fy, W / 2.0 - 0.25, H / 2.0 - 0.25),
                          image=image.to(dev), mask=None, depth_min=0.0, depth_trunc=float("inf")))
    return views


def torch_integrate(planes, lattice, views, trunc, max_weight):
    """The header's rule, voxel-major, as PyTorch statements over the whole volume; ``planes``: (5, n), ``lattice``: (px, py, pz)."""
    px, py, pz = lattice
    tsdf, weight = planes[0], planes[1]
    for V in views:
        R, T = V["R"], V["T"]
        fx, fy, cx, cy = V["intrinsics"]
        H, W = V["depth"].shape
        x = R[0, 0] * px + R[0, 1] * py + R[0, 2] * pz + T[0]
        y = R[1, 0] * px + R[1, 1] * py + R[1, 2] * pz + T[1]
        z = R[2, 0] * px + R[2, 1] * py + R[2, 2] * pz + T[2]
        uf, vf = torch.floor(fx * (x / z) + cx + 0.5), torch.floor(fy * (y / z) + cy + 0.5)
        ok = (z > V["depth_min"]) & (uf >= 0) & (uf < W) & (vf >= 0) & (vf < H)
        pix = torch.where(ok, vf * W + uf, torch.zeros_like(uf)).long()
        d = V["depth"].reshape(-1)[pix]
        sdf = d - z
        ok &= (d > 0) & (d <= V["depth_trunc"]) & (sdf >= -trunc)
        t = torch.clamp(sdf / trunc, max=1.0)
        w1 = weight + 1.0
        tsdf.copy_(torch.where(ok, (tsdf * weight + t) / w1, tsdf))
        for ch in range(3):
            c = V["image"][ch].reshape(-1)[pix]
            planes[2 + ch].copy_(torch.where(ok, (planes[2 + ch] * weight + c) / w1, planes[2 + ch]))
        weight.copy_(torch.where(ok, torch.clamp(w1, max=max_weight), weight))


def shape_record(dims, W, H, dev, repeats, warmup):
    voxel = 0.02
    vol = TsdfVolume((0.0, 0.0, 0.0), voxel, dims, device=dev)
    views = make_views(dims, voxel, W, H, dev)
    n = dims[0] * dims[1] * dims[2]
    rec = dict(volume="x".join(str(d) for d in dims), frame=f"{W}x{H}", voxels=n)
    vol.integrate_views(views)      # state: every later call reads and writes the rows it touches
    touched = int((vol.weight > 0).sum())
    rec["voxels_some_view_touches"] = touched
    rec["integrate_1_view"] = events_ms(lambda: vol.integrate_views(views[:1]), repeats, warmup, dev)
    rec["integrate_16_views"] = events_ms(lambda: vol.integrate_views(views), repeats, warmup, dev)
    rec["integrate_16_calls_of_1"] = events_ms(lambda: [vol.integrate_views([v]) for v in views], repeats, warmup, dev)
    one_view = int(_touched_by(vol, views[:1], dev))
    frame_bytes = W * H * (4 + 12)
    for key, count, voxels in (("integrate_1_view", 1, one_view), ("integrate_16_views", 16, touched)):
        least = 40 * voxels + count * frame_bytes
        rec[key].update(bytes_at_least=least, voxels_touched=voxels,
                        fraction_of_hbm_rate=round(least / (rec[key]["ms"] * 1e-3) / (HBM_TB_PER_S * 1e12), 4))
    # the PyTorch restatement on a copy of the planes
    idx = torch.arange(n, device=dev)
    lattice = tuple((voxel * c.float()) for c in (idx % dims[0], (idx // dims[0]) % dims[1], idx // (dims[0] * dims[1])))
    del idx
    planes = vol.planes.clone()
    for key, count in (("torch_1_view", 1), ("torch_16_views", 16)):
        rec[key] = events_ms(lambda: torch_integrate(planes, lattice, views[:count], vol.trunc, vol.max_weight), max(repeats // 3, 2), 1, dev)
    del planes, lattice
    rec["speedup_1_view"] = round(rec["torch_1_view"]["ms"] / rec["integrate_1_view"]["ms"], 1)
    rec["speedup_16_views"] = round(rec["torch_16_views"]["ms"] / rec["integrate_16_views"]["ms"], 1)
    # the mesh of the fused volume
    vol.reset()
    vol.integrate_views(views)
    vol.extract_mesh()
    rec["extract_mesh"] = events_ms(lambda: vol.extract_mesh(), repeats, warmup, dev)
    nv, nf = vol.last_counts
    rec["extract_mesh"].update(vertices=nv, faces=nf, bytes_at_least=13 * n + 24 * nv + 12 * nf,
                               fraction_of_hbm_rate=round((13 * n + 24 * nv + 12 * nf) / (rec["extract_mesh"]["ms"] * 1e-3) / (HBM_TB_PER_S * 1e12), 4))
    _lib.profile_enable(True)
    _lib.profile_reset()
    for _ in range(repeats):
        vol.extract_mesh()
    vol.integrate_views(views)
    torch.cuda.synchronize(dev)
    prof = _lib.profile_read()
    _lib.profile_enable(False)
    rec["launch_us"] = {k: round(1e3 * ms / cnt, 2) for k, (cnt, ms) in prof.items() if k.startswith("tsdf")}
    return rec


def _touched_by(vol, views, dev):
    probe = TsdfVolume(vol.origin, vol.voxel_size, vol.dims, color=False, device=dev)
    probe.integrate_views([dict(v, image=None) for v in views])
    return (probe.weight > 0).sum()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tsdf_timing.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    out = dict(device=torch.cuda.get_device_name(dev), repeats=a.repeats, warmup=a.warmup, hbm_tb_per_s_assumed=HBM_TB_PER_S,
               note="ms: median device time between two stream events around the call(s); torch_*: the same rule as PyTorch statements "
                    "over the whole volume; bytes_at_least: what the call must move (module docstring)",
               shapes=[shape_record((256, 256, 256), 1226, 370, dev, a.repeats, a.warmup),
                       shape_record((512, 512, 256), 1920, 1280, dev, a.repeats, a.warmup)])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
