#!/usr/bin/env python3
"""Times the block-sparse TSDF volume (``lvdgs.tsdf_blocks``) beside the dense one (``lvdgs.tsdf``) on the device:

    python tools/tsdf_blocks_timing.py [--repeats 10] [--out profiles/tsdf_blocks_timing.json]

For both scenes of tools/tsdf_timing.py (a wavy wall across a 256^3 and a 512 x 512 x 256 volume of 2 cm voxels, 16 views), fused
into the dense volume and into blocks on the same lattice at the same voxel size:
 (a) ``integrate_views`` with 1 view and with 16 views per call, on a volume that already holds state -- device time between two
     stream events; for the blocks, the share of it that is the allocation launch (the library's own events);
 (b) ``extract_mesh`` with its one wait, and the launches of both by the library's events;
 (c) the bytes each holds, the blocks in use, and both meshes' counts (the blocks are not clipped to the dense box: their mesh also
     covers what the views see beside it).
And a corridor: a wall 200 m long that runs diagonally through x and z, 16 views along it, 5 cm voxels.  Its bounding box has 9.5e8
samples, so the dense class would raise the voxel size (reported: the size ``TsdfVolume.from_bounds`` would fall back to); only the
blocks are measured.  No time is asserted anywhere."""
import argparse
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import lvdgs  # noqa: E402,F401
from lvdgs import _lib  # noqa: E402
from lvdgs.tsdf import TsdfVolume  # noqa: E402
from lvdgs.tsdf_blocks import TsdfBlockVolume  # noqa: E402
from tsdf_timing import events_ms, make_views  # noqa: E402


def launches(fn, repeats, dev, prefix):
    _lib.profile_enable(True)
    _lib.profile_reset()
    for _ in range(repeats):
        fn()
    torch.cuda.synchronize(dev)
    prof = _lib.profile_read()
    _lib.profile_enable(False)
    return {k: round(1e3 * ms / cnt, 2) for k, (cnt, ms) in prof.items() if k.startswith(prefix)}


def fused_blocks(origin, voxel, views, pool, dev):
    """A block volume that holds ``views`` with nothing dropped (the pool doubles until it does)."""
    while True:
        vol = TsdfBlockVolume(origin, voxel, pool, device=dev)
        vol.integrate_views(views)
        s = vol.stats()
        if not s["dropped"] and not s["table_full"]:
            return vol, s
        del vol
        pool *= 2


def blocks_record(vol, stats, views, repeats, warmup, dev):
    rec = dict(pool_blocks=vol.pool_blocks, table_slots=vol.table_slots, bytes_held=vol.bytes_held(), bytes_in_use=stats["blocks"] * 512 * 4 * 5, **stats)
    rec["integrate_1_view"] = events_ms(lambda: vol.integrate_views(views[:1]), repeats, warmup, dev)
    rec["integrate_16_views"] = events_ms(lambda: vol.integrate_views(views), repeats, warmup, dev)
    us = launches(lambda: vol.integrate_views(views), repeats, dev, "tsdf_blocks")
    rec["integrate_launch_us"] = us
    rec["allocation_share_16_views"] = round(us["tsdf_blocks_alloc"] / sum(us.values()), 3)
    vol.reset()
    vol.integrate_views(views)
    vol.extract_mesh()
    rec["extract_mesh"] = events_ms(lambda: vol.extract_mesh(), repeats, warmup, dev)
    rec["extract_mesh"].update(vertices=vol.last_counts[0], faces=vol.last_counts[1])
    rec["mesh_launch_us"] = {k: v for k, v in launches(lambda: vol.extract_mesh(), repeats, dev, "tsdf_blocks").items() if k not in us}
    return rec


def shape_record(dims, W, H, dev, repeats, warmup):
    voxel = 0.02
    views = make_views(dims, voxel, W, H, dev)
    rec = dict(volume="x".join(str(d) for d in dims), frame=f"{W}x{H}", voxel_size=voxel)
    dense = TsdfVolume((0.0, 0.0, 0.0), voxel, dims, device=dev)
    dense.integrate_views(views)
    d = dict(bytes_held=dense.planes.numel() * 4)
    d["integrate_1_view"] = events_ms(lambda: dense.integrate_views(views[:1]), repeats, warmup, dev)
    d["integrate_16_views"] = events_ms(lambda: dense.integrate_views(views), repeats, warmup, dev)
    dense.reset()
    dense.integrate_views(views)
    dense.extract_mesh()
    d["extract_mesh"] = events_ms(lambda: dense.extract_mesh(), repeats, warmup, dev)
    d["extract_mesh"].update(vertices=dense.last_counts[0], faces=dense.last_counts[1])
    rec["dense"] = d
    del dense
    torch.cuda.empty_cache()
    vol, stats = fused_blocks((0.0, 0.0, 0.0), voxel, views, 1 << 15, dev)
    rec["blocks"] = blocks_record(vol, stats, views, repeats, warmup, dev)
    return rec


def corridor_views(W, H, dev, length=200.0, distance=5.0, count=16):
    """Cameras ``distance`` in front of a wall of ``length`` metres that runs along (1, 0, 1) / sqrt 2, each looking straight at it."""
    a = math.pi / 4.0
    along = torch.tensor([math.cos(a), 0.0, math.sin(a)])
    normal = torch.tensor([-math.sin(a), 0.0, math.cos(a)])      # the cameras look along it
    R = torch.stack([along, torch.tensor([0.0, 1.0, 0.0]), normal])
    fx = fy = 0.25 * W
    vi, ui = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    g = torch.Generator().manual_seed(2)
    views = []
    for n in range(count):
        C = along * (length * (n + 0.5) / count) + torch.tensor([0.0, 3.0, 0.0])
        depth = distance * (1.0 + 0.01 * torch.sin(ui / 41.0 + n) * torch.cos(vi / 23.0))
        views.append(dict(depth=depth.to(dev).contiguous(), R=R.to(dev), T=(-R @ C).to(dev), intrinsics=(fx, fy, W / 2.0 - 0.25, H / 2.0 - 0.25),
                          image=torch.rand(3, H, W, generator=g).to(dev), mask=None, depth_min=0.0, depth_trunc=float("inf")))
    return views


def dense_fallback_voxel(lo, hi, voxel, max_voxels=1 << 28):
    """The voxel size ``TsdfVolume.from_bounds`` would use for the box (its loop, without the allocation)."""
    dims_of = lambda s: [max(int(math.ceil((b - a) / s)) + 1, 2) for a, b in zip(lo, hi)]
    size = voxel
    while math.prod(dims_of(size)) > max_voxels:
        size *= 1.05
    return size, dims_of(voxel)


def corridor_record(dev, repeats, warmup):
    W, H, voxel = 1226, 370, 0.05
    views = corridor_views(W, H, dev)
    lo, hi = (-8.0, -2.0, -2.0), (146.0, 8.0, 150.0)      # the wall's bounding box with the cameras' side of it
    fallback, dims = dense_fallback_voxel(lo, hi, voxel)
    rec = dict(scene="a wall of 200 m along (1, 0, 1), 16 views of 1226x370 at 5 m", voxel_size=voxel,
               dense=dict(dims_at_the_voxel_size_asked=dims, samples=math.prod(dims), bytes_with_colour=20 * math.prod(dims),
                          voxel_size_from_bounds_falls_back_to=round(fallback, 4)))
    vol, stats = fused_blocks(lo, voxel, views, 1 << 15, dev)
    rec["blocks"] = blocks_record(vol, stats, views, repeats, warmup, dev)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tsdf_blocks_timing.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    out = dict(device=torch.cuda.get_device_name(dev), repeats=a.repeats, warmup=a.warmup,
               note="ms: median device time between two stream events around the call(s); *_launch_us: the library's own events per launch; "
                    "dense and blocks are measured in the same process on the same views",
               shapes=[shape_record((256, 256, 256), 1226, 370, dev, a.repeats, a.warmup),
                       shape_record((512, 512, 256), 1920, 1280, dev, a.repeats, a.warmup)],
               corridor=corridor_record(dev, a.repeats, a.warmup))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
