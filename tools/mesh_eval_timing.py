#!/usr/bin/env python3
"""Times mesh scoring on the device (``lvdgs.mesh_eval``: ``lvdgs_mesh_sample``, ``lvdgs_cloud_distance``):

    python tools/mesh_eval_timing.py [--repeats 10] [--out profiles/mesh_eval_timing.json]

The two surfaces are the wavy wall of tools/tsdf_timing.py as a mesh of 511 x 511 x 2 triangles over 5.1 x 5.1 m and its copy displaced
by one voxel (0.02 m) along z.  For 200 k x 200 k and 1 M x 1 M samples:
 (a) ``sample_mesh`` of one surface -- device time between two stream events around the call, medians of ``--repeats`` after
     ``--warmup``, with the fastest and the slowest run;
 (b) ``nearest`` in both directions (estimate -> truth, truth -> estimate), ``d2`` and ``idx`` written, and with only the row asked
     for; the launches by the library's own events;
 (c) the same nearest neighbours by brute force in PyTorch on the same device: ``torch.cdist`` over blocks of queries against the whole
     reference cloud plus ``min`` (fewer repeats: it is seconds at 1 M);
 (d) the bytes a search must move at the least -- both clouds read once (12 bytes a point) and ``d2`` / ``idx`` written (8 bytes a
     query) -- against the HBM rate.
No time is asserted anywhere."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import lvdgs  # noqa: E402,F401
from lvdgs import _lib, mesh_eval  # noqa: E402

HBM_TB_PER_S = 8.0      # MI355X peak
VOXEL = 0.02


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
    return dict(ms=round(statistics.median(times), 4), ms_best=round(min(times), 4), ms_worst=round(max(times), 4))


def wavy_wall(dev, n=512, size=5.1, offset=0.0):
    """(vertices (n*n, 3), faces (2 (n-1)^2, 3)): z = 3.4 * (1 + 0.04 sin(x / 0.74) cos(y / 0.58)) + offset over [0, size]^2."""
    u = torch.linspace(0.0, size, n, device=dev)
    y, x = torch.meshgrid(u, u, indexing="ij")
    z = 3.4 * (1.0 + 0.04 * torch.sin(x / 0.74) * torch.cos(y / 0.58)) + offset
    vertices = torch.stack([x, y, z], -1).reshape(-1, 3).contiguous()
    j, i = torch.meshgrid(torch.arange(n - 1, device=dev), torch.arange(n - 1, device=dev), indexing="ij")
    p = (j * n + i).reshape(-1)
    faces = torch.cat([torch.stack([p, p + 1, p + n], 1), torch.stack([p + 1, p + n + 1, p + n], 1)]).to(torch.int32).contiguous()
    return vertices, faces


def torch_nearest(q, r, block):
    """Brute force: ``cdist`` of a block of queries against every reference point, ``min`` over them."""
    d = torch.empty(q.shape[0], dtype=torch.float32, device=q.device)
    i = torch.empty(q.shape[0], dtype=torch.int64, device=q.device)
    for first in range(0, q.shape[0], block):
        v, j = torch.cdist(q[first:first + block], r).min(1)
        d[first:first + block], i[first:first + block] = v, j
    return d, i


def size_record(n, est, gt, dev, repeats, warmup):
    rec = dict(samples=n)
    rec["sample_mesh"] = events_ms(lambda: mesh_eval.sample_mesh(est, n, seed=0), repeats, warmup, dev)
    rec["sample_mesh"].update(bytes_at_least=12 * n + 36 * int(est[1].shape[0]))
    a, b = mesh_eval.sample_mesh(est, n, seed=0), mesh_eval.sample_mesh(gt, n, seed=1)
    table = mesh_eval.Table(dev, rows=2)
    least = 12 * 2 * n + 8 * n
    for row, (key, (q, r)) in enumerate((("est_to_gt", (a, b)), ("gt_to_est", (b, a)))):
        rec[key] = events_ms(lambda: mesh_eval.nearest(q, r, (2 * VOXEL,), table=table, row=row), repeats, warmup, dev)
        rec[key].update(bytes_at_least=least, fraction_of_hbm_rate=round(least / (rec[key]["ms"] * 1e-3) / (HBM_TB_PER_S * 1e12), 5))
        rec[key + "_row_only"] = events_ms(lambda: mesh_eval.nearest(q, r, (2 * VOXEL,), want_d2=False, want_idx=False, table=table, row=row), repeats, warmup, dev)
    rows = table.read()[0]
    rec["mean_distance"] = [float(rows[i]["sum_distance"]) / max(int(rows[i]["n_counted"]), 1) for i in range(2)]
    _lib.profile_enable(True)
    _lib.profile_reset()
    for _ in range(repeats):
        mesh_eval.sample_mesh(est, n, seed=0)
        mesh_eval.nearest(a, b, (2 * VOXEL,), table=table)
    torch.cuda.synchronize(dev)
    prof = _lib.profile_read()
    _lib.profile_enable(False)
    rec["launch_us"] = {k: round(1e3 * ms / cnt, 2) for k, (cnt, ms) in prof.items() if k.startswith(("cloud_", "mesh_sample_"))}
    block = max(256, min(8192, (1 << 31) // max(n, 1)))      # a block of distances stays under 8 GiB
    few = max(2, repeats // 5)
    rec["torch_cdist_min"] = events_ms(lambda: torch_nearest(a, b, block), few, 1, dev)
    rec["torch_cdist_min"].update(block=block, repeats=few)
    d2, idx, _ = mesh_eval.nearest(a, b)
    td, ti = torch_nearest(a, b, block)
    rec["torch_cdist_min"].update(indices_that_differ=int((ti != idx.long()).sum()), worst_distance_difference=float((td - d2.sqrt()).abs().max()))
    rec["speedup_against_torch"] = round(rec["torch_cdist_min"]["ms"] / rec["est_to_gt"]["ms"], 1)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", type=int, nargs="+", default=[200_000, 1_000_000])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_eval_timing.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    est, gt = wavy_wall(dev), wavy_wall(dev, offset=VOXEL)
    out = dict(device=torch.cuda.get_device_name(dev), repeats=a.repeats, warmup=a.warmup, hbm_tb_per_s_assumed=HBM_TB_PER_S,
               faces=int(est[1].shape[0]),
               note="ms: median device time between two stream events around the call, ms_best / ms_worst: the spread of the runs; "
                    "torch_cdist_min: the same nearest neighbours by torch.cdist over blocks of queries plus min (its own, smaller number of "
                    "repeats); bytes_at_least: what the call must move (module docstring)",
               sizes=[size_record(n, est, gt, dev, a.repeats, a.warmup) for n in a.sizes])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
