#!/usr/bin/env python3
"""Times mesh culling on the device (``lvdgs.mesh_eval``: ``lvdgs_mesh_visibility``, ``lvdgs_mesh_cull``):

    python tools/mesh_cull_timing.py [--repeats 10] [--out profiles/mesh_cull_timing.json]

The mesh is the wavy wall of tools/mesh_eval_timing.py at 512 and 1024 vertices a side (522 k and 2.09 M triangles over 5.1 x 5.1 m); the
views are 16 cameras of 640 x 480 pixels in a 4 x 4 grid three and a half metres in front of it, each with a depth plane that hides the
wall's far half-waves.  Per size:
 (a) ``visibility`` with 1 view and with 16 views per call -- device time between two stream events around the call, medians of
     ``--repeats`` after ``--warmup``, with the fastest and the slowest run;
 (b) ``cull_mesh`` from the finished ``seen`` plane (its one wait included), and its launches by the library's own events;
 (c) the same rules as PyTorch statements on the same device (``index_select`` for the depth gather, boolean indexing and ``cumsum`` for
     the compaction);
 (d) the bytes each call must move at the least: 13 a vertex (12 read, the ``seen`` byte read, and written where it changes) and 4 per
     depth gather for the visibility; for the compaction the used plane (V cleared, V read twice), 12 F of faces and 3 F ``seen`` gathers, a
     byte per face written and read, per kept vertex 12 (24 with colours) in and out and 4 of its new number, per kept face 12 in, three
     gathers of 4 and 12 out -- against the HBM rate.
No time is asserted anywhere."""
import argparse
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lvdgs  # noqa: E402,F401
from lvdgs import _lib, mesh_eval  # noqa: E402
from mesh_eval_timing import HBM_TB_PER_S, events_ms, wavy_wall  # noqa: E402

EPS = 0.02
W, H, FOCAL = 640, 480, 400.0


def make_views(dev, n=16):
    """n cameras looking along +z at the wall (z = 3.4 +- 0.14) from z = 0, on a grid over it; depth planes at 3.43."""
    views, side = [], int(math.ceil(math.sqrt(n)))
    for k in range(n):
        eye = torch.tensor([5.1 * (k % side + 0.5) / side, 5.1 * (k // side + 0.5) / side, 0.0], device=dev)
        views.append(dict(depth=torch.full((H, W), 3.43, device=dev), R=torch.eye(3, device=dev), T=-eye, intrinsics=(FOCAL, FOCAL, W / 2 - 0.5, H / 2 - 0.5)))
    return views


def project(vertices, v):
    """Steps 1 and 2 as PyTorch statements -> (z, inside the view, the pixel or 0)."""
    px, py, pz = vertices.unbind(1)
    R, T = v["R"].reshape(-1), v["T"]
    fx, fy, cx, cy = v["intrinsics"]
    x = ((R[0] * px + R[1] * py) + R[2] * pz) + T[0]
    y = ((R[3] * px + R[4] * py) + R[5] * pz) + T[1]
    z = ((R[6] * px + R[7] * py) + R[8] * pz) + T[2]
    uf, vf = torch.floor(fx * (x / z) + cx + 0.5), torch.floor(fy * (y / z) + cy + 0.5)
    ok = (z > 0) & (uf >= 0) & (uf < W) & (vf >= 0) & (vf < H)
    return z, ok, torch.where(ok, vf * W + uf, torch.zeros_like(uf)).long()


def in_view_counts(vertices, views):
    return [int(project(vertices, v)[1].sum()) for v in views]


def torch_visibility(vertices, views, eps, seen):
    """The rule as PyTorch statements."""
    for v in views:
        z, ok, pix = project(vertices, v)
        d = v["depth"].reshape(-1).index_select(0, pix)
        seen |= (ok & (d > 0) & ~((d - z) < -eps)).to(torch.uint8)
    return seen


def torch_cull(vertices, faces, seen):
    V = vertices.shape[0]
    inside = ((faces >= 0) & (faces < V)).all(1)
    keep = inside & seen.bool()[faces.clamp(0, V - 1).long()].all(1)
    kept = faces[keep].long()
    used = torch.zeros(V, dtype=torch.bool, device=vertices.device)
    used[kept.reshape(-1)] = True
    new = torch.cumsum(used, 0) - 1
    return vertices[used], new[kept].to(torch.int32)


def fraction(nbytes, ms):
    return round(nbytes / (ms * 1e-3) / (HBM_TB_PER_S * 1e12), 5)


def size_record(n, dev, repeats, warmup):
    vertices, faces = wavy_wall(dev, n=n)
    V, F = int(vertices.shape[0]), int(faces.shape[0])
    views = make_views(dev)
    rec = dict(side=n, vertices=V, faces=F)
    gathers = in_view_counts(vertices, views)
    for count in (1, 16):
        key = f"visibility_{count}"
        seen = torch.zeros(V, dtype=torch.uint8, device=dev)

        def run():
            seen.zero_()      # (a plane that fills up would let later runs stop early)
            mesh_eval.visibility(vertices, views[:count], EPS, seen=seen)
        rec[key] = events_ms(run, repeats, warmup, dev)
        least = 13 * V + 4 * sum(gathers[:count])
        rec[key].update(bytes_at_least=least, fraction_of_hbm_rate=fraction(least, rec[key]["ms"]), seen=int(seen.count_nonzero()))
        tseen = torch.zeros(V, dtype=torch.uint8, device=dev)
        rec["torch_" + key] = events_ms(lambda: torch_visibility(vertices, views[:count], EPS, tseen.zero_()), max(2, repeats // 2), 1, dev)
        rec["torch_" + key].update(planes_differ_in=int((tseen != seen).sum()))
        rec["speedup_" + key] = round(rec["torch_" + key]["ms"] / rec[key]["ms"], 1)
    seen = mesh_eval.visibility(vertices, views, EPS)
    out = []
    rec["cull_mesh"] = events_ms(lambda: out.append(mesh_eval.cull_mesh((vertices, faces), seen=seen)), repeats, warmup, dev)
    kept, counts = out[-1]
    nv, nf = counts["vertices"], counts["faces"]
    least = 3 * V + 12 * F + 3 * F + 2 * F + (24 + 4) * nv + (12 + 12 + 12) * nf
    rec["cull_mesh"].update(kept_vertices=nv, kept_faces=nf, bytes_at_least=least, fraction_of_hbm_rate=fraction(least, rec["cull_mesh"]["ms"]))
    tv, tf = torch_cull(vertices, faces, seen)
    rec["torch_cull"] = events_ms(lambda: torch_cull(vertices, faces, seen), max(2, repeats // 2), 1, dev)
    rec["torch_cull"].update(same_result=bool(torch.equal(tv, kept.vertices) and torch.equal(tf, kept.faces)))
    rec["speedup_cull"] = round(rec["torch_cull"]["ms"] / rec["cull_mesh"]["ms"], 1)
    _lib.profile_enable(True)
    _lib.profile_reset()
    for _ in range(repeats):
        mesh_eval.visibility(vertices, views, EPS)
        mesh_eval.cull_mesh((vertices, faces), seen=seen)
    torch.cuda.synchronize(dev)
    prof = _lib.profile_read()
    _lib.profile_enable(False)
    rec["launch_us"] = {k: round(1e3 * ms / cnt, 2) for k, (cnt, ms) in prof.items() if k.startswith("mesh_")}
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sides", type=int, nargs="+", default=[512, 1024])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_cull_timing.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    out = dict(device=torch.cuda.get_device_name(dev), repeats=a.repeats, warmup=a.warmup, hbm_tb_per_s_assumed=HBM_TB_PER_S, views=16,
               image=[W, H], occlusion_eps=EPS,
               note="ms: median device time between two stream events around the call, ms_best / ms_worst: the spread of the runs; cull_mesh "
                    "includes its one wait; torch_*: the same rule as PyTorch statements on the same device (their own, smaller number of "
                    "repeats); bytes_at_least: what the call must move (module docstring)",
               sizes=[size_record(n, dev, a.repeats, a.warmup) for n in a.sides])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
