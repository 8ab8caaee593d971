#!/usr/bin/env python3
"""Times depth rendered from a mesh on the device (``lvdgs.mesh_eval.render_depth``: ``lvdgs_mesh_depth``):

    python tools/mesh_depth_timing.py [--repeats 10] [--out profiles/mesh_depth_timing.json]

Scene "wall": the wavy wall of tools/mesh_cull_timing.py at 512 and 1024 vertices a side (522 k and 2.09 M triangles over 5.1 x 5.1 m, each
well under a pixel) against 1 and 16 of its cameras of 640 x 480 pixels -- every face is walked by its own lane.  Scene "wall + sheets": the
same wall with four image-sized triangles two metres in front of it, which go through the wave path and hide most of the wall.  Per
scene, size and view count:
 (a) ``render_depth`` with depth and face planes -- device time between two stream events around the call, medians of ``--repeats`` after
     ``--warmup``, with the fastest and the slowest run --, and its fill, raster and resolve launches by the library's own events;
 (b) the bytes each launch must move at the least: the fill 8 P written (P pixels over the views); the raster 12 F of indices and three
     vertex gathers of 12 per face, once per call, and 8 per atomic; the resolve 8 P read and 8 P written -- against the HBM rate;
 (c) the candidates -- (face, pixel) pairs that are covered and inside the depth limits -- and the pixels hit, counted by the PyTorch
     statements below: without the plain load in front of the atomic every candidate is an atomic; with it the atomics issued lie between
     the pixels hit (each pixel's winner must be issued) and the candidates, depending on arrival order -- the product kernel carries no
     counter;
 (d) the same rule as PyTorch statements on the same device, faces in chunks, ``scatter_reduce_(..., "amin")`` on the 64-bit keys, and
     in how many pixels its planes differ from the library's.
No time is asserted anywhere."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lvdgs  # noqa: E402,F401
from lvdgs import _lib, mesh_eval  # noqa: E402
from mesh_cull_timing import FOCAL, H, W, fraction, make_views  # noqa: E402
from mesh_eval_timing import HBM_TB_PER_S, events_ms, wavy_wall  # noqa: E402

CHUNK_PAIRS = 1 << 23
EMPTY = 2 ** 63 - 1


def views_of(dev, n):
    return [dict({k: x for k, x in v.items() if k != "depth"}, size=(H, W)) for v in make_views(dev)[:n]]


def with_sheets(vertices, faces, dev):
    """Four triangles of about the image's size each, two metres in front of the wall, appended."""
    corners = torch.tensor([[-1.0, -1.0, 1.4], [7.0, -1.0, 1.4], [-1.0, 7.0, 1.4], [7.0, 7.0, 1.45], [-1.0, 7.0, 1.45], [7.0, -1.0, 1.45],
                            [0.5, 0.5, 1.5], [4.5, 0.5, 1.5], [0.5, 4.5, 1.5], [4.6, 4.6, 1.55], [0.6, 4.6, 1.55], [4.6, 0.6, 1.55]], device=dev)
    first = vertices.shape[0]
    extra = torch.arange(first, first + 12, dtype=torch.int32, device=dev).reshape(4, 3)
    return torch.cat([vertices, corners]).contiguous(), torch.cat([faces, extra]).contiguous()


def torch_render(vertices, faces, v, keys=None):
    """The rule of include/lvdgs.h as PyTorch statements -> (depth (H, W), face index (H, W), candidates, pixels hit)."""
    dev = vertices.device
    Hh, Ww = v["size"]
    R, T = v["R"].reshape(-1), v["T"]
    fx, fy, cx, cy = v["intrinsics"]
    px, py, pz = vertices.unbind(1)
    x = ((R[0] * px + R[1] * py) + R[2] * pz) + T[0]
    y = ((R[3] * px + R[4] * py) + R[5] * pz) + T[1]
    z = ((R[6] * px + R[7] * py) + R[8] * pz) + T[2]
    u, w = fx * (x / z) + cx, fy * (y / z) + cy
    dm, trunc = max(float(v.get("depth_min", 0.0)), 0.0), float(v.get("depth_trunc", float("inf")))
    idx = faces.long()
    fz, fu, fv = z[idx], u[idx], w[idx]
    ok = (fz > dm).all(1) & torch.isfinite(fu).all(1) & torch.isfinite(fv).all(1)
    ar = (fu[:, 1] - fu[:, 0]) * (fv[:, 2] - fv[:, 0]) - (fv[:, 1] - fv[:, 0]) * (fu[:, 2] - fu[:, 0])
    ulo, uhi = torch.ceil(fu.min(1).values), torch.floor(fu.max(1).values)
    vlo, vhi = torch.ceil(fv.min(1).values), torch.floor(fv.max(1).values)
    ok &= (ar != 0) & (ulo < Ww) & (uhi >= 0) & (ulo <= uhi) & (vlo < Hh) & (vhi >= 0) & (vlo <= vhi)
    f = torch.nonzero(ok).reshape(-1)
    i0, i1 = ulo[f].clamp(min=0).long(), uhi[f].clamp(max=Ww - 1).long()
    j0, j1 = vlo[f].clamp(min=0).long(), vhi[f].clamp(max=Hh - 1).long()
    bw = i1 - i0 + 1
    n = bw * (j1 - j0 + 1)
    ends = torch.cumsum(n, 0)
    keys = torch.full((Hh * Ww,), EMPTY, dtype=torch.int64, device=dev) if keys is None else keys.fill_(EMPTY)
    candidates, lo, total = torch.zeros((), dtype=torch.int64, device=dev), 0, int(ends[-1]) if len(f) else 0
    done = 0
    while done < total:
        hi = int(torch.searchsorted(ends, torch.tensor(done + CHUNK_PAIRS, device=dev), right=True))
        hi = max(hi, lo + 1)
        nn = n[lo:hi]
        start = torch.cumsum(nn, 0) - nn
        rows = torch.arange(lo, hi, device=dev).repeat_interleave(nn)
        t = torch.arange(int(nn.sum()), device=dev) - start.repeat_interleave(nn)
        row = torch.div(t, bw[rows], rounding_mode="floor")
        i, j = i0[rows] + (t - row * bw[rows]), j0[rows] + row
        face = f[rows]
        a = idx[face]
        fi, fj = i.float(), j.float()
        E = []
        for k in range(3):
            p, q = a[:, (k + 1) % 3], a[:, (k + 2) % 3]
            flip = q < p
            l, h = torch.where(flip, q, p), torch.where(flip, p, q)
            s = (u[h] - u[l]) * (fj - w[l]) - (w[h] - w[l]) * (fi - u[l])
            E.append(torch.where(flip, -s, s))
        covered = ((E[0] >= 0) & (E[1] >= 0) & (E[2] >= 0)) | ((E[0] <= 0) & (E[1] <= 0) & (E[2] <= 0))
        A = (E[0] + E[1]) + E[2]
        za = z[a]
        inv = ((E[0] / A) * (1.0 / za[:, 0]) + (E[1] / A) * (1.0 / za[:, 1])) + (E[2] / A) * (1.0 / za[:, 2])
        zp = 1.0 / inv
        passes = covered & (zp > dm) & (zp <= trunc)
        key = (zp[passes].view(torch.int32).long() << 32) | face[passes]
        keys.scatter_reduce_(0, (j * Ww + i)[passes], key, "amin")
        candidates += passes.sum()
        done, lo = int(ends[hi - 1]), hi
    hit = keys != EMPTY
    depth = torch.where(hit, (keys >> 32).to(torch.int32).view(torch.float32), torch.zeros((), device=dev))
    index = torch.where(hit, keys & 0xFFFFFFFF, torch.full((), -1, dtype=torch.int64, device=dev)).to(torch.int32)
    return depth.reshape(Hh, Ww), index.reshape(Hh, Ww), int(candidates), int(hit.sum())


def case_record(name, vertices, faces, count, dev, repeats, warmup, torch_repeats):
    V, F = int(vertices.shape[0]), int(faces.shape[0])
    views = views_of(dev, count)
    P = count * H * W
    rec = dict(scene=name, vertices=V, faces=F, views=count, pixels=P)
    out = []
    rec["render_depth"] = events_ms(lambda: out.append(mesh_eval.render_depth((vertices, faces), views, want_faces=True)), repeats, warmup, dev)
    planes, indices = out[-1]
    _lib.profile_enable(True)
    _lib.profile_reset()
    for _ in range(repeats):
        mesh_eval.render_depth((vertices, faces), views, want_faces=True)
    torch.cuda.synchronize(dev)
    prof = _lib.profile_read()
    _lib.profile_enable(False)
    rec["launch_us"] = {k: round(1e3 * ms / cnt, 2) for k, (cnt, ms) in prof.items() if k.startswith("mesh_depth_")}
    if torch_repeats > 0:
        keys = torch.empty(H * W, dtype=torch.int64, device=dev)
        results = [torch_render(vertices, faces, v, keys) for v in views]
        rec["candidates"], rec["pixels_hit"] = sum(r[2] for r in results), sum(r[3] for r in results)
        rec["planes_differ_in"] = sum(int((r[0].view(torch.int32) != d.view(torch.int32)).sum()) + int((r[1] != i).sum())
                                      for r, d, i in zip(results, planes, indices))
        rec["torch"] = events_ms(lambda: [torch_render(vertices, faces, v, keys) for v in views], torch_repeats, 1, dev)
        rec["speedup"] = round(rec["torch"]["ms"] / rec["render_depth"]["ms"], 1)
        rec["atomics"] = dict(without_preload=rec["candidates"], with_preload_at_least=rec["pixels_hit"], with_preload_at_most=rec["candidates"],
                              skipped_at_most=rec["candidates"] - rec["pixels_hit"])
    else:
        rec["pixels_hit"] = sum(int((d > 0).sum()) for d in planes)
    atomics = rec.get("candidates", rec["pixels_hit"])
    least = dict(fill=8 * P, raster=12 * F + 36 * F + 8 * atomics, resolve=16 * P)
    rec["bytes_at_least"] = least
    rec["fraction_of_hbm_rate"] = {k: fraction(b, rec["launch_us"]["mesh_depth_" + k] * 1e-3) for k, b in least.items()
                                   if rec["launch_us"].get("mesh_depth_" + k)}
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--torch-repeats", type=int, default=3, help="0: no PyTorch comparison (and no candidate counts)")
    ap.add_argument("--sides", type=int, nargs="+", default=[512, 1024])
    ap.add_argument("--counts", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_depth_timing.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    cases = []
    for n in a.sides:
        wall = wavy_wall(dev, n=n)
        for name, (vertices, faces) in (("wall", wall), ("wall + sheets", with_sheets(*wall, dev))):
            for count in a.counts:
                cases.append(case_record(name, vertices, faces, count, dev, a.repeats, a.warmup, a.torch_repeats))
                print(json.dumps(cases[-1]), file=sys.stderr)
    out = dict(device=torch.cuda.get_device_name(dev), library=_lib.LIB_PATH, repeats=a.repeats, warmup=a.warmup, torch_repeats=a.torch_repeats,
               hbm_tb_per_s_assumed=HBM_TB_PER_S, image=[W, H], focal=FOCAL,
               note="ms: median device time between two stream events around render_depth(want_faces=True), ms_best / ms_worst: the spread of "
                    "the runs; launch_us: the library's own events, per call; torch: the same rule as PyTorch statements on the same device; "
                    "candidates, pixels_hit, atomics: module docstring (c); bytes_at_least: module docstring (b)",
               cases=cases)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
