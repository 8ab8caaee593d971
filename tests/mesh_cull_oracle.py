"""The rules of ``lvdgs_mesh_visibility`` / ``lvdgs_mesh_cull`` (include/lvdgs.h, "Mesh scoring") as NumPy statements.

``dtype`` is the type every per-vertex quantity has.  float32: the MIRROR -- every expression as the header writes it, one rounding per
operation, what the device code is compared with bit for bit.  float64: the STATEMENT -- the same text from the same float32 inputs in
double, which stands in for exact arithmetic (its own rounding is 2^-29 of the float32 one).  ``near_a_boundary`` marks, from the
statement alone, the vertices that lie within the header's margins of a decision boundary of some view: the only ones on which the two
may disagree.

A view is the dict ``mesh_eval.visibility`` takes, with NumPy arrays: ``depth`` (H, W) float32 or None with ``size=(H, W)``, ``R`` (3, 3),
``T`` (3,), ``intrinsics`` (fx, fy, cx, cy), ``mask`` or None, ``depth_min``, ``depth_trunc``.
"""
import numpy as np

ALL, ANY = 0, 1
U = 2.0 ** -24


def view(R, T, intrinsics, depth=None, size=None, mask=None, depth_min=0.0, depth_trunc=np.inf):
    """A view dict; the pose and the depth plane as contiguous float32 arrays."""
    v = dict(R=np.ascontiguousarray(R, np.float32).reshape(3, 3), T=np.ascontiguousarray(T, np.float32).reshape(3),
             intrinsics=tuple(float(x) for x in intrinsics), depth_min=float(depth_min), depth_trunc=float(depth_trunc))
    if depth is not None:
        v["depth"] = np.ascontiguousarray(depth, np.float32)
    else:
        v["depth"], v["size"] = None, (int(size[0]), int(size[1]))
    if mask is not None:
        v["mask"] = np.ascontiguousarray(mask).astype(np.uint8)
    return v


def size_of(v):
    return tuple(v["depth"].shape) if v.get("depth") is not None else tuple(v["size"])


def project(vertices, v, dtype=np.float32):
    """Steps 1 and 2 of "TSDF fusion" for every vertex -> dict(x, y, z, u, v, ok, pix): ``ok``: z > depth_min and the half-up pixel is
    inside the image; ``pix``: vi * width + ui there, 0 elsewhere."""
    t = dtype
    H, W = size_of(v)
    p = np.asarray(vertices, np.float32).astype(t)
    R, T = v["R"].astype(t).reshape(9), v["T"].astype(t)
    fx, fy, cx, cy = (t(np.float32(x)) for x in v["intrinsics"])
    px, py, pz = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        x = ((R[0] * px + R[1] * py) + R[2] * pz) + T[0]
        y = ((R[3] * px + R[4] * py) + R[5] * pz) + T[1]
        z = ((R[6] * px + R[7] * py) + R[8] * pz) + T[2]
        u = fx * (x / z) + cx
        vv = fy * (y / z) + cy
        uf, vf = np.floor(u + t(0.5)), np.floor(vv + t(0.5))
        ok = (z > t(np.float32(v["depth_min"]))) & (uf >= t(0)) & (uf < t(np.float32(W))) & (vf >= t(0)) & (vf < t(np.float32(H)))
    ui = np.where(ok, uf, 0).astype(np.int64)
    vi = np.where(ok, vf, 0).astype(np.int64)
    return dict(x=x, y=y, z=z, u=u, v=vv, ok=ok, pix=vi * W + ui)


def sees(vertices, v, eps, dtype=np.float32):
    """Which vertices the view sees -> bool (V,)."""
    t = dtype
    at = project(vertices, v, dtype)
    trunc = t(np.float32(v["depth_trunc"]))
    with np.errstate(all="ignore"):
        if v.get("depth") is None:
            return at["ok"] & (at["z"] <= trunc)
        d = v["depth"].reshape(-1)[at["pix"]].astype(t)
        m = v["mask"].reshape(-1)[at["pix"]] if v.get("mask") is not None else np.ones(len(d), np.uint8)
        return at["ok"] & (d > t(0)) & (d <= trunc) & (m != 0) & ~((d - at["z"]) < -t(np.float32(eps)))


def visibility(vertices, views, eps, seen=None, dtype=np.float32):
    """``seen`` (V,) uint8 after the views: a byte that is non-0 stays as it is, a byte that is 0 becomes 1 when a view sees the vertex."""
    vertices = np.asarray(vertices, np.float32).reshape(-1, 3)
    seen = np.zeros(len(vertices), np.uint8) if seen is None else np.array(seen, np.uint8)
    for v in views:
        seen[(seen == 0) & sees(vertices, v, eps, dtype)] = 1
    return seen


def near_a_boundary(vertices, views, eps, factor=2.0):
    """From the float64 statement: the vertices that, in some view, lie within ``factor`` times the header's margins of a decision
    boundary -- z = depth_min; a pixel edge 0 .. width, 0 .. height; z = depth_trunc (frustum only); d - z = -eps.  The tests follow
    each other as in the rule: a vertex clearly behind depth_min is not asked about its pixel, one clearly outside the image not about
    its depth."""
    vertices = np.asarray(vertices, np.float32).reshape(-1, 3)
    p = np.abs(vertices.astype(np.float64))
    near = np.zeros(len(vertices), bool)
    for v in views:
        H, W = size_of(v)
        at = project(vertices, v, np.float64)
        R, T = np.abs(v["R"].astype(np.float64)), np.abs(v["T"].astype(np.float64))
        M = [R[r, 0] * p[:, 0] + R[r, 1] * p[:, 1] + R[r, 2] * p[:, 2] + T[r] for r in range(3)]
        fx, fy, cx, cy = (float(np.float32(x)) for x in v["intrinsics"])
        dmin, trunc = float(np.float32(v["depth_min"])), float(np.float32(v["depth_trunc"]))
        with np.errstate(all="ignore"):
            z = at["z"]
            finite = np.isfinite(at["x"]) & np.isfinite(at["y"]) & np.isfinite(z)
            mz = factor * 4 * U * M[2]
            at_min = finite & (np.abs(z - dmin) <= mz)
            front = finite & (z > dmin) & ~at_min
            edge = np.zeros(len(vertices), bool)
            for c, f, c0, Mc, n in ((at["x"], fx, cx, M[0], W), (at["y"], fy, cy, M[1], H)):
                q = c / z
                uu = f * q + c0
                margin = factor * (abs(f) * (4 * U * Mc + np.abs(q) * 4 * U * M[2]) / np.abs(z) + 4 * U * (np.abs(uu) + abs(c0) + 1.0))
                k = np.rint(uu + 0.5)
                edge |= (np.abs(uu + 0.5 - k) <= margin) & (k >= 0) & (k <= n)
            edge &= front
            inside = front & at["ok"] & ~edge
            if v.get("depth") is None:
                last = inside & (np.abs(z - trunc) <= mz)
            else:
                d = v["depth"].reshape(-1)[at["pix"]].astype(np.float64)
                m = v["mask"].reshape(-1)[at["pix"]] if v.get("mask") is not None else np.ones(len(d), np.uint8)
                usable = inside & (d > 0) & (d <= trunc) & (m != 0) & np.isfinite(d)      # (d = +inf under an infinite depth_trunc: seen by both)
                last = usable & (np.abs((d - z) + float(np.float32(eps))) <= factor * 5 * U * (M[2] + np.abs(d)))
        near |= at_min | edge | last
    return near


def cull(vertices, faces, seen, face_rule=ALL, colors=None):
    """The kept part of the mesh -> dict(vertices, colors or None, faces (int32, renumbered), vertex_origin, face_origin (int32))."""
    vertices = np.asarray(vertices, np.float32).reshape(-1, 3)
    faces = np.asarray(faces, np.int32).reshape(-1, 3)
    V = len(vertices)
    s = np.asarray(seen).reshape(-1) != 0
    inside = ((faces >= 0) & (faces < V)).all(axis=1)
    safe = np.where(inside[:, None], faces, 0)
    of = s[safe] if V else np.zeros(faces.shape, bool)
    keep = inside & (of.any(axis=1) if face_rule == ANY else of.all(axis=1))
    used = np.zeros(V, bool)
    used[faces[keep].reshape(-1)] = True
    new = np.cumsum(used) - 1
    return dict(vertices=vertices[used], colors=None if colors is None else np.asarray(colors, np.float32).reshape(-1, 3)[used],
                faces=new[faces[keep]].astype(np.int32).reshape(-1, 3), vertex_origin=np.flatnonzero(used).astype(np.int32),
                face_origin=np.flatnonzero(keep).astype(np.int32))


def look_at(eye, target, up=(0.0, 1.0, 0.0)):
    """(R, T) float32 of a camera at ``eye`` looking at ``target``, p_cam = R p_world + T with +z forward and +y along ``up``'s side."""
    eye, target, up = (np.asarray(a, np.float64) for a in (eye, target, up))
    fwd = target - eye
    fwd /= np.linalg.norm(fwd)
    right = np.cross(up, fwd)
    right /= np.linalg.norm(right)
    R = np.stack([right, np.cross(fwd, right), fwd])
    return R.astype(np.float32), (-R @ eye).astype(np.float32)


def plane_depth(v, z):
    """The depth plane a view of size ``size_of(v)`` has of a surface at camera depth z everywhere."""
    return np.full(size_of(v), z, np.float32)
