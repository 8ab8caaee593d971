"""The TSDF rules of include/lvdgs.h ("TSDF fusion") in NumPy, each written twice:

``integrate_f32`` / ``mesh_f32``   float32 mirrors of the header, operation for operation (every intermediate is a float32 array, so
                                   NumPy rounds where the kernel rounds; no contraction on either side);
``integrate_f64`` / ``mesh_f64``   the same rules stated in float64, written independently (matrix products, loops over cells).

A volume is a dict: ``dims`` (nx, ny, nz), ``origin`` (3,), ``voxel_size``, ``trunc``, ``max_weight`` and the planes ``tsdf``, ``weight`` and
optionally ``r``, ``g``, ``b`` as flat arrays indexed ``i + nx * (j + ny * k)``.  A view is a dict: ``depth`` (H, W), ``R`` (3, 3), ``T`` (3,),
``intrinsics`` (fx, fy, cx, cy), ``image`` (3, H, W) or None, ``mask`` (H, W) or None, ``depth_min``, ``depth_trunc``.
"""
import numpy as np

F = np.float32
PLANES = ("tsdf", "weight", "r", "g", "b")


def empty_volume(dims, origin, voxel_size, trunc=None, max_weight=64.0, color=True, dtype=np.float32):
    n = int(dims[0]) * int(dims[1]) * int(dims[2])
    vol = dict(dims=tuple(int(d) for d in dims), origin=np.asarray(origin, np.float32), voxel_size=float(voxel_size),
               trunc=4.0 * float(voxel_size) if trunc is None else float(trunc), max_weight=float(max_weight))
    for name in PLANES[:5 if color else 2]:
        vol[name] = np.zeros(n, dtype)
    return vol


def copy_volume(vol, dtype=None):
    out = dict(vol)
    for name in PLANES:
        if name in vol:
            out[name] = vol[name].astype(dtype or vol[name].dtype, copy=True)
    return out


def make_view(depth, R, T, intrinsics, image=None, mask=None, depth_min=0.0, depth_trunc=np.inf):
    return dict(depth=np.ascontiguousarray(depth, np.float32), R=np.asarray(R, np.float32).reshape(3, 3), T=np.asarray(T, np.float32).reshape(3),
                intrinsics=tuple(float(np.float32(v)) for v in intrinsics), image=None if image is None else np.ascontiguousarray(image, np.float32),
                mask=None if mask is None else np.ascontiguousarray(mask), depth_min=float(np.float32(depth_min)),
                depth_trunc=float(np.float32(depth_trunc)))


def lattice_indices(dims):
    nx, ny, nz = dims
    s = np.arange(nx * ny * nz, dtype=np.int64)
    return s % nx, (s // nx) % ny, s // (nx * ny)


# ---------------------------------------------------------------- integration, float32 mirror ----
def integrate_f32(vol, views):
    """Steps 1-5 of the header for every voxel, the views in list order; in place.  -> touched (views, n) bool."""
    i, j, k = lattice_indices(vol["dims"])
    vs, trunc, maxw = F(vol["voxel_size"]), F(vol["trunc"]), F(vol["max_weight"])
    o = vol["origin"].astype(F)
    px, py, pz = o[0] + vs * i.astype(F), o[1] + vs * j.astype(F), o[2] + vs * k.astype(F)
    touched = np.zeros((len(views), px.size), bool)
    with np.errstate(all="ignore"):
        for n, V in enumerate(views):
            R, T = V["R"].astype(F), V["T"].astype(F)
            fx, fy, cx, cy = (F(v) for v in V["intrinsics"])
            H, W = V["depth"].shape
            x = ((R[0, 0] * px + R[0, 1] * py) + R[0, 2] * pz) + T[0]
            y = ((R[1, 0] * px + R[1, 1] * py) + R[1, 2] * pz) + T[1]
            z = ((R[2, 0] * px + R[2, 1] * py) + R[2, 2] * pz) + T[2]
            assert x.dtype == F and z.dtype == F
            ok = z > F(V["depth_min"])
            u, v = fx * (x / z) + cx, fy * (y / z) + cy
            uf, vf = np.floor(u + F(0.5)), np.floor(v + F(0.5))
            assert uf.dtype == F
            ok &= (uf >= 0) & (uf < F(W)) & (vf >= 0) & (vf < F(H))
            ui, vi = np.where(ok, uf, 0).astype(np.int64), np.where(ok, vf, 0).astype(np.int64)
            pix = vi * W + ui
            d = V["depth"].reshape(-1)[pix]
            ok &= (d > 0) & (d <= F(V["depth_trunc"]))
            if V["mask"] is not None:
                ok &= V["mask"].reshape(-1)[pix] != 0
            sdf = d - z
            ok &= ~(sdf < -trunc)
            t = np.minimum(F(1.0), sdf / trunc)
            w0 = vol["weight"]
            w1 = w0 + F(1.0)
            assert t.dtype == F and w1.dtype == F
            vol["tsdf"] = np.where(ok, (vol["tsdf"] * w0 + t) / w1, vol["tsdf"])
            if V["image"] is not None:
                assert "r" in vol, "a colour view on a volume without colour planes"
                for ch, name in enumerate("rgb"):
                    c = V["image"][ch].reshape(-1)[pix]
                    vol[name] = np.where(ok, (vol[name] * w0 + c) / w1, vol[name])
            vol["weight"] = np.where(ok, np.minimum(w1, maxw), w0)
            touched[n] = ok
    for name in PLANES:
        assert name not in vol or vol[name].dtype == F
    return touched


# ---------------------------------------------------------------- integration, float64 statement ----
def integrate_f64(vol, views):
    """The rule in float64 (``vol``'s planes float64; the inputs are the float32 values).  -> (touched, fragile), both (views, n)
    bool: fragile marks the voxels whose decisions sit on an edge a float32 rounding can cross (the module tests/test_tsdf.py says
    which)."""
    nx, ny, nz = vol["dims"]
    i, j, k = lattice_indices(vol["dims"])
    p = vol["origin"].astype(np.float64)[None, :] + np.float64(F(vol["voxel_size"])) * np.stack([i, j, k], 1).astype(np.float64)
    trunc, maxw = np.float64(F(vol["trunc"])), np.float64(F(vol["max_weight"]))
    touched = np.zeros((len(views), len(p)), bool)
    fragile = np.zeros_like(touched)
    with np.errstate(all="ignore"):
        for n, V in enumerate(views):
            pc = p @ V["R"].astype(np.float64).T + V["T"].astype(np.float64)
            fx, fy, cx, cy = V["intrinsics"]
            H, W = V["depth"].shape
            z = pc[:, 2]
            dmin = np.float64(V["depth_min"])
            front = z > dmin
            u, v = fx * pc[:, 0] / z + cx, fy * pc[:, 1] / z + cy
            col, row = np.floor(u + 0.5), np.floor(v + 0.5)
            inside = front & (col >= 0) & (col < W) & (row >= 0) & (row < H)
            pix = np.where(inside, row * W + col, 0).astype(np.int64)
            d = V["depth"].reshape(-1).astype(np.float64)[pix]
            seen = inside & (d > 0) & (d <= np.float64(V["depth_trunc"]))
            if V["mask"] is not None:
                seen &= V["mask"].reshape(-1)[pix] != 0
            sdf = d - z
            ok = seen & (sdf >= -trunc)
            t = np.minimum(1.0, sdf / trunc)
            w = vol["weight"]
            vol["tsdf"] = np.where(ok, (vol["tsdf"] * w + t) / (w + 1.0), vol["tsdf"])
            if V["image"] is not None:
                for ch, name in enumerate("rgb"):
                    c = V["image"][ch].reshape(-1).astype(np.float64)[pix]
                    vol[name] = np.where(ok, (vol[name] * w + c) / (w + 1.0), vol[name])
            vol["weight"] = np.where(ok, np.minimum(w + 1.0, maxw), w)
            touched[n] = ok
            near = lambda a: np.abs(a - np.round(a)) < 1e-4
            frag = front & np.isfinite(u) & np.isfinite(v) & (near(u + 0.5) | near(v + 0.5))
            frag |= np.abs(z - dmin) <= 1e-6 * max(abs(dmin), np.finfo(np.float64).tiny)
            frag |= seen & (np.abs(sdf + trunc) <= 1e-6 * trunc)
            fragile[n] = frag
    return touched, fragile


# ---------------------------------------------------------------- surface nets ----
# the 12 edges of a cell in the header's order: (axis, low corner (dx, dy, dz))
EDGES = ([(0, (0, dy, dz)) for dz in (0, 1) for dy in (0, 1)] + [(1, (dx, 0, dz)) for dz in (0, 1) for dx in (0, 1)]
         + [(2, (dx, dy, 0)) for dy in (0, 1) for dx in (0, 1)])
QUAD = ((-1, -1), (0, -1), (0, 0), (-1, 0))      # c0 .. c3: the offsets in (b, c)


def mesh_f32(vol):
    """-> (vertices (V, 3) float32, colors (V, 3) float32 or None, faces (F, 3) int32), the header's rule, vectorised over cells."""
    nx, ny, nz = vol["dims"]
    f = vol["tsdf"].astype(F).reshape(nz, ny, nx)
    obs = (vol["weight"].reshape(nz, ny, nx) > 0)
    ins = f < 0
    color = "r" in vol
    planes = [vol[c].astype(F).reshape(nz, ny, nx) for c in "rgb"] if color else []
    cx, cy, cz = nx - 1, ny - 1, nz - 1
    corner = lambda a, d: a[d[2]:d[2] + cz, d[1]:d[1] + cy, d[0]:d[0] + cx]
    corners = [(dx, dy, dz) for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)]
    all_obs = np.logical_and.reduce([corner(obs, d) for d in corners])
    n_in = sum(corner(ins, d).astype(np.int32) for d in corners)
    active = all_obs & (n_in > 0) & (n_in < 8)                       # (cz, cy, cx)
    total = [np.zeros(active.shape, F) for _ in range(3)]
    ctotal = [np.zeros(active.shape, F) for _ in range(3)]
    count = np.zeros(active.shape, np.int32)
    with np.errstate(all="ignore"):
        for axis, lo in EDGES:
            hi = tuple(lo[a] + (1 if a == axis else 0) for a in range(3))
            f0, f1 = corner(f, lo), corner(f, hi)
            cross = active & ((f0 < 0) != (f1 < 0))
            q = f0 / (f0 - f1)
            for a in range(3):
                term = q if a == axis else np.full(active.shape, F(lo[a]))
                total[a] = np.where(cross, total[a] + term, total[a])
            for ch in range(len(planes)):
                c0, c1 = corner(planes[ch], lo), corner(planes[ch], hi)
                ctotal[ch] = np.where(cross, ctotal[ch] + (c0 + q * (c1 - c0)), ctotal[ch])
            count += cross
        kk, jj, ii = np.nonzero(active)                               # C order: k slowest -- the order of the low corner's sample index
        cnt = count[kk, jj, ii].astype(F)
        o, vs = vol["origin"].astype(F), F(vol["voxel_size"])
        cell = (ii, jj, kk)
        vertices = np.stack([o[a] + vs * (cell[a].astype(F) + total[a][kk, jj, ii] / cnt) for a in range(3)], 1).astype(F)
        colors = np.stack([ctotal[ch][kk, jj, ii] / cnt for ch in range(3)], 1).astype(F) if color else None
    assert all(t.dtype == F for t in total + ctotal)
    number = np.full((nz, ny, nx), -1, np.int64)                      # vertex number at the low corner's sample
    number[kk, jj, ii] = np.arange(len(kk))
    act = np.zeros((nz, ny, nx), bool)
    act[:cz, :cy, :cx] = active
    rows = []                                                          # (sample, axis, two triangles)
    K, J, I = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    for axis in range(3):
        b, c = (axis + 1) % 3, (axis + 2) % 3
        coord = [I, J, K]
        dims = (nx, ny, nz)
        ok = (coord[axis] < dims[axis] - 1) & (coord[b] >= 1) & (coord[c] >= 1)
        hi = [coord[0] + (axis == 0), coord[1] + (axis == 1), coord[2] + (axis == 2)]
        hi = [np.minimum(h, d - 1) for h, d in zip(hi, dims)]
        ok &= ins != ins[hi[2], hi[1], hi[0]]
        quad = []
        for ob, oc in QUAD:
            cc = [coord[0].copy(), coord[1].copy(), coord[2].copy()]
            cc[b] = np.maximum(cc[b] + ob, 0)
            cc[c] = np.maximum(cc[c] + oc, 0)
            ok &= act[cc[2], cc[1], cc[0]]
            quad.append(number[cc[2], cc[1], cc[0]])
        sel = np.nonzero(ok.reshape(-1))[0]
        v0, v1, v2, v3 = (q.reshape(-1)[sel] for q in quad)
        low_in = ins.reshape(-1)[sel]
        tri_a = np.where(low_in[:, None], np.stack([v0, v1, v2], 1), np.stack([v0, v2, v1], 1))
        tri_b = np.where(low_in[:, None], np.stack([v0, v2, v3], 1), np.stack([v0, v3, v2], 1))
        rows.append((sel * 3 + axis, tri_a, tri_b))
    key = np.concatenate([r[0] for r in rows])
    order = np.argsort(key, kind="stable")
    tri_a = np.concatenate([r[1] for r in rows])[order]
    tri_b = np.concatenate([r[2] for r in rows])[order]
    faces = np.stack([tri_a, tri_b], 1).reshape(-1, 3).astype(np.int32)
    return vertices, colors, faces


def mesh_f64(vol):
    """The same rule cell by cell in float64 (plain loops: for the small volumes of the tests)."""
    nx, ny, nz = vol["dims"]
    at = lambda i, j, k: i + nx * (j + ny * k)
    f = vol["tsdf"].astype(np.float64)
    w = vol["weight"]
    color = "r" in vol
    origin, vs = vol["origin"].astype(np.float64), np.float64(F(vol["voxel_size"]))
    number, vertices, colors = {}, [], []
    for k in range(nz - 1):
        for j in range(ny - 1):
            for i in range(nx - 1):
                ids = [at(i + dx, j + dy, k + dz) for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)]
                inside = [f[s] < 0 for s in ids]
                if not all(w[s] > 0 for s in ids) or all(inside) or not any(inside):
                    continue
                points, cols = [], []
                for axis, lo in EDGES:
                    hi = [lo[0], lo[1], lo[2]]
                    hi[axis] += 1
                    s0, s1 = at(i + lo[0], j + lo[1], k + lo[2]), at(i + hi[0], j + hi[1], k + hi[2])
                    if (f[s0] < 0) == (f[s1] < 0):
                        continue
                    q = f[s0] / (f[s0] - f[s1])
                    pt = np.array(lo, np.float64)
                    pt[axis] += q
                    points.append(pt)
                    if color:
                        cols.append([vol[c][s0] + q * (np.float64(vol[c][s1]) - vol[c][s0]) for c in "rgb"])
                number[(i, j, k)] = len(vertices)
                vertices.append(origin + vs * (np.array([i, j, k], np.float64) + np.mean(points, 0)))
                if color:
                    colors.append(np.mean(np.asarray(cols, np.float64), 0))
    faces = []
    for k in range(nz):
        for j in range(ny):
            for i in range(nx):
                s = [i, j, k]
                for axis in range(3):
                    b, c = (axis + 1) % 3, (axis + 2) % 3
                    e = list(s)
                    e[axis] += 1
                    if e[axis] >= (nx, ny, nz)[axis] or (f[at(*s)] < 0) == (f[at(*e)] < 0):
                        continue
                    quad = []
                    for ob, oc in QUAD:
                        cell = list(s)
                        cell[b] += ob
                        cell[c] += oc
                        quad.append(number.get(tuple(cell)))
                    if any(v is None for v in quad):
                        continue
                    v0, v1, v2, v3 = quad
                    faces += [(v0, v1, v2), (v0, v2, v3)] if f[at(*s)] < 0 else [(v0, v2, v1), (v0, v3, v2)]
    return (np.asarray(vertices, np.float64).reshape(-1, 3), np.asarray(colors, np.float64).reshape(-1, 3) if color else None,
            np.asarray(faces, np.int32).reshape(-1, 3))


# ---------------------------------------------------------------- mesh properties ----
def manifold_report(faces, n_vertices):
    """(closed oriented manifold?, V - E + F) of a triangle list: every directed edge once, its reverse once."""
    faces = np.asarray(faces, np.int64)
    directed = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]])
    keys = directed[:, 0] * (n_vertices + 1) + directed[:, 1]
    back = directed[:, 1] * (n_vertices + 1) + directed[:, 0]
    once = len(np.unique(keys)) == len(keys)
    paired = np.array_equal(np.sort(keys), np.sort(back))
    used = len(np.unique(faces))
    return bool(once and paired and used == n_vertices), n_vertices - len(keys) // 2 + len(faces)


def signed_volume(vertices, faces):
    v = np.asarray(vertices, np.float64)
    a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)


def face_normals(vertices, faces):
    v = np.asarray(vertices, np.float64)
    return np.cross(v[faces[:, 1]] - v[faces[:, 0]], v[faces[:, 2]] - v[faces[:, 0]])
