"""The rule of ``lvdgs_mesh_depth`` (include/lvdgs.h, "Mesh scoring") as NumPy statements.

The vertex stage -- x, y, z, u, v of every vertex -- is float32 in both: the header's error analysis takes the float32 u, v, z as its
operands.  ``dtype`` is the type of everything per pixel.  float32: the MIRROR -- every expression as the header writes it, one rounding
per operation, what the device code is compared with bit for bit.  float64: the STATEMENT -- the same text in double, which stands in for
exact arithmetic (its own rounding is 2^-29 of the float32 one), the tie among equal depths broken by the face index as in the rule.
``fragile`` marks, from the statement alone, the pixels on which the two may disagree, by the header's two bounds.

A view is the dict ``mesh_eval.render_depth`` takes, with NumPy arrays: ``R`` (3, 3), ``T`` (3,), ``intrinsics`` (fx, fy, cx, cy),
``size=(H, W)``, ``depth_min``, ``depth_trunc`` (``mesh_cull_oracle.view`` makes one).
"""
import numpy as np

U = 2.0 ** -24
F32 = np.float32
CHUNK_PAIRS = 1 << 21      # (face, pixel) pairs evaluated at once


def size_of(v):
    return tuple(v["depth"].shape) if v.get("depth") is not None else tuple(v["size"])


def project(vertices, v):
    """Step 1 of "TSDF fusion" and the continuous expressions of step 2, float32 -> (z, u, v) per vertex."""
    p = np.asarray(vertices, F32).reshape(-1, 3)
    R, T = v["R"].astype(F32).reshape(9), v["T"].astype(F32).reshape(3)
    fx, fy, cx, cy = (F32(x) for x in v["intrinsics"])
    px, py, pz = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        x = ((R[0] * px + R[1] * py) + R[2] * pz) + T[0]
        y = ((R[3] * px + R[4] * py) + R[5] * pz) + T[1]
        z = ((R[6] * px + R[7] * py) + R[8] * pz) + T[2]
        return z, fx * (x / z) + cx, fy * (y / z) + cy


def limits(v):
    """(dm, depth_trunc) as float32: dm = fmaxf(depth_min, 0)."""
    dmin = F32(v.get("depth_min", 0.0))
    return (dmin if dmin > 0 else F32(0.0)), F32(v.get("depth_trunc", np.inf))      # (a NaN depth_min: 0, as fmaxf gives)


def face_boxes(vertices, faces, v, dtype=F32):
    """Which faces take part and their pixel boxes -> dict(ok (F,), i0, i1, j0, j1 (int64, 0 where not ok), idx (F, 3) with 0 for the
    indices of a face that is out of range, z, u, v (V,) float32).  ``dtype``: the type the area is computed in."""
    H, W = size_of(v)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    V = len(np.asarray(vertices).reshape(-1, 3))
    z, u, w = project(vertices, v) if V else (np.zeros(0, F32),) * 3
    dm, _ = limits(v)
    inside = ((faces >= 0) & (faces < V)).all(axis=1)
    idx = np.where(inside[:, None], faces, 0)
    if V == 0:
        nothing = np.zeros(len(faces), np.int64)
        return dict(ok=np.zeros(len(faces), bool), i0=nothing, i1=nothing, j0=nothing, j1=nothing, idx=idx, z=z, u=u, v=w)
    fz, fu, fv = z[idx], u[idx], w[idx]
    with np.errstate(all="ignore"):
        ok = inside & (fz > dm).all(axis=1) & (np.abs(fu) < F32(np.inf)).all(axis=1) & (np.abs(fv) < F32(np.inf)).all(axis=1)
        au, av = fu.astype(dtype), fv.astype(dtype)
        ar = (au[:, 1] - au[:, 0]) * (av[:, 2] - av[:, 0]) - (av[:, 1] - av[:, 0]) * (au[:, 2] - au[:, 0])
        ok &= (ar > 0) | (ar < 0)
        ulo, uhi = np.ceil(fu.min(axis=1)), np.floor(fu.max(axis=1))
        vlo, vhi = np.ceil(fv.min(axis=1)), np.floor(fv.max(axis=1))
        ok &= (ulo < F32(W)) & (uhi >= 0) & (ulo <= uhi) & (vlo < F32(H)) & (vhi >= 0) & (vlo <= vhi)

    def clamp(lo, hi, n):      # max(0, lo) .. min(n - 1, hi), decided on the floats
        with np.errstate(all="ignore"):
            first = np.where(ok & (lo > 0), lo, 0).astype(np.int64)
            last = np.where(ok, np.where(hi < F32(n), hi, n - 1), 0).astype(np.int64)
        return first, last

    (i0, i1), (j0, j1) = clamp(ulo, uhi, W), clamp(vlo, vhi, H)
    return dict(ok=ok, i0=i0, i1=i1, j0=j0, j1=j1, idx=idx, z=z, u=u, v=w)


def _pairs(box, lo, hi):
    """The (face, i, j) of every pixel of the boxes of faces lo .. hi-1 that take part."""
    f = np.flatnonzero(box["ok"][lo:hi]) + lo
    bw = box["i1"][f] - box["i0"][f] + 1
    n = bw * (box["j1"][f] - box["j0"][f] + 1)
    start = np.cumsum(n) - n
    face = np.repeat(f, n)
    t = np.arange(int(n.sum()), dtype=np.int64) - np.repeat(start, n)
    w = np.repeat(bw, n)
    row = t // w
    return face, np.repeat(box["i0"][f], n) + (t - row * w), np.repeat(box["j0"][f], n) + row


def candidates(vertices, faces, v, dtype=F32):
    """Every (face, pixel) pair of the boxes -> dict of arrays over the pairs: face, pix, E (n, 3), A, zp, covered, passes (covered and
    zp inside (dm, depth_trunc]), and -- float64 numbers for the header's bounds -- edge_bound (n, 3) and depth_bound (relative)."""
    H, W = size_of(v)
    t = dtype
    box = face_boxes(vertices, faces, v, dtype)
    dm, trunc = limits(v)
    sizes = np.where(box["ok"], (box["i1"] - box["i0"] + 1) * (box["j1"] - box["j0"] + 1), 0)
    ends = np.cumsum(sizes)
    out = {k: [] for k in ("face", "pix", "E", "A", "zp", "covered", "passes", "edge_bound", "depth_bound")}
    lo = 0
    while lo < len(sizes):
        hi = int(np.searchsorted(ends, (ends[lo - 1] if lo else 0) + CHUNK_PAIRS, side="right"))
        hi = max(hi, lo + 1)
        face, i, j = _pairs(box, lo, hi)
        lo = hi
        if len(face) == 0:
            continue
        idx = box["idx"][face]
        fi, fj = i.astype(F32).astype(t), j.astype(F32).astype(t)
        E, bound = [], []
        with np.errstate(all="ignore"):
            for k in range(3):      # the edge opposite vertex k: a1 -> a2, a2 -> a0, a0 -> a1
                a, b = idx[:, (k + 1) % 3], idx[:, (k + 2) % 3]
                flip = b < a
                l, h = np.where(flip, b, a), np.where(flip, a, b)
                ul, vl, uh, vh = (box[c][n].astype(t) for c, n in (("u", l), ("v", l), ("u", h), ("v", h)))
                du, dv, dj, di = uh - ul, vh - vl, fj - vl, fi - ul
                s = du * dj - dv * di
                E.append(np.where(flip, -s, s))
                bound.append(4 * U * (np.abs(du.astype(np.float64)) * np.abs(dj.astype(np.float64))
                                      + np.abs(dv.astype(np.float64)) * np.abs(di.astype(np.float64))))
            E, bound = np.stack(E, axis=1), np.stack(bound, axis=1)
            covered = (E >= 0).all(axis=1) | (E <= 0).all(axis=1)
            A = (E[:, 0] + E[:, 1]) + E[:, 2]
            z = box["z"][idx].astype(t)
            one = t(1.0)
            wgt = E / A[:, None]
            inv = (wgt[:, 0] * (one / z[:, 0]) + wgt[:, 1] * (one / z[:, 1])) + wgt[:, 2] * (one / z[:, 2])
            zp = one / inv
            passes = covered & (zp > t(dm)) & (zp <= t(trunc))
            z64 = z.astype(np.float64)
            depth_bound = 8 * U + bound.sum(axis=1) / np.abs(A.astype(np.float64)) * (z64.max(axis=1) / z64.min(axis=1) - 1.0)
        for k, a in (("face", face), ("pix", j * W + i), ("E", E), ("A", A), ("zp", zp), ("covered", covered), ("passes", passes),
                     ("edge_bound", bound), ("depth_bound", depth_bound)):
            out[k].append(a)
    empty = dict(face=np.zeros(0, np.int64), pix=np.zeros(0, np.int64), E=np.zeros((0, 3), t), A=np.zeros(0, t), zp=np.zeros(0, t),
                 covered=np.zeros(0, bool), passes=np.zeros(0, bool), edge_bound=np.zeros((0, 3)), depth_bound=np.zeros(0))
    return {k: (np.concatenate(a) if a else empty[k]) for k, a in out.items()}


def resolve(c, size):
    """The winner per pixel among the passing candidates: the smallest zp, among equal zp the smallest face -> (depth (H, W) of the
    candidates' dtype, 0 where none; face_index (H, W) int32, -1 where none)."""
    H, W = size
    ok = c["passes"]
    zp, pix, face = c["zp"][ok], c["pix"][ok], c["face"][ok]
    best = np.full(H * W, np.inf, zp.dtype)
    np.minimum.at(best, pix, zp)
    first = np.full(H * W, np.iinfo(np.int64).max, np.int64)
    won = zp == best[pix]
    np.minimum.at(first, pix[won], face[won])
    hit = first != np.iinfo(np.int64).max
    return np.where(hit, best, 0).astype(zp.dtype).reshape(H, W), np.where(hit, first, -1).astype(np.int32).reshape(H, W)


def render(vertices, faces, v, dtype=F32):
    """One view -> (depth (H, W), face_index (H, W) int32)."""
    return resolve(candidates(vertices, faces, v, dtype), size_of(v))


def fragile(vertices, faces, v, factor=2.0):
    """From the float64 statement: the pixels (H, W) bool where the float32 rule may decide otherwise than exact arithmetic -- some face
    whose box holds the pixel has an edge value within ``factor`` times the header's edge bound of 0; or the two nearest candidate
    depths, or a candidate and dm or depth_trunc, lie within ``factor`` times the header's depth bounds of each other."""
    H, W = size_of(v)
    c = candidates(vertices, faces, v, np.float64)
    dm, trunc = (float(x) for x in limits(v))
    out = np.zeros(H * W, bool)
    out[c["pix"][(np.abs(c["E"]) <= factor * c["edge_bound"]).any(axis=1)]] = True
    cov = c["covered"] & np.isfinite(c["zp"])
    zp, pix, slack = c["zp"][cov], c["pix"][cov], factor * c["depth_bound"][cov] * np.abs(c["zp"][cov])
    out[pix[(np.abs(zp - dm) <= slack) | (np.abs(zp - trunc) <= slack)]] = True
    ok = c["passes"][cov]
    zp, pix, slack = zp[ok], pix[ok], slack[ok]
    order = np.lexsort((zp, pix))
    zp, pix, slack = zp[order], pix[order], slack[order]
    first = np.flatnonzero(np.r_[True, pix[1:] != pix[:-1]]) if len(pix) else np.zeros(0, np.int64)
    second = first + 1
    has = second < len(pix)
    has[has] = pix[second[has]] == pix[first[has]]
    a, b = first[has], second[has]
    out[pix[a][zp[b] - zp[a] <= slack[a] + slack[b]]] = True
    return out.reshape(H, W)


def depth_bounds(vertices, faces, v, face_index, factor=2.0):
    """Per pixel the header's absolute depth bound, ``factor`` times, of the winning face ``face_index`` (H, W) gives (0 where -1)."""
    H, W = size_of(v)
    c = candidates(vertices, faces, v, np.float64)
    out = np.zeros(H * W)
    win = c["face"] == face_index.reshape(-1)[c["pix"]]
    out[c["pix"][win]] = factor * c["depth_bound"][win] * np.abs(c["zp"][win])
    return out.reshape(H, W)


# ---------------------------------------------------------------- scenes ----
def soup(n, seed, lo=(-0.5, -0.5, -0.3), hi=(2.5, 2.5, 0.9), extent=0.5):
    """``n`` triangles with corners within ``extent`` of random centres in the box: (vertices (3n, 3), faces (n, 3))."""
    rng = np.random.default_rng(seed)
    centre = rng.random((n, 1, 3)) * (np.asarray(hi) - np.asarray(lo)) + np.asarray(lo)
    v = (centre + (rng.random((n, 3, 3)) - 0.5) * 2 * extent).reshape(-1, 3).astype(F32)
    return v, np.arange(3 * n, dtype=np.int32).reshape(n, 3)


def fan(centre, radius, n=7, z=1.0, phase=0.3):
    """A closed fan of ``n`` faces around the vertex ``centre`` = (x, y), in the plane z: (vertices (n + 1, 3), faces (n, 3))."""
    a = phase + 2 * np.pi * np.arange(n) / n
    rim = np.stack([centre[0] + radius * np.cos(a), centre[1] + radius * np.sin(a), np.full(n, z)], axis=1)
    v = np.concatenate([[[centre[0], centre[1], z]], rim]).astype(F32)
    k = np.arange(n)
    return v, np.stack([np.zeros(n, np.int64), 1 + k, 1 + (k + 1) % n], axis=1).astype(np.int32)


def erode(mask):
    """``mask`` (H, W) bool less every pixel with a neighbour (of its eight, or the image's border) outside it."""
    p = np.pad(mask, 1, constant_values=False)
    out = mask.copy()
    for dj in (0, 1, 2):
        for di in (0, 1, 2):
            out &= p[dj:dj + mask.shape[0], di:di + mask.shape[1]]
    return out
