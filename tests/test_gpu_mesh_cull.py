"""``lvdgs_mesh_visibility`` / ``lvdgs_mesh_cull`` through ``lvdgs.mesh_eval`` on the GPU against the float32 mirror of
tests/mesh_cull_oracle.py: the ``seen`` plane, the counts, vertices, colours, faces and both origin arrays BIT FOR BIT, the sentinel rows
behind the counts untouched, two calls the same bytes.  Then what culling means on two squares, and ``SlamSequence.eval_mesh`` with a
ground-truth mesh and ``cull`` over the toy sequence.  Every case is a few thousand elements unless its name says otherwise.
"""
import math

import numpy as np
import pytest
import torch

import mesh_cull_oracle as orc
import mesh_eval_oracle as meo
from lvdgs import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAD = 64
F32 = np.float32


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _device_view(v):
    out = {k: (_t(x) if isinstance(x, np.ndarray) else x) for k, x in v.items()}
    if out.get("depth") is not None:
        out.pop("size", None)
    return out


# ---------------------------------------------------------------- visibility ----
def _visibility(vertices, views, eps, seen0=None, batches=None):
    """``mesh_eval.visibility`` into a plane with PAD sentinel bytes behind it -> (seen (V,), the sentinels).  ``batches``: the views
    in several accumulating calls of those sizes."""
    from lvdgs import mesh_eval
    V = len(vertices)
    plane = torch.full((V + PAD,), 0xAB, dtype=torch.uint8, device=DEV)
    plane[:V] = 0 if seen0 is None else _t(np.asarray(seen0, np.uint8))
    views = [_device_view(v) for v in views]
    first = 0
    for n in (batches or [len(views)]):
        out = mesh_eval.visibility(_t(vertices), views[first:first + n], eps, seen=plane[:V])
        assert out.data_ptr() == plane.data_ptr()
        first += n
    got = plane.cpu().numpy()
    return got[:V], got[V:]


def _check_visibility(vertices, views, eps, seen0=None, batches=None):
    vertices = np.ascontiguousarray(vertices, F32).reshape(-1, 3)
    want = orc.visibility(vertices, views, eps, seen=seen0)
    got, pad = _visibility(vertices, views, eps, seen0, batches)
    assert (pad == 0xAB).all()
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:10]
    again, _ = _visibility(vertices, views, eps, seen0, batches)
    assert np.array_equal(again, got)      # two calls, the same bytes
    return got


def _cloud(seed, n):
    """Points around and between two walls at z = 0 and z = 0.6 over [0, 2]^2, some well outside."""
    rng = np.random.default_rng(seed)
    return (rng.random((n, 3)) * [3.0, 3.0, 1.2] - [0.5, 0.5, 0.3]).astype(F32)


def _orbit(k, n, size=(48, 64), seed=0, depth=True, **kw):
    """View k of n on an arc in front of the walls, with a noisy depth plane (pixels of 0, NaN and +inf among them)."""
    rng = np.random.default_rng(1000 * seed + k)
    a = -0.9 + 1.8 * (k + 0.5) / n
    R, T = orc.look_at((1.0 + 2.6 * math.sin(a), 0.9 + 0.1 * k / n, -2.6 * math.cos(a)), (1.0, 1.0, 0.2))
    H, W = size
    f = 0.9 * W
    if not depth:
        return orc.view(R, T, (f, f * 1.05, W / 2 - 0.3, H / 2 - 0.4), size=size, **kw)
    d = rng.uniform(1.6, 3.6, size).astype(F32)
    flat = d.reshape(-1)
    for value, share in ((0.0, 20), (np.nan, 40), (np.inf, 40)):
        flat[rng.integers(0, flat.size, max(flat.size // share, 1) if flat.size > 1 else 0)] = value
    return orc.view(R, T, (f, f * 1.05, W / 2 - 0.3, H / 2 - 0.4), depth=d, **kw)


@pytest.mark.parametrize("V", [1, 255, 256, 257, 70_000])
def test_visibility_sizes(V):
    views = [_orbit(0, 3), _orbit(1, 3, depth_trunc=3.0), _orbit(2, 3, depth=False, depth_trunc=2.9)]
    got = _check_visibility(_cloud(V, V), views, 0.05)
    if V >= 255:
        assert 0 < got.sum() < V


@pytest.mark.parametrize("sizes", [[(1, 1)], [(48, 64)], [(48, 64), (30, 100)]])
def test_visibility_image_sizes(sizes):
    views = [_orbit(k, len(sizes), size=s) for k, s in enumerate(sizes)]
    if sizes == [(1, 1)]:      # one pixel: a narrow cone around the axis, its depth beyond everything
        views[0]["depth"][:] = 9.0
        views[0]["intrinsics"] = (3.0, 3.0, 0.0, 0.0)
    got = _check_visibility(_cloud(5, 3000), views, 0.05)
    assert 0 < got.sum() < 3000


@pytest.mark.parametrize("count, batches", [(0, None), (1, None), (16, None), (17, [16, 1]), (17, [5, 12])])
def test_visibility_view_counts(count, batches):
    """17 views go through as two accumulating calls and equal the mirror over all 17."""
    views = [_orbit(k, max(count, 1), size=(24, 32), seed=3, mask=(np.random.default_rng(k).random((24, 32)) > 0.2) if k % 3 == 0 else None)
             for k in range(count)]
    got = _check_visibility(_cloud(9, 2500), views, 0.03, batches=batches)
    assert (got.sum() == 0) == (count == 0)


def _up(x):
    return np.nextafter(F32(x), F32(np.inf))


def _down(x):
    return np.nextafter(F32(x), F32(-np.inf))


def test_visibility_on_the_boundaries():
    """An axis-aligned camera at the origin (z = pz, u = fx * (px / pz) + cx: every boundary can be hit exactly): pixel edges, the last
    column and row, z at depth_min and depth_trunc, d - z at -eps and one ulp either side, depths of 0, NaN and +inf, a masked pixel,
    non-finite vertices, a frustum-only view among depth views, and bytes that were set before the call."""
    R, T = np.eye(3, dtype=F32), np.zeros(3, F32)
    W, H, fx, fy, cx, cy = 8, 6, 4.0, 4.0, 3.5, 2.5      # at pz = 1: u + 0.5 = 4 px + 4, v + 0.5 = 4 py + 3
    eps = F32(0.25)
    depth = np.full((H, W), 2.0, F32)
    depth[0, 0], depth[0, 1], depth[0, 2] = 0.0, np.nan, np.inf
    mask = np.ones((H, W), np.uint8)
    mask[1, 0] = 0
    with_depth = orc.view(R, T, (fx, fy, cx, cy), depth=depth, mask=mask, depth_min=0.5)
    frustum = orc.view(R, T, (fx, fy, cx, cy), size=(H, W), depth_min=0.5, depth_trunc=3.0)

    def at(u_half, v_half, z):      # the vertex with u + 0.5 = u_half and v + 0.5 = v_half at depth z (exact for these values)
        return [(u_half - 4.0) / 4.0 * z, (v_half - 3.0) / 4.0 * z, z]

    rows = [
        # frustum only: name, vertex, seen
        ("inside", at(4.5, 3.5, 1.0), 1),
        ("on a pixel edge: the pixel to the right", at(5.0, 3.5, 1.0), 1),
        ("on the image's left edge: inside", at(0.0, 3.5, 1.0), 1),
        ("just left of it", [-1.01, 0.125, 1.0], 0),
        ("on the right edge: u + 0.5 = W, outside", at(8.0, 3.5, 1.0), 0),
        ("in the last column", [0.99, 0.125, 1.0], 1),
        ("on the bottom edge: v + 0.5 = H, outside", at(4.5, 6.0, 1.0), 0),
        ("in the last row", [0.125, 0.74, 1.0], 1),
        ("z == depth_min: not in front of it", at(4.5, 3.5, 0.5), 0),
        ("one ulp in front", at(4.5, 3.5, 1.0)[:2] + [_up(0.5)], 1),
        ("z == 0", [0.0, 0.0, 0.0], 0),
        ("z < 0", at(4.5, 3.5, -1.0), 0),
        ("z == depth_trunc: seen", [0.0, 0.0, 3.0], 1),
        ("one ulp beyond", [0.0, 0.0, _up(3.0)], 0),
        ("a NaN", [np.nan, 0.0, 1.0], 0), ("an infinity", [0.0, np.inf, 1.0], 0), ("an infinite depth", [0.0, 0.0, np.inf], 0),
        ("minus infinity", [-np.inf, 0.0, 1.0], 0),
    ]
    vertices = np.array([r[1] for r in rows], F32)
    got = _check_visibility(vertices, [frustum], eps)
    assert got.tolist() == [r[2] for r in rows], [(r[0], int(g)) for r, g in zip(rows, got) if g != r[2]]

    rows = [
        # against the depth plane (2.0 everywhere but the pixels above): name, vertex, seen
        ("in front of the surface", at(4.5, 3.5, 1.0), 1),
        ("on it", [0.0, 0.0, 2.0], 1),
        ("d - z == -eps exactly: seen", [0.0, 0.0, 2.25], 1),
        ("one ulp nearer", [0.0, 0.0, _down(2.25)], 1),
        ("one ulp farther: d - z < -eps", [0.0, 0.0, _up(2.25)], 0),
        ("well behind", [0.0, 0.0, 2.9], 0),
        ("a depth of 0", at(0.5, 0.5, 1.0), 0),
        ("a depth of NaN", at(1.5, 0.5, 1.0), 0),
        ("a depth of +inf under an infinite depth_trunc", at(2.5, 0.5, 1.0), 1),
        ("a masked pixel", at(0.5, 1.5, 1.0), 0),
        ("its neighbour", at(1.5, 1.5, 1.0), 1),
        ("z == depth_min", at(4.5, 3.5, 0.5), 0),
        ("a NaN", [0.0, np.nan, 1.0], 0), ("an infinity", [np.inf, np.inf, np.inf], 0),
    ]
    vertices = np.array([r[1] for r in rows], F32)
    got = _check_visibility(vertices, [with_depth], eps)
    assert got.tolist() == [r[2] for r in rows], [(r[0], int(g)) for r, g in zip(rows, got) if g != r[2]]
    finite_trunc = dict(with_depth, depth_trunc=2.0)      # d == depth_trunc passes, +inf no longer
    got = _check_visibility(vertices, [finite_trunc], eps)
    assert got[[0, 1, 8]].tolist() == [1, 1, 0]
    # the frustum-only view sees what the surface hides; bytes set before the call survive, whatever they hold
    mixed = _check_visibility(vertices, [with_depth, frustum, with_depth], eps)
    assert mixed[5] == 1 and mixed[4] == 1 and mixed[6] == 1 and mixed[11] == 0
    before = np.zeros(len(rows), np.uint8)
    before[[0, 5, 12]] = (7, 200, 1)
    got = _check_visibility(vertices, [with_depth], eps, seen0=before)
    assert got[[0, 5, 12]].tolist() == [7, 200, 1] and got[1] == 1 and got[4] == 0
    assert _check_visibility(vertices, [], eps, seen0=before).tolist() == before.tolist()


def test_visibility_refuses_what_is_not_on_the_gpu_or_misshapen():
    from lvdgs import mesh_eval
    v = _cloud(1, 10)
    view = _orbit(0, 1)
    with pytest.raises(_lib.LvdgsError, match="no CPU path"):
        mesh_eval.visibility(torch.from_numpy(v), [_device_view(view)], 0.0)
    with pytest.raises(_lib.LvdgsError, match="seen must be"):
        mesh_eval.visibility(_t(v), [_device_view(view)], 0.0, seen=torch.zeros(9, dtype=torch.uint8, device=DEV))
    with pytest.raises(_lib.LvdgsError, match="needs size"):
        mesh_eval.visibility(_t(v), [dict(_device_view(view), depth=None)], 0.0)
    with pytest.raises(_lib.LvdgsError, match="occlusion_eps"):
        mesh_eval.visibility(_t(v), [_device_view(view)], -1.0)


# ---------------------------------------------------------------- compaction ----
def _cull_raw(v, f, seen, rule, c=None, origins=True):
    """One call into buffers with PAD sentinel rows behind the inputs' capacity -> dict of the outputs whole, and the counts."""
    from lvdgs import mesh_eval
    V, F = len(v), len(f)
    out = dict(vertices=torch.full((V + PAD, 3), -7.5, dtype=torch.float32, device=DEV), faces=torch.full((F + PAD, 3), -77, dtype=torch.int32, device=DEV),
               colors=torch.full((V + PAD, 3), -7.5, dtype=torch.float32, device=DEV) if c is not None else None,
               vertex_origin=torch.full((V + PAD,), -77, dtype=torch.int32, device=DEV) if origins else None,
               face_origin=torch.full((F + PAD,), -77, dtype=torch.int32, device=DEV) if origins else None)
    nv, nf = mesh_eval.cull_raw(_t(np.ascontiguousarray(v, F32).reshape(-1, 3)), _t(np.ascontiguousarray(f, np.int32).reshape(-1, 3)),
                                _t(np.ascontiguousarray(seen, np.uint8)), rule, out["vertices"], out["faces"], vertex_colors=_t(c),
                                out_colors=out["colors"], vertex_origin=out["vertex_origin"], face_origin=out["face_origin"])
    return {k: None if x is None else x.cpu().numpy() for k, x in out.items()}, nv, nf


def _check_cull(v, f, seen, rule, c=None, origins=True):
    want = orc.cull(v, f, seen, rule, colors=c)
    got, nv, nf = _cull_raw(v, f, seen, rule, c, origins)
    assert (nv, nf) == (len(want["vertices"]), len(want["faces"]))
    for key, n, sentinel in (("vertices", nv, -7.5), ("colors", nv, -7.5), ("faces", nf, -77), ("vertex_origin", nv, -77), ("face_origin", nf, -77)):
        if got[key] is None:
            assert key != "vertices" and key != "faces"
            continue
        assert (got[key][n:] == sentinel).all(), key      # rows beyond the counts are not touched
        assert np.array_equal(_bits(got[key][:n]), _bits(want[key])), key
    again, nv2, nf2 = _cull_raw(v, f, seen, rule, c, origins)
    assert (nv2, nf2) == (nv, nf) and all(again[k] is None or np.array_equal(_bits(again[k]), _bits(got[k])) for k in got)      # two calls, the same bytes
    return want


def _random_mesh(seed, F, V=None):
    rng = np.random.default_rng(seed)
    V = max(F // 2, 3) if V is None else V
    v = rng.standard_normal((V, 3)).astype(F32)
    c = rng.random((V, 3)).astype(F32)
    f = rng.integers(0, V, (F, 3)).astype(np.int32)
    seen = (rng.random(V) < 0.7).astype(np.uint8) * rng.integers(1, 256, V).astype(np.uint8)      # any non-0 byte counts
    return v, f, c, seen


@pytest.mark.parametrize("rule", [orc.ALL, orc.ANY])
@pytest.mark.parametrize("F", [1, 255, 256, 257, 70_000])
def test_cull_sizes(F, rule):
    v, f, c, seen = _random_mesh(F, F)
    want = _check_cull(v, f, seen, rule, c)
    if F >= 255:
        assert 0 < len(want["faces"]) < F


def test_cull_more_faces_than_2048_spans_of_a_tile():
    """525 312 faces: 2052 tiles of 256, so the spans are two tiles long and a workgroup walks more than one."""
    v, f, c, seen = _random_mesh(77, 525_312, V=300_000)
    want = _check_cull(v, f, seen, orc.ALL, c)
    assert 100_000 < len(want["faces"]) < 300_000 and len(want["vertices"]) < 300_000


@pytest.mark.parametrize("colors, origins", [(True, True), (True, False), (False, True), (False, False)])
def test_cull_with_and_without_colours_and_origins(colors, origins):
    v, f, c, seen = _random_mesh(5, 3000)
    _check_cull(v, f, seen, orc.ALL, c if colors else None, origins)


def test_cull_nothing_everything_and_every_other_face():
    v, f, c, seen = _random_mesh(6, 2000)
    assert len(_check_cull(v, f, np.zeros_like(seen), orc.ANY, c)["faces"]) == 0
    want = _check_cull(v, f, np.ones_like(seen), orc.ALL, c)
    assert len(want["faces"]) == len(f)
    # disjoint triangles, those with an odd number seen
    F = 1001
    v = np.random.default_rng(1).standard_normal((3 * F, 3)).astype(F32)
    f = np.arange(3 * F, dtype=np.int32).reshape(F, 3)
    seen = np.repeat((np.arange(F) % 2).astype(np.uint8), 3)
    want = _check_cull(v, f, seen, orc.ALL)
    assert want["face_origin"].tolist() == list(range(1, F, 2)) and len(want["vertices"]) == 3 * (F // 2)
    assert np.array_equal(want["faces"], np.arange(3 * (F // 2), dtype=np.int32).reshape(-1, 3))


def test_cull_indices_out_of_range_and_unreferenced_vertices():
    v, f, c, seen = _random_mesh(8, 1500, V=900)
    f[3, 0], f[77, 1], f[500, 2], f[1499, 0] = -1, len(v), 2 ** 31 - 1, -2 ** 31
    f[f == 123] = 124      # vertex 123 is seen and no face references it
    seen[:] = 1
    for rule in (orc.ALL, orc.ANY):
        want = _check_cull(v, f, seen, rule, c)
        assert not np.isin([3, 77, 500, 1499], want["face_origin"]).any() and len(want["faces"]) == len(f) - 4
        assert 123 not in want["vertex_origin"]
    # without vertices every face is out of range; without faces no vertex is referenced
    assert len(_check_cull(v[:0], f, seen[:0], orc.ANY)["faces"]) == 0
    assert len(_check_cull(v, f[:0], seen, orc.ANY, c)["vertices"]) == 0


def test_cull_the_two_rules_on_a_strip():
    """Vertices 0 .. 5 in a strip of four triangles, vertices 0, 1, 2 seen: ALL keeps the first triangle, ANY the first three and with
    them the unseen vertices 3 and 4; vertex 5 goes either way."""
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [0, 2, 0], [1, 2, 0]], F32)
    f = np.array([[0, 1, 2], [1, 3, 2], [2, 3, 4], [3, 5, 4]], np.int32)
    seen = np.array([1, 1, 1, 0, 0, 0], np.uint8)
    want = _check_cull(v, f, seen, orc.ALL)
    assert want["faces"].tolist() == [[0, 1, 2]] and want["vertex_origin"].tolist() == [0, 1, 2]
    want = _check_cull(v, f, seen, orc.ANY)
    assert want["face_origin"].tolist() == [0, 1, 2] and want["vertex_origin"].tolist() == [0, 1, 2, 3, 4]
    assert want["faces"].tolist() == [[0, 1, 2], [1, 3, 2], [2, 3, 4]]


def test_cull_refuses_outputs_that_alias_an_input():
    from lvdgs import mesh_eval
    v, f, c, seen = _random_mesh(9, 100)
    tv, tf, ts = _t(v), _t(f), _t(seen)
    ov, of = torch.empty_like(tv), torch.empty_like(tf)
    with pytest.raises(_lib.LvdgsError, match="out_vertices overlaps vertices"):
        mesh_eval.cull_raw(tv, tf, ts, orc.ALL, tv, of)
    with pytest.raises(_lib.LvdgsError, match="out_faces overlaps faces"):
        mesh_eval.cull_raw(tv, tf, ts, orc.ALL, ov, tf)
    with pytest.raises(_lib.LvdgsError, match="face_origin overlaps faces"):
        mesh_eval.cull_raw(tv, tf, ts, orc.ALL, ov, of, face_origin=tf.view(-1)[50:])
    with pytest.raises(_lib.LvdgsError, match="face_rule"):
        mesh_eval.cull_raw(tv, tf, ts, 2, ov, of)
    assert mesh_eval.cull_raw(tv, tf, ts, orc.ALL, ov, of) == tuple(len(orc.cull(v, f, seen)[k]) for k in ("vertices", "faces"))


def test_cull_mesh_returns_a_sliced_mesh_and_a_record():
    from lvdgs import mesh_eval
    from lvdgs.tsdf import Mesh
    w, g, c = meo.wavy_wall(40, 30, seed=3)
    views = [_orbit(0, 2, depth=False), _orbit(1, 2, depth=False, depth_trunc=2.7)]
    mesh = Mesh(_t(w), _t(c), _t(g))
    seen = orc.visibility(w, views, 0.0)
    for rule, code in (("all", orc.ALL), ("any", orc.ANY)):
        want = orc.cull(w, g, seen, code, colors=c)
        kept, record = mesh_eval.cull_mesh(mesh, views=[_device_view(v) for v in views], face_rule=rule, want_origin=True)
        assert isinstance(kept, Mesh) and (record["vertices_before"], record["faces_before"]) == (len(w), len(g))
        assert (record["vertices"], record["faces"]) == (len(want["vertices"]), len(want["faces"])) == (kept.vertices.shape[0], kept.faces.shape[0])
        assert 0 < record["faces"] <= len(g) and (rule == "any" or record["faces"] < len(g))
        for got, key in ((kept.vertices, "vertices"), (kept.colors, "colors"), (kept.faces, "faces"), (record["vertex_origin"], "vertex_origin"),
                         (record["face_origin"], "face_origin")):
            assert np.array_equal(_bits(got.cpu().numpy()), _bits(want[key])), key
    kept, record = mesh_eval.cull_mesh((mesh.vertices, mesh.faces), seen=_t(seen))      # a pair, a plane of the caller's
    assert kept.colors is None and record["faces"] == len(orc.cull(w, g, seen)["faces"]) and "vertex_origin" not in record
    with pytest.raises(_lib.LvdgsError, match="views, a seen plane"):
        mesh_eval.cull_mesh(mesh)
    with pytest.raises(_lib.LvdgsError, match="face_rule"):
        mesh_eval.cull_mesh(mesh, seen=_t(seen), face_rule="most")


# ---------------------------------------------------------------- what it means ----
def _grid_square(lo, hi, n, z):
    """The square [lo, hi]^2 at height z as 2 (n - 1)^2 triangles."""
    t = np.linspace(lo, hi, n)
    x, y = np.meshgrid(t, t, indexing="xy")
    v = np.stack([x.reshape(-1), y.reshape(-1), np.full(n * n, z)], axis=1).astype(F32)
    i = (np.arange(n - 1)[None, :] + n * np.arange(n - 1)[:, None]).reshape(-1)
    f = np.concatenate([np.stack([i, i + 1, i + n], axis=1), np.stack([i + 1, i + n + 1, i + n], axis=1)]).astype(np.int32)
    return v, f


def _two_squares():
    """The unit square at z = 0 and the square [-1, 2]^2 one behind it, and a camera two in front of the first that sees all of both:
    (vertices, faces, the camera's (R, T), its intrinsics and size, the depth plane a renderer of both squares gives it)."""
    (v0, f0), (v1, f1) = _grid_square(0.0, 1.0, 21, 0.0), _grid_square(-1.0, 2.0, 31, 1.0)
    v, f = np.concatenate([v0, v1]), np.concatenate([f0, f1 + len(v0)])
    R, T = orc.look_at((0.5, 0.5, -2.0), (0.5, 0.5, 0.0))
    H, W, focal = 96, 96, 50.0
    intr = (focal, focal, 47.5, 47.5)
    ui, vi = np.meshgrid(np.arange(W), np.arange(H), indexing="xy")
    x2, y2 = (ui - intr[2]) / focal * 2.0 + 0.5, (vi - intr[3]) / focal * 2.0 + 0.5      # where the pixel's ray meets z = 0
    depth = np.where((x2 >= 0) & (x2 <= 1) & (y2 >= 0) & (y2 <= 1), 2.0, 3.0).astype(F32)
    return v, f, len(v0), (R, T), intr, (H, W), depth


def test_two_parallel_squares_and_one_camera():
    from lvdgs import mesh_eval
    v, f, n_front, (R, T), intr, size, depth = _two_squares()
    mesh = (_t(v), _t(f))
    frustum = orc.view(R, T, intr, size=size)
    kept, record = mesh_eval.cull_mesh(mesh, views=[_device_view(frustum)])
    assert (record["vertices"], record["faces"]) == (len(v), len(f))      # the frustum holds both squares
    assert np.array_equal(_bits(kept.vertices.cpu().numpy()), _bits(v)) and np.array_equal(kept.faces.cpu().numpy(), f)

    visible = orc.view(R, T, intr, depth=depth)
    kept, record = mesh_eval.cull_mesh(mesh, views=[_device_view(visible)], occlusion_eps=0.05, want_origin=True)
    want = orc.cull(v, f, orc.visibility(v, [visible], 0.05))
    origin = record["vertex_origin"].cpu().numpy()
    assert np.array_equal(origin, want["vertex_origin"]) and np.array_equal(kept.faces.cpu().numpy(), want["faces"])
    assert (origin[:n_front] == np.arange(n_front)).all()      # the front square whole
    back = v[origin[n_front:]]
    assert len(back) > 0 and (back[:, 2] == 1.0).all()
    # the back square's rim only: the front square, half a unit wide at depth 2, shadows |x - 0.5| <= 0.75 at depth 3 (a pixel there is 0.06)
    hidden = (np.abs(back[:, 0] - 0.5) < 0.7) & (np.abs(back[:, 1] - 0.5) < 0.7)
    assert not hidden.any()
    all_back = v[n_front:]
    outside = (np.abs(all_back[:, 0] - 0.5) > 0.95) | (np.abs(all_back[:, 1] - 0.5) > 0.95)      # two grid steps clear of the shadow
    assert outside.sum() > 0 and np.isin(np.flatnonzero(outside) + n_front, origin).all()


def test_a_camera_turned_away_keeps_nothing_and_score_says_so():
    from lvdgs import mesh_eval
    v, f, _, _, intr, size, _ = _two_squares()
    R, T = orc.look_at((0.5, 0.5, -2.0), (0.5, 0.5, -4.0))
    kept, record = mesh_eval.cull_mesh((_t(v), _t(f)), views=[_device_view(orc.view(R, T, intr, size=size))], want_origin=True)
    assert (record["vertices"], record["faces"]) == (0, 0) and kept.vertices.shape == (0, 3) and kept.faces.shape == (0, 3)
    assert record["vertex_origin"].numel() == 0
    with pytest.raises(_lib.LvdgsError, match="no faces"):
        mesh_eval.score(kept, (_t(v), _t(f)), n_samples=100)


# ---------------------------------------------------------------- the system ----
def _toy():
    import test_gpu_mesh_eval as base      # its run of the toy sequence, made once for both files
    return base._toy_run(), base._count_waits_and_reads


def _bounds(seq, voxel):
    xyz = seq.frontend_gaussians.get_xyz.detach()
    return ((xyz.min(0).values - 4 * voxel).tolist(), (xyz.max(0).values + 4 * voxel).tolist())


def test_eval_mesh_defaults_are_what_they_were():
    (seq, voxel), _ = _toy()
    score, record = seq.eval_mesh(voxel, n_samples=5000)
    again, record2 = seq.eval_mesh(voxel, n_samples=5000, gt_mesh=None, cull=None)
    assert again == score and record2 == record
    assert "cull" not in record["est"] and "faces_before" not in record["gt"]


def test_eval_mesh_with_a_ground_truth_mesh_and_cull():
    from lvdgs import mesh_eval
    from lvdgs.tsdf import Mesh, TsdfVolume
    (seq, voxel), count = _toy()
    bounds = _bounds(seq, voxel)
    truth = TsdfVolume.from_bounds(bounds[0], bounds[1], voxel, color=False, device=DEV)
    assert seq._fuse_dataset_depth(truth, sorted(seq.cameras), "gt", None) == len(seq.cameras) > len(seq.kf_indices)
    fused = truth.extract_mesh()      # every frame's depth: at least the surface the keyframes saw
    # and, as a scene mesh has, surface that no keyframe saw: a copy of it three scene extents beyond it along the first keyframe's axis
    forward = seq.cameras[seq.kf_indices[0]].R_gt.detach().to(DEV, torch.float32)[2]
    extent = max(b - a for a, b in zip(*bounds))
    gt_mesh = Mesh(torch.cat([fused.vertices, fused.vertices + 3.0 * extent * forward]).contiguous(), None,
                   torch.cat([fused.faces, fused.faces + fused.vertices.shape[0]]).contiguous())

    out = []
    c0 = count(lambda: out.append(seq.eval_mesh(voxel, bounds=bounds, n_samples=5000, gt_mesh=gt_mesh)))
    c = count(lambda: out.append(seq.eval_mesh(voxel, bounds=bounds, n_samples=5000, gt_mesh=gt_mesh, cull="visible")))
    (whole, whole_record), (score, record) = out
    assert whole_record["gt"]["faces"] == gt_mesh.faces.shape[0] and "cull" not in whole_record["gt"]
    print("whole", whole, "\nculled", score, record, "\nwaits", c0, c)
    # the documented waits: the estimate's mesh (HostCall.wait, a Stream.synchronize inside it) and the score's own synchronise; culling
    # adds one wait per culled mesh
    assert (c0["wait"], c0["sync"]) == (1, 2), c0
    assert (c["wait"], c["sync"]) == (3, 4), c
    eps = 4 * record["voxel_size"]
    for name, how in (("est", "frustum"), ("gt", "visible")):
        r = record[name]
        assert 0 < r["faces"] <= r["faces_before"] and 0 < r["vertices"] <= r["vertices_before"] and r["cull"] == how and r["cull_eps"] == eps
    assert record["gt"]["faces_before"] == gt_mesh.faces.shape[0] and record["est"]["faces_before"] == whole_record["est"]["faces"]
    assert record["gt"]["faces"] <= fused.faces.shape[0] < record["gt"]["faces_before"]      # the copy is behind what every keyframe's depth shows
    assert score["completion"] < whole["completion"] and score["recall"] > whole["recall"]      # which the whole mesh's completion had counted
    for name in ("accuracy", "completion", "completion_ratio", "precision", "recall", "fscore", "chamfer"):
        assert math.isfinite(score[name]), name

    # the culled ground truth is the mirror's, bit for bit
    views = seq._frame_views(seq.kf_indices, "gt", None, torch.device(DEV, torch.cuda.current_device()))
    assert len(views) == len(seq.kf_indices)
    mirror_views = [orc.view(v["R"].cpu().numpy(), v["T"].cpu().numpy(), v["intrinsics"], depth=v["depth"].cpu().numpy(), depth_trunc=v["depth_trunc"])
                    for v in views]
    gv, gf = gt_mesh.vertices.cpu().numpy(), gt_mesh.faces.cpu().numpy()
    want = orc.cull(gv, gf, orc.visibility(gv, mirror_views, eps))
    kept = seq.last_eval_meshes[1]
    assert np.array_equal(_bits(kept.vertices.cpu().numpy()), _bits(want["vertices"])) and np.array_equal(kept.faces.cpu().numpy(), want["faces"])
    assert record["gt"]["faces"] == len(want["faces"])

    # "frustum" keeps at least what "visible" keeps; a path is read like a mesh
    _, frustum = seq.eval_mesh(voxel, bounds=bounds, n_samples=2000, gt_mesh=gt_mesh, cull="frustum")
    assert frustum["gt"]["faces"] >= record["gt"]["faces"] and frustum["gt"]["cull"] == frustum["est"]["cull"] == "frustum"
    assert frustum["est"]["faces"] == record["est"]["faces"]


def test_eval_mesh_reads_a_ground_truth_file_and_refuses_what_it_cannot_do(tmp_path):
    from lvdgs.tsdf import TsdfVolume, save_mesh_ply
    (seq, voxel), _ = _toy()
    bounds = _bounds(seq, voxel)
    truth = TsdfVolume.from_bounds(bounds[0], bounds[1], voxel, color=False, device=DEV)
    seq._fuse_dataset_depth(truth, seq.kf_indices, "gt", None)
    gt_mesh = truth.extract_mesh()
    path = tmp_path / "gt.ply"
    save_mesh_ply(str(path), gt_mesh)
    from_mesh, _ = seq.eval_mesh(voxel, bounds=bounds, n_samples=3000, gt_mesh=gt_mesh, cull="frustum")
    from_file, record = seq.eval_mesh(voxel, bounds=bounds, n_samples=3000, gt_mesh=path, cull="frustum")
    assert from_file == from_mesh and record["gt"]["source"] == str(path)
    with pytest.raises(ValueError, match="cull"):
        seq.eval_mesh(voxel, cull="seen")
    # a dataset without metric depth: a ground-truth mesh still scores, frustum-culled; "visible" has no plane to test against
    saved, held = seq.dataset.depths, {i: cam.depth for i, cam in seq.cameras.items()}
    try:
        seq.dataset.depths = None
        for cam in seq.cameras.values():
            cam.depth = None
        score, _ = seq.eval_mesh(voxel, bounds=bounds, n_samples=3000, gt_mesh=gt_mesh, cull="frustum")
        assert score == from_mesh
        with pytest.raises(_lib.LvdgsError, match="needs the frames' dataset depth"):
            seq.eval_mesh(voxel, bounds=bounds, n_samples=3000, gt_mesh=gt_mesh, cull="visible")
    finally:
        seq.dataset.depths = saved
        for i, cam in seq.cameras.items():
            cam.depth = held[i]
