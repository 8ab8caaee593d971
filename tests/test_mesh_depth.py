"""Depth rendered from a mesh, without a GPU: the refusals of ``lvdgs_mesh_depth`` (it returns before any launch) and of its scratch
size, the float32 mirror of tests/mesh_depth_oracle.py against its float64 statement, watertightness and the inclusive edges of the
mirror.

The mirror and the statement decide alike except at a pixel within rounding of a decision; the header ("THE FLOAT32 RULE AGAINST EXACT
ARITHMETIC") derives how near that is: an edge value within 4u (|du| |j - v_lo| + |dv| |i - u_lo|) of 0, or two candidate depths (or one
and a depth limit) within (8u + (e0 + e1 + e2) / |A| * (z_max / z_min - 1)) zp of each other, u = 2^-24.  ``fragile`` takes twice those
bounds from the statement alone; exactly those pixels are set aside, and they may be at most 1 % of the pixels the statement covers.
"""
import ctypes as C
import math

import numpy as np
import pytest

import mesh_cull_oracle as mco
import mesh_depth_oracle as orc
import mesh_eval_oracle as meo
import refusal_recording
from lvdgs import _lib

F32 = np.float32
MOST_FRAGILE = 0.01


# ---------------------------------------------------------------- refusals ----
def _at(address):
    return C.c_void_p(address)


def _view(**kw):
    v = _lib.TsdfViewArgs(width=64, height=48, fx=50.0, fy=50.0, cx=32.0, cy=24.0, depth_min=0.0, depth_trunc=math.inf, R=_at(0x20000), T=_at(0x21000))
    for k, x in kw.items():
        setattr(v, k, x)
    return v


PLANE = 64 * 48 * 4


def _args(views=None, depth=None, faces=None, **kw):
    """10 vertices, 6 faces, two views of 64 x 48; every buffer at least 0x4000 bytes from the next: no overlap."""
    views = [_view(), _view(R=_at(0x22000), T=_at(0x23000))] if views is None else list(views)
    n = len(views)
    depth = [0x30000 + 0x4000 * k for k in range(n)] if depth is None else depth
    faces = [0x80000 + 0x4000 * k for k in range(n)] if faces is None else faces
    ptrs = (C.POINTER(_lib.TsdfViewArgs) * max(n, 1))(*[C.pointer(v) if v is not None else None for v in views])
    dlist = (C.c_void_p * max(len(depth), 1))(*depth)
    flist = (C.c_void_p * max(len(faces), 1))(*faces) if faces != "none" else None
    a = _lib.MeshDepthArgs(num_vertices=10, num_faces=6, vertices=_at(0x10000), faces=_at(0x11000), views=C.cast(ptrs, C.c_void_p), count=n,
                           depth=C.cast(dlist, C.c_void_p), face_index=None if flist is None else C.cast(flist, C.c_void_p),
                           scratch=_at(0x100000), scratch_bytes=1 << 30)
    for k, x in kw.items():
        setattr(a, k, x)
    return a, (ptrs, views, dlist, flist)


@pytest.mark.parametrize("build, status, words", [
    (dict(num_vertices=-1), "E_INVALID", b"negative count"), (dict(num_faces=-1), "E_INVALID", b"negative count"),
    (dict(num_vertices=2 ** 31), "E_INVALID", b"above 2^31 - 1"), (dict(num_faces=2 ** 31), "E_INVALID", b"above 2^31 - 1"),
    (dict(vertices=None), "E_INVALID", b"vertices is NULL"), (dict(faces_ptr=None), "E_INVALID", b"faces is NULL"),
    (dict(count=-1), "E_INVALID", b"count -1"), (dict(count=17), "E_INVALID", b"count 17"),
    (dict(views=None), "E_INVALID", b"view list is NULL"), (dict(depth=None), "E_INVALID", b"depth list is NULL"),
    (dict(view_list=[_view(), None]), "E_INVALID", b"view 1 is NULL"),
    (dict(view_list=[_view(R=None)]), "E_INVALID", b"view 0: R / T is NULL"),
    (dict(view_list=[_view(), _view(T=None)]), "E_INVALID", b"view 1: R / T is NULL"),
    (dict(depth_list=[0x30000, 0]), "E_INVALID", b"view 1: depth output is NULL"),
    (dict(face_list=[0, 0x84000]), "E_INVALID", b"view 0: face_index output is NULL"),
    (dict(view_list=[_view(width=0)]), "E_RANGE", b"image size 0x48"),
    (dict(view_list=[_view(height=-3)]), "E_RANGE", b"image size"),
    (dict(view_list=[_view(width=65536, height=32768)]), "E_RANGE", b"image size"),
    (dict(scratch=None), "E_INVALID", b"scratch is NULL"),
    (dict(scratch_bytes=2 * 64 * 48 * 8 - 1), "E_INVALID", b"scratch too small"),
    (dict(scratch=_at(0x100004)), "E_INVALID", b"8-byte aligned"),
    # aliasing, byte by byte: an output on an input, one byte into one, its last byte on one's first; on another output; in the scratch
    (dict(depth_list=[0x10000, 0x34000]), "E_INVALID", b"depth[0] overlaps vertices"),
    (dict(depth_list=[0x30000, 0x10000 + 119]), "E_INVALID", b"depth[1] overlaps vertices"),
    (dict(depth_list=[0x10000 - PLANE + 1, 0x34000]), "E_INVALID", b"depth[0] overlaps vertices"),
    (dict(face_list=[0x11000 + 71, 0x84000]), "E_INVALID", b"face_index[0] overlaps faces"),
    (dict(depth_list=[0x30000, 0x22000 + 35]), "E_INVALID", b"depth[1] overlaps R[1]"),
    (dict(face_list=[0x80000, 0x21000 + 11]), "E_INVALID", b"face_index[1] overlaps T[0]"),
    (dict(depth_list=[0x30000, 0x30000 + PLANE - 1]), "E_INVALID", b"depth[1] overlaps depth[0]"),
    (dict(face_list=[0x34000 + 4, 0x84000]), "E_INVALID", b"depth[1] overlaps face_index[0]"),
    (dict(face_list=[0x80000, 0x80000 - PLANE + 1]), "E_INVALID", b"face_index[1] overlaps face_index[0]"),
    (dict(depth_list=[0x100000 + 2 * 64 * 48 * 8 - 1, 0x34000]), "E_INVALID", b"depth[0] overlaps scratch"),
])
def test_mesh_depth_refusals(build, status, words, request):
    L = _lib.lib()
    build = dict(build)
    a, keep = _args(views=build.pop("view_list", None), depth=build.pop("depth_list", None), faces=build.pop("face_list", None))
    for k, x in build.items():
        setattr(a, "faces" if k == "faces_ptr" else k, x)
    assert L.lvdgs_mesh_depth(C.byref(a), None) == getattr(_lib, status)
    assert b"mesh depth" in L.lvdgs_last_error() and words in L.lvdgs_last_error(), L.lvdgs_last_error()
    refusal_recording.check(request.node.module.__name__ + "::" + request.node.name, getattr(_lib, status), L.lvdgs_last_error())


def test_mesh_depth_refuses_null_accepts_nothing_to_do_and_neighbours_are_no_overlap():
    L = _lib.lib()
    assert L.lvdgs_mesh_depth(None, None) == _lib.E_INVALID and b"args is NULL" in L.lvdgs_last_error()
    a, keep = _args(views=[], depth=[], faces="none")
    a.views, a.depth, a.scratch = None, None, None      # no view: no launch, nothing is needed
    assert L.lvdgs_mesh_depth(C.byref(a), None) == _lib.OK
    a, keep = _args(views=[_view(width=0)], num_vertices=0, num_faces=0, vertices=None)      # the views are checked all the same
    a.faces = None
    assert L.lvdgs_mesh_depth(C.byref(a), None) == _lib.E_RANGE
    # planes that touch end to start are fine: the outputs are checked in the order depth[0], face_index[0], depth[1], face_index[1], and
    # with the first three laid end to start the refusal names the last one, which lies a byte into the plane in front of it
    a, keep = _args(depth=[0x30000, 0x30000 + 2 * PLANE], faces=[0x30000 + PLANE, 0x30000 + 3 * PLANE - 1])
    assert L.lvdgs_mesh_depth(C.byref(a), None) == _lib.E_INVALID and b"face_index[1] overlaps depth[1]" in L.lvdgs_last_error()


def test_scratch_size_is_eight_bytes_a_pixel_and_zero_where_refused():
    L = _lib.lib()
    prev = 0
    for n in (0, 1, 32, 33, 64 * 48, 640 * 480 * 16, 2 ** 31 - 1, 16 * (2 ** 31 - 1)):
        b = L.lvdgs_mesh_depth_scratch_bytes(n)
        assert b % 256 == 0 and b >= 8 * n and b >= prev and b > 0 and b < 8 * n + 512
        prev = b
    assert [L.lvdgs_mesh_depth_scratch_bytes(n) for n in (-1, 16 * (2 ** 31 - 1) + 1, 2 ** 62)] == [0, 0, 0]


# ---------------------------------------------------------------- the mirror against the float64 statement ----
def _camera(size, eye=(1.07, 0.94, -2.5), target=(1.0, 1.0, 0.0), **kw):
    """A camera in front of the wall over [0, 2]^2 that sees it whole, a little off its axis."""
    H, W = size
    focal = 0.41 * min(H / 1.0, W / 1.0) * 2.5 / 1.0 * 0.95
    R, T = mco.look_at(eye, target)
    return mco.view(R, T, (focal, focal * 1.03, W / 2 - 0.37, H / 2 - 0.41), size=size, **kw)


def _scene(name):
    if name == "wall":
        v, f, _ = meo.wavy_wall(33, 33, seed=4)
        return v, f
    if name == "soup":
        return orc.soup(500, seed=7)
    raise KeyError(name)


CASES = [(scene, size) for scene in ("wall", "soup") for size in ((48, 64), (9, 17))]
_rendered = {}


def _render(scene, size):
    """Mirror, statement and fragile pixels of a case, made once."""
    if (scene, size) not in _rendered:
        v, f = _scene(scene)
        view = _camera(size)
        _rendered[scene, size] = (v, f, view, orc.render(v, f, view), orc.render(v, f, view, np.float64), orc.fragile(v, f, view))
    return _rendered[scene, size]


@pytest.mark.parametrize("scene, size", CASES)
def test_mirror_against_the_float64_statement(scene, size):
    """Observed shares of fragile pixels among the covered ones: wall 64 x 48: 0 of 1434, wall 17 x 9: 0 of 49, soup 64 x 48: 0 of 2883,
    soup 17 x 9: 0 of 114 -- all 0.0000 (the camera is a little off the wall's axis, so no edge runs through a pixel centre; that ``fragile``
    finds the pixels on edges is checked in test_edges_and_vertices_on_pixel_centres_are_inclusive)."""
    v, f, view, (depth, face), (depth64, face64), fragile = _render(scene, size)
    covered = depth64 > 0
    share = float((fragile & covered).sum()) / max(int(covered.sum()), 1)
    sure = ~fragile
    differing = int(((depth > 0) != covered).sum())
    print(scene, size, "covered", int(covered.sum()), "of", covered.size, "fragile", int((fragile & covered).sum()), "share %.5f" % share,
          "coverage differing anywhere", differing, "faces differing", int((face != face64).sum()))
    assert 0.2 * covered.size < covered.sum() and (scene == "wall" or covered.sum() < covered.size)      # the case decides both ways
    assert share <= MOST_FRAGILE
    assert np.array_equal((depth > 0)[sure], covered[sure])
    assert np.array_equal((face >= 0), depth > 0) and np.array_equal(face64 >= 0, covered)
    both = sure & covered & (depth > 0)
    bound = orc.depth_bounds(v, f, view, face64)
    assert both.any() and (bound[both] > 0).all()
    assert (np.abs(depth.astype(np.float64) - depth64)[both] <= bound[both]).all()
    assert np.array_equal(face[both], face64[both])      # away from ties and crossings the same face wins


def test_depth_is_the_surface_and_limits_cut_it():
    """The wall's depth lies between its nearest and farthest vertex; depth_min and depth_trunc remove what lies outside them."""
    v, f, view, (depth, face), _, _ = _render("wall", (48, 64))
    z, _, _ = orc.project(v, view)
    hit = depth > 0
    assert z.min() <= depth[hit].min() and depth[hit].max() <= z.max()
    mid = float(np.median(depth[hit]))
    near, _ = orc.render(v, f, dict(view, depth_trunc=mid))
    assert 0 < (near > 0).sum() < hit.sum() and near[near > 0].max() <= F32(mid)
    assert np.array_equal(near[near > 0], depth[near > 0])
    far, _ = orc.render(v, f, dict(view, depth_min=mid))      # faces with a vertex at or in front of depth_min are dropped whole
    assert 0 < (far > 0).sum() < hit.sum() and far[far > 0].min() > F32(mid)
    behind, _ = orc.render(v, f, dict(view, depth_min=float(z.max())))
    assert not (behind > 0).any()
    assert np.array_equal(orc.render(v, f, dict(view, depth_min=-3.0))[0], depth)      # dm = fmaxf(depth_min, 0)


# ---------------------------------------------------------------- watertightness ----
def _axis_view(size, fx, fy, cx, cy, **kw):
    """A camera at the origin looking along +z: z = pz, u = fx * (px / pz) + cx -- exact for the values used here."""
    return mco.view(np.eye(3, dtype=F32), np.zeros(3, F32), (fx, fy, cx, cy), size=size, **kw)


def fan_scene():
    """A closed fan of 7 faces around a vertex that projects exactly onto the centre of pixel (8, 8) of a 16 x 16 view."""
    v, f = orc.fan((0.5, 0.5), 0.6, n=7, z=1.0)
    return v, f, _axis_view((16, 16), 8.0, 8.0, 4.0, 4.0)


@pytest.mark.parametrize("scene", ["wall 64x48", "wall 17x9", "fan"])
def test_the_mirror_is_watertight(scene):
    if scene == "fan":
        v, f, view = fan_scene()
        _, u, w = orc.project(v, view)
        assert (u[0], w[0]) == (8.0, 8.0)
        depth, depth64 = orc.render(v, f, view)[0], orc.render(v, f, view, np.float64)[0]
        assert depth[8, 8] == 1.0
    else:
        _, _, _, (depth, _), (depth64, _), _ = _render("wall", (48, 64) if scene == "wall 64x48" else (9, 17))
    inside = orc.erode(depth64 > 0)
    assert inside.sum() >= (16 if scene != "wall 17x9" else 6)
    assert (depth[inside] > 0).all(), np.argwhere(inside & ~(depth > 0))[:10]


# ---------------------------------------------------------------- inclusive edges ----
def _up(x):
    return np.nextafter(F32(x), F32(np.inf))


def test_edges_and_vertices_on_pixel_centres_are_inclusive():
    """fx = 1, cx = 0, z = 1: u = px.  A vertex and two edges exactly on pixel centres cover those pixels, under either winding; moved
    one ulp outside they do not."""
    view = _axis_view((8, 8), 1.0, 1.0, 0.0, 0.0)
    tri = np.array([[2, 2, 1], [6, 2, 1], [2, 6, 1]], F32)
    for faces in ([[0, 1, 2]], [[0, 2, 1]]):
        depth, face = orc.render(tri, np.array(faces, np.int32), view)
        assert depth[2, 2] == 1 and depth[2, 6] == 1 and depth[6, 2] == 1                   # the vertices
        assert (depth[2, 2:7] == 1).all() and (depth[2:7, 2] == 1).all()                    # the edges along a row and a column
        assert depth[4, 4] == 1 and depth[3, 5] == 1 and depth[5, 3] == 1                   # the diagonal one
        assert depth[4, 5] == 0 and depth[1, 3] == 0 and depth[3, 1] == 0 and (depth > 0).sum() == 15
        assert np.array_equal(depth, orc.render(tri, np.array(faces, np.int32), view, np.float64)[0])
        fragile = orc.fragile(tri, np.array(faces, np.int32), view)      # the pixels on the edges are the ones rounding could move
        assert fragile[2, 2:7].all() and fragile[2:7, 2].all() and fragile[4, 4] and not fragile[3, 3] and not fragile[4, 5]
    moved = tri.copy()
    moved[0, :2] = _up(2)                                                                   # the vertex, one ulp inwards
    depth, _ = orc.render(moved, np.array([[0, 1, 2]], np.int32), view)
    assert depth[2, 2] == 0 and depth[2, 6] == 1 and depth[6, 2] == 1 and depth[3, 3] > 0      # the other two vertices stay on theirs
    moved = tri.copy()
    moved[:2, 1] = _up(2)                                                                   # the edge along row 2, one ulp down
    depth, _ = orc.render(moved, np.array([[0, 1, 2]], np.int32), view)
    assert (depth[2, :] == 0).all() and (depth[3, 2:6] > 0).all()


def test_ties_go_to_the_lower_face_index_and_dropped_faces_leave_the_rest():
    view = _axis_view((8, 8), 1.0, 1.0, 0.0, 0.0)
    tri = np.array([[2, 2, 1], [6, 2, 1], [2, 6, 1], [np.nan, 0, 1], [0, 0, -1], [3, 3, 0.5]], F32)
    alone = orc.render(tri, np.array([[0, 1, 2]], np.int32), view)
    faces = np.array([[0, 1, 9], [3, 1, 2], [0, 1, 2], [0, 2, 1], [-1, 1, 2], [0, 1, 1], [0, 4, 2], [4, 5, 2]], np.int32)
    depth, face = orc.render(tri, faces, dict(view, depth_min=0.75))      # face 7 crosses depth_min: dropped whole
    assert np.array_equal(depth, alone[0]) and set(np.unique(face)) == {-1, 2}
