"""Mesh culling without a GPU: the refusals of ``lvdgs_mesh_visibility`` / ``lvdgs_mesh_cull`` (they return before any launch), the scratch
size, the float32 mirror of tests/mesh_cull_oracle.py against its float64 statement, and the compaction against a plain loop.

The mirror and the statement decide alike except for a vertex that, in some view, lies within rounding of a decision boundary; the
header ("THE FLOAT32 RULE AGAINST EXACT ARITHMETIC") derives how near that is: 4u M around depth_min and depth_trunc, 5u (M + |d|) around
d - z = -eps, fx (4u Mx + |x/z| 4u Mz) / |z| + 4u (|u| + |cx| + 1) around a pixel edge, u = 2^-24.  ``near_a_boundary`` takes twice those
margins from the statement alone; exactly those vertices are excluded, and they may be at most 1 % of a case's vertices.
"""
import ctypes as C
import math

import numpy as np
import pytest

import mesh_cull_oracle as orc
import mesh_eval_oracle as meo
import refusal_recording
from lvdgs import _lib

P256, P4096 = C.c_void_p(256), C.c_void_p(4096)      # never dereferenced: every call that gets them is refused before a launch
MOST_EXCLUDED = 0.01


# ---------------------------------------------------------------- refusals ----
def _view(**kw):
    v = _lib.TsdfViewArgs(width=64, height=48, fx=50.0, fy=50.0, cx=32.0, cy=24.0, depth_min=0.0, depth_trunc=math.inf, R=P256, T=P256, depth=P256)
    for k, x in kw.items():
        setattr(v, k, x)
    return v


def _visibility_args(blocks=(), **kw):
    views = list(blocks)
    ptrs = (C.POINTER(_lib.TsdfViewArgs) * max(len(views), 1))(*[C.pointer(v) if v is not None else None for v in views])
    a = _lib.MeshVisibilityArgs(num_vertices=10, vertices=P256, views=C.cast(ptrs, C.c_void_p), count=len(views), occlusion_eps=0.01, seen=P256)
    for k, x in kw.items():
        setattr(a, k, x)
    return a, (ptrs, views)


@pytest.mark.parametrize("views, change, status, words", [
    ([_view()], dict(num_vertices=-1), "E_INVALID", b"negative count"),
    ([_view()], dict(num_vertices=2 ** 31), "E_INVALID", b"above 2^31 - 1"),
    ([_view()], dict(count=-1), "E_INVALID", b"count -1"),
    ([_view()], dict(count=17), "E_INVALID", b"count 17"),
    ([_view()], dict(occlusion_eps=-0.5), "E_RANGE", b"occlusion_eps"),
    ([_view()], dict(occlusion_eps=math.nan), "E_RANGE", b"occlusion_eps"),
    ([_view()], dict(occlusion_eps=math.inf), "E_RANGE", b"occlusion_eps"),
    ([_view()], dict(vertices=None), "E_INVALID", b"NULL"),
    ([_view()], dict(seen=None), "E_INVALID", b"NULL"),
    ([_view()], dict(views=None), "E_INVALID", b"view list is NULL"),
    ([_view(), None], {}, "E_INVALID", b"view 1 is NULL"),
    ([_view(R=None)], {}, "E_INVALID", b"view 0: R / T is NULL"),
    ([_view(), _view(T=None)], {}, "E_INVALID", b"view 1: R / T is NULL"),
    ([_view(width=0)], {}, "E_RANGE", b"image size 0x48"),
    ([_view(height=-3)], {}, "E_RANGE", b"image size"),
    ([_view(width=65536, height=32768)], {}, "E_RANGE", b"image size"),
])
def test_mesh_visibility_refusals(views, change, status, words, request):
    L = _lib.lib()
    a, keep = _visibility_args(views, **change)
    assert L.lvdgs_mesh_visibility(C.byref(a), None) == getattr(_lib, status)
    assert b"mesh visibility" in L.lvdgs_last_error() and words in L.lvdgs_last_error(), L.lvdgs_last_error()
    refusal_recording.check(request.node.module.__name__ + "::" + request.node.name, getattr(_lib, status), L.lvdgs_last_error())


def test_mesh_visibility_refuses_null_and_accepts_nothing_to_do():
    L = _lib.lib()
    assert L.lvdgs_mesh_visibility(None, None) == _lib.E_INVALID and b"args is NULL" in L.lvdgs_last_error()
    a, keep = _visibility_args([_view(depth=None)], num_vertices=0, vertices=None, seen=None)      # no vertex: no launch; a view without depth is one
    assert L.lvdgs_mesh_visibility(C.byref(a), None) == _lib.OK
    a, keep = _visibility_args([], views=None)                                                      # no view: no launch
    assert L.lvdgs_mesh_visibility(C.byref(a), None) == _lib.OK
    a, keep = _visibility_args([_view(width=0)], num_vertices=0)                                    # the views are checked all the same
    assert L.lvdgs_mesh_visibility(C.byref(a), None) == _lib.E_RANGE


def _at(address):
    return C.c_void_p(address)


def _cull_args(**kw):
    """10 vertices, 6 faces; every buffer 4096 bytes from the next: no overlap."""
    a = _lib.MeshCullArgs(num_vertices=10, num_faces=6, vertices=_at(0x10000), vertex_colors=_at(0x11000), faces=_at(0x12000), seen=_at(0x13000),
                          face_rule=_lib.MESH_CULL_ALL, out_vertices=_at(0x14000), out_colors=_at(0x15000), out_faces=_at(0x16000),
                          vertex_origin=_at(0x17000), face_origin=_at(0x18000), host_state=_at(0x19000), scratch=_at(0x100000), scratch_bytes=1 << 30)
    for k, x in kw.items():
        setattr(a, k, x)
    return a


@pytest.mark.parametrize("change, words", [
    (dict(num_vertices=-1), b"negative count"), (dict(num_faces=-1), b"negative count"),
    (dict(num_vertices=2 ** 31), b"above 2^31 - 1"), (dict(num_faces=2 ** 31), b"above 2^31 - 1"),
    (dict(face_rule=2), b"face_rule 2"), (dict(face_rule=-1), b"face_rule -1"),
    (dict(vertices=None), b"NULL"), (dict(seen=None), b"NULL"), (dict(out_vertices=None), b"NULL"),
    (dict(faces=None), b"NULL"), (dict(out_faces=None), b"NULL"), (dict(host_state=None), b"NULL"), (dict(scratch=None), b"NULL"),
    (dict(vertex_colors=None), b"without vertex_colors"),
    (dict(scratch_bytes=1000), b"scratch too small"), (dict(scratch=_at(0x100002)), b"aligned"),
    # aliasing: an output on an input, inside one, one byte into one; an output on another output; an output in the scratch
    (dict(out_vertices=_at(0x10000)), b"out_vertices overlaps vertices"),
    (dict(out_faces=_at(0x12000 + 24)), b"out_faces overlaps faces"),
    (dict(out_vertices=_at(0x10000 + 119)), b"out_vertices overlaps vertices"),
    (dict(out_colors=_at(0x11000 - 119)), b"out_colors overlaps vertex_colors"),
    (dict(vertex_origin=_at(0x13000 + 9)), b"vertex_origin overlaps seen"),
    (dict(face_origin=_at(0x16000 + 71)), b"face_origin overlaps out_faces"),
    (dict(out_colors=_at(0x14000 + 60)), b"out_colors overlaps out_vertices"),
    (dict(out_faces=_at(0x100000 + 512)), b"out_faces overlaps scratch"),
])
def test_mesh_cull_refusals(change, words, request):
    L = _lib.lib()
    assert L.lvdgs_mesh_cull(C.byref(_cull_args(**change)), None) == _lib.E_INVALID
    assert b"mesh cull" in L.lvdgs_last_error() and words in L.lvdgs_last_error(), L.lvdgs_last_error()
    refusal_recording.check(request.node.module.__name__ + "::" + request.node.name, _lib.E_INVALID, L.lvdgs_last_error())


def test_mesh_cull_refuses_null_and_neighbours_are_no_overlap():
    L = _lib.lib()
    assert L.lvdgs_mesh_cull(None, None) == _lib.E_INVALID and b"args is NULL" in L.lvdgs_last_error()
    # buffers that touch end to start are fine: the call gets as far as its host block, which an address that is no pinned memory fails
    a = _cull_args(out_vertices=_at(0x10000 + 120), vertex_colors=None, out_colors=None)
    assert L.lvdgs_mesh_cull(C.byref(a), None) != _lib.OK and b"overlaps" not in L.lvdgs_last_error() and b"host_state" in L.lvdgs_last_error()


def test_scratch_size_is_aligned_monotone_and_zero_where_refused():
    L = _lib.lib()
    prev = 0
    for n in (0, 1, 257, 70_000, 10 ** 6, 2 ** 31 - 1):
        b = L.lvdgs_mesh_cull_scratch_bytes(n, n)
        assert b % 256 == 0 and b >= prev and (b > prev or n == 1) and b >= 5 * n + n      # the used plane and the new numbers per vertex, a byte per face
        if n < 2 ** 31 - 1:
            assert L.lvdgs_mesh_cull_scratch_bytes(n + 1, n) >= b and L.lvdgs_mesh_cull_scratch_bytes(n, n + 1) >= b
        prev = b
    assert [L.lvdgs_mesh_cull_scratch_bytes(v, f) for v, f in ((-1, 5), (5, -1), (2 ** 31, 5), (5, 2 ** 31))] == [0, 0, 0, 0]


# ---------------------------------------------------------------- the mirror against the float64 statement ----
def _two_walls(nu, nv, seed):
    """A wavy wall around z = 0 and a second one 0.6 behind it, over [0, 2]^2."""
    v0, _, _ = meo.wavy_wall(nu, nv, seed=seed)
    v1, _, _ = meo.wavy_wall(nu + 3, nv - 2, seed=seed + 1, offset=0.6)
    return np.concatenate([v0, v1])


def _noisy_depth(rng, size, lo, hi):
    """Depths on both sides of the walls, with pixels of 0, NaN and +inf among them."""
    d = rng.uniform(lo, hi, size).astype(np.float32)
    flat = d.reshape(-1)
    n = flat.size
    flat[rng.integers(0, n, n // 20)] = 0.0
    flat[rng.integers(0, n, n // 50)] = np.nan
    flat[rng.integers(0, n, n // 50)] = np.inf
    return d


def _scene(name):
    rng = np.random.default_rng(len(name))
    if name == "one view":
        vertices = _two_walls(60, 50, 3)
        R, T = orc.look_at((1.1, 0.9, -2.5), (1.0, 1.0, 0.0))
        views = [orc.view(R, T, (100.0, 100.0, 47.5, 35.5), depth=_noisy_depth(rng, (72, 96), 2.0, 3.6))]
        return vertices, views, 0.05
    if name == "four views":
        vertices = _two_walls(70, 45, 5)
        poses = [orc.look_at(eye, at) for eye, at in (((1.0, 1.0, -2.5), (1.0, 1.0, 0.0)), ((-0.5, 0.8, -2.0), (1.2, 1.0, 0.0)),
                                                      ((2.4, 1.7, -1.8), (0.7, 0.8, 0.3)), ((1.0, 0.2, -3.0), (1.0, 1.4, 0.0)))]
        views = [orc.view(*poses[0], (100.0, 100.0, 47.3, 35.6), depth=_noisy_depth(rng, (72, 96), 2.0, 3.6), depth_trunc=3.4),
                 orc.view(*poses[1], (90.0, 95.0, 60.2, 50.7), depth=_noisy_depth(rng, (100, 128), 1.5, 3.5), depth_min=1.9,
                          mask=rng.random((100, 128)) > 0.1),
                 orc.view(*poses[2], (70.0, 70.0, 31.5, 23.5), size=(48, 64), depth_trunc=2.6),      # frustum only, cut between the walls
                 orc.view(*poses[3], (60.0, 64.0, 40.0, 29.0), depth=_noisy_depth(rng, (60, 80), 2.5, 4.0))]
        return vertices, views, 0.02
    raise KeyError(name)


@pytest.mark.parametrize("name", ["one view", "four views"])
def test_visibility_mirror_against_the_float64_statement(name):
    vertices, views, eps = _scene(name)
    assert len(views) <= 4 and all(max(orc.size_of(v)) <= 128 for v in views)
    near = orc.near_a_boundary(vertices, views, eps)
    share = float(near.mean())
    mirror, statement = orc.visibility(vertices, views, eps), orc.visibility(vertices, views, eps, dtype=np.float64)
    per_view = [int(orc.sees(vertices, v, eps).sum()) for v in views]
    print(name, len(vertices), "vertices;", int(near.sum()), "within the margins (share %.5f);" % share, "seen", int(mirror.sum()), "per view", per_view,
          "; differing anywhere", int((mirror != statement).sum()))
    assert share <= MOST_EXCLUDED
    assert np.array_equal(mirror[~near], statement[~near])
    assert 0.05 * len(vertices) < mirror.sum() < 0.95 * len(vertices) and all(per_view)      # the case decides something either way


def test_the_margins_catch_vertices_placed_on_the_boundaries():
    """Vertices put (in float64) exactly on z = depth_min, on a pixel edge, on z = depth_trunc and on d - z = -eps are all within the
    margins; their neighbours a thousand margins away are not."""
    R, T = orc.look_at((0.3, -0.2, -1.0), (0.1, 0.1, 1.0))
    fx, fy, cx, cy = 80.0, 75.0, 31.5, 23.5
    frustum = orc.view(R, T, (fx, fy, cx, cy), size=(48, 64), depth_min=0.5, depth_trunc=3.0)
    with_depth = orc.view(R, T, (fx, fy, cx, cy), depth=np.full((48, 64), 2.0, np.float32), depth_min=0.5)
    eps = 0.25
    Rd, Td = R.astype(np.float64), T.astype(np.float64)

    def world(u, v, z):      # the point that projects to (u, v) at camera depth z
        cam = np.array([(u - cx) / fx * z, (v - cy) / fy * z, z])
        return Rd.T @ (cam - Td)

    on = np.array([world(20.2, 11.7, 0.5), world(20.5, 11.7, 1.3), world(20.2, 30.5, 1.3), world(20.2, 11.7, 3.0)], np.float32)
    off = np.array([world(20.2, 11.7, 0.5 + 1e-3), world(20.5 + 1e-2, 11.7, 1.3), world(20.2, 30.5 - 1e-2, 1.3), world(20.2, 11.7, 3.0 - 1e-3)], np.float32)
    assert orc.near_a_boundary(on, [frustum], eps).all() and not orc.near_a_boundary(off, [frustum], eps).any()
    on_d, off_d = np.array([world(20.2, 11.7, 2.25)], np.float32), np.array([world(20.2, 11.7, 2.25 - 1e-3)], np.float32)
    assert orc.near_a_boundary(on_d, [with_depth], eps).all() and not orc.near_a_boundary(off_d, [with_depth], eps).any()


def test_seen_bytes_survive_and_non_finite_vertices_are_never_seen():
    R, T = orc.look_at((0.0, 0.0, -2.0), (0.0, 0.0, 0.0))
    v = orc.view(R, T, (40.0, 40.0, 15.5, 11.5), size=(24, 32))
    vertices = np.array([[0, 0, 0], [50, 0, 0], [np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [50, 0, 0]], np.float32)
    for dtype in (np.float32, np.float64):
        assert orc.visibility(vertices, [v], 0.0, dtype=dtype).tolist() == [1, 0, 0, 0, 0, 0]
        assert orc.visibility(vertices, [v], 0.0, seen=[7, 0, 0, 3, 0, 9], dtype=dtype).tolist() == [7, 0, 0, 3, 0, 9]
        assert orc.visibility(vertices, [], 0.0, dtype=dtype).tolist() == [0] * 6


# ---------------------------------------------------------------- the compaction against a plain loop ----
def _cull_loop(vertices, faces, seen, rule, colors=None):
    V = len(vertices)
    kept_faces = []
    for f, face in enumerate(faces):
        if any(i < 0 or i >= V for i in face):
            continue
        marks = [seen[i] != 0 for i in face]
        if any(marks) if rule == orc.ANY else all(marks):
            kept_faces.append(f)
    used = sorted({int(i) for f in kept_faces for i in faces[f]})
    new = {old: k for k, old in enumerate(used)}
    return dict(vertices=[vertices[i].tolist() for i in used], colors=None if colors is None else [colors[i].tolist() for i in used],
                faces=[[new[int(i)] for i in faces[f]] for f in kept_faces], vertex_origin=used, face_origin=kept_faces)


@pytest.mark.parametrize("rule", [orc.ALL, orc.ANY])
@pytest.mark.parametrize("case", ["wall", "spoiled", "nothing", "everything", "no faces", "no vertices"])
def test_compaction_against_a_plain_loop(case, rule):
    rng = np.random.default_rng(11)
    v, f, c = meo.wavy_wall(9, 7, seed=2)
    seen = (rng.random(len(v)) < 0.6).astype(np.uint8) * 5
    if case == "spoiled":      # indices of -1 and V, a vertex no face references (appended), a repeated index
        f = f.copy()
        f[4], f[9], f[13] = (-1, f[4][1], f[4][2]), (f[9][0], len(v) + 1, f[9][2]), (f[13][0], f[13][0], f[13][1])
        v, c, seen = np.concatenate([v, v[:1] + 1]), np.concatenate([c, c[:1]]), np.concatenate([seen, [1]]).astype(np.uint8)
        f[9][1] = len(v)
    elif case == "nothing":
        seen[:] = 0
    elif case == "everything":
        seen[:] = 1
    elif case == "no faces":
        f = f[:0]
    elif case == "no vertices":
        v, c, seen = v[:0], c[:0], seen[:0]
    got, want = orc.cull(v, f, seen, rule, colors=c), _cull_loop(v, f, seen, rule, colors=c)
    for key in want:
        assert got[key].tolist() == want[key], key
    assert got["faces"].dtype == np.int32 and got["vertex_origin"].dtype == np.int32 and got["face_origin"].dtype == np.int32
    if case == "everything":
        assert len(got["faces"]) == len(f) and np.array_equal(got["vertices"], v)
    if case in ("nothing", "no faces", "no vertices"):
        assert len(got["faces"]) == 0 and len(got["vertices"]) == 0
    if case == "wall":      # the two rules differ, and ANY keeps vertices that were not seen
        kept = seen[got["vertex_origin"]] != 0
        assert kept.all() if rule == orc.ALL else (not kept.all() and kept.any())
