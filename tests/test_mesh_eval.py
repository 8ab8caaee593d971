"""Mesh scoring without a GPU: the refusals and scratch sizes of ``lvdgs_mesh_sample`` / ``lvdgs_cloud_distance``, the row against its
dtype, the float32 mirrors of tests/mesh_eval_oracle.py against the float64 statements, the score's arithmetic and the PLY round trip.

Bounds, with u = 2^-24 the unit roundoff of float32 and every operand a float32:
  * a sampled coordinate p = (a + r1 * (b - a)) + r2 * (c - a), |a|, |b|, |c| <= m, r1 + r2 <= 1 exact multiples of 2^-24:  b - a and
    c - a are off by 2mu each at most, the products r1 * (b - a) and r2 * (c - a) carry that times r and add a rounding of at most
    2mu * r each -- 4mu * (r1 + r2) <= 4mu together; a + r1 * (b - a) lies on the edge and the final sum in the triangle, so both
    are at most m and round by mu each:  |p32 - p64| <= 6mu to first order; (1 + 2^-20) covers the second.
  * d2 = (dx*dx + dy*dy) + dz*dz:  dx is off by u relative, dx*dx by 3u, the first sum by 4u, the second by 5u -- all terms are
    non-negative, so relative errors do not grow in the sums:  |d2_32 - d2_64| <= 5u * d2_64 to first order, and the minimum of values
    each within 5u of its float64 twin is within 5u of the float64 minimum.
  * a float64 sum of M non-negative terms in ANY order is within (M - 1) * 2^-53 relative of the exact sum (``math.fsum``).
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import mesh_eval_oracle as orc
import refusal_recording
from lvdgs import _abi, _lib

U = 2.0 ** -24
SLACK = 1.0 + 2.0 ** -20
P256 = C.c_void_p(256)      # never dereferenced: every call that gets it is refused before a launch


def _kind(t):
    if issubclass(t, C.Array):
        return _kind(t._type_)
    return {**dict.fromkeys("bhilq", "i"), **dict.fromkeys("BHILQ", "u"), "f": "f", "d": "f"}[t._type_]


@pytest.mark.parametrize("struct, dtype, nbytes", [(_abi.CloudDistanceRow, _abi.CLOUD_DISTANCE_ROW_DTYPE, _abi.CLOUD_DISTANCE_ROW_BYTES),
                                                   (_abi.MeshSampleInfo, _abi.MESH_SAMPLE_INFO_DTYPE, _abi.MESH_SAMPLE_INFO_BYTES)])
def test_the_rows_are_their_dtypes(struct, dtype, nbytes):
    assert C.sizeof(struct) == nbytes == dtype.itemsize
    assert dtype.names == tuple(f for f, _ in struct._fields_)
    for f, t in struct._fields_:
        dt, offset = dtype.fields[f][:2]
        assert (offset, dt.itemsize, dt.base.kind) == (getattr(struct, f).offset, C.sizeof(t), _kind(t)), f


# ---------------------------------------------------------------- refusals ----
def _sample_args(**kw):
    a = _lib.MeshSampleArgs(num_vertices=4, num_faces=2, num_samples=10, vertices=P256, faces=P256, points=P256, info=P256, scratch=P256,
                            scratch_bytes=1 << 30)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _distance_args(**kw):
    a = _lib.CloudDistanceArgs(num_queries=10, num_reference=10, queries=P256, reference=P256, out_row=P256, scratch=P256, scratch_bytes=1 << 30)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("change, words", [
    (dict(vertices=None), b"NULL"), (dict(faces=None), b"NULL"), (dict(points=None), b"NULL"), (dict(info=None), b"NULL"),
    (dict(scratch=None), b"NULL"), (dict(colors=P256), b"vertex_colors"),
    (dict(num_vertices=-1), b"negative count"), (dict(num_faces=-1), b"negative count"), (dict(num_samples=-1), b"negative count"),
    (dict(num_vertices=2 ** 31), b"above 2^31 - 1"), (dict(num_faces=2 ** 31), b"above 2^31 - 1"), (dict(num_samples=2 ** 31), b"above 2^31 - 1"),
    (dict(num_faces=0), b"no faces"), (dict(scratch_bytes=1000), b"scratch too small"), (dict(scratch=C.c_void_p(260)), b"aligned"),
    (dict(info=C.c_void_p(260)), b"aligned"),
])
def test_mesh_sample_refusals(change, words, request):
    L = _lib.lib()
    assert L.lvdgs_mesh_sample(C.byref(_sample_args(**change)), None) == _lib.E_INVALID
    assert b"mesh sample" in L.lvdgs_last_error() and words in L.lvdgs_last_error(), L.lvdgs_last_error()
    refusal_recording.check(request.node.module.__name__ + "::" + request.node.name, _lib.E_INVALID, L.lvdgs_last_error())


def test_mesh_sample_refuses_null_and_accepts_nothing_to_do():
    L = _lib.lib()
    assert L.lvdgs_mesh_sample(None, None) == _lib.E_INVALID and b"args is NULL" in L.lvdgs_last_error()
    assert L.lvdgs_mesh_sample(C.byref(_sample_args(num_samples=0)), None) == _lib.OK      # nothing to do: no launch


@pytest.mark.parametrize("change, words", [
    (dict(queries=None), b"NULL"), (dict(reference=None), b"NULL"), (dict(out_row=None), b"NULL"), (dict(scratch=None), b"NULL"),
    (dict(num_queries=-1), b"negative count"), (dict(num_reference=-1), b"negative count"),
    (dict(num_queries=2 ** 31), b"above 2^31 - 1"), (dict(num_reference=2 ** 31), b"above 2^31 - 1"),
    (dict(num_thresholds=5), b"5 thresholds, at most 4"), (dict(num_thresholds=-1), b"thresholds, at most 4"),
    (dict(scratch_bytes=1000), b"scratch too small"), (dict(scratch=C.c_void_p(264)), b"aligned"), (dict(out_row=C.c_void_p(260)), b"aligned"),
])
def test_cloud_distance_refusals(change, words, request):
    L = _lib.lib()
    assert L.lvdgs_cloud_distance(C.byref(_distance_args(**change)), None) == _lib.E_INVALID
    assert b"cloud distance" in L.lvdgs_last_error() and words in L.lvdgs_last_error(), L.lvdgs_last_error()
    refusal_recording.check(request.node.module.__name__ + "::" + request.node.name, _lib.E_INVALID, L.lvdgs_last_error())


@pytest.mark.parametrize("bad", [-0.5, math.nan, math.inf, -math.inf])
def test_cloud_distance_refuses_a_bad_threshold(bad):
    L = _lib.lib()
    a = _distance_args(num_thresholds=2, thresholds=(C.c_float * 4)(0.0, bad, 0.0, 0.0))
    assert L.lvdgs_cloud_distance(C.byref(a), None) == _lib.E_INVALID and b"threshold 1" in L.lvdgs_last_error()
    a = _distance_args(num_thresholds=1, thresholds=(C.c_float * 4)(0.0, bad, 0.0, 0.0))      # beyond num_thresholds: not looked at
    a.num_queries = 0
    assert L.lvdgs_cloud_distance(C.byref(a), None) == _lib.OK


def test_cloud_distance_refuses_null_and_accepts_nothing_to_do():
    L = _lib.lib()
    assert L.lvdgs_cloud_distance(None, None) == _lib.E_INVALID and b"args is NULL" in L.lvdgs_last_error()
    assert L.lvdgs_cloud_distance(C.byref(_distance_args(num_queries=0)), None) == _lib.OK                      # nothing to do: no launch
    assert L.lvdgs_cloud_distance(C.byref(_distance_args(num_queries=0, num_reference=0, reference=None)), None) == _lib.OK


def test_scratch_sizes_are_aligned_monotone_and_zero_where_refused():
    L = _lib.lib()
    prev = 0
    for f in (1, 2, 257, 70_000, 10 ** 6, 2 ** 31 - 1):      # (1 and 2 share a 256-byte step: not decreasing, growing beyond a step)
        b = L.lvdgs_mesh_sample_scratch_bytes(f)
        assert b % 256 == 0 and b >= prev and (b > prev or f == 2) and b >= 8 * f
        prev = b
    assert [L.lvdgs_mesh_sample_scratch_bytes(f) for f in (0, -1, 2 ** 31)] == [0, 0, 0]
    prev = 0
    for n in (0, 1, 1000, 200_000, 10 ** 6, 2 ** 31 - 1):
        b = L.lvdgs_cloud_distance_scratch_bytes(n, n)
        assert b % 256 == 0 and b >= prev and (b > prev or n == 1) and b >= 2 * 16 * n + 2 * 4 * n      # both clouds sorted, d2 and idx
        if n < 2 ** 31 - 1:
            assert L.lvdgs_cloud_distance_scratch_bytes(n + 1, n) >= b and L.lvdgs_cloud_distance_scratch_bytes(n, n + 1) >= b
        prev = b
    assert [L.lvdgs_cloud_distance_scratch_bytes(m, n) for m, n in ((-1, 5), (5, -1), (2 ** 31, 5), (5, 2 ** 31))] == [0, 0, 0, 0]


# ---------------------------------------------------------------- the mirrors against the float64 statements ----
def test_the_vectorised_keys_are_the_keys():
    for seed in (0, 1, 0xDEADBEEF12345678, 2 ** 64 - 1):
        k = orc.sample_keys(50, seed)
        assert [int(x) for x in k.reshape(-1)] == [orc.key(i, seed) for i in range(150)]
    assert orc.key(2 ** 32 + 5, 7) != orc.key(5, 7)      # the high half of a long index enters


MESHES = {"three": lambda: orc.three_triangles()[:2], "wall": lambda: orc.wavy_wall(9, 7, seed=1)[:2]}


def _spoiled_wall():
    """A wall with a zero-area face, a face with an index out of range and a NaN vertex."""
    v, f, c = orc.wavy_wall(8, 6, seed=2)
    f = f.copy()
    f[3] = (f[3][0], f[3][0], f[3][1])
    f[10] = (f[10][0], len(v), f[10][2])
    f[11] = (-1, f[11][1], f[11][2])
    v = v.copy()
    v[17, 1] = np.nan
    return v, f, c


MESHES["spoiled"] = lambda: _spoiled_wall()[:2]


@pytest.mark.parametrize("name", sorted(MESHES))
def test_sampling_mirror_against_the_float64_statement(name):
    v, f = MESHES[name]()
    n, seed = 700, 0x1234567800000009
    got = orc.sample_f32(v, f, n, seed)
    points, faces = orc.sample_f64(v, f, n, seed)
    assert np.array_equal(got["face_index"], faces)
    m = float(np.nanmax(np.abs(v)))
    worst = float(np.abs(got["points"].astype(np.float64) - points).max())
    print(name, "worst coordinate difference", worst, "in units of u * m:", worst / (U * m))
    assert worst <= 6 * U * SLACK * m
    areas = orc.face_areas(v, f)
    assert (areas[np.unique(faces)] > 0).all() and got["n_weighted"] == int((areas > 0).sum())
    if name == "spoiled":
        bad = {3, 10, 11} | {i for i, face in enumerate(f) if 17 in face}
        assert got["n_weighted"] == len(f) - len(bad) and not bad & set(faces.tolist())


def test_a_mesh_without_area_is_flagged():
    v = np.zeros((3, 3), np.float32)
    got = orc.sample_f32(v, np.array([[0, 1, 2], [0, 0, 7]]), 5, 0)
    assert got["flags"] == orc.NO_AREA and got["n_weighted"] == 0 and got["total"] == 0 and got["points"] is None


def test_face_frequencies_are_the_prefix_intervals():
    """Areas 1 : 2 : 5, n = 8000: the mirror's face counts are the counts of t_k in the integer prefix intervals, exactly."""
    v, f, _ = orc.three_triangles()
    areas = orc.face_areas(v, f)
    assert areas.tolist() == [0.5, 1.0, 2.5]
    q, prefix, total = orc.weights(areas)
    assert q == [2 ** 32 // 5, 2 * 2 ** 32 // 5, 2 ** 32] and prefix[-1] == total
    n, seed = 8000, 42
    t, _, _ = orc.draws(n, seed, total)
    want = [sum(1 for x in t if lo <= x < hi) for lo, hi in zip([0] + prefix[:-1], prefix)]
    got = np.bincount(orc.sample_f32(v, f, n, seed)["face_index"], minlength=3).tolist()
    print("counts", got, "expected shares", [n / 8, n / 4, 5 * n / 8])
    assert got == want and sum(got) == n and all(0 <= x < total for x in t)


def _clouds(seed=0, M=300, N=500):
    rng = np.random.default_rng(seed)
    r = (rng.random((N, 3)) * [4.0, 2.0, 1.0] - [1.0, 0.5, 0.0]).astype(np.float32)
    q = (rng.random((M, 3)) * [5.0, 3.0, 2.0] - [1.5, 1.0, 0.5]).astype(np.float32)
    return q, r


def test_search_mirror_against_the_float64_statement():
    q, r = _clouds()
    q[7], r[11], r[12, 2] = np.nan, np.inf, np.nan
    r[40] = r[20]      # a duplicate: the lower index wins
    q[9] = r[40]
    d2, idx = orc.nearest_f32(q, r)
    want = orc.nearest_f64(q, r)
    assert idx[7] == -1 and np.isinf(d2[7]) and np.isnan(want[7]) and idx[9] == 20 and d2[9] == 0
    assert not np.isin(idx, (11, 12)).any()
    keep = idx >= 0
    rel = np.abs(d2[keep].astype(np.float64) - want[keep]) / np.maximum(want[keep], np.finfo(np.float64).tiny)
    print("worst relative difference of d2 in units of u:", float(rel.max()) / U)
    assert float(rel.max()) <= 5 * U * SLACK
    row = orc.row_of(d2, idx, (0.05, 0.2))
    d = np.sqrt(d2[keep]).astype(np.float64)
    assert row["n_counted"] == int(keep.sum()) == len(q) - 1 and row["n_skipped"] == 1
    for mine, exact in ((float(np.sum(d)), row["sum_distance"]), (float(np.sum(d2[keep].astype(np.float64))), row["sum_squared"])):
        assert abs(mine - exact) <= len(q) * 2.0 ** -53 * exact
    assert row["n_below"][:2] == [int((np.sqrt(d2[keep]) < np.float32(0.05)).sum()), int((np.sqrt(d2[keep]) < np.float32(0.2)).sum())]


def test_search_mirror_without_a_usable_reference():
    q, r = _clouds(M=5, N=3)
    r[:, 0] = np.nan
    d2, idx = orc.nearest_f32(q, r)
    assert np.isinf(d2).all() and (idx == -1).all()
    assert orc.row_of(d2, idx, (), n_reference=0)["flags"] == orc.NO_REFERENCE


# ---------------------------------------------------------------- the score and the file ----
def _row(sum_distance, n_counted, below, skipped=0, flags=0):
    row = np.zeros((), _abi.CLOUD_DISTANCE_ROW_DTYPE)
    row["sum_distance"], row["n_counted"], row["n_skipped"], row["flags"] = sum_distance, n_counted, skipped, flags
    row["n_below"][0] = below
    return row


def test_score_arithmetic_from_rows():
    from lvdgs.mesh_eval import score_from_rows
    s = score_from_rows(_row(12.0, 400, 100, skipped=3), _row(30.0, 600, 300, flags=0), threshold=0.05)
    assert s["accuracy"] == 12.0 / 400 and s["completion"] == 30.0 / 600 and s["chamfer"] == 0.5 * (12.0 / 400 + 30.0 / 600)
    assert s["precision"] == 0.25 and s["recall"] == s["completion_ratio"] == 0.5 and s["fscore"] == 2 * 0.25 * 0.5 / 0.75
    assert (s["n_est"], s["n_gt"], s["skipped_est"], s["skipped_gt"], s["threshold"]) == (400, 600, 3, 0, 0.05)
    s = score_from_rows(_row(1.0, 10, 0), _row(1.0, 10, 0))
    assert s["precision"] == s["recall"] == s["fscore"] == 0.0      # nothing within the threshold: 0, not 0 / 0
    s = score_from_rows(_row(0.0, 0, 0, skipped=9, flags=1), _row(2.0, 4, 4))
    assert math.isnan(s["accuracy"]) and math.isnan(s["precision"]) and math.isnan(s["fscore"]) and math.isnan(s["chamfer"])
    assert s["completion"] == 0.5 and s["recall"] == 1.0 and s["flags_est"] == 1


@pytest.mark.parametrize("colors", [True, False])
def test_ply_round_trip(tmp_path, colors):
    from lvdgs.mesh_eval import load_mesh_ply
    from lvdgs.tsdf import Mesh, save_mesh_ply
    v, f, c = orc.wavy_wall(6, 5, seed=4)
    c8 = np.random.default_rng(1).integers(0, 256, c.shape).astype(np.float32) / np.float32(255)
    mesh = Mesh(torch.from_numpy(v), torch.from_numpy(c8) if colors else None, torch.from_numpy(f))
    path = str(tmp_path / "wall.ply")
    save_mesh_ply(path, mesh)
    back = load_mesh_ply(path, device="cpu")
    assert back.vertices.dtype is torch.float32 and back.faces.dtype is torch.int32
    assert np.array_equal(back.vertices.numpy().view(np.uint32), v.view(np.uint32)) and np.array_equal(back.faces.numpy(), f)
    if colors:
        assert np.array_equal(np.round(back.colors.numpy() * 255), np.round(c8 * 255))
        again = str(tmp_path / "again.ply")
        save_mesh_ply(again, back)
        assert open(again, "rb").read() == open(path, "rb").read()
    else:
        assert back.colors is None
    (tmp_path / "text.ply").write_bytes(b"ply\nformat ascii 1.0\nend_header\n")
    with pytest.raises(_lib.LvdgsError):
        load_mesh_ply(str(tmp_path / "text.ply"), device="cpu")


def test_cpu_tensors_are_refused():
    from lvdgs import mesh_eval
    v, f, _ = orc.three_triangles()
    q, r = _clouds(M=4, N=4)
    with pytest.raises(_lib.LvdgsError, match="no CPU path"):
        mesh_eval.sample_mesh((torch.from_numpy(v), torch.from_numpy(f)), 10)
    with pytest.raises(_lib.LvdgsError, match="no CPU path"):
        mesh_eval.nearest(torch.from_numpy(q), torch.from_numpy(r))
    with pytest.raises(_lib.LvdgsError, match="no CPU path"):
        mesh_eval.score((torch.from_numpy(v), torch.from_numpy(f)), torch.from_numpy(r))
