"""``lvdgs_mesh_sample`` / ``lvdgs_cloud_distance`` through ``lvdgs.mesh_eval`` on the GPU against the mirrors of tests/mesh_eval_oracle.py.

Sampling: points, face indices, colours and the info row BIT FOR BIT.  The search: ``d2`` and ``idx`` bit for bit against the float32 brute
force, the row's counts and maximum exact, its two float64 sums within M * 2^-53 relative of ``math.fsum`` (any order of a float64 sum of M
non-negative terms is that close; tests/test_mesh_eval.py states the bounds).  Every case is a few thousand points at most.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import mesh_eval_oracle as orc
from lvdgs import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAD = 64


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---------------------------------------------------------------- sampling ----
def _sample_raw(v, f, n, seed, c=None):
    """One call into buffers with PAD sentinel rows behind the n samples -> (points, face_index, colors, info record)."""
    from lvdgs import mesh_eval
    table = mesh_eval.Table(torch.device(DEV, torch.cuda.current_device()), rows=0, infos=1)
    points = torch.full((n + PAD, 3), -7.5, dtype=torch.float32, device=DEV)
    face_index = torch.full((n + PAD,), -77, dtype=torch.int32, device=DEV)
    colors = torch.full((n + PAD, 3), -7.5, dtype=torch.float32, device=DEV) if c is not None else None
    mesh_eval.sample_raw(_t(v), _t(f), n, seed, points, table.info_ptr(0), vertex_colors=_t(c), colors=colors, face_index=face_index)
    info = table.read()[1][0]
    return points.cpu().numpy(), face_index.cpu().numpy(), None if colors is None else colors.cpu().numpy(), info


def _check_sampling(v, f, n, seed, c=None):
    want = orc.sample_f32(v, f, n, seed, colors=c)
    p, fi, col, info = _sample_raw(v, f, n, seed, c)
    assert (int(info["flags"]), int(info["n_weighted"]), int(info["total"])) == (want["flags"], want["n_weighted"], want["total"])
    assert (p[n:] == -7.5).all() and (fi[n:] == -77).all() and (col is None or (col[n:] == -7.5).all())
    if want["points"] is None:
        assert (p == -7.5).all() and (fi == -77).all() and (col is None or (col == -7.5).all())      # nothing sampled, nothing touched
    else:
        assert np.array_equal(fi[:n], want["face_index"])
        assert np.array_equal(_bits(p[:n]), _bits(want["points"]))
        if c is not None:
            assert np.array_equal(_bits(col[:n]), _bits(want["colors"]))
    again = _sample_raw(v, f, n, seed, c)
    assert np.array_equal(_bits(again[0]), _bits(p)) and np.array_equal(again[1], fi)      # two calls, the same bytes
    return want, p[:n], fi[:n]


@pytest.mark.parametrize("n", [1, 255, 256, 257, 10_007])
def test_sampling_the_three_triangles(n):
    v, f, c = orc.three_triangles()
    want, p, fi = _check_sampling(v, f, n, seed=0xABCDEF0123456789, c=c)
    if n == 10_007:
        print("face counts", np.bincount(fi, minlength=3).tolist(), "of", n, "for areas 1 : 2 : 5")


def test_sampling_one_triangle():
    v = np.array([[0.5, -1.0, 2.0], [3.0, 0.25, 2.5], [-1.0, 4.0, 1.0]], np.float32)
    _check_sampling(v, np.array([[0, 1, 2]], np.int32), 500, seed=1)
    _check_sampling(v, np.array([[0, 1, 2]], np.int32), 500, seed=2 ** 64 - 1)


def test_sampling_skips_faces_without_weight():
    """A zero-area face, two faces with an index out of range and the faces of a NaN vertex: never chosen, the count exact."""
    v, f, c = orc.wavy_wall(8, 6, seed=2)
    f = f.copy()
    f[3] = (f[3][0], f[3][0], f[3][1])
    f[10] = (f[10][0], len(v), f[10][2])
    f[11] = (-1, f[11][1], f[11][2])
    v = v.copy()
    v[17, 1] = np.nan
    want, p, fi = _check_sampling(v, f, 3000, seed=5, c=c)
    bad = {3, 10, 11} | {i for i, face in enumerate(f) if 17 in face}
    assert want["n_weighted"] == len(f) - len(bad) and not bad & set(fi.tolist()) and np.isfinite(p).all()


@pytest.mark.parametrize("faces", [257, 70_000, 525_312])
def test_sampling_a_prefix_over_several_workgroups(faces):
    """257 faces: two rounds of a workgroup's scan; 70 000: 274 spans, two rounds of the scan over the spans; 525 312: above 2048 x 256,
    so a span is two tiles of 256 faces long and the prefix pass carries its sum from the first tile into the second."""
    nx, ny = (514, 513) if faces == 525_312 else (176, 201)
    v, f, c = orc.wavy_wall(nx, ny, seed=7)
    assert len(f) == max(faces, 70_000)
    _check_sampling(v, f[:faces], 2000, seed=11, c=c if faces == 257 else None)


def test_sampling_a_mesh_of_degenerate_faces():
    v = np.array([[0, 0, 0], [1, 1, 1], [2, 2, 2], [np.inf, 0, 0]], np.float32)
    want, _, _ = _check_sampling(v, np.array([[0, 1, 2], [0, 0, 1], [0, 1, 3], [0, 1, 9]], np.int32), 300, seed=3, c=np.ones((4, 3), np.float32))
    assert want["flags"] == orc.NO_AREA


def test_sample_mesh_returns_colours_for_a_coloured_mesh():
    from lvdgs import mesh_eval
    from lvdgs.tsdf import Mesh
    v, f, c = orc.three_triangles()
    want = orc.sample_f32(v, f, 400, 9, colors=c)
    points, colors = mesh_eval.sample_mesh(Mesh(_t(v), _t(c), _t(f)), 400, seed=9)
    assert np.array_equal(_bits(points.cpu().numpy()), _bits(want["points"])) and np.array_equal(_bits(colors.cpu().numpy()), _bits(want["colors"]))
    plain = mesh_eval.sample_mesh((_t(v), _t(f.astype(np.int64))), 400, seed=9)      # a pair, int64 faces
    assert torch.equal(plain, points)
    flat = mesh_eval.sample_mesh((_t(np.zeros((3, 3), np.float32)), _t(np.array([[0, 1, 2]], np.int32))), 5)
    assert bool(torch.isnan(flat).all())      # no area: NaN rows


# ---------------------------------------------------------------- the search ----
def _search_raw(q, r, thresholds=(), ppc=0, want_d2=True, want_idx=True):
    """One call into buffers with PAD sentinels behind the M results -> (d2, idx, row record)."""
    from lvdgs import mesh_eval
    dev = torch.device(DEV, torch.cuda.current_device())
    L = _lib.lib()
    M, N = len(q), len(r)
    table = mesh_eval.Table(dev, rows=3)
    scratch = mesh_eval._distance_scratch.get(dev, int(L.lvdgs_cloud_distance_scratch_bytes(M, N)))
    d2 = torch.full((M + PAD,), -7.5, dtype=torch.float32, device=DEV)
    idx = torch.full((M + PAD,), -77, dtype=torch.int32, device=DEV)
    tq, tr = _t(np.asarray(q, np.float32).reshape(-1, 3)), _t(np.asarray(r, np.float32).reshape(-1, 3))
    a = _lib.CloudDistanceArgs(num_queries=M, num_reference=N, queries=tq.data_ptr(), reference=tr.data_ptr() if N else None,
                               num_thresholds=len(thresholds), points_per_cell=ppc, thresholds=(C.c_float * 4)(*thresholds),
                               d2=d2.data_ptr() if want_d2 else None, idx=idx.data_ptr() if want_idx else None, out_row=table.row_ptr(1),
                               scratch=scratch.data_ptr(), scratch_bytes=scratch.numel())
    _lib.check(L.lvdgs_cloud_distance(C.byref(a), _lib.raw_stream(dev)), "lvdgs_cloud_distance")
    rows = table.read()[0]
    assert not rows[0].tobytes().strip(b"\0") and not rows[2].tobytes().strip(b"\0")      # the rows beside it: untouched
    return d2.cpu().numpy(), idx.cpu().numpy(), rows[1]


_BRUTE = {}


def _brute(key, q, r):
    """The float32 brute force of a named case, computed once."""
    if key not in _BRUTE:
        _BRUTE[key] = orc.nearest_f32(q, r)
    return _BRUTE[key]


def _check_search(key, q, r, thresholds=(), ppc=0):
    q, r = np.asarray(q, np.float32).reshape(-1, 3), np.asarray(r, np.float32).reshape(-1, 3)
    M = len(q)
    want_d2, want_idx = _brute(key, q, r)
    d2, idx, row = _search_raw(q, r, thresholds, ppc)
    assert (d2[M:] == -7.5).all() and (idx[M:] == -77).all()
    bad = np.flatnonzero((idx[:M] != want_idx) | (_bits(d2[:M]) != _bits(want_d2)))
    assert not len(bad), (key, ppc, len(bad), bad[:5], idx[bad[:5]], want_idx[bad[:5]], d2[bad[:5]], want_d2[bad[:5]])
    n_ref = int(np.isfinite(r).all(1).sum())
    want = orc.row_of(want_d2, want_idx, thresholds, n_reference=n_ref)
    assert (int(row["n_counted"]), int(row["n_skipped"]), row["n_below"].tolist(), int(row["flags"]), int(row["n_reference"])) == \
        (want["n_counted"], want["n_skipped"], want["n_below"], want["flags"], n_ref), (key, ppc, row, want)
    assert float(row["max_distance"]) == want["max_distance"] and not row["reserved"].any()
    for name in ("sum_distance", "sum_squared"):
        assert abs(float(row[name]) - want[name]) <= M * 2.0 ** -53 * want[name], (key, name, float(row[name]), want[name])
    return d2[:M], idx[:M], row


def _cloud(seed, n, lo=(-1.0, -0.5, 0.0), size=(4.0, 2.0, 1.0)):
    rng = np.random.default_rng(seed)
    return (rng.random((n, 3)) * size + lo).astype(np.float32)


@pytest.mark.parametrize("ppc", [0, 1, 10 ** 9])
@pytest.mark.parametrize("M", [1, 255, 257, 5003])
def test_search_general_clouds(M, ppc):
    """N = 1000, no multiple of 256; default cells, one point per cell (many cells), everything in one cell."""
    r = _cloud(1, 1000)
    q = _cloud(2, M, lo=(-1.2, -0.7, -0.2), size=(4.4, 2.4, 1.4))      # some of them outside the box
    _check_search(("general", M), q, r, thresholds=(0.05, 0.1), ppc=ppc)


def test_search_one_reference_point():
    _check_search("one", _cloud(3, 300), np.array([[0.25, -0.125, 0.5]], np.float32), thresholds=(1.0,))


def test_search_duplicates_and_exact_hits():
    """Duplicated reference points: the lowest index wins; queries equal to reference points: d2 == 0."""
    r = _cloud(4, 700)
    r[300:400] = r[100:200]
    r[650] = r[5]
    q = np.concatenate([r[350:380], r[650:651], r[::7], _cloud(5, 100)])
    for ppc in (0, 1):
        d2, idx, _ = _check_search("duplicates", q, r, thresholds=(0.0, 1e-3), ppc=ppc)
        assert (idx[:30] == np.arange(150, 180)).all() and idx[30] == 5 and (d2[:31 + 100] == 0).all()


def test_search_queries_on_cell_borders():
    """Queries at lo + extent * c / n for n = 1 .. 24 along every axis: whatever resolution the grid took, some lie on its planes."""
    r = _cloud(6, 2000, lo=(0, 0, 0), size=(1, 1, 1))
    r[0], r[1] = (0, 0, 0), (1, 1, 1)
    fr = np.unique(np.concatenate([np.arange(n + 1) / n for n in range(1, 25)])).astype(np.float32)
    rng = np.random.default_rng(7)
    q = np.stack([rng.choice(fr, 3000), rng.choice(fr, 3000), rng.choice(fr, 3000)], 1).astype(np.float32)
    for ppc in (1, 8, 64):
        _check_search("borders", q, r, ppc=ppc)


def test_search_queries_far_outside_the_box():
    r = _cloud(8, 1500)
    far = []
    for axis in range(3):
        for sign in (-1.0, 1.0):
            p = _cloud(9 + axis, 40)
            p[:, axis] += sign * 50.0
            far.append(p)
    diag = _cloud(12, 40) + np.float32(30.0)
    q = np.concatenate(far + [diag, -diag, _cloud(13, 5) * np.float32(1e4)])
    for ppc in (1, 8):
        _check_search("far", q, r, thresholds=(40.0,), ppc=ppc)


def test_search_two_clusters_and_an_empty_middle():
    """Two tight clusters in opposite corners, queries in the empty middle, the finest grid the scratch allows: the call returns, exactly."""
    a = _cloud(14, 1000, lo=(0, 0, 0), size=(0.01, 0.01, 0.01))
    b = _cloud(15, 1000, lo=(9.99, 9.99, 9.99), size=(0.01, 0.01, 0.01))
    r = np.concatenate([a, b])
    q = np.concatenate([_cloud(16, 1500, lo=(3, 3, 3), size=(4, 4, 4)), _cloud(17, 300, lo=(0, 0, 0), size=(10, 10, 10))])
    _check_search("clusters", q, r, thresholds=(5.0, 9.0), ppc=1)


def test_search_a_cell_with_more_points_than_the_tile():
    """3000 points in one cell (the LDS tile holds 512: six rounds), alone and beside a sparse cloud."""
    dense = _cloud(18, 3000, lo=(0.4, 0.4, 0.4), size=(0.02, 0.02, 0.02))
    q = np.concatenate([_cloud(19, 400, lo=(0.39, 0.39, 0.39), size=(0.04, 0.04, 0.04)), _cloud(20, 200, lo=(0, 0, 0), size=(1, 1, 1))])
    _check_search("tile-one-cell", q, dense, ppc=10 ** 9)
    r = np.concatenate([dense, _cloud(21, 200, lo=(0, 0, 0), size=(1, 1, 1))])
    _check_search("tile-among-cells", q, r, ppc=8)


def test_search_a_grid_of_more_cells_than_one_tile_a_span():
    """The scan over the cells has 256 spans of 256-cell tiles, so it takes more than 65 536 cells for a span to be two tiles long.
    The grid cannot be read back; by the header's rule 120 000 points uniform in a cube at one point per cell give: target = 120 000
    cells = the budget, h = extent / 49.3, 50 cells an axis = 125 000 > budget, h * 1.1 = extent / 44.8, 45 cells an axis = 91 125
    cells <= budget.  Above 65 536: spans of 512 cells, 178 of them with cells."""
    r = _cloud(22, 120_000, lo=(0, 0, 0), size=(1, 1, 1))
    q = _cloud(23, 1500, lo=(-0.05, -0.05, -0.05), size=(1.1, 1.1, 1.1))
    assert math.floor(1 / ((1 / 120_000) ** (1 / 3) * 1.1)) + 1 == 45 and 50 ** 3 > 120_000 >= 45 ** 3 > 65_536
    _check_search("many-cells", q, r, thresholds=(0.01,), ppc=1)


def test_search_coplanar_and_collinear_reference_points():
    r = _cloud(22, 1200)
    r[:, 2] = 0.75      # a zero-extent axis
    q = _cloud(23, 900, lo=(-1.5, -1, -1), size=(5, 3, 3))
    for ppc in (1, 8):
        _check_search("coplanar", q, r, ppc=ppc)
    r[:, 1] = -0.25     # two of them
    _check_search("collinear", q, r, ppc=2)
    r[:] = r[0]         # and three: every point the same
    _, idx, _ = _check_search("coincident", q, r, ppc=1)
    assert (idx == 0).all()


def test_search_non_finite_points():
    """NaN / inf among the queries: skipped, counted as such, idx -1; among the reference points: never chosen."""
    r, q = _cloud(24, 900), _cloud(25, 600)
    r[0, 0], r[100, 1], r[899, 2], r[450] = np.nan, np.inf, -np.inf, np.nan
    q[0, 2], q[17, 0], q[599] = np.nan, np.inf, (-np.inf, np.nan, 0)
    q[5] = (0.5, 0.1, 1e15)      # finite and far: counted
    d2, idx, row = _check_search("non-finite", q, r, thresholds=(0.1,), ppc=4)
    assert int(row["n_skipped"]) == 3 and (idx[[0, 17, 599]] == -1).all() and np.isinf(d2[[0, 17, 599]]).all()
    assert not np.isin(idx, (0, 100, 899, 450)).any() and int(row["n_reference"]) == 896


@pytest.mark.parametrize("N", [0, 3])
def test_search_without_a_usable_reference(N):
    r = np.full((N, 3), np.nan, np.float32)
    d2, idx, row = _check_search(("no-reference", N), _cloud(26, 300), r, thresholds=(1.0,))
    assert int(row["flags"]) == _lib.CLOUD_DISTANCE_NO_REFERENCE and int(row["n_skipped"]) == 300 and int(row["n_counted"]) == 0
    assert float(row["sum_distance"]) == 0.0 and (idx == -1).all() and np.isinf(d2).all()


def test_search_thresholds_are_strict():
    """Thresholds at 0, at an exactly attained distance (strict <) and far above."""
    r = np.array([[0, 0, 0], [4, 0, 0]], np.float32)
    q = np.array([[0, 0, 0], [0, 3, 0], [0, 0.5, 0], [4, 0, 3], [1, 0, 0]], np.float32)      # distances 0, 3, 0.5, 3, 1
    d2, idx, row = _check_search("thresholds", q, r, thresholds=(0.0, 3.0, 1e6, 0.5))
    assert d2.tolist() == [0.0, 9.0, 0.25, 9.0, 1.0] and idx.tolist() == [0, 0, 0, 1, 0]
    assert row["n_below"].tolist() == [0, 3, 5, 1] and float(row["max_distance"]) == 3.0


def test_search_is_independent_of_the_grid():
    """The same inputs with three values of points_per_cell: identical bytes, the row's sums included."""
    r, q = _cloud(27, 3000), _cloud(28, 2500, lo=(-1.1, -0.6, -0.1), size=(4.2, 2.2, 1.2))
    runs = [_search_raw(q, r, (0.03, 0.06), ppc) for ppc in (2, 8, 300)]
    for d2, idx, row in runs[1:]:
        assert np.array_equal(_bits(d2), _bits(runs[0][0])) and np.array_equal(idx, runs[0][1]) and row.tobytes() == runs[0][2].tobytes()
    again = _search_raw(q, r, (0.03, 0.06), 8)
    assert again[2].tobytes() == runs[1][2].tobytes()      # two calls, the same bits


def test_search_with_only_the_row_asked_for():
    r, q = _cloud(29, 800), _cloud(30, 700)
    full = _search_raw(q, r, (0.05,), 0)
    d2, idx, row = _search_raw(q, r, (0.05,), 0, want_d2=False, want_idx=False)
    assert (d2 == -7.5).all() and (idx == -77).all() and row.tobytes() == full[2].tobytes()
    d2, idx, row = _search_raw(q, r, (0.05,), 0, want_idx=False)
    assert np.array_equal(_bits(d2), _bits(full[0])) and (idx == -77).all() and row.tobytes() == full[2].tobytes()


def test_nearest_returns_tensors_and_a_table():
    from lvdgs import mesh_eval
    r, q = _cloud(31, 500), _cloud(32, 400)
    d2, idx, table = mesh_eval.nearest(_t(q), _t(r), thresholds=(0.1,))
    want_d2, want_idx = orc.nearest_f32(q, r)
    row = table.read()[0][0]
    assert np.array_equal(_bits(d2.cpu().numpy()), _bits(want_d2)) and np.array_equal(idx.cpu().numpy(), want_idx) and int(row["n_counted"]) == 400


# ---------------------------------------------------------------- the score ----
def test_a_mesh_scores_zero_against_itself():
    from lvdgs import mesh_eval
    v, f, _ = orc.wavy_wall(12, 9, seed=8)
    mesh = (_t(v), _t(f))
    s = mesh_eval.score(mesh, mesh, n_samples=4000, threshold=0.05, seed=3, seed_gt=3)
    assert s["accuracy"] == 0.0 and s["completion"] == 0.0 and s["chamfer"] == 0.0
    assert s["completion_ratio"] == 1.0 and s["precision"] == 1.0 and s["recall"] == 1.0 and s["fscore"] == 1.0
    assert (s["n_est"], s["n_gt"], s["skipped_est"], s["skipped_gt"], s["flags_est"], s["flags_gt"]) == (4000, 4000, 0, 0, 0, 0)
    other = mesh_eval.score(mesh, mesh, n_samples=4000, threshold=0.05, seed=3)      # seed + 1 for the ground truth: near, not zero
    assert 0.0 < other["chamfer"] < 0.1 and other["fscore"] > 0.5


def test_two_parallel_squares():
    from lvdgs import mesh_eval
    h, n, seed = 0.25, 3000, 21
    (v0, f0), (v1, f1) = orc.unit_square(0.0), orc.unit_square(h)
    est, gt = (_t(v0), _t(f0)), (_t(v1), _t(f1))
    p0, p1 = orc.sample_f32(v0, f0, n, seed)["points"], orc.sample_f32(v1, f1, n, seed + 1)["points"]
    d2, _, _ = mesh_eval.nearest(mesh_eval.sample_mesh(est, n, seed), mesh_eval.sample_mesh(gt, n, seed + 1))
    assert float(d2.min()) ** 0.5 >= h * (1 - 2.0 ** -20)
    s = mesh_eval.score(est, gt, n_samples=n, threshold=h / 2, seed=seed)
    assert s["precision"] == 0.0 and s["recall"] == 0.0 and s["completion_ratio"] == 0.0 and s["fscore"] == 0.0
    d_est = np.sqrt(orc.nearest_f32(p0, p1)[0])
    d_gt = np.sqrt(orc.nearest_f32(p1, p0)[0])
    for threshold in (h / 2, 0.26):
        s = mesh_eval.score(est, gt, n_samples=n, threshold=threshold, seed=seed)
        want = orc.score_of(d_est, d_gt, threshold)
        for name in ("precision", "recall", "completion_ratio"):
            assert s[name] == want[name], (threshold, name)
        for name in ("accuracy", "completion", "chamfer", "fscore"):
            assert abs(s[name] - want[name]) <= 2 * n * 2.0 ** -53 * max(want[name], 1e-300), (threshold, name, s[name], want[name])
        assert s["accuracy"] >= h * (1 - 2.0 ** -20) and s["completion"] >= h * (1 - 2.0 ** -20)
    clouds = mesh_eval.score(_t(p0), _t(p1), threshold=0.26)      # clouds are used as given
    assert clouds["accuracy"] == s["accuracy"] and clouds["completion"] == s["completion"] and clouds["n_est"] == n


def _count_waits_and_reads(fn):
    """tests/test_gpu_tsdf.py's idiom: calls of HostCall.wait, of any synchronize, of Tensor.cpu / .item / .tolist while ``fn`` runs."""
    counts = {"wait": 0, "sync": 0, "read": 0}
    saved = [(_lib.HostCall, "wait", _lib.HostCall.wait), (torch.cuda, "synchronize", torch.cuda.synchronize),
             (torch.cuda.Stream, "synchronize", torch.cuda.Stream.synchronize), (torch.cuda.Event, "synchronize", torch.cuda.Event.synchronize),
             (torch.Tensor, "cpu", torch.Tensor.cpu), (torch.Tensor, "item", torch.Tensor.item), (torch.Tensor, "tolist", torch.Tensor.tolist)]

    def counting(kind, real):
        def f(*a, **k):
            counts[kind] += 1
            return real(*a, **k)
        return f
    for owner, name, real in saved:
        setattr(owner, name, counting("wait" if owner is _lib.HostCall else "sync" if name == "synchronize" else "read", real))
    try:
        fn()
    finally:
        for owner, name, real in saved:
            setattr(owner, name, real)
    return counts


def test_score_makes_one_synchronise_and_no_other_read():
    from lvdgs import mesh_eval
    v, f, _ = orc.wavy_wall(12, 9, seed=8)
    w, g, _ = orc.wavy_wall(10, 11, seed=9, offset=0.02)
    est, gt = (_t(v), _t(f)), (_t(w), _t(g))
    mesh_eval.score(est, gt, n_samples=2000)      # (the first call allocates the scratch, the table and its pinned copy)
    out = []
    c = _count_waits_and_reads(lambda: out.append(mesh_eval.score(est, gt, n_samples=2000, threshold=0.05)))
    assert c == {"wait": 0, "sync": 1, "read": 0}, c
    assert 0.0 < out[0]["chamfer"] < 0.1
    c = _count_waits_and_reads(lambda: (mesh_eval.sample_mesh(est, 500), mesh_eval.nearest(_t(w), _t(v))))
    assert c == {"wait": 0, "sync": 0, "read": 0}, c


# ---------------------------------------------------------------- the system ----
_SEQ = {}


def _toy_run():
    if not _SEQ:
        import random
        import sequence_scene as ss
        from lvdgs.slam_sequence import SlamSequence
        cfg, ds, _, _, _ = ss.toy_sequence_on_cpu()
        ds.depths = [d.copy() for d in ds.mono_depths]      # a depth sensor for the evaluation; the run is monocular and reads none
        torch.manual_seed(0)
        random.seed(0)
        _SEQ["seq"] = SlamSequence(cfg, ds.to("cuda"), ss.empty_map(cfg, "cuda"), ss.PIPE, torch.zeros(3, device="cuda"), idle_map_iters=2).run()
        g = _SEQ["seq"].frontend_gaussians
        _SEQ["voxel"] = float((g.get_xyz.detach().max(0).values - g.get_xyz.detach().min(0).values).max()) / 48.0
    return _SEQ["seq"], _SEQ["voxel"]


def test_eval_mesh_over_the_toy_sequence():
    seq, voxel = _toy_run()
    score, record = seq.eval_mesh(voxel, n_samples=5000)
    print(score, record)
    assert record["est"]["faces"] > 0 and record["gt"]["faces"] > 0 and record["est"]["dims"] == record["gt"]["dims"]
    assert record["threshold"] == 2 * record["voxel_size"] and record["gt"]["frames"] == len(seq.kf_indices)
    for name in ("accuracy", "completion", "completion_ratio", "precision", "recall", "fscore", "chamfer"):
        assert math.isfinite(score[name]), name
    assert score["n_est"] == score["n_gt"] == 5000 and score["accuracy"] > 0 and 0 <= score["fscore"] <= 1
    again, _ = seq.eval_mesh(voxel, n_samples=5000)
    assert again == score      # bit for bit


def test_eval_mesh_at_the_true_poses_with_the_dataset_depth_scores_zero():
    seq, voxel = _toy_run()
    saved = {i: (cam.R.clone(), cam.T.clone()) for i, cam in seq.cameras.items()}
    try:
        for cam in seq.cameras.values():
            cam.update_RT(cam.R_gt.to(cam.R.dtype), cam.T_gt.to(cam.T.dtype))
        score, record = seq.eval_mesh(voxel, n_samples=5000, est_depth="dataset", seed=4, seed_gt=4)
    finally:
        for i, cam in seq.cameras.items():
            cam.update_RT(*saved[i])
    assert record["est"]["faces"] == record["gt"]["faces"] > 0
    assert score["accuracy"] == 0.0 and score["completion"] == 0.0 and score["chamfer"] == 0.0 and score["fscore"] == 1.0


def test_eval_mesh_refuses_a_dataset_without_metric_depth():
    seq, voxel = _toy_run()
    saved, held = seq.dataset.depths, {i: cam.depth for i, cam in seq.cameras.items()}      # (keyframes keep the plane they were made with)
    try:
        seq.dataset.depths = [np.zeros_like(d) for d in saved]      # the KITTI / dl3dv placeholders: all-zero planes
        for i, cam in seq.cameras.items():
            cam.depth = None if held[i] is None else np.zeros_like(np.asarray(held[i]))
        with pytest.raises(_lib.LvdgsError, match="without metric depth"):
            seq.eval_mesh(voxel, n_samples=1000)
        seq.dataset.depths = None                                   # and no planes at all
        for cam in seq.cameras.values():
            cam.depth = None
        with pytest.raises(_lib.LvdgsError, match="without metric depth"):
            seq.eval_mesh(voxel, n_samples=1000)
    finally:
        seq.dataset.depths = saved
        for i, cam in seq.cameras.items():
            cam.depth = held[i]
