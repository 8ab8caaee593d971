"""``lvdgs_mesh_depth`` through ``lvdgs.mesh_eval`` on the GPU against the float32 mirror of tests/mesh_depth_oracle.py: depth planes and
face planes BIT FOR BIT, sentinels behind every plane untouched, two calls the same bytes.  Then what occlusion culling means on two
squares, and ``SlamSequence.eval_mesh`` with ``cull="occlusion"`` and ``depth_l1`` over the toy sequence.  Every case is a few thousand
pixels and, unless its name says otherwise, a few hundred faces.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import mesh_cull_oracle as mco
import mesh_depth_oracle as orc
import mesh_eval_oracle as meo
import test_mesh_depth as cpu
from lvdgs import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAD = 64
F32 = np.float32
LANE_PIXELS = 16      # csrc/mesh_depth.hip: the largest box a lane walks alone


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _device_view(v):
    return {k: (_t(x) if isinstance(x, np.ndarray) else x) for k, x in v.items() if k != "depth"}


def _mesh(v, f):
    return _t(np.ascontiguousarray(v, F32).reshape(-1, 3)), _t(np.ascontiguousarray(f, np.int32).reshape(-1, 3))


def _raw(v, f, views, want_faces=True):
    """One ``lvdgs_mesh_depth`` call (at most 16 views) into planes with PAD sentinel elements behind each -> [(depth, face or None)] as
    NumPy arrays, the sentinels checked."""
    from lvdgs.tsdf import view_block
    tv, tf = _mesh(v, f)
    dev = tv.device
    blocks = [view_block("test", dev, False, None, size=orc.size_of(w), **{k: x for k, x in _device_view(w).items() if k != "size"}) for w in views]
    sizes = [orc.size_of(w) for w in views]
    depth = [torch.full((h * w + PAD,), -7.5, dtype=torch.float32, device=dev) for h, w in sizes]
    index = [torch.full((h * w + PAD,), -77, dtype=torch.int32, device=dev) for h, w in sizes] if want_faces else None
    L = _lib.lib()
    n = len(views)
    scratch = torch.empty(int(L.lvdgs_mesh_depth_scratch_bytes(sum(h * w for h, w in sizes))), dtype=torch.uint8, device=dev)
    ptrs = (C.POINTER(_lib.TsdfViewArgs) * max(n, 1))(*[C.pointer(a) for a, _ in blocks])
    planes = (C.c_void_p * max(n, 1))(*[d.data_ptr() for d in depth])
    indices = (C.c_void_p * max(n, 1))(*[d.data_ptr() for d in index]) if want_faces else None
    a = _lib.MeshDepthArgs(num_vertices=tv.shape[0], num_faces=tf.shape[0], vertices=tv.data_ptr() if tv.shape[0] else None,
                           faces=tf.data_ptr() if tf.shape[0] else None, views=C.cast(ptrs, C.c_void_p), count=n, depth=C.cast(planes, C.c_void_p),
                           face_index=None if indices is None else C.cast(indices, C.c_void_p), scratch=scratch.data_ptr(), scratch_bytes=scratch.numel())
    _lib.check(L.lvdgs_mesh_depth(C.byref(a), _lib.raw_stream(dev)), "lvdgs_mesh_depth")
    out = []
    for k, (h, w) in enumerate(sizes):
        d = depth[k].cpu().numpy()
        i = index[k].cpu().numpy() if want_faces else None
        assert (d[h * w:] == -7.5).all() and (i is None or (i[h * w:] == -77).all())      # nothing behind height*width elements is touched
        out.append((d[:h * w].reshape(h, w), None if i is None else i[:h * w].reshape(h, w)))
    return out


def _check(v, f, views, want=None):
    """The raw call against the mirror bit for bit, twice, and ``render_depth`` (which batches by 16) the same -> the mirror's planes."""
    from lvdgs import mesh_eval
    want = [orc.render(v, f, w) for w in views] if want is None else want
    for first in range(0, max(len(views), 1), 16):
        chunk = views[first:first + 16]
        got = _raw(v, f, chunk)
        for k, ((d, i), (wd, wi)) in enumerate(zip(got, want[first:first + 16])):
            assert np.array_equal(_bits(d), _bits(wd)), (first + k, np.argwhere(_bits(d) != _bits(wd))[:10])
            assert np.array_equal(i, wi), (first + k, np.argwhere(i != wi)[:10])
        again = _raw(v, f, chunk)
        assert all(np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(a[1], b[1]) for a, b in zip(again, got))      # two calls, the same bytes
    planes, indices = mesh_eval.render_depth(_mesh(v, f), [_device_view(w) for w in views], want_faces=True)
    assert len(planes) == len(indices) == len(views)
    for d, i, (wd, wi) in zip(planes, indices, want):
        assert d.dtype is torch.float32 and i.dtype is torch.int32 and tuple(d.shape) == tuple(i.shape) == wd.shape
        assert np.array_equal(_bits(d.cpu().numpy()), _bits(wd)) and np.array_equal(i.cpu().numpy(), wi)
    only = mesh_eval.render_depth(_mesh(v, f), [_device_view(w) for w in views])
    assert all(np.array_equal(_bits(d.cpu().numpy()), _bits(wd)) for d, (wd, _) in zip(only, want))
    return want


def _axis(size, f=1.0, c=0.0, **kw):
    return cpu._axis_view(size, f, f, c, c, **kw)


def _orbit(k, n, size=(48, 64), **kw):
    """View k of n on an arc in front of the wall over [0, 2]^2."""
    a = -0.8 + 1.6 * (k + 0.5) / max(n, 1)
    R, T = mco.look_at((1.0 + 2.6 * math.sin(a), 0.9 + 0.1 * k / max(n, 1), -2.6 * math.cos(a)), (1.0, 1.0, 0.1))
    H, W = size
    return mco.view(R, T, (0.8 * W, 0.84 * W, W / 2 - 0.3, H / 2 - 0.4), size=size, **kw)


# ---------------------------------------------------------------- single faces and small meshes ----
def test_one_triangle_in_an_8x8_view_and_a_1x1_view():
    tri, f = np.array([[2, 2, 1], [6, 2, 1], [2, 6, 1]], F32), np.array([[0, 1, 2]], np.int32)
    (depth, face), = _check(tri, f, [_axis((8, 8))])
    assert (depth > 0).sum() == 15 and depth[2, 2] == 1 and face[2, 2] == 0 and face[7, 7] == -1      # edges and vertices inclusive
    one = np.array([[-1, -1, 2], [3, -1, 2], [-1, 3, 2]], F32)
    (depth, face), = _check(one, f, [_axis((1, 1))])
    assert abs(depth[0, 0] - 2) < 1e-5 and face[0, 0] == 0
    (depth, face), = _check(one + F32(5), f, [_axis((1, 1))])      # beside the only pixel
    assert depth[0, 0] == 0 and face[0, 0] == -1


def test_views_of_two_sizes_in_one_call():
    v, f, _ = meo.wavy_wall(12, 9, seed=2)
    want = _check(v, f, [_orbit(0, 2, size=(48, 64)), _orbit(1, 2, size=(9, 17)), _orbit(1, 2, size=(31, 5), depth_trunc=2.7)])
    assert all((d > 0).any() for d, _ in want)


@pytest.mark.parametrize("count", [0, 1, 16, 17])
def test_view_counts(count):
    """17 views go through ``render_depth`` as two library calls."""
    v, f, _ = meo.wavy_wall(10, 8, seed=3)
    views = [_orbit(k, count, size=(24, 32)) for k in range(count)]
    want = _check(v, f, views)
    assert len(want) == count and all((d > 0).any() for d, _ in want)


@pytest.mark.parametrize("what", ["no faces", "no vertices"])
def test_empty_inputs_give_empty_planes(what):
    v, f, _ = meo.wavy_wall(5, 5, seed=1)
    v, f = (v, f[:0]) if what == "no faces" else (v[:0], f)
    for depth, face in _check(v, f, [_orbit(0, 2), _orbit(1, 2, size=(9, 17))]):
        assert (depth == 0).all() and (face == -1).all()


# ---------------------------------------------------------------- face counts, box sizes ----
@pytest.mark.parametrize("F", [1, 63, 64, 65])
def test_face_counts_around_a_wave(F):
    v, f = orc.soup(F, seed=F, lo=(0.6, 0.6, -0.1), hi=(1.4, 1.4, 0.3), extent=0.4)
    (depth, face), = _check(v, f, [_orbit(0, 1)])
    assert (depth > 0).any() and face.max() <= F - 1


def test_seventy_thousand_faces_are_many_workgroups():
    v, f, _ = meo.wavy_wall(188, 188, seed=6)
    assert len(f) == 69_938
    (depth, face), (d2, _) = _check(v, f, [_orbit(0, 2), _orbit(1, 2, size=(30, 40))])
    assert (depth > 0).sum() > 1000 and len(np.unique(face)) > 1000 and (d2 > 0).any()


def test_boxes_at_the_wave_path_threshold():
    """Boxes of one pixel fewer than, exactly and one more than the threshold between the two walks, side by side and alone."""
    def tri(x0, x1, y0, y1, z):
        return [[x0, y0, z], [x1, y0, z], [x0, y1, z]]
    v = np.array(tri(1.5, 6.5, 1.5, 4.5, 1.0) + tri(8.5, 12.5, 1.5, 5.5, 2.0) + tri(0.5, 17.5, 5.8, 7.4, 3.0), F32)      # 5 x 3, 4 x 4, 17 x 2 - ...
    v[:, :2] *= v[:, 2:3]      # u = px / pz
    f = np.arange(9, dtype=np.int32).reshape(3, 3)
    view = _axis((8, 24))
    box = orc.face_boxes(v, f, view)
    pixels = ((box["i1"] - box["i0"] + 1) * (box["j1"] - box["j0"] + 1)).tolist()
    assert pixels == [LANE_PIXELS - 1, LANE_PIXELS, 17 * 2] and box["ok"].all()
    v[6:, 1] = np.array([5.8, 5.8, 6.4], F32) * F32(3.0)      # the third box one row high: 17 pixels
    box = orc.face_boxes(v, f, view)
    assert ((box["i1"] - box["i0"] + 1) * (box["j1"] - box["j0"] + 1)).tolist() == [LANE_PIXELS - 1, LANE_PIXELS, LANE_PIXELS + 1]
    (depth, face), = _check(v, f, [view])
    assert set(np.unique(face)) == {-1, 0, 1, 2}
    for k in range(3):
        (_, alone), = _check(v, f[k:k + 1], [view])
        assert np.array_equal(alone == 0, face == k)


def test_one_face_covers_the_image_and_several_lanes_hold_large_faces():
    big = np.array([[-200, -200, 2], [1750, -250, 2.5], [-300, 2100, 3]], F32)      # u = px / pz
    (depth, face), = _check(big, np.array([[0, 1, 2]], np.int32), [_axis((48, 64))])
    assert (face == 0).all() and depth.min() >= 2 and depth.max() <= 3
    # a wave of 64 faces, every third one image-sized, the others a pixel or two
    small, _ = orc.soup(64, seed=5, lo=(0, 0, 1), hi=(60, 44, 2), extent=1.2)
    large, _ = orc.soup(64, seed=6, lo=(10, 10, 2), hi=(50, 40, 4), extent=40.0)
    small[:, 2], large[:, 2] = 1 + small[:, 2] % 1, 2 + large[:, 2] % 2      # all in front of the camera
    v = np.where((np.arange(64) % 3 == 0).repeat(3)[:, None], large, small).astype(F32)
    f = np.arange(192, dtype=np.int32).reshape(64, 3)
    box = orc.face_boxes(v, f, _axis((48, 64)))
    n = (box["i1"] - box["i0"] + 1) * (box["j1"] - box["j0"] + 1) * box["ok"]
    assert (n > LANE_PIXELS).sum() >= 15 and ((n > 0) & (n <= LANE_PIXELS)).sum() >= 15
    (depth, face), = _check(v, f, [_axis((48, 64))])
    assert len(np.unique(face)) > 20


# ---------------------------------------------------------------- dropped faces, limits, ties ----
def test_dropped_faces_leave_every_other_face_alone():
    """Indices of -1 and V, a NaN and an infinite vertex, a zero-area face, a face behind the camera, one crossing depth_min."""
    view = _axis((8, 8), depth_min=0.75)
    v = np.array([[2, 2, 1], [6, 2, 1], [2, 6, 1], [np.nan, 0, 1], [0, 0, -1], [3, 3, 0.5], [0, np.inf, 1], [5, 5, -2], [1, 6, -2]], F32)
    good = np.array([[0, 1, 2]], np.int32)
    f = np.array([[0, 1, 9], [3, 1, 2], [0, 1, 2], [0, 2, 1], [-1, 1, 2], [0, 1, 1], [0, 4, 2], [4, 5, 2], [6, 1, 2], [4, 7, 8], [2 ** 31 - 1, 0, 1],
                  [0, 1, 5]], np.int32)
    (alone, _), = _check(v, good, [view])
    (depth, face), = _check(v, f, [view])
    assert np.array_equal(_bits(depth), _bits(alone)) and set(np.unique(face)) == {-1, 2} and (depth > 0).sum() == 15


def _down(x):
    return np.nextafter(F32(x), F32(-np.inf))


@pytest.mark.parametrize("limit", ["depth_trunc", "depth_min"])
def test_depths_on_and_an_ulp_either_side_of_a_limit(limit):
    """Three flat faces side by side whose depths are three consecutive floats, with the limit on the middle one."""
    c = F32(1.5)
    zs = [_down(c), c, cpu._up(c)]
    v = np.array([[x, y, z] for k, z in enumerate(zs) for x, y in ((1 + 7 * k, 1), (6 + 7 * k, 1), (1 + 7 * k, 6))], F32)
    v[:, :2] *= v[:, 2:3]      # u = px / pz: back onto the pixel grid (up to rounding, which the mirror shares)
    f = np.arange(9, dtype=np.int32).reshape(3, 3)
    (base, _), = _check(v, f, [_axis((8, 24))])
    values = np.unique(base[base > 0])
    m = values[len(values) // 2]
    assert len(values) >= 3 and _down(m) in values and cpu._up(m) in values      # zp on the limit and one ulp either side of it
    (depth, face), = _check(v, f, [_axis((8, 24), **{limit: float(m)})])
    if limit == "depth_trunc":      # zp <= depth_trunc: on it stays, one ulp beyond goes
        assert np.array_equal(depth > 0, (base > 0) & (base <= m)) and (depth == m).any()
    else:                           # zp > depth_min, and a face with a vertex at or in front of it goes whole
        assert (depth > 0).any() and (base[depth > 0] > m).all() and not (depth == m).any() and (depth[depth > 0] == base[depth > 0]).all()


def test_ties_and_the_nearer_of_two_squares():
    v, f = meo.unit_square(z=2.0)
    v[:, :2] = v[:, :2] * 8 + 3
    both = np.concatenate([f, f])      # faces 2 and 3 coincide with 0 and 1
    (depth, face), = _check(v, both, [_axis((16, 16), f=2.0)])
    assert (depth > 0).any() and set(np.unique(face)) <= {-1, 0, 1}
    (_, swapped), = _check(v, both[[2, 1, 0, 3]], [_axis((16, 16), f=2.0)])
    assert set(np.unique(swapped)) <= {-1, 0, 1}
    (v0, f0), (v1, f1) = meo.unit_square(z=3.0), meo.unit_square(z=2.0)      # the far one first in the list
    v0[:, :2] *= 2
    v1[:, :2] = v1[:, :2] * 0.5 + 0.25
    v2, f2 = np.concatenate([v0, v1]), np.concatenate([f0, f1 + 4])
    (depth, face), = _check(v2, f2, [_axis((32, 32), f=40.0, c=-4.0)])
    near = np.isin(face, (2, 3))
    assert near.sum() > 20 and np.isin(face, (0, 1)).sum() > 20 and (np.abs(depth[near] - 2) < 1e-5).all()
    (solo, _), = _check(v1, f1, [_axis((32, 32), f=40.0, c=-4.0)])
    assert np.array_equal(solo > 0, near)      # the nearer square wins everywhere it covers


# ---------------------------------------------------------------- watertightness ----
@pytest.mark.parametrize("scene", ["wall", "fan"])
def test_watertight_on_the_device(scene):
    if scene == "fan":
        v, f, view = cpu.fan_scene()
    else:
        (v, f), view = cpu._scene("wall"), cpu._camera((48, 64))
    (depth, face), = _check(v, f, [view])
    inside = orc.erode(orc.render(v, f, view, np.float64)[0] > 0)
    assert inside.sum() >= 16 and (depth[inside] > 0).all()


# ---------------------------------------------------------------- what it means ----
def _two_squares():
    import test_gpu_mesh_cull as base
    return base._two_squares()


def test_two_parallel_squares_cull_against_their_own_depth():
    """No depth plane anywhere: the far square goes but for its rim, which the near one does not shadow; the near one stays whole."""
    from lvdgs import mesh_eval
    v, f, n_front, (R, T), intr, size, _ = _two_squares()
    view = mco.view(R, T, intr, size=size)
    kept, record = mesh_eval.cull_mesh(_mesh(v, f), views=[_device_view(view)], occlusion_eps=0.05, want_origin=True, occlusion="self")
    depth, _ = orc.render(v, f, view)
    want = mco.cull(v, f, mco.visibility(v, [dict(view, depth=depth)], 0.05))
    origin = record["vertex_origin"].cpu().numpy()
    assert np.array_equal(origin, want["vertex_origin"]) and np.array_equal(kept.faces.cpu().numpy(), want["faces"])
    assert np.array_equal(_bits(kept.vertices.cpu().numpy()), _bits(want["vertices"]))
    assert (origin[:n_front] == np.arange(n_front)).all()      # the front square whole
    back = v[origin[n_front:]]
    assert len(back) > 0 and (back[:, 2] == 1.0).all()
    assert not ((np.abs(back[:, 0] - 0.5) < 0.7) & (np.abs(back[:, 1] - 0.5) < 0.7)).any()      # the shadow: |x - 0.5| <= 0.75 at depth 3
    frustum, whole = mesh_eval.cull_mesh(_mesh(v, f), views=[_device_view(view)])
    assert whole["faces"] == len(f) > record["faces"]      # which the frustum alone had kept
    with pytest.raises(_lib.LvdgsError, match="occlusion"):
        mesh_eval.cull_mesh(_mesh(v, f), views=[_device_view(view)], occlusion="other")
    with pytest.raises(_lib.LvdgsError, match="size"):
        mesh_eval.render_depth(_mesh(v, f), [{k: x for k, x in _device_view(view).items() if k != "size"}])


def test_a_camera_turned_away_keeps_nothing():
    from lvdgs import mesh_eval
    v, f, _, _, intr, size, _ = _two_squares()
    R, T = mco.look_at((0.5, 0.5, -2.0), (0.5, 0.5, -4.0))
    view = _device_view(mco.view(R, T, intr, size=size))
    kept, record = mesh_eval.cull_mesh(_mesh(v, f), views=[view], occlusion_eps=0.05, occlusion="self")
    assert (record["vertices"], record["faces"]) == (0, 0) and kept.faces.shape == (0, 3)
    assert all((d == 0).all() for d in mesh_eval.render_depth(_mesh(v, f), [view]))


# ---------------------------------------------------------------- the system ----
def _toy():
    import test_gpu_mesh_cull as cull
    import test_gpu_mesh_eval as base      # its run of the toy sequence, made once for all three files
    return base._toy_run(), base._count_waits_and_reads, cull._bounds


def _mirror_views(views):
    return [mco.view(v["R"].cpu().numpy(), v["T"].cpu().numpy(), v["intrinsics"], size=v["size"], depth_trunc=v["depth_trunc"]) for v in views]


def test_eval_mesh_defaults_are_key_for_key_what_they_are():
    (seq, voxel), _, _ = _toy()
    score, record = seq.eval_mesh(voxel, n_samples=5000)
    again, record2 = seq.eval_mesh(voxel, n_samples=5000, cull=None, depth_l1=False)
    assert again == score and record2 == record
    assert sorted(record) == ["est", "est_depth", "gt", "n_samples", "seed", "seed_gt", "threshold", "voxel_size"]
    assert "cull" not in record["est"] and "depth_l1" not in record
    with pytest.raises(ValueError, match="cull"):
        seq.eval_mesh(voxel, cull="self")


def test_eval_mesh_culls_both_meshes_against_their_own_depth():
    """The ground truth carries a second copy of its surface behind the first, as the first keyframe sees it (every vertex pushed away
    from that camera along its ray): occlusion culling at that frame removes the copy, without any dataset depth."""
    from lvdgs.tsdf import Mesh, TsdfVolume
    (seq, voxel), count, _bounds = _toy()
    bounds = _bounds(seq, voxel)
    kf = seq.kf_indices[0]
    truth = TsdfVolume.from_bounds(bounds[0], bounds[1], voxel, color=False, device=DEV)
    seq._fuse_dataset_depth(truth, [kf], "gt", None)
    fused = truth.extract_mesh()
    cam = seq.cameras[kf]
    Rg, Tg = cam.R_gt.detach().to(DEV, torch.float32), cam.T_gt.detach().to(DEV, torch.float32)
    centre = -(Rg.T @ Tg)
    nearest = float((fused.vertices @ Rg.T + Tg)[:, 2].min())
    assert nearest > 0
    scale = 1.0 + max(1.0, 3.0 * 4.0 * truth.voxel_size / nearest)      # the copy lies three culling margins or more behind its original
    gt_mesh = Mesh(torch.cat([fused.vertices, centre + scale * (fused.vertices - centre)]).contiguous(), None,
                   torch.cat([fused.faces, fused.faces + fused.vertices.shape[0]]).contiguous())
    saved, held = seq.dataset.depths, {i: c.depth for i, c in seq.cameras.items()}
    out = []
    try:
        seq.dataset.depths = None      # a dataset without metric depth
        for c in seq.cameras.values():
            c.depth = None
        seq.eval_mesh(voxel, bounds=bounds, frames=[kf], n_samples=3000, gt_mesh=gt_mesh, cull="occlusion", depth_l1=True)      # (allocations)
        c0 = count(lambda: out.append(seq.eval_mesh(voxel, bounds=bounds, frames=[kf], n_samples=3000, gt_mesh=gt_mesh, cull="occlusion")))
        kept_est, kept_gt = seq.last_eval_meshes
        c1 = count(lambda: out.append(seq.eval_mesh(voxel, bounds=bounds, frames=[kf], n_samples=3000, gt_mesh=gt_mesh, cull="occlusion",
                                                    depth_l1=True)))
    finally:
        seq.dataset.depths = saved
        for i, c in seq.cameras.items():
            c.depth = held[i]
    (score, record), (score1, record1) = out
    print("culled", score, record, "\nwith depth L1", record1, "\nwaits", c0, c1)
    # the waits of cull="visible" (tests/test_gpu_mesh_cull.py): the estimate's mesh, one per culled mesh, the score; the depth L1 adds one
    assert (c0["wait"], c0["sync"], c0["read"]) == (3, 4, 0), c0
    assert (c1["wait"], c1["sync"], c1["read"]) == (3, 5, 0), c1
    eps = 4 * record["voxel_size"]
    for name in ("est", "gt"):
        r = record[name]
        assert 0 < r["faces"] <= r["faces_before"] and r["cull"] == "occlusion" and r["cull_eps"] == eps
    assert record["gt"]["faces_before"] == 2 * fused.faces.shape[0] and record["gt"]["faces"] <= fused.faces.shape[0]      # the copy is gone
    assert score1 == score and {k: x for k, x in record1.items() if not k.startswith("depth_l1")} == record

    # the culled ground truth is the mirror's, bit for bit
    dev = torch.device(DEV, torch.cuda.current_device())
    gt_views = _mirror_views(seq._frame_views([kf], "gt", None, dev, depth=None))
    gv, gf = gt_mesh.vertices.cpu().numpy(), gt_mesh.faces.cpu().numpy()
    rendered = [dict(v, depth=orc.render(gv, gf, v)[0]) for v in gt_views]
    want = mco.cull(gv, gf, mco.visibility(gv, rendered, eps))
    assert np.array_equal(_bits(kept_gt.vertices.cpu().numpy()), _bits(want["vertices"])) and np.array_equal(kept_gt.faces.cpu().numpy(), want["faces"])
    assert (want["face_origin"] < fused.faces.shape[0]).all() and len(want["faces"]) == record["gt"]["faces"]

    # the depth L1 is the mirror's planes through the same statements on the CPU
    from lvdgs import mesh_eval
    est_views = _mirror_views(seq._frame_views([kf], "estimated", None, dev, depth=None))
    ev, ef = kept_est.vertices.cpu().numpy(), kept_est.faces.cpu().numpy()
    total, pixels = mesh_eval.depth_l1_terms(torch.from_numpy(orc.render(ev, ef, est_views[0])[0]),
                                             torch.from_numpy(orc.render(want["vertices"], want["faces"], gt_views[0])[0]), None)
    assert int(pixels) == record1["depth_l1_pixels"] > 100
    assert record1["depth_l1"] == pytest.approx(float(total) / int(pixels), rel=1e-12) and 0 < record1["depth_l1"] < math.inf
    d_est, d_gt = seq.last_eval_depths
    assert np.array_equal(_bits(d_gt[0].cpu().numpy()), _bits(orc.render(want["vertices"], want["faces"], gt_views[0])[0]))


def test_depth_l1_of_a_mesh_against_itself_is_zero():
    (seq, voxel), _, _bounds = _toy()
    bounds = _bounds(seq, voxel)
    saved = {i: (cam.R.clone(), cam.T.clone()) for i, cam in seq.cameras.items()}
    try:
        for cam in seq.cameras.values():      # the estimated poses are the true ones: both meshes are rendered from the same cameras
            cam.update_RT(cam.R_gt.to(cam.R.dtype), cam.T_gt.to(cam.T.dtype))
        seq.eval_mesh(voxel, bounds=bounds, n_samples=2000)
        own = seq.last_eval_meshes[0]
        _, record = seq.eval_mesh(voxel, bounds=bounds, n_samples=2000, gt_mesh=own, depth_l1=True)
    finally:
        for i, cam in seq.cameras.items():
            cam.update_RT(*saved[i])
    assert record["depth_l1"] == 0.0 and record["depth_l1_pixels"] > 100 * len(seq.kf_indices)
