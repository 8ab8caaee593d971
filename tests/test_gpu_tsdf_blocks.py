"""``lvdgs_tsdf_blocks_*`` through ``lvdgs.tsdf_blocks`` on the GPU against the float32 mirrors of tests/tsdf_blocks_oracle.py and
against the dense volume (``lvdgs.tsdf``) on the same lattice.

Held to include/lvdgs.h: the set of blocks, weights, counts and faces exact; tsdf, colours and vertices BIT FOR BIT (both sides evaluate
the header's float32 expressions as written; no tolerance is in use anywhere below).  Scenes: voxels of 0.1 m, frames of 40 x 30
pixels, at most 64 blocks.  Pool order is not part of the contract: everything is compared in key order.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import tsdf_blocks_oracle as borc
import tsdf_cases as cases
import tsdf_oracle as orc
from lvdgs import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
VS, H, W = 0.1, 30, 40
ORIGIN = np.array([-1.6, -1.6, -1.6], np.float32)      # every scene below allocates blocks at non-negative coordinates from here
CENTRE = np.array([0.43, 0.31, 0.22])


# ---------------------------------------------------------------- scenes (NumPy) ----
def wavy_view(eye, seed, base, intrinsics=(34.0, 33.0, 19.7, 14.3), color=True, amplitude=0.25, **kw):
    """A camera at CENTRE + eye looking at CENTRE over a wavy depth map around ``base`` with zero patches and noise."""
    rng = np.random.default_rng(seed)
    vi, ui = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    d = base + amplitude * np.sin(ui / 6.0 + seed) * np.cos(vi / 5.0 - seed) + 0.01 * rng.standard_normal((H, W))
    d[rng.random((H, W)) < 0.05] = 0.0
    d[4:8, 22:31] = 0.0
    R, T = cases.look_at(CENTRE + np.asarray(eye), CENTRE, up=(0.0, 1.0, 0.0))
    image = rng.random((3, H, W)).astype(np.float32) * 1.2 - 0.1 if color else None
    return orc.make_view(d.astype(np.float32), R, T, intrinsics, image=image, **kw)


@functools.lru_cache(maxsize=None)
def general_views(color=True):
    """Three views: a mask and a depth_trunc that cuts the far pixels; a depth_min inside the band and a depth map with values past
    depth_trunc; one without an image."""
    rng = np.random.default_rng(11)
    a = wavy_view((0.1, -0.05, -1.3), 1, 1.3, color=color, mask=rng.random((H, W)) > 0.2, depth_trunc=1.45)
    b = wavy_view((-1.2, 0.2, -0.4), 2, 1.25, color=color, depth_min=1.0, depth_trunc=1.6)
    c = wavy_view((0.3, 0.9, -0.9), 3, 1.3, color=False)
    return [a, b, c]


@functools.lru_cache(maxsize=None)
def layered_views():
    """A far surface first, then two near ones in front of it from the same camera: the near blocks lie in the far view's free space.
    30 blocks."""
    eye = (0.1, -0.05, -1.3)
    return [wavy_view(eye, 1, 1.9, amplitude=0.1), wavy_view(eye, 2, 1.0, amplitude=0.1), wavy_view(eye, 3, 1.05, amplitude=0.1, color=False)]


def plane_views():
    """A fronto-parallel plane 1.2 m in front of a camera that looks along +z: footprint 1.2 / 40 = 0.3 voxels."""
    R, T = np.eye(3, dtype=np.float32), -np.array([0.413, 0.307, -0.9], np.float32)
    return [orc.make_view(np.full((H, W), 1.2137, np.float32), R, T, (40.0, 40.0, 19.3, 14.7))]


def near_plane_views():
    """The plane at 0.71 m: 13 blocks, for a pool that cannot hold them and a table of 16 slots that can."""
    R, T = np.eye(3, dtype=np.float32), -np.array([0.413, 0.307, -0.3], np.float32)
    return [orc.make_view(np.full((H, W), 0.7137, np.float32), R, T, (40.0, 40.0, 19.3, 14.7))]


@functools.lru_cache(maxsize=None)
def sphere_views():
    """A sphere of radius 0.45 m at CENTRE from six axis views at 2 m, f = 70: footprint 1.55 / 70 = 0.22 voxels at the surface."""
    views = []
    for axis in range(3):
        for sign in (-1.0, 1.0):
            cam = CENTRE.copy()
            cam[axis] += sign * 2.0
            cam += np.array([0.0137, -0.0091, 0.0113])
            views.append(cases.sphere_view(cam, CENTRE, 0.45, (70.0, 70.0, 19.3, 14.7), H, W, far=None))
    return views


def mirror_for(calls, origin=ORIGIN, color=True, from_zero=True, **kw):
    """The mirror fed ``calls`` (lists of views), over the box of everything they allocate (from block 0 when ``from_zero``)."""
    m = borc.BlockMirror.around(origin, VS, [v for call in calls for v in call], color=color, **kw)
    if from_zero:
        assert min(m.lo) >= 0
        m = borc.BlockMirror(origin, VS, (0, 0, 0), tuple(l + n for l, n in zip(m.lo, m.nb)), color=color, **kw)
    for call in calls:
        m.integrate_blocks_f32(call)
    return m


# ---------------------------------------------------------------- the device side ----
def device_view(v):
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return dict(depth=t(v["depth"]), R=t(v["R"]), T=t(v["T"]), intrinsics=v["intrinsics"], image=t(v["image"]), mask=t(v["mask"]),
                depth_min=v["depth_min"], depth_trunc=v["depth_trunc"])


def device_volume(calls=(), origin=ORIGIN, pool=64, color=True, **kw):
    from lvdgs.tsdf_blocks import TsdfBlockVolume
    tv = TsdfBlockVolume(origin, VS, pool, color=color, **kw)
    for call in calls:
        tv.integrate_views([device_view(v) for v in call])
    return tv


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def names(color):
    return orc.PLANES[:5 if color else 2]


def assert_holds(tv, mirror, keys=None, what=""):
    """``blocks()`` is the mirror's key set and every plane of every block the mirror's, bit for bit."""
    keys = np.sort(mirror.keys if keys is None else keys)
    assert np.array_equal(tv.blocks().cpu().numpy(), borc.unpack_keys(keys)), what
    for name in names(tv.color):
        got, want = tv.block_planes(name).cpu().numpy(), mirror.block_planes(name, keys)
        bad = bits(got) != bits(want)
        assert not bad.any(), (what, name, int(bad.sum()), float(np.abs(got[bad] - want[bad]).max()))


def assert_mesh_is(mesh, want):
    v, c, f = want
    assert mesh.vertices.shape[0] == len(v) and mesh.faces.shape[0] == len(f)
    assert np.array_equal(mesh.faces.cpu().numpy(), f)
    assert np.array_equal(bits(mesh.vertices.cpu().numpy()), bits(v))
    if c is None:
        assert mesh.colors is None
    else:
        assert np.array_equal(bits(mesh.colors.cpu().numpy()), bits(c))


def mesh_sets(mesh):
    return borc.mesh_as_sets(mesh.vertices.cpu().numpy(), None if mesh.colors is None else mesh.colors.cpu().numpy(), mesh.faces.cpu().numpy())


# ---------------------------------------------------------------- integration ----
@pytest.mark.parametrize("color", [True, False])
def test_blocks_and_planes_against_the_mirror_and_the_dense_volume(color):
    from lvdgs.tsdf import TsdfVolume
    views = general_views(color)
    mirror = mirror_for([views], color=color)
    assert 12 <= len(mirror.keys) <= 64
    tv = device_volume([views], color=color)
    assert_holds(tv, mirror)
    s = tv.stats()
    assert s == dict(blocks=len(mirror.keys), dropped=0, out_of_range=0, table_full=False) and tv.frames == 3
    # the dense kernel on the same lattice, fed the same views: equal on every sample of an allocated block
    mine = tv.to_dense()
    assert mine.origin == tuple(float(o) for o in ORIGIN) and mine.index_offset == (0, 0, 0)
    dense = TsdfVolume(ORIGIN, VS, mine.dims, color=color)
    dense.integrate_views([device_view(v) for v in views])
    assert mine.dims == mirror.vol["dims"]
    keep = torch.from_numpy(mirror.allocated_samples()).to(DEV)
    for name in names(color):
        a, b = mine.plane(name)[keep], dense.plane(name)[keep]
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), name
        assert not mine.plane(name)[~keep].any()
    assert (mine.plane("weight")[keep] > 0).sum() > 2000


def test_three_views_in_one_call_and_in_three_calls():
    """A block that a later call allocates starts from zero at that call: the two differ, and each is its own mirror."""
    views = layered_views()
    one, three = mirror_for([views]), mirror_for([[v] for v in views])
    assert np.array_equal(one.keys, three.keys) and len(one.keys) <= 64
    assert ((one.vol["weight"] == 3.0) & (three.vol["weight"] < 3.0)).sum() > 200
    assert_holds(device_volume([views]), one, what="one call")
    assert_holds(device_volume([[v] for v in views]), three, what="three calls")


def test_nineteen_views_in_chunks():
    views = [wavy_view((0.1 + 0.01 * n, -0.05, -1.3 + 0.005 * n), 1, 1.3 + 0.002 * n, color=(n % 3 != 2)) for n in range(19)]
    mirror = mirror_for([views[:16], views[16:]])
    assert len(mirror.keys) <= 64
    tv = device_volume([views])
    assert_holds(tv, mirror)
    assert tv.frames == 19 and float(tv.block_planes("weight").max()) == float(mirror.vol["weight"].max()) > 16.0


def test_a_second_call_allocates_beside_blocks_that_hold_state():
    first, second = [general_views()[0]], [general_views()[1]]
    mirror = mirror_for([first])
    before = mirror.keys.copy()
    new = mirror.integrate_blocks_f32(second)
    assert len(np.setdiff1d(new, before)) >= 2 and len(np.intersect1d(new, before)) >= 4
    assert mirror.vol["weight"].max() == 2.0
    tv = device_volume([first])
    assert tv.stats()["blocks"] == len(before)
    tv.integrate_views([device_view(v) for v in second])
    assert_holds(tv, mirror)


def test_the_weight_cap():
    view = general_views()[1]
    mirror = mirror_for([[view] * 3, [view] * 2], max_weight=3.0)
    tv = device_volume([[view] * 3, [view] * 2], max_weight=3.0)
    assert_holds(tv, mirror)
    assert float(tv.block_planes("weight").max()) == 3.0


def test_negative_block_coordinates():
    origin = np.array([2.1, 1.8, 2.1], np.float32)
    views = general_views()
    mirror = mirror_for([views], origin=origin, from_zero=False)
    assert max(l + n for l, n in zip(mirror.lo, mirror.nb)) <= 0 and len(mirror.keys) <= 64
    tv = device_volume([views], origin=origin)
    assert_holds(tv, mirror)
    assert int(tv.blocks().max()) < 0
    dense = tv.to_dense()      # its box starts at the lowest block: the same samples at shifted indices
    assert dense.index_offset == tuple(8 * l for l in mirror.lo)
    assert dense.dims == mirror.vol["dims"]
    for name in orc.PLANES:      # (the mirror's box is the blocks' bounding box too; outside the allocated blocks both hold zeros)
        assert np.array_equal(bits(dense.plane(name).cpu().numpy().reshape(-1)), bits(mirror.vol[name])), name


def test_a_pose_with_a_nan_allocates_nothing_and_is_counted():
    view = dict(general_views()[2])
    view["T"] = np.array([np.nan, 0.0, 1.0], np.float32)
    keys, outside = borc.allocation_keys_f32(ORIGIN, VS, 4 * VS, [view])
    assert len(keys) == 0 and outside > 10000
    tv = device_volume([[view]])
    assert tv.stats() == dict(blocks=0, dropped=0, out_of_range=outside, table_full=False)
    assert tv.blocks().shape == (0, 3) and not tv.planes.any()


# ---------------------------------------------------------------- capacity of the pool and the table ----
def test_a_pool_of_eight_drops_the_rest_and_grows():
    views = near_plane_views()
    full = mirror_for([views], color=False)
    n = len(full.keys)
    assert 12 <= n <= 16      # all of them fit the 16 slots: the dropped count is exact
    tv = device_volume([views], pool=8, color=False)
    assert (tv.pool_blocks, tv.table_slots) == (8, 16)
    assert tv.stats() == dict(blocks=8, dropped=n - 8, out_of_range=0, table_full=False)
    got = borc.pack_keys(tv.blocks().cpu().numpy())
    assert len(got) == 8 and np.isin(got, full.keys).all()
    part = borc.BlockMirror(ORIGIN, VS, (0, 0, 0), full.nb, color=False)
    part.integrate_blocks_f32(views, keys=got)
    assert_holds(tv, part, what="the eight blocks")
    mesh = tv.extract_mesh()
    assert_mesh_is(mesh, part.mesh_blocks_f32())
    assert tv.last_stats == dict(blocks=8, dropped=n - 8, out_of_range=0, table_full=False)
    tv.integrate_views([device_view(v) for v in views])      # the dropped keys stay in the table: counted once
    assert tv.stats()["dropped"] == n - 8
    tv.grow(64)
    assert (tv.pool_blocks, tv.table_slots) == (64, 128) and tv.stats() == dict(blocks=8, dropped=0, out_of_range=0, table_full=False)
    assert np.array_equal(borc.pack_keys(tv.blocks().cpu().numpy()), np.sort(got))      # what it held, it holds
    tv.reset()
    tv.integrate_views([device_view(v) for v in views])
    assert_holds(tv, full, what="after grow, reset and the fusion again")
    assert_mesh_is(tv.extract_mesh(), full.mesh_blocks_f32())


def test_growing_keeps_the_planes_and_finds_the_neighbours():
    views = general_views()
    mirror = mirror_for([views])
    tv = device_volume([views])
    tv.grow(100)
    assert tv.table_slots == 256
    assert_holds(tv, mirror)
    assert_mesh_is(tv.extract_mesh(), mirror.mesh_blocks_f32())


def test_table_collisions():
    """30 keys in 64 slots: by the birthday bound several of them share a first slot and are found along a chain."""
    views = layered_views()
    mirror = mirror_for([views])
    assert len(mirror.keys) == 30
    tv = device_volume([views], pool=32)
    assert tv.table_slots == 64
    assert_holds(tv, mirror)
    assert_mesh_is(tv.extract_mesh(), mirror.mesh_blocks_f32())


# ---------------------------------------------------------------- extraction ----
def load_analytic(tv, mirror, sdf):
    """Overwrite what ``tv`` and ``mirror`` hold with tsdf = sdf(p) / trunc clipped, weight 1 and smooth colours, on the allocated blocks."""
    box = cases.analytic_volume(mirror.vol["dims"], sdf, voxel_size=VS, origin=ORIGIN, color=True)
    for name in orc.PLANES:
        mirror.vol[name] = box[name]
    keys = tv.block_key.cpu().numpy().view(np.uint64)[:tv.stats()["blocks"]]
    for name in orc.PLANES:
        getattr(tv, name).view(tv.pool_blocks, 8, 8, 8)[:len(keys)] = torch.from_numpy(mirror.block_planes_unsorted(name, keys)).to(DEV)


@functools.lru_cache(maxsize=None)
def sphere_blocks():
    m = mirror_for([sphere_views()])
    assert len(m.keys) <= 64
    return m


def blocks_around_a_corner(mirror):
    """A lattice corner whose eight blocks are all allocated, and two allocated blocks that are not adjacent."""
    have = {tuple(b) for b in borc.unpack_keys(mirror.keys)}
    corner = next(b for b in sorted(have) if all((b[0] - dx, b[1] - dy, b[2] - dz) in have for dx in (0, 1) for dy in (0, 1) for dz in (0, 1)))
    far = next((a, b) for a in sorted(have) for b in sorted(have) if max(abs(p - q) for p, q in zip(a, b)) >= 2)
    return corner, far


def extraction_case(name):
    if name == "plane":
        views = plane_views()
        return device_volume([views], color=False), mirror_for([views], color=False)
    if name == "sphere":
        return device_volume([sphere_views()]), mirror_for([sphere_views()])
    mirror = mirror_for([sphere_views()])
    tv = device_volume([sphere_views()])
    corner, (a, b) = blocks_around_a_corner(mirror)
    at = lambda block, inside: ORIGIN.astype(np.float64) + 0.8 * (np.asarray(block) + inside)
    if name == "corner":      # a blob about the point where eight blocks meet
        c = at(corner, 0.0) + np.array([0.013, -0.021, 0.017])
        sdf = lambda p: np.linalg.norm(p - c, axis=1) - 0.33
    else:                     # "blobs": one in the middle of each of two blocks that do not touch
        ca, cb = at(a, 0.5) + 0.011, at(b, 0.5) - 0.013
        sdf = lambda p: np.minimum(np.linalg.norm(p - ca, axis=1) - 0.27, np.linalg.norm(p - cb, axis=1) - 0.31)
    load_analytic(tv, mirror, sdf)
    return tv, mirror


@pytest.mark.parametrize("name", ["plane", "sphere", "blobs", "corner"])
def test_extraction_against_the_mirror_and_the_dense_extraction(name):
    tv, mirror = extraction_case(name)
    want = mirror.mesh_blocks_f32()
    assert len(want[0]) > 80 and len(want[2]) > 100
    mesh = tv.extract_mesh()
    assert tv.last_counts == (len(want[0]), len(want[2]))
    assert_mesh_is(mesh, want)
    again = tv.extract_mesh()      # sized by the first call's counts this time: the same bytes
    for a, b in zip(mesh, again):
        assert (a is None and b is None) or torch.equal(a, b)
    assert mesh_sets(mesh) == mesh_sets(tv.to_dense().extract_mesh())
    if name == "corner":      # the surface does cross the corner: vertices in all eight blocks
        cells = borc.active_cells(mirror.masked_volume()) // 8
        assert len({tuple(c) for c in cells}) >= 8


def raw_mesh(tv, vcap, fcap, pad=64):
    """One ``lvdgs_tsdf_blocks_mesh`` call into buffers with ``pad`` sentinel rows behind each capacity -> (buffers, block words)."""
    from lvdgs import tsdf_blocks
    L = _lib.lib()
    block, scratch = tsdf_blocks._mesh_call.resources(tv.device, _lib.TSDF_BLOCKS_HOST_BYTES, L.lvdgs_tsdf_blocks_mesh_scratch_bytes(tv.pool_blocks))
    order = tv._order().to(torch.int32)
    vertices = torch.full((vcap + pad, 3), -7.5, dtype=torch.float32, device=DEV)
    colors = torch.full((vcap + pad, 3), -7.5, dtype=torch.float32, device=DEV)
    faces = torch.full((fcap + pad, 3), -77, dtype=torch.int32, device=DEV)
    a = _lib.TsdfBlocksMeshArgs(vol=tv._vol, vertex_capacity=vcap, face_capacity=fcap, cell_lo=(C.c_int32 * 3)(*[-2 ** 31] * 3),
                                cell_hi=(C.c_int32 * 3)(*[2 ** 31 - 1] * 3), order=order.data_ptr(), vertices=vertices.data_ptr(),
                                colors=colors.data_ptr(), faces=faces.data_ptr(), host_state=block.data_ptr(), scratch=scratch.data_ptr(),
                                scratch_bytes=scratch.numel())
    words = tsdf_blocks._mesh_call.run(tv.device, a).copy()
    return (vertices, colors, faces), words


def test_capacity_overflow_reports_exact_counts_and_writes_nothing_behind():
    tv, mirror = extraction_case("sphere")
    v, c, f = mirror.mesh_blocks_f32()
    for vcap, fcap, bit in ((len(v) // 3, len(f), _lib.TSDF_OVERFLOW_VERTICES), (len(v), len(f) // 3 + 1, _lib.TSDF_OVERFLOW_FACES),
                            (0, 0, _lib.TSDF_OVERFLOW_VERTICES | _lib.TSDF_OVERFLOW_FACES)):
        (gv, gc, gf), words = raw_mesh(tv, vcap, fcap)
        assert (int(words[_lib.TSDF_BLOCKS_N_VERTICES]), int(words[_lib.TSDF_BLOCKS_N_FACES])) == (len(v), len(f))
        assert int(words[_lib.TSDF_BLOCKS_OVERFLOW]) == bit and int(words[_lib.TSDF_BLOCKS_USED]) == len(mirror.keys)
        assert bool((gv[vcap:] == -7.5).all()) and bool((gc[vcap:] == -7.5).all()) and bool((gf[fcap:] == -77).all())
        assert np.array_equal(bits(gv[:vcap].cpu().numpy()), bits(v[:vcap])) and np.array_equal(gf[:fcap].cpu().numpy(), f[:fcap])
    (gv, gc, gf), words = raw_mesh(tv, len(v), len(f))      # the retry, sized by the counts
    assert int(words[_lib.TSDF_BLOCKS_OVERFLOW]) == 0
    assert np.array_equal(bits(gv[:len(v)].cpu().numpy()), bits(v)) and np.array_equal(gf[:len(f)].cpu().numpy(), f)
    assert bool((gv[len(v):] == -7.5).all()) and bool((gf[len(f):] == -77).all())
    assert_mesh_is(tv.extract_mesh(vertex_capacity=10, face_capacity=10), (v, c, f))      # the wrapper retries by itself


def test_the_empty_volume():
    tv = device_volume()
    assert tv.stats() == dict(blocks=0, dropped=0, out_of_range=0, table_full=False)
    assert tv.blocks().shape == (0, 3) and tv.block_planes("tsdf").shape == (0, 8, 8, 8)
    mesh = tv.extract_mesh()
    assert mesh.vertices.shape == (0, 3) and mesh.faces.shape == (0, 3) and tv.last_counts == (0, 0)
    with pytest.raises(_lib.LvdgsError, match="holds no block"):
        tv.to_dense()
    with pytest.raises(_lib.LvdgsError, match="no CPU path"):
        tv.integrate(**{**device_view(general_views()[0]), "depth": torch.zeros(H, W)})


def test_two_volumes_fed_the_same_calls_agree():
    calls = [[general_views()[0]], general_views()[1:]]
    a, b = device_volume(calls), device_volume(calls)
    assert torch.equal(a.blocks(), b.blocks())
    for name in orc.PLANES:
        assert torch.equal(a.block_planes(name).view(torch.int32), b.block_planes(name).view(torch.int32)), name
    for x, y in zip(a.extract_mesh(), b.extract_mesh()):
        assert torch.equal(x, y)


def test_integrate_makes_no_wait_extract_mesh_one_and_stats_one():
    views = [device_view(v) for v in general_views()]
    tv = device_volume()
    tv.integrate_views(views)
    tv.extract_mesh()      # (the first call allocates the scratch and the pinned block, and learns the capacities)
    counts = {"wait": 0, "sync": 0, "read": 0}
    saved = [(_lib.HostCall, "wait", _lib.HostCall.wait), (torch.cuda, "synchronize", torch.cuda.synchronize),
             (torch.cuda.Stream, "synchronize", torch.cuda.Stream.synchronize), (torch.cuda.Event, "synchronize", torch.cuda.Event.synchronize),
             (torch.Tensor, "cpu", torch.Tensor.cpu), (torch.Tensor, "item", torch.Tensor.item), (torch.Tensor, "tolist", torch.Tensor.tolist)]

    def counting(kind, real):
        def f(*a, **k):
            counts[kind] += 1
            return real(*a, **k)
        return f

    def counted(fn):
        for k in counts:
            counts[k] = 0
        for owner, name, real in saved:
            setattr(owner, name, counting("wait" if owner is _lib.HostCall else "sync" if name == "synchronize" else "read", real))
        try:
            fn()
        finally:
            for owner, name, real in saved:
                setattr(owner, name, real)
        return dict(counts)

    assert counted(lambda: (tv.integrate_views(views), tv.integrate(**views[0]))) == {"wait": 0, "sync": 0, "read": 0}
    out = []
    assert counted(lambda: out.append(tv.extract_mesh())) == {"wait": 1, "sync": 1, "read": 0}      # (HostCall.wait is the one Stream.synchronize)
    assert out[0].faces.shape[0] > 100
    assert counted(lambda: out.append(tv.stats())) == {"wait": 0, "sync": 0, "read": 1}             # one blocking copy of the header
    assert out[1]["blocks"] > 10


def test_fuse_mesh_with_blocks_over_the_toy_sequence():
    """``SlamSequence.fuse_mesh(volume="blocks")`` gives the dense ``fuse_mesh``'s vertices and faces, as sets, when no block is dropped
    (the two lattices share the origin, so a vertex has the same bits in both)."""
    import os
    import random
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))
    import sequence_scene as ss
    from lvdgs.slam_sequence import SlamSequence
    cfg, ds, _, _, _ = ss.toy_sequence_on_cpu()
    torch.manual_seed(0)
    random.seed(0)
    seq = SlamSequence(cfg, ds.to("cuda"), ss.empty_map(cfg, "cuda"), ss.PIPE, torch.zeros(3, device="cuda"), idle_map_iters=2).run()
    g = seq.frontend_gaussians
    extent = float((g.get_xyz.detach().max(0).values - g.get_xyz.detach().min(0).values).max())
    voxel = extent / 48.0
    dense, dense_record = seq.fuse_mesh(voxel)
    sparse, record = seq.fuse_mesh(voxel, volume="blocks", pool_blocks=2048)
    print("dense", dense_record, "blocks", record)
    assert record["volume"] == "blocks" and record["dropped"] == 0 and 0 < record["blocks"] <= record["pool_blocks"]
    assert record["voxel_size"] == record["voxel_size_requested"] == voxel
    dv, df = mesh_sets(dense)
    sv, sf = mesh_sets(sparse)
    print("vertices", len(dv), len(sv), "only dense", len(dv - sv), "only blocks", len(sv - dv), "faces", len(df), len(sf))
    assert dv == sv and df == sf
