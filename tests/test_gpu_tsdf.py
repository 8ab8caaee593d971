"""``lvdgs_tsdf_integrate`` / ``lvdgs_tsdf_mesh`` through ``lvdgs.tsdf`` on the GPU against the float32 mirrors of tests/tsdf_oracle.py.

The kernels are held to include/lvdgs.h: weights, counts and faces exact, tsdf, colours and vertices BIT FOR BIT -- for the
integration on the voxels that are not fragile (tests/test_tsdf.py defines them; a fragile voxel may take another pixel or branch
in either float32 evaluation only if the two evaluations differ, which -ffp-contract=off and IEEE division rule out, so they are
compared too and merely reported).  Should bit equality ever not hold, the fallback is twice the float32-against-float64 difference
recorded in tests/test_tsdf.py (1.7e-6 for tsdf, 1.6e-7 for colours); it is not in use.
"""
import numpy as np
import pytest
import torch

import tsdf_cases as cases
import tsdf_oracle as orc
from lvdgs import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _device_volume(vol):
    """A ``TsdfVolume`` holding the planes of an oracle volume."""
    from lvdgs.tsdf import TsdfVolume
    tv = TsdfVolume(vol["origin"], vol["voxel_size"], vol["dims"], trunc=vol["trunc"], max_weight=vol["max_weight"], color="r" in vol)
    for name in orc.PLANES:
        if name in vol:
            getattr(tv, name).copy_(torch.from_numpy(vol[name]))
    return tv


def _device_view(v):
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return dict(depth=t(v["depth"]), R=t(v["R"]), T=t(v["T"]), intrinsics=v["intrinsics"], image=t(v["image"]), mask=t(v["mask"]),
                depth_min=v["depth_min"], depth_trunc=v["depth_trunc"])


def _planes(tv):
    return {name: getattr(tv, name).cpu().numpy() for name in orc.PLANES if hasattr(tv, name)}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _assert_planes_equal(got, want, keep=None, what=""):
    for name in orc.PLANES:
        if name in want:
            g, w = got[name], want[name]
            if keep is not None:
                g, w = g[keep], w[keep]
            bad = _bits(g) != _bits(w)
            assert not bad.any(), (what, name, int(bad.sum()), float(np.abs(g[bad] - w[bad]).max()))


@pytest.mark.parametrize("color", [True, False])
def test_integration_against_the_float32_mirror(color):
    case = cases.general_case(color)
    want = orc.copy_volume(case["vol"])
    touched = orc.integrate_f32(want, case["views"])
    _, fragile = orc.integrate_f64(orc.copy_volume(case["vol"], np.float64), case["views"])
    tv = _device_volume(case["vol"])
    tv.integrate_views([_device_view(v) for v in case["views"]])
    got = _planes(tv)
    assert touched.any(0).sum() > 5000 and not touched.any(0).all()
    assert np.array_equal(got["weight"], want["weight"])                          # exact, fragile voxels included
    _assert_planes_equal(got, want, ~fragile.any(0), "non-fragile")
    differing = sum(int((_bits(got[n]) != _bits(want[n])).sum()) for n in got)
    print("fragile voxels", int(fragile.any(0).sum()), "planes' elements that differ anywhere", differing)
    assert tv.frames == 3


def test_three_views_in_one_call_equal_three_calls():
    case = cases.general_case(True)
    views = [_device_view(v) for v in case["views"]]
    one, three = _device_volume(case["vol"]), _device_volume(case["vol"])
    one.integrate_views(views)
    for v in views:
        three.integrate(**v)
    assert torch.equal(one.planes.view(torch.int32), three.planes.view(torch.int32))
    assert float(one.weight.max()) == 3.0


def _stateful_volume(dims=(37, 22, 19), color=True, seed=11):
    vol = orc.empty_volume(dims, np.array([-1.41, -0.83, 0.21], np.float32), 0.08, trunc=0.3, color=color)
    rng = np.random.default_rng(seed)
    n = vol["tsdf"].size
    vol["weight"] = rng.integers(0, 5, n).astype(np.float32)
    vol["tsdf"] = np.where(vol["weight"] > 0, rng.uniform(-1, 1, n), 0).astype(np.float32)
    for name in "rgb" if color else "":
        vol[name] = rng.random(n).astype(np.float32)
    return vol


def test_a_view_of_one_corner_leaves_every_other_voxel_its_bytes():
    vol = _stateful_volume()
    dims, vs, origin = vol["dims"], vol["voxel_size"], vol["origin"].astype(np.float64)
    corner = origin + vs * (np.asarray(dims) - 1)
    H, W = 48, 64
    R, T = cases.look_at(corner + np.array([0.9, 0.7, 0.8]), corner + np.array([0.4, 0.3, 0.35]))
    rng = np.random.default_rng(2)
    view = orc.make_view(np.full((H, W), 1.35, np.float32), R, T, (150.0, 150.0, 31.7, 23.6), image=rng.random((3, H, W)).astype(np.float32))
    want = orc.copy_volume(vol)
    touched = orc.integrate_f32(want, [view])[0]
    assert 20 < touched.sum() < 0.05 * touched.size      # the corner and nothing but the corner
    tv = _device_volume(vol)
    tv.integrate(**_device_view(view))
    got = _planes(tv)
    _assert_planes_equal({k: v[~touched] for k, v in got.items()}, {k: v[~touched] for k, v in vol.items() if k in orc.PLANES}, what="skipped voxels")
    _assert_planes_equal(got, want, what="against the mirror")


def test_max_weight_caps_the_running_mean():
    case = cases.general_case(True)
    vol = orc.copy_volume(case["vol"])
    vol["max_weight"] = 3.0
    rng = np.random.default_rng(9)
    views = []
    for n in range(5):
        v = dict(case["views"][1])
        v["depth"] = (v["depth"] * np.float32(1.0 + 0.01 * n)).astype(np.float32)
        v["image"] = rng.random(v["image"].shape).astype(np.float32)
        views.append(v)
    want = orc.copy_volume(vol)
    orc.integrate_f32(want, views)
    tv = _device_volume(vol)
    tv.integrate_views([_device_view(v) for v in views])
    got = _planes(tv)
    assert want["weight"].max() == 3.0 and (want["weight"] == 3.0).sum() > 1000
    _assert_planes_equal(got, want, what="five views, cap 3")


def test_more_than_sixteen_views_go_in_chunks():
    case = cases.general_case(False)
    views = [case["views"][n % 3] for n in range(19)]
    want = orc.copy_volume(case["vol"])
    orc.integrate_f32(want, views)
    tv = _device_volume(case["vol"])
    tv.integrate_views([_device_view(v) for v in views])
    _assert_planes_equal(_planes(tv), want, what="19 views")
    assert tv.frames == 19


@pytest.mark.parametrize("dims", [(2, 2, 2), (5, 1, 3), (64, 4, 4), (8, 5, 3)])
def test_degenerate_volume_shapes(dims):
    """2 x 2 x 2: one cell; 5 x 1 x 3: integrate is fine, a mesh is refused; 64 x 4 x 4: exactly one brick, rows of float4;
    8 x 5 x 3: rows of float4 that do not fill a brick."""
    origin = np.array([-0.1, -0.05, 0.9], np.float32)
    vol = orc.empty_volume(dims, origin, 0.05, color=True)
    H, W = 48, 64
    vi, ui = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    depth = (0.93 + 0.004 * ui + 0.003 * vi).astype(np.float32)      # crosses the first cell
    rng = np.random.default_rng(4)
    view = orc.make_view(depth, np.eye(3, dtype=np.float32), np.array([0.011, 0.007, 0.1], np.float32), (14.0, 14.0, 12.3, 20.6),
                         image=rng.random((3, H, W)).astype(np.float32))
    want = orc.copy_volume(vol)
    touched = orc.integrate_f32(want, [view])
    assert touched.all()
    tv = _device_volume(vol)
    tv.integrate(**_device_view(view))
    _assert_planes_equal(_planes(tv), want, what=str(dims))
    if min(dims) < 2:
        with pytest.raises(_lib.LvdgsError):
            tv.extract_mesh()
        return
    mesh = tv.extract_mesh()
    v, c, f = orc.mesh_f32(want)
    assert len(mesh.vertices) == len(v) and len(mesh.faces) == len(f)
    if dims == (2, 2, 2):
        assert len(v) == 1 and len(f) == 0      # one active cell, no edge with four cells around it
    assert np.array_equal(_bits(mesh.vertices.cpu().numpy()), _bits(v)) and np.array_equal(mesh.faces.cpu().numpy(), f)


_EXTRACTION = {}


def _extraction(name):
    if not _EXTRACTION:
        for key, vol in cases.extraction_cases().items():
            _EXTRACTION[key] = (vol, orc.mesh_f32(vol))
    return _EXTRACTION[name]


@pytest.mark.parametrize("name", ["sphere", "slanted", "blobs", "holes", "rounds", "tiles"])
def test_extraction_against_the_mirror(name):
    vol, (v, c, f) = _extraction(name)
    tv = _device_volume(vol)
    mesh = tv.extract_mesh()
    assert tv.last_counts == (len(v), len(f)) and len(v) > 100 and len(f) > 100
    assert np.array_equal(mesh.faces.cpu().numpy(), f)
    assert np.array_equal(_bits(mesh.vertices.cpu().numpy()), _bits(v))
    if c is None:
        assert mesh.colors is None
    else:
        assert np.array_equal(_bits(mesh.colors.cpu().numpy()), _bits(c))
    again = tv.extract_mesh()      # sized by the first call's counts this time: the same bytes
    for a, b in zip(mesh, again):
        assert (a is None and b is None) or torch.equal(a, b)


def _raw_mesh(tv, vcap, fcap, pad=64):
    """One ``lvdgs_tsdf_mesh`` call into buffers with ``pad`` sentinel rows behind each capacity -> (buffers, block words)."""
    from lvdgs import tsdf
    L = _lib.lib()
    block, scratch = tsdf._mesh_call.resources(tv.device, _lib.TSDF_HOST_BYTES, L.lvdgs_tsdf_mesh_scratch_bytes(*tv.dims))
    vertices = torch.full((vcap + pad, 3), -7.5, dtype=torch.float32, device=DEV)
    colors = torch.full((vcap + pad, 3), -7.5, dtype=torch.float32, device=DEV)
    faces = torch.full((fcap + pad, 3), -77, dtype=torch.int32, device=DEV)
    a = _lib.TsdfMeshArgs(vol=tv._vol, vertex_capacity=vcap, face_capacity=fcap, vertices=vertices.data_ptr(), colors=colors.data_ptr(),
                          faces=faces.data_ptr(), host_state=block.data_ptr(), scratch=scratch.data_ptr(), scratch_bytes=scratch.numel())
    words = tsdf._mesh_call.run(tv.device, a).copy()
    return (vertices, colors, faces), words


def test_capacity_overflow_reports_exact_counts_and_writes_nothing_behind():
    vol, (v, c, f) = _extraction("blobs")
    tv = _device_volume(vol)
    nv, nf = len(v), len(f)
    for vcap, fcap, flag in ((nv - 5, nf + 8, 1), (nv, nf - 3, 2), (7, 11, 3), (0, 0, 3), (nv, nf, 0)):      # (nf - 3: the cut falls inside a pair)
        (vertices, colors, faces), w = _raw_mesh(tv, vcap, fcap)
        assert (int(w[_lib.TSDF_N_VERTICES]), int(w[_lib.TSDF_N_FACES]), int(w[_lib.TSDF_OVERFLOW])) == (nv, nf, flag), (vcap, fcap)
        assert not w[_lib.TSDF_OVERFLOW + 1:].any()
        assert bool((vertices[vcap:] == -7.5).all()) and bool((colors[vcap:] == -7.5).all()) and bool((faces[fcap:] == -77).all())
        assert np.array_equal(_bits(vertices[:min(vcap, nv)].cpu().numpy()), _bits(v[:vcap]))
        assert np.array_equal(_bits(colors[:min(vcap, nv)].cpu().numpy()), _bits(c[:vcap]))
        assert np.array_equal(faces[:min(fcap, nf)].cpu().numpy(), f[:fcap])
    # the Python layer: capacities too small, one retry with the exact sizes
    mesh = tv.extract_mesh(vertex_capacity=3, face_capacity=5)
    assert np.array_equal(mesh.faces.cpu().numpy(), f) and np.array_equal(_bits(mesh.vertices.cpu().numpy()), _bits(v))


def test_an_empty_volume_has_no_mesh():
    from lvdgs.tsdf import TsdfVolume
    tv = TsdfVolume((0, 0, 0), 0.1, (9, 6, 7))
    mesh = tv.extract_mesh()
    assert tuple(mesh.vertices.shape) == (0, 3) and tuple(mesh.faces.shape) == (0, 3) and tv.last_counts == (0, 0)
    tv.tsdf.fill_(-0.5)      # unobserved everywhere: still nothing; observed and all inside: nothing either
    assert tv.extract_mesh().faces.shape[0] == 0
    tv.weight.fill_(1.0)
    assert tv.extract_mesh().vertices.shape[0] == 0
    tv.reset()
    assert not tv.planes.any() and tv.frames == 0


def test_two_calls_give_the_same_bytes():
    case = cases.sphere_case()
    views = [_device_view(v) for v in case["views"]]
    a, b = _device_volume(case["vol"]), _device_volume(case["vol"])
    a.integrate_views(views)
    b.integrate_views(views)
    assert torch.equal(a.planes.view(torch.int32), b.planes.view(torch.int32))
    ma, mb = a.extract_mesh(), b.extract_mesh()
    for x, y in zip(ma, mb):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    vol, (v, c, f) = _extraction("sphere")      # and they are the mirror's
    _assert_planes_equal(_planes(a), vol, what="sphere planes")
    assert np.array_equal(ma.faces.cpu().numpy(), f)


def _count_waits_and_reads(fn):
    """(calls of any HostCall.wait, of torch.cuda.synchronize / Stream.synchronize / Event.synchronize, of Tensor.cpu / .item / .tolist)
    while ``fn`` runs (tests/test_gpu_frame_eval.py's idiom)."""
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


def test_integrate_makes_no_wait_and_extract_mesh_one():
    case = cases.sphere_case()
    views = [_device_view(v) for v in case["views"]]
    tv = _device_volume(case["vol"])
    tv.integrate_views(views)
    tv.extract_mesh()      # (the first call allocates the scratch and the pinned block, and learns the capacities)
    c = _count_waits_and_reads(lambda: (tv.integrate_views(views), tv.integrate(**views[0])))
    assert c == {"wait": 0, "sync": 0, "read": 0}, c
    out = []
    c = _count_waits_and_reads(lambda: out.append(tv.extract_mesh()))
    assert c == {"wait": 1, "sync": 1, "read": 0}, c      # (HostCall.wait is the one Stream.synchronize)
    assert out[0].faces.shape[0] > 100


def test_through_the_renderer():
    """Three views of a small map rendered with ``render()`` and fused with ``integrate_camera``: the planes are the mirror's, fed the same
    rendered depth, colour and cameras."""
    from types import SimpleNamespace
    from lvdgs import synthetic
    from lvdgs.camera_utils import Camera
    from lvdgs.gaussian_model import GaussianModel
    from lvdgs.gaussian_renderer import render
    from lvdgs.graphics_utils import focal2fov, getProjectionMatrix2
    from lvdgs.pose_utils import SE3_exp
    from lvdgs.tsdf import TsdfVolume
    W, H = 64, 48
    g = synthetic.make_gaussians(1500, W, H, seed=5, r_min=3.0, r_max=10.0, z_min=2.0, z_max=4.0)
    with torch.no_grad():
        g["opacities"].clamp_(min=0.7)
    model = GaussianModel.from_activated(g["means3D"], g["scales"], g["rotations"], g["opacities"], shs=g["shs"])
    pipe, bg = SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=False), torch.zeros(3, device=DEV)
    fx = fy = float(W)
    cx, cy = W / 2.0 - 0.3, H / 2.0 + 0.2
    proj = getProjectionMatrix2(znear=0.01, zfar=100.0, fx=fx, fy=fy, cx=cx, cy=cy, W=W, H=H).transpose(0, 1)
    tv = TsdfVolume((-1.6, -1.2, 1.6), 0.1, (33, 25, 28), trunc=0.3)
    want = orc.empty_volume(tv.dims, tv.origin, tv.voxel_size, trunc=tv.trunc)
    views = []
    for n in range(3):
        cam = Camera(n, torch.zeros(3, H, W, device=DEV), None, None, torch.eye(4), proj.to(DEV), fx, fy, cx, cy, focal2fov(fx, W), focal2fov(fy, H),
                     H, W, device=DEV)
        pose = SE3_exp(torch.tensor([0.05 * n, -0.03 * n, 0.02 * n, 0.02 * n, -0.03 * n, 0.01 * n]))
        cam.update_RT(pose[:3, :3].to(DEV), pose[:3, 3].to(DEV))
        with torch.no_grad():
            pkg = render(cam, model, pipe, bg)
        depth, image = pkg["depth"].detach()[0].contiguous(), pkg["render"].detach().contiguous()
        tv.integrate_camera(cam, depth, image=image, depth_trunc=5.0)
        views.append(orc.make_view(depth.cpu().numpy(), cam.R.cpu().numpy(), cam.T.cpu().numpy(), (fx, fy, cx, cy), image=image.cpu().numpy(),
                                   depth_trunc=5.0))
    touched = orc.integrate_f32(want, views)
    assert touched.any(0).sum() > 1000
    _assert_planes_equal(_planes(tv), want, what="rendered views")
    assert tv.extract_mesh().faces.shape[0] > 0


def test_fuse_mesh_over_the_toy_sequence(tmp_path):
    """``SlamSequence.fuse_mesh``: the keyframes rendered at their estimated poses and fused -- the planes are those of a volume fed the same
    renders through ``integrate_camera``, the mesh is non-empty, its faces index its vertices, and it saves."""
    import os
    import random
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))
    import sequence_scene as ss
    from lvdgs.slam_sequence import SlamSequence
    from lvdgs.tsdf import TsdfVolume, save_mesh_ply
    cfg, ds, _, _, _ = ss.toy_sequence_on_cpu()
    torch.manual_seed(0)
    random.seed(0)
    seq = SlamSequence(cfg, ds.to("cuda"), ss.empty_map(cfg, "cuda"), ss.PIPE, torch.zeros(3, device="cuda"), idle_map_iters=2).run()
    g = seq.frontend_gaussians
    extent = float((g.get_xyz.detach().max(0).values - g.get_xyz.detach().min(0).values).max())
    voxel = extent / 48.0
    mesh, record = seq.fuse_mesh(voxel)
    print(record)
    assert record["frames"] == len(seq.kf_indices) >= 1 and record["voxel_size"] == record["voxel_size_requested"] == voxel
    assert record["vertices"] == mesh.vertices.shape[0] > 0 and record["faces"] == mesh.faces.shape[0] > 0
    assert int(mesh.faces.min()) >= 0 and int(mesh.faces.max()) < record["vertices"] and mesh.colors.shape == mesh.vertices.shape
    lo, hi = mesh.vertices.min(0).values, mesh.vertices.max(0).values
    assert bool((hi - lo).max() <= extent + 10 * voxel)
    # the same volume by hand
    xyz = g.get_xyz.detach()
    opaque = g.get_opacity.detach().reshape(-1) >= 0.5
    points = xyz[opaque] if bool(opaque.any()) else xyz
    again = TsdfVolume.from_bounds((points.min(0).values - 4 * voxel).tolist(), (points.max(0).values + 4 * voxel).tolist(), voxel, max_voxels=1 << 26)
    assert list(again.dims) == record["dims"]
    with torch.no_grad():
        for idx in seq.kf_indices:
            frame = seq.cameras[idx]
            pkg = seq.render_fn(frame, g, seq.pipeline_params, seq.background)
            static = getattr(frame, "expanded_static_mask", None)
            static = getattr(frame, "static_mask", None) if static is None else static
            again.integrate_camera(frame, pkg["depth"].detach()[0].contiguous(), image=pkg["render"].detach().contiguous(), mask=static)
    other = again.extract_mesh()
    assert torch.equal(other.faces, mesh.faces) and torch.equal(other.vertices.view(torch.int32), mesh.vertices.view(torch.int32))
    path = tmp_path / "toy.ply"
    save_mesh_ply(str(path), mesh)
    assert os.path.getsize(path) > 15 * record["vertices"] + 13 * record["faces"]
