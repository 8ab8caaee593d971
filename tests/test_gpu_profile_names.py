"""The library's profiling slots, pinned: which names a short call sequence of every family of entry points records under
``lvdgs_profile_enable`` and how many launches each counts, against ``tests/golden/profile_names.json``.  tools/*_timing.py,
tools/map_bench.py and tests/test_gpu_tile_sort.py read these names; a slot renamed, a launch that moves to another slot or a launch that
comes or goes fails here.  The times are not compared.

Every case runs on a thread of its own: the forward calls keep their hints (the previous frame's longest list and queue) per thread, so
a fresh thread meets every call sequence in the same state whatever ran in the process before -- its first frame has no hint and sorts
its long lists, if any, in ``tile_sort_long``.  The profile itself is global to the process and counts the launches of every thread.

``LVDGS_RECORD_PROFILE_NAMES=1 pytest tests/test_gpu_profile_names.py`` records the golden anew from the library in place (a build known
to be good); its ``not_exercised`` list -- the slots no case reaches, each with its reason -- is kept as it is."""
import contextlib
import json
import os
import random
import sys
import threading
from types import SimpleNamespace

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, HERE)

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(HERE, "golden", "profile_names.json")
RECORD = os.environ.get("LVDGS_RECORD_PROFILE_NAMES") == "1"
DEV = "cuda"
W, H, N = 400, 240, 3000      # the rasterizer cases: 25 x 15 tiles, enough of them for two-level grouping, few enough for the fused blend


def _up(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)      # (a copy: some cases hand out read-only arrays)


def _seed():
    torch.manual_seed(0)
    np.random.seed(0)
    random.seed(0)


# ---- the rasterizer -----------------------------------------------------------------------------------------------
def _single_view(super_tiles=False, size=(W, H), n=N):
    import hip_runner
    from lvdgs import synthetic
    w, h = size
    g = synthetic.make_gaussians(n, w, h, seed=0)
    cam = synthetic.make_camera(w, h, pose_seed=1)
    hip_runner.run_hip(g, cam, w, h, torch.tensor([0.1, 0.2, 0.3]), grads=synthetic.make_image_grads(w, h, 0), super_tiles=super_tiles)


@contextlib.contextmanager
def _super_tiles(on):
    """rasterizer.super_tiles_flag forced on / off for the block (what LVDGS_SUPER_TILES=1 / 0 in the environment does)."""
    from lvdgs import rasterizer
    before = rasterizer._SUPER_TILES_ENV
    rasterizer._SUPER_TILES_ENV = "1" if on else "0"
    try:
        yield
    finally:
        rasterizer._SUPER_TILES_ENV = before


def _workload():
    from lvdgs import synthetic
    synthetic.CONFIGS.setdefault("tmp_profile_names", dict(N=N, W=W, H=H))
    return "tmp_profile_names"


def case_raster_forward_backward():
    """lvdgs_forward + lvdgs_backward of one view, one-level grouping."""
    _single_view()


def case_raster_two_level():
    """The same view with LVDGS_FLAG_SUPER_TILES forced: the super-tile count, scan, scatter and expansion, preprocess_bwd's helper waves."""
    _single_view(super_tiles=True)


def case_raster_radix():
    """129 x 129 tiles, more than the counting path takes: pairs emitted, radix-sorted by tile, ranges found."""
    _single_view(size=(2064, 2064), n=1500)


def case_tracking_fused():
    """Two iterations of a tracking session: the fused forward + backward blend, then lvdgs_tracking_tail, whose one launch finishes the
    loss and takes the pose step."""
    import bench
    from lvdgs.fast_tracking import TrackingSession
    dev = torch.device("cuda", 0)
    pipe = SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=False)
    with _super_tiles(False):
        model, cam, _, _ = bench.build_scene(_workload(), 0, dev)
        s = TrackingSession(cam, model, bench.CONFIG, pipe, torch.zeros(3, device=dev), gaussian_gradients=True, converged_threshold=-1.0)
        for _ in range(2):
            s.step()
        s.finish()


def case_mapping_window_batch():
    """One iteration over a window of two keyframes with static masks in lvdgs_forward_batch: the batched stages, the masked loss, the
    map's statistics and its Adam step."""
    import bench
    from lvdgs import backend_map
    dev = torch.device("cuda", 0)
    before = os.environ.get("LVDGS_MAP_BATCH")
    os.environ["LVDGS_MAP_BATCH"] = "1"
    try:
        with _super_tiles(False):
            model, _, _, _ = bench.build_scene(_workload(), 0, dev)
            be, window = bench.build_window(_workload(), 2, dev, model, n_window=2, masked=True)
            backend_map.map_window(be, window, iters=1)
        assert getattr(be, "_lvdgs_window_batch", None) is not None, "the batch path did not run"
    finally:
        if before is None:
            os.environ.pop("LVDGS_MAP_BATCH", None)
        else:
            os.environ["LVDGS_MAP_BATCH"] = before


# ---- the losses ---------------------------------------------------------------------------------------------------
def case_losses():
    """The photometric loss forward and backward, L1 + D-SSIM with and without a gradient, the masked depth L1."""
    from lvdgs import loss_utils
    from lvdgs.fused_loss import photometric_loss
    g = torch.Generator().manual_seed(0)
    h, w = 48, 80
    image = torch.rand(3, h, w, generator=g).to(DEV).requires_grad_(True)
    gt = torch.rand(3, h, w, generator=g).to(DEV)
    photometric_loss(image, gt).backward()
    loss_utils.l1_dssim_loss(image.detach(), gt, 0.2)
    loss_utils.l1_dssim_loss(image, gt, 0.2).backward()
    depth = (torch.rand(h, w, generator=g) + 0.5).to(DEV).requires_grad_(True)
    mono = (torch.rand(h, w, generator=g) + 0.5).to(DEV)
    loss_utils.masked_depth_l1(depth, mono, (torch.rand(h, w, generator=g) > 0.3).to(DEV)).backward()


def case_loss_entry_points():
    """lvdgs_photometric_loss_forward, _backward and _value_and_grad (twice) on one small frame."""
    import step_cases
    import test_gpu_step_kernels as sk
    sk._run_loss(step_cases.loss_case(33, 31, "tracking_rgbd"))


def case_map_statistics():
    """lvdgs_view_stats of one view and lvdgs_mark_visible, as backend_map.py and the rasterizer's markVisible call them."""
    from lvdgs import _lib
    n = 300
    g = torch.Generator().manual_seed(0)
    radii = torch.randint(0, 9, (n,), generator=g, dtype=torch.int32).to(DEV)
    touched = torch.randint(0, 3, (n,), generator=g, dtype=torch.int32).to(DEV)
    grad = torch.randn(n, 3, generator=g).to(DEV)
    radii_max = torch.zeros(n, dtype=torch.int32, device=DEV)
    norm_sum, vis_count = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    row = torch.zeros(n, dtype=torch.uint8, device=DEV)
    stream = _lib.raw_stream(radii.device)
    P = _lib.ptr
    _lib.check(_lib.lib().lvdgs_view_stats(n, P(radii), P(touched), P(grad), P(radii_max), P(norm_sum), P(vis_count), P(row), None, stream), "lvdgs_view_stats")
    pos = torch.randn(n, 3, generator=g).to(DEV)
    eye = torch.eye(4, device=DEV).contiguous()
    _lib.check(_lib.lib().lvdgs_mark_visible(n, P(pos), P(eye), P(eye), P(row), stream), "lvdgs_mark_visible")


def case_aux_ops():
    """distCUDA2 of a small cloud and a 2-D rotary embedding."""
    from lvdgs.curope import rope_2d
    from lvdgs.simple_knn import distCUDA2
    g = torch.Generator().manual_seed(0)
    distCUDA2((torch.rand(257, 3, generator=g) * 10 - 5).to(DEV))
    tokens = torch.randn(1, 7, 1, 4, generator=g).to(DEV)
    pos = torch.stack([torch.randint(0, 37, (1, 7), generator=g), torch.randint(0, 53, (1, 7), generator=g)], -1).to(DEV)
    rope_2d(tokens, pos, 100.0, 1.0)


# ---- the front end ------------------------------------------------------------------------------------------------
def case_depth_align():
    import depth_align_cases as dc
    from lvdgs import depth_utils
    r, m, kw, remedy = dc.make_case(sorted(dc.CASES)[0])
    depth_utils.process_depth(r, m, None, None, None, None, scale_remedy=dc.RecordedRemedy(remedy) if remedy else None, **kw)


def case_pnp():
    import pnp_cases as pc
    from lvdgs import init_pose
    c = pc.make_case("rot1_seed0")
    init_pose.pnp_ransac(_up(c["depth"]), c["m1"], c["m2"], c["K"], c["dist"], **c["kw"])


def case_recip_nn():
    from lvdgs import init_pose
    g = torch.Generator().manual_seed(0)
    d1 = torch.randn(12, 16, 16, generator=g).to(DEV)
    d2 = (d1.cpu() + 0.05 * torch.randn(12, 16, 16, generator=g)).to(DEV)
    init_pose.reciprocal_matches(d1, d2, subsample=4, max_iter=3)


def case_matcher_io():
    import matcher_io_cases as mc
    from lvdgs import depth_utils, init_pose
    name = sorted(mc.FORMAT_CASES)[0]
    init_pose.format_image(_up(mc.image(name, "noise")), mc.FORMAT_CASES[name][2])
    m1, m2, d1, d2 = mc.sweep_case(65, False)
    depth_utils.scale_from_matches(_up(m1), _up(m2), d1, d2, mc.RASTER)


def case_frame_stats():
    import frame_stats_cases as fc
    from lvdgs import frame_stats
    h, w = fc.MEDIAN_SIZES[0]
    frame_stats.edge_mask_call(_up(fc.image(h, w)), fc.EDGE_THRESHOLD, "kitti", loss_mask=True, magnitude=True, stats=True)
    h, w = fc.BLOCK_SIZES[0]
    frame_stats.edge_mask_call(_up(fc.image(h, w)), fc.EDGE_THRESHOLD, "replica", stats=True)
    n = 1000
    pkg = dict(depth=_up(fc.depths("random", n)), opacity=_up(fc.opacities("third", n)), n_touched=_up(np.arange(65, dtype=np.int32) % 3))
    frame_stats.frame_summary(pkg, [_up(fc.visibility("random", 65, seed=k)) for k in range(3)])


def case_ms_deform_attn():
    import ms_deform_attn_cases as cases
    from lvdgs import ms_deform_attn as mda
    c = cases.case("tiny")
    v, shapes, starts, loc, w = (_up(x) for x in (c.value, c.shapes, c.starts, cases.locations(c, "generic"), c.weights))
    mda.ms_deform_attn_forward(v, shapes, starts, loc, w, 64)
    mda.ms_deform_attn_backward(v, shapes, starts, loc, w, _up(c.grad_out), 64)


def case_dynamic_mask():
    import dynamic_mask_cases as cases
    import dynamic_mask_oracle as oracle
    from lvdgs import dynamic_mask as dm
    w, h = 96, 64
    history = dm.MaskHistory(w, h, 5, DEV)
    for n, first in ((0, True), (1, False)):
        case = cases.random_frame(n, w, h, 4, 2)
        vehicle = np.array([oracle.is_vehicle(s) for s in case["labels"]], np.uint8)
        dm.assemble(w, h, _up(case["boxes"]), _up(vehicle), _up(case["sam"]), first_frame=first, history=history, expand_kernel=5,
                    image=_up(case["image"]), rgb_boundary_threshold=0.3, depth=_up(case["depth"]), outputs=dm.OUTPUTS)


def case_optical_flow():
    import optical_flow_cases as cases
    from lvdgs import _lib
    from lvdgs import optical_flow as of
    w, h = cases.SIZES[1]
    f1, f2 = cases.moving_rectangle(w, h)[:2]
    state = of.MotionState(w, h, DEV)
    of.motion_mask(_up(cases.as_image(f1)), state, _lib.MOTION_OBSERVE)
    of.motion_mask(_up(cases.as_image(f2)), state, None, motion_threshold=3.0, dilate_kernel=7, want_flow=True)


def case_seeding():
    import seeding_cases as cases
    from lvdgs.seeding import seed_points
    w, h = cases.SIZES[0]
    R, T = cases.pose()
    seed_points(_up(cases.image(w, h)), _up(cases.depth_map(w, h)), cases.INTRINSICS, _up(R), _up(T), 4, 7, want_median=True)


def case_map_edit():
    import map_edit_cases as cases
    from lvdgs import map_edit
    c = cases.make_case("mixed", 1025)
    p = map_edit.plan_densify(_up(c["grad_accum"]), _up(c["denom"]), _up(c["scaling"]), _up(c["opacity"]), c["max_grad"],
                              c["percent_dense"] * c["extent"], c["min_opacity"], c["max_screen_size"], 0.1 * c["extent"])
    column = torch.rand(1025, 3, device=DEV)
    map_edit.apply(p, [(column, torch.empty(p.n_out, 3, device=DEV), map_edit.COPY)])
    mask = torch.zeros(1025, dtype=torch.bool, device=DEV)
    mask[::3] = True
    map_edit.plan_prune(1025, torch.device(DEV, 0), mask)


def case_ingest():
    import ingest_cases as ic
    from lvdgs import dataset as D
    name = "67x35"
    c = ic.case(name)
    dev = torch.device(DEV, 0)
    sx, sy = D.undistort_map_device(c["W"], c["H"], c["fx"], c["fy"], c["cx"], c["cy"], c["dist"], dev)
    rows = torch.from_numpy(ic.source(name, "noise").copy()).to(dev)
    src = rows.as_strided((c["H"], c["W"], 3), (rows.stride(0), 3, 1))
    D.ingest_frame(src, sx, sy, want_u8=True)
    D.ingest_frame(src)
    D.ingest_depth(torch.arange(24 * 40, dtype=torch.int16, device=dev).reshape(24, 40), 5000.0)
    D.ingest_depth(src[:, :, 0], 1.0)


def case_frame_eval():
    from lvdgs.eval_utils import FrameEvaluator
    g = torch.Generator().manual_seed(0)
    h, w = 37, 53
    gt = torch.rand(3, h, w, generator=g)
    render = (gt + 0.1 * torch.randn(3, h, w, generator=g)).contiguous()
    ev = FrameEvaluator(h, w, DEV, 1, want_images=True)
    ev.add(render.to(DEV), gt.to(DEV), (torch.rand(h, w, generator=g) > 0.35).to(DEV), None, (torch.rand(h, w, generator=g) * 40 + 0.5).to(DEV))


# ---- meshing ------------------------------------------------------------------------------------------------------
def _device_view(v):
    return dict(depth=_up(v["depth"]), R=_up(v["R"]), T=_up(v["T"]), intrinsics=v["intrinsics"], image=_up(v["image"]), mask=_up(v["mask"]),
                depth_min=v["depth_min"], depth_trunc=v["depth_trunc"])


def case_tsdf_and_mesh():
    """A sphere fused into the dense volume from six views, meshed; the mesh scored against itself, culled by what two views see past
    its own first surface."""
    import tsdf_cases
    from lvdgs import mesh_eval
    from lvdgs.tsdf import TsdfVolume
    case = tsdf_cases.sphere_case()
    vol = case["vol"]
    tv = TsdfVolume(vol["origin"], vol["voxel_size"], vol["dims"], trunc=vol["trunc"], max_weight=vol["max_weight"], color=True)
    views = [_device_view(v) for v in case["views"]]
    tv.integrate_views(views)
    mesh = tv.extract_mesh()
    assert mesh.faces.shape[0] > 0
    mesh_eval.score(mesh, mesh, n_samples=2000, threshold=0.05, seed=3)
    mesh_eval.cull_mesh(mesh, views=views[:2], occlusion_eps=0.05, occlusion="self")


def case_tsdf_blocks():
    """The same views into the block-sparse volume: allocation, integration, a mesh, and a rehash when the pool grows."""
    import tsdf_cases
    from lvdgs.tsdf_blocks import TsdfBlockVolume
    case = tsdf_cases.sphere_case()
    tv = TsdfBlockVolume(np.zeros(3, np.float32), case["vol"]["voxel_size"], 256, color=True)
    tv.integrate_views([_device_view(v) for v in case["views"]])
    assert tv.extract_mesh().faces.shape[0] > 0
    tv.grow(512)


CASES = {name[len("case_"):]: fn for name, fn in sorted(globals().items()) if name.startswith("case_")}


def _profiled(fn):
    """fn() on a fresh thread with the launch profile on -> {slot name: launches}."""
    from lvdgs import _lib
    box = {}

    def work():
        try:
            torch.cuda.set_device(0)
            _seed()
            _lib.profile_reset()
            _lib.profile_enable(True)
            try:
                fn()
                torch.cuda.synchronize()
                box["profile"] = _lib.profile_read()
            finally:
                _lib.profile_enable(False)
        except BaseException as e:      # (re-raised on the test's thread)
            box["error"] = e

    t = threading.Thread(target=work)
    t.start()
    t.join()
    if "error" in box:
        raise box["error"]
    assert 0 < len(box["profile"]) < 64, "profile_read returns at most 64 slots: split the case"
    return {name: launches for name, (launches, _) in sorted(box["profile"].items())}


def _golden():
    return json.load(open(GOLDEN)) if os.path.exists(GOLDEN) else {"cases": {}, "not_exercised": {}}


@pytest.mark.parametrize("case", list(CASES))
def test_profile_names_and_launch_counts(case):
    got = _profiled(CASES[case])
    print(case, got)
    if RECORD:
        g = _golden()
        g["cases"][case] = got
        with open(GOLDEN, "w") as f:
            json.dump(g, f, indent=1, sort_keys=True)
            f.write("\n")
        return
    assert got == _golden()["cases"][case]


def test_golden_covers_the_cases_and_names_few_exceptions():
    """Every case has its record; the slots left out are listed with a reason and are at most a tenth of the names recorded."""
    g = _golden()
    if RECORD:
        return
    assert sorted(g["cases"]) == sorted(CASES)
    names = set().union(*[set(c) for c in g["cases"].values()])
    assert not names & set(g["not_exercised"]), names & set(g["not_exercised"])
    assert all(isinstance(r, str) and r for r in g["not_exercised"].values())
    assert 10 * len(g["not_exercised"]) <= len(names), (len(g["not_exercised"]), len(names))
