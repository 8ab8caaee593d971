"""The import names the reference's files use resolve to the lvdgs implementation, and what the reference's own
utils/camera_utils.py and utils/slam_backend.py did when loaded through the shim (tests/golden/dropin_reference.json,
written by tests/golden/make_golden.py) is what the build's Camera, shim and GaussianModel give."""
import json
import os


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DROPIN = os.path.join(ROOT, "lvd_gs-slam_amd", "dropin")


def test_shim_names_resolve(monkeypatch):
    monkeypatch.syspath_prepend(DROPIN)
    import lvdgs.rasterizer as R
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    from gaussian_splatting.gaussian_renderer import render, render_with_custom_resolution
    from gaussian_splatting.utils.graphics_utils import getProjectionMatrix2, getWorld2View2
    from simple_knn._C import distCUDA2
    assert GaussianRasterizer is R.GaussianRasterizer and GaussianRasterizationSettings is R.GaussianRasterizationSettings
    assert callable(render) and callable(render_with_custom_resolution) and callable(distCUDA2)
    assert GaussianRasterizationSettings._fields == (
        "image_height", "image_width", "tanfovx", "tanfovy", "bg", "scale_modifier", "viewmatrix", "projmatrix",
        "projmatrix_raw", "sh_degree", "campos", "prefiltered", "debug")
    P = getProjectionMatrix2(znear=0.01, zfar=100.0, fx=500.0, fy=500.0, cx=320.0, cy=240.0, W=640, H=480)
    assert P.shape == (4, 4) and float(P[3, 2]) == 1.0
    assert getWorld2View2.__module__ == "lvdgs.graphics_utils"


def _reference():
    """What the reference's own Camera and BackEnd did when loaded through the shim (tests/golden/make_golden.py gen_dropin)."""
    return json.load(open(os.path.join(ROOT, "tests", "golden", "dropin_reference.json")))


def test_reference_camera_imports_through_the_shim(monkeypatch):
    """utils/camera_utils.py:4 imports gaussian_splatting.utils.graphics_utils; with the shim on the path that import resolves, and
    the reference's own Camera class, loaded through it, produced the matrices and parameters the mirror produces."""
    import importlib
    import torch
    monkeypatch.syspath_prepend(DROPIN)
    gu = importlib.import_module("gaussian_splatting.utils.graphics_utils")
    assert callable(gu.getProjectionMatrix2) and callable(gu.getWorld2View2)
    from lvdgs.camera_utils import Camera
    from lvdgs.pose_utils import SE3_exp
    ref = _reference()["camera"]
    c = ref["inputs"]
    proj = gu.getProjectionMatrix2(znear=0.01, zfar=100.0, fx=c["fx"], fy=c["fy"], cx=c["cx"], cy=c["cy"], W=c["W"], H=c["H"]).transpose(0, 1)
    b = Camera(0, torch.rand(3, 8, 8), None, None, torch.eye(4), proj, c["fx"], c["fy"], c["cx"], c["cy"], c["FoVx"], c["FoVy"], c["H"], c["W"],
               device="cpu")
    T = SE3_exp(torch.tensor(c["tau"]))
    b.update_RT(T[:3, :3], T[:3, 3])
    for name in ("world_view_transform", "full_proj_transform", "camera_center"):
        assert torch.allclose(torch.tensor(ref[name]), getattr(b, name), atol=1e-6), name
    assert ref["parameter_names"] == sorted(n for n, _ in b.named_parameters())


def test_reference_backend_constructs_and_resets_on_the_shim(monkeypatch):
    """utils/slam_backend.py imports render / l1_loss / ssim / getProjectionMatrix2 / getWorld2View2 from gaussian_splatting (:10-12):
    through the shim they are the objects the reference's own BackEnd received; BackEnd.set_hyperparams took the KITTI-07
    hyper-parameters the build's make_backend holds; BackEnd.reset (:79-92) leaves the state make_backend starts in and drives
    GaussianModel.prune_points of the shim's model down to an empty map."""
    import importlib
    import torch
    monkeypatch.syspath_prepend(DROPIN)
    ref = _reference()
    where = {"render": "gaussian_splatting.gaussian_renderer", "l1_loss": "gaussian_splatting.utils.loss_utils",
             "ssim": "gaussian_splatting.utils.loss_utils", "getProjectionMatrix2": "gaussian_splatting.utils.graphics_utils",
             "getWorld2View2": "gaussian_splatting.utils.graphics_utils"}
    assert set(where) == set(ref["backend_imports"])
    for n, mod in where.items():
        o = getattr(importlib.import_module(mod), n)
        assert o.__module__ + "." + o.__qualname__ == ref["backend_imports"][n], n
    import lvdgs.gaussian_renderer
    import lvdgs.loss_utils
    assert importlib.import_module("gaussian_splatting.gaussian_renderer").render is lvdgs.gaussian_renderer.render
    assert importlib.import_module("gaussian_splatting.utils.loss_utils").ssim is lvdgs.loss_utils.ssim

    # the build's BackEnd state (lvdgs.slam_sequence.make_backend) holds the hyper-parameters the reference's set_hyperparams took from the
    # same configuration, and starts where the reference's reset leaves the back end
    from lvdgs.slam_sequence import make_backend
    cfg = json.load(open(os.path.join(ROOT, "tests", "golden", "config_07.json")))
    cfg["Training"]["monocular"] = cfg["Dataset"]["sensor_type"] == "monocular"
    hp = ref["backend_hyperparams"]
    be = make_backend(cfg, None, None, None, cameras_extent=hp["cameras_extent"])
    for n, v in hp.items():
        assert getattr(be, n) == v, n
    assert be.window_size == 8 and be.gaussian_extent == 6.0 and be.init_gaussian_extent == 180.0
    rs = ref["backend_reset"]
    assert (be.iteration_count, be.current_window, be.initialized) == (rs["iteration_count"], rs["current_window"], rs["initialized"])

    from gaussian_splatting.scene.gaussian_model import GaussianModel
    g = GaussianModel.from_activated(torch.rand(9, 3), torch.rand(9, 3) + 0.1, torch.nn.functional.normalize(torch.randn(9, 4)),
                                     torch.rand(9, 1), colors=torch.rand(9, 3), device="cpu")
    g.init_lr(6.0)
    g.training_setup(cfg["opt_params"])
    assert g.get_xyz.shape[0] == rs["gaussians_before"]
    g.prune_points(g.unique_kfIDs >= 0)   # what BackEnd.reset asks of the model
    assert g.get_xyz.shape[0] == rs["gaussians_after"] == 0
    assert all(p.shape[0] == 0 for p in g.parameters())
