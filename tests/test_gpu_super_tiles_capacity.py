"""Two-level grouping (LVDGS_FLAG_SUPER_TILES) when the SUPER lists outgrow the pair capacity and the tile lists do not.

A Gaussian whose rectangle spans more than 64 super-tiles is listed on every one of them (csrc/binning.hpp: super_rect_of), however
few of its tiles are kept: huge faint Gaussians centred near the frame's corners keep a block or two of their tiles and list a
hundred or more super-tiles.  On such a frame the super pair count Ds exceeds the tile pair count D, and a capacity between the two
(D <= cap < Ds) is what the autograd path re-renders at after an overflow.  The library must then still return the hint-off bits
(it redoes the view one-level inside the call): checked against the hint-off run bit for bit, and the forward and backward against the
oracle.  The host model (super_tile_model.py) establishes the premise from a hint-off run before anything runs with the hint."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import super_tile_model as stm  # noqa: E402
import test_gpu_parity as tp  # noqa: E402

pytestmark = pytest.mark.gpu

W, H = 1280, 720
NUM_HUGE = 600   # (the first Gaussians of the scene)
FWD_KEYS = ("point_list", "ranges", "n_contrib", "final_T", "color", "depth", "opacity", "radii", "n_touched", "slot_base", "tiles_touched")


def _scene():
    """An opaque-surface background behind 600 huge (3-sigma radius 600-900 px) Gaussians of opacity 0.0040, centred near the
    frame's corners: alpha >= 1/255 only within ~0.2 sigma of the centre, a block or two of a rectangle of 40-60 x 45 tiles."""
    from lvdgs import synthetic
    bg = synthetic.make_surface_gaussians(200, W, H, seed=5)
    n = NUM_HUGE
    gen = torch.Generator().manual_seed(11)
    u = lambda *s: torch.rand(*s, generator=gen)
    # centres: within 3 % of the frame's size from one of its corners
    right, bottom = u(n) < 0.5, u(n) < 0.5
    px = torch.where(right, W - u(n) * 0.03 * W, u(n) * 0.03 * W)
    py = torch.where(bottom, H - u(n) * 0.03 * H, u(n) * 0.03 * H)
    fx = float(W)
    z = 2.0 + u(n)
    r = 600.0 + 300.0 * u(n)                                   # 3-sigma radius in pixels
    s = (r * z / (3.0 * fx))[:, None].expand(n, 3).contiguous()
    means = torch.stack([(px - W / 2.0) * z / fx, (py - H / 2.0) * z / fx, z], 1)
    huge = dict(means3D=means, scales=s, rotations=torch.tensor([1.0, 0.0, 0.0, 0.0]).expand(n, 4).contiguous(),
                opacities=torch.full((n, 1), 0.0040), colors=u(n, 3), shs=torch.zeros(n, 1, 3))
    g = {k: torch.cat([huge[k], bg[k]], 0).contiguous().float() for k in ("means3D", "scales", "rotations", "opacities", "colors", "shs")}
    return g, synthetic.make_camera(W, H)


class _capacity:
    """The rasterizer's capacity knobs for the block: the first call of a frame sizes its buffers for exactly `pairs`."""

    def __init__(self, pairs):
        self.pairs = pairs

    def __enter__(self):
        from lvdgs import rasterizer as rz
        self.before = (rz._MIN_PAIR_CAPACITY, rz._PAIRS_PER_GAUSSIAN_GUESS, dict(rz._PAIR_CAPACITY))
        rz._MIN_PAIR_CAPACITY, rz._PAIRS_PER_GAUSSIAN_GUESS = self.pairs, 0
        rz._PAIR_CAPACITY.clear()

    def __exit__(self, *exc):
        from lvdgs import rasterizer as rz
        rz._MIN_PAIR_CAPACITY, rz._PAIRS_PER_GAUSSIAN_GUESS = self.before[0], self.before[1]
        rz._PAIR_CAPACITY.clear(); rz._PAIR_CAPACITY.update(self.before[2])
        return False


@pytest.fixture(scope="module")
def case():
    import hip_runner
    from lvdgs import synthetic
    g, cam = _scene()
    bgc = torch.tensor([0.1, 0.2, 0.3])
    grads = synthetic.make_image_grads(W, H, 4)
    f0, b0 = hip_runner.run_hip(g, cam, W, H, bgc, grads=grads, super_tiles=False)
    D = int(f0["num_rendered"])
    Di, Dsi, per_super = stm.frame_counts(f0["rec"], W, H, f0["radii"] > 0)
    Ds = int(Dsi.sum())
    return SimpleNamespace(g=g, cam=cam, bg=bgc, grads=grads, f0=f0, b0=b0, D=D, Ds=Ds, Di=Di, Dsi=Dsi, per_super=per_super)


def test_premise_super_lists_outgrow_the_tile_lists(case):
    from lvdgs import _lib
    gx, gy = -(-W // 16), -(-H // 16)
    assert 64 <= gx * gy <= 16384
    assert not (case.f0["flags"] & _lib.FLAG_SUPER_TILES)
    assert int(case.Di.sum()) == case.D, (int(case.Di.sum()), case.D)          # the model's tile level is the library's
    assert np.array_equal(case.Di, case.f0["tiles_touched"].astype(np.int64))
    n = NUM_HUGE
    assert case.Ds >= case.D + 1000, (f"D={case.D} Ds={case.Ds}: huge Gaussians D={int(case.Di[:n].sum())} Ds={int(case.Dsi[:n].sum())}, "
                                      f"background D={int(case.Di[n:].sum())} Ds={int(case.Dsi[n:].sum())}")


def _same(f, b, case, what):
    for k in FWD_KEYS:
        assert np.array_equal(f[k], case.f0[k]), f"{what}: {k} (D={case.D} Ds={case.Ds} cap={f['capacity']})"
    for k, v in case.b0.items():
        assert np.array_equal(b[k], v), f"{what}: grad {k} (D={case.D} Ds={case.Ds} cap={f['capacity']})"


def test_autograd_rerender_after_overflow_at_exactly_D(case):
    """The first call carries the hint with room for 1000 pairs < D: LVDGS_E_CAPACITY, and its super scan counts Ds (the library's count
    equals the model's).  The re-render (lvdgs_forward_render) then runs with buffers of exactly D < Ds pairs and DROPS the hint -- it
    cannot know Ds -- so this leg checks that the frame actually rendered at D is the hint-off one, bit for bit."""
    import hip_runner
    from lvdgs import _lib
    with _capacity(1000):
        f, b = hip_runner.run_hip(case.g, case.cam, W, H, case.bg, grads=case.grads, super_tiles=True)
    assert f["flags"] & _lib.FLAG_SUPER_TILES          # (the flag of the first call; lvdgs_forward_render ignores it)
    assert f["num_rendered_super"] == case.Ds, (f["num_rendered_super"], case.Ds)
    cap = f["binning_pairs"]
    assert f["overflowed"] and f["num_rendered"] == case.D and cap == case.D and cap < case.Ds, f"D={case.D} cap={cap} Ds={case.Ds}"
    _same(f, b, case, "re-render at D")


def test_forward_with_capacity_exactly_D_matches_hint_off_and_oracle(case):
    """lvdgs_forward with pair_capacity == D < Ds (the library's own super count says so: the one-level redo inside the call ran).
    The bits of the hint-off run, and the oracle's results."""
    import hip_runner
    from lvdgs import _lib
    orc, hr, _ = tp._mods()
    with _capacity(case.D):
        f, b = hip_runner.run_hip(case.g, case.cam, W, H, case.bg, grads=case.grads, super_tiles=True)
    assert f["flags"] & _lib.FLAG_SUPER_TILES
    cap, Ds = f["binning_pairs"], f["num_rendered_super"]
    assert Ds == case.Ds, (Ds, case.Ds)
    assert not f["overflowed"] and f["num_rendered"] == case.D <= cap == case.D < Ds, f"D={f['num_rendered']} cap={cap} Ds={Ds}"
    _same(f, b, case, "lvdgs_forward, cap == D")
    f_ora, b_ora = hr.run_oracle(orc, case.g, case.cam, W, H, case.bg, grads=case.grads)
    tp._check_forward(f, f_ora, W, H)
    with _capacity(case.D):   # (the masked re-runs take the same path)
        tp._check_backward(b, b_ora, ["means3D", "means2D", "opacities", "scales", "rotations", "colors", "tau"], f_ora, W, H,
                           rerun=tp.masked_rerun(hr, orc, case.g, case.cam, W, H, case.bg, case.grads, super_tiles=True))


def _session_model(g, dev):
    """The scene as a GaussianModel and a Camera, as bench.build_scene makes them."""
    from lvdgs.camera_utils import Camera
    from lvdgs.gaussian_model import GaussianModel
    from lvdgs.graphics_utils import focal2fov, getProjectionMatrix2
    fx = fy = float(W)
    cx, cy = W / 2.0, H / 2.0
    proj = getProjectionMatrix2(znear=0.01, zfar=100.0, fx=fx, fy=fy, cx=cx, cy=cy, W=W, H=H).transpose(0, 1).contiguous().to(dev)
    gen = torch.Generator().manual_seed(77)
    image = torch.rand(3, H, W, generator=gen).to(dev)
    cam = Camera(1, image, None, (torch.rand(H, W, generator=gen) * 40 + 1).numpy(), torch.eye(4), proj, fx, fy, cx, cy,
                 focal2fov(fx, W), focal2fov(fy, H), H, W, device=dev)
    cam.grad_mask = (torch.rand(1, H, W, generator=gen) > 0.5).to(dev)
    model = GaussianModel.from_activated(g["means3D"], g["scales"], g["rotations"], g["opacities"], shs=g["shs"], sh_degree=0, device=dev)
    return model, cam


class _hint:
    """rasterizer.super_tiles_flag forced on / off for the block."""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        from lvdgs import rasterizer as rz
        self.before = rz._SUPER_TILES_ENV
        rz._SUPER_TILES_ENV = "1" if self.on else "0"

    def __exit__(self, *exc):
        from lvdgs import rasterizer as rz
        rz._SUPER_TILES_ENV = self.before
        return False


def _state(L, N, geom, image, D):
    """ranges, final_T, n_contrib of an image state; the model's and the library's super counts from geom_state (uint8 tensors)."""
    import ctypes as C
    import hip_runner
    from lvdgs import _lib
    lay = _lib.StateLayout()
    _lib.check(L.lvdgs_state_layout_query(N, max(int(D), 1), W, H, C.byref(lay)), "layout")
    T_, P_ = (-(-W // 16)) * (-(-H // 16)), W * H
    # the rectangles the grouping reads (GeomView::rect, zero for a culled Gaussian: csrc/api.hip geom_layout, behind tiles_touched and
    # depth_bits, every array 256-byte aligned)
    off = int(lay.geom_tiles_touched) + 2 * (((4 * N + 255) // 256) * 256)
    rects = geom[off:off + 16 * N].cpu().numpy().view(np.uint32).reshape(N, 4)
    _, Dsi, _ = stm.frame_counts(rects, W, H)
    out = dict(ranges=image[lay.img_ranges:lay.img_ranges + 8 * T_].clone(), final_T=image[lay.img_final_T:lay.img_final_T + 4 * P_].clone(),
               n_contrib=image[lay.img_n_contrib:lay.img_n_contrib + 4 * P_].clone())
    return out, int(Dsi.sum()), hip_runner.geom_super_count(geom, lay, N)


def test_tracking_session_with_capacity_between_D_and_Ds(case):
    """TrackingSession (lvdgs_forward_backward_fused_loss: forward, loss and backward in one call, the backward stood down on the device)
    with pair_capacity == D < Ds: a step gives the hint-off run's bits -- images, image state, pose, exposure, loss, every gradient."""
    import bench
    from lvdgs import _lib
    from lvdgs.fast_tracking import TrackingSession
    dev = torch.device("cuda", 0)
    pipe = SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=False)
    res = {}
    for on in (False, True):
        with _capacity(case.D), _hint(on):
            model, cam = _session_model(case.g, dev)
            s = TrackingSession(cam, model, bench.CONFIG, pipe, torch.zeros(3, device=dev), gaussian_gradients=True, converged_threshold=-1.0)
            cap = int(s.cap)
            s.step()      # (one step: the next would render from the updated pose, a frame of its own pair count)
            s.finish()
            torch.cuda.synchronize()
        assert bool(s.a.flags & _lib.FLAG_SUPER_TILES) is on
        st, Ds_model, Ds_lib = _state(s.L, s.N, s.geom, s.image, s.num_rendered)
        if on:
            assert Ds_lib == Ds_model, (Ds_lib, Ds_model)
            assert s.num_rendered <= cap == case.D < Ds_lib, f"D={s.num_rendered} cap={cap} Ds={Ds_lib}"
        tensors = dict(st, R=s.R, T=s.T, exposure_a=cam.exposure_a, exposure_b=cam.exposure_b, color=s.color, depth=s.depth, opacity=s.opacity,
                       radii=s.radii, n_touched=s.n_touched, loss=s.loss, d_tau=s.d_tau, d_a=s.d_a, d_b=s.d_b, d_m3=s.d_m3, d_m2=s.d_m2,
                       d_op=s.d_op, d_sc=s.d_sc, d_rot=s.d_rot, d_sh=s.d_sh)
        res[on] = ({k: t.detach().clone() for k, t in tensors.items()}, int(s.num_rendered), cap, Ds_model)
    (a, D0, _, _), (b, D1, cap, Ds) = res[False], res[True]
    assert D0 == D1
    for k in a:
        assert torch.equal(a[k], b[k]), f"{k} (D={D1} Ds={Ds} cap={cap})"


def test_mapping_window_batch_with_one_view_between_D_and_Ds():
    """A MapWindowBatch window of 3 views of the scene (lvdgs_forward_batch) whose capacity is the largest view's D, below the super count
    of at least one view: that view is redone one-level inside the call.  The map, poses and every view's image state after an
    iteration are the hint-off window's bits."""
    import bench
    from lvdgs import _lib, backend_map, synthetic
    dev = torch.device("cuda", 0)
    g, _ = _scene()
    name = "tmp_super_tiles_capacity"
    synthetic.CONFIGS[name] = dict(N=int(g["means3D"].shape[0]), W=W, H=H)

    def window(on, cap):
        with _capacity(cap), _hint(on):
            torch.manual_seed(0)
            model, _ = _session_model(g, dev)
            be, win = bench.build_window(name, 4, dev, model, n_window=3, masked=False)
            before = os.environ.get("LVDGS_MAP_BATCH")
            os.environ["LVDGS_MAP_BATCH"] = "1"
            try:
                backend_map.map_window(be, win, iters=1)
            finally:
                if before is None:
                    os.environ.pop("LVDGS_MAP_BATCH", None)
                else:
                    os.environ["LVDGS_MAP_BATCH"] = before
            torch.cuda.synchronize()
            wb = be._lvdgs_window_batch
            views = []
            for p in wb.passes[:3]:
                assert bool(p.a.flags & _lib.FLAG_SUPER_TILES) is on
                st, Ds_model, Ds_lib = _state(p.L, p.N, p.geom, p.image, p.a.num_rendered)
                views.append((st, int(p.a.num_rendered), int(p.cap), Ds_model, Ds_lib))
            params = [q.detach().clone() for q in be.gaussians.parameters()]
            poses = [torch.cat([vp.cam_rot_delta.detach().flatten(), vp.cam_trans_delta.detach().flatten(), vp.exposure_a.detach().flatten(),
                                vp.exposure_b.detach().flatten()]).clone() for vp in be.viewpoints.values()]
            return views, params, poses

    try:
        probe, _, _ = window(False, 1 << 20)
        cap = max(v[1] for v in probe)
        over = [k for k, v in enumerate(probe) if v[3] > cap]
        assert over, f"no view's super count exceeds the capacity: D={[v[1] for v in probe]} Ds={[v[3] for v in probe]} cap={cap}"
        off, params0, poses0 = window(False, cap)
        on, params1, poses1 = window(True, cap)
    finally:
        synthetic.CONFIGS.pop(name, None)
    for k in range(3):
        (s0, D0, c0, _, _), (s1, D1, c1, Dsm, Dsl) = off[k], on[k]
        what = f"view {k}: D={D1} cap={c1} Ds={Dsl}"
        assert D0 == D1 == probe[k][1] and c1 == cap, what
        assert Dsl == Dsm, (what, Dsm)
        if k in over:
            assert D1 <= c1 < Dsl, what
        for key in s0:
            assert torch.equal(s0[key], s1[key]), f"{key}: {what}"
    for i, (x, y) in enumerate(zip(params0 + poses0, params1 + poses1)):
        assert torch.equal(x, y), f"params / poses {i}: views {[(v[1], v[2], v[4]) for v in on]} (D, cap, Ds)"
