"""A 96x64 scene (24 tiles, 96 quadrants, 2000 Gaussians) built to stress the blend kernels' quadrant reach test
(csrc/common.hpp: quad_prepare / reaches_rect_prepared), and everything the library computes on it through the entry points
whose blend passes run that test:

  * lvdgs_forward + lvdgs_backward -- full and LVDGS_FLAG_POSE_ONLY, with and without a depth / opacity gradient;
  * lvdgs_forward_backward_fused_loss (a TrackingSession's iteration: at this size both blend passes in one launch) -- full
    and pose-only, monocular (no depth gradient) and RGB-D.

Which (entry, quadrant) combinations survive the test decides the order a pixel's gradients are summed in, so any change of
a single boolean shows in the gradient bits.  collect() returns every result as a flat dict of numpy arrays;
tests/golden/make_quadrant_test_golden.py records it, tests/test_gpu_quadrant_test.py compares bit for bit.

The scene (seeded, float32, identity pose, fx = fy = 96):
  * 500 thin slanted ellipses (sigma 6-20 px by 0.05-0.6 px, every angle) centred within 1.5 px of a quadrant corner;
  * 400 small blobs (sigma 1-4 px) and 400 tiny ones (0.3-2 px) anywhere: means inside a quadrant, inside exactly one span of
    their neighbours, and outside the image;
  * 300 with opacities straddling 1/255 (the threshold -3 .. +3 ulps, 0.0039, 0.004, 0.0045) and large footprints;
  * 300 faint ones crowded into tile 0 and 100 into tile 3: one list longer than 256 entries, one longer than 64, so both
    kernels stage more than one round.
Opacities are low enough that most pixels never saturate: the lists are walked to their ends."""
import ctypes as C
import hashlib
import math
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

W, H, N = 96, 64, 2000
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "quadrant_test.npz")
WHOLE_LIMIT = 16384   # arrays of up to this many bytes are recorded whole, larger ones as the SHA-256 of their bytes


def make_scene():
    """dict of float32 CPU tensors as synthetic.make_gaussians() returns it (means3D, scales, rotations, opacities, colors, shs)."""
    g = torch.Generator().manual_seed(96064)
    u = lambda *s: torch.rand(*s, generator=g)
    logu = lambda n, lo, hi: torch.exp(u(n) * (math.log(hi) - math.log(lo)) + math.log(lo))
    fx = float(W)
    px, py, s_long, s_thin, angle, opac = [], [], [], [], [], []

    def add(x, y, sl, st, an, op):
        px.append(x); py.append(y); s_long.append(sl); s_thin.append(st); angle.append(an); opac.append(op)

    n = 500   # thin slanted ellipses across quadrant corners
    add(8.0 * torch.randint(0, W // 8 + 1, (n,), generator=g) - 0.5 + 3.0 * (u(n) - 0.5),
        8.0 * torch.randint(0, H // 8 + 1, (n,), generator=g) - 0.5 + 3.0 * (u(n) - 0.5),
        logu(n, 6.0, 20.0), logu(n, 0.05, 0.6), math.pi * u(n), logu(n, 0.02, 0.5))
    n = 400   # small blobs anywhere, a tenth of them outside the image
    add((1.2 * u(n) - 0.1) * W, (1.2 * u(n) - 0.1) * H, logu(n, 1.0, 4.0), logu(n, 1.0, 4.0), math.pi * u(n), logu(n, 0.02, 0.6))
    n = 400   # tiny ones: most of them inside one quadrant only
    add(u(n) * W, u(n) * H, logu(n, 0.3, 2.0), logu(n, 0.3, 2.0), math.pi * u(n), logu(n, 0.05, 0.9))
    n = 300   # opacities straddling 1/255
    amin = np.float32(1.0) / np.float32(255.0)
    ulps = (np.frombuffer(amin.tobytes(), np.uint32)[0] + np.arange(-3, 4)).astype(np.uint32).view(np.float32)
    choices = torch.tensor(np.concatenate([ulps, np.float32([0.0039, 0.004, 0.0045])]))
    add(u(n) * W, u(n) * H, logu(n, 2.0, 12.0), logu(n, 0.5, 6.0), math.pi * u(n), choices[torch.randint(0, len(choices), (n,), generator=g)])
    n = 300   # tile 0: a list of more than 256 entries
    add(16.0 * u(n), 16.0 * u(n), logu(n, 0.5, 3.0), logu(n, 0.3, 1.5), math.pi * u(n), logu(n, 0.01, 0.05))
    n = 100   # tile 3: more than 64
    add(48.0 + 16.0 * u(n), 16.0 * u(n), logu(n, 0.5, 3.0), logu(n, 0.3, 1.5), math.pi * u(n), logu(n, 0.01, 0.08))
    px, py, s_long, s_thin, angle, opac = (torch.cat(t).float() for t in (px, py, s_long, s_thin, angle, opac))
    assert px.numel() == N
    z = 1.0 + 19.0 * u(N)
    means3D = torch.stack([(px - W / 2.0) * z / fx, (py - H / 2.0) * z / fx, z], 1)
    scales = torch.stack([s_long * z / fx, s_thin * z / fx, 0.01 * z / fx * torch.ones(N)], 1)
    rotations = torch.stack([torch.cos(angle / 2), torch.zeros(N), torch.zeros(N), torch.sin(angle / 2)], 1)   # about the optical axis
    rgb = u(N, 3)
    return dict(means3D=means3D.contiguous(), scales=scales.contiguous(), rotations=rotations.contiguous(),
                opacities=opac.reshape(N, 1).contiguous(), colors=rgb.contiguous(), shs=((rgb - 0.5) / 0.28209479177387814)[:, None, :].contiguous())


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _separate_calls(g, out):
    """lvdgs_forward, then lvdgs_backward four times: full / pose-only, with the depth and opacity images' gradients / colour alone."""
    from lvdgs import _lib, synthetic
    L = _lib.lib()
    dev = torch.device("cuda")
    cam = synthetic.make_camera(W, H)
    t = {k: v.to(dev).contiguous() for k, v in g.items()}
    mats = {k: getattr(cam, k).to(dev).contiguous() for k in ("world_view_transform", "full_proj_transform", "projection_matrix", "camera_center")}
    bg = torch.tensor([0.1, 0.2, 0.3], device=dev)
    buf = lambda n: torch.zeros(max(int(n), 256), dtype=torch.uint8, device=dev)
    cap = 100_000
    a = _lib.Args()
    a.image_height, a.image_width, a.tanfovx, a.tanfovy = H, W, cam.tanfovx, cam.tanfovy
    a.scale_modifier, a.sh_degree = 1.0, 0
    a.bg, a.viewmatrix, a.projmatrix = _p(bg), _p(mats["world_view_transform"]), _p(mats["full_proj_transform"])
    a.projmatrix_raw, a.campos = _p(mats["projection_matrix"]), _p(mats["camera_center"])
    a.num_gaussians, a.sh_coeffs = N, 0
    a.means3D, a.opacities, a.scales, a.rotations, a.colors_precomp = _p(t["means3D"]), _p(t["opacities"]), _p(t["scales"]), _p(t["rotations"]), _p(t["colors"])
    radii, n_touched = torch.zeros(N, dtype=torch.int32, device=dev), torch.zeros(N, dtype=torch.int32, device=dev)
    color, depth, opacity = (torch.zeros(c, H, W, device=dev) for c in (3, 1, 1))
    geom, image, binning = buf(L.lvdgs_geom_bytes(N)), buf(L.lvdgs_image_bytes(W, H)), buf(L.lvdgs_binning_bytes(cap))
    scratch = buf(max(L.lvdgs_prepare_scratch_bytes(N), L.lvdgs_render_scratch_bytes(N, cap, W, H), L.lvdgs_backward_scratch_bytes(N, cap)))
    a.radii, a.n_touched, a.out_color, a.out_depth, a.out_opacity = _p(radii), _p(n_touched), _p(color), _p(depth), _p(opacity)
    a.geom_state, a.geom_bytes, a.image_state, a.image_bytes = _p(geom), geom.numel(), _p(image), image.numel()
    a.binning_state, a.binning_bytes, a.scratch, a.scratch_bytes = _p(binning), binning.numel(), _p(scratch), scratch.numel()
    a.pair_capacity = cap
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    D = C.c_int64()
    _lib.check(L.lvdgs_forward(C.byref(a), C.byref(D), stream), "lvdgs_forward")
    torch.cuda.synchronize()
    a.num_rendered = D.value
    lay = _lib.StateLayout()
    _lib.check(L.lvdgs_state_layout_query(N, cap, W, H, C.byref(lay)), "layout")
    view = lambda b, off, n, dt: b[off:off + n * np.dtype(dt).itemsize].cpu().numpy().view(dt).copy()
    T = ((W + 15) // 16) * ((H + 15) // 16)
    ranges = view(image, lay.img_ranges, 2 * T, np.uint32).reshape(T, 2).astype(np.int64)
    out["calls/pairs"] = np.int64([D.value])
    out["calls/list_lengths"] = (ranges[:, 1] - ranges[:, 0]).astype(np.int32)
    out["calls/color"], out["calls/depth"], out["calls/opacity"] = color.cpu().numpy(), depth.cpu().numpy(), opacity.cpu().numpy()
    out["calls/radii"], out["calls/n_touched"] = radii.cpu().numpy(), n_touched.cpu().numpy()
    out["calls/n_contrib"] = view(image, lay.img_n_contrib, W * H, np.uint32).astype(np.uint16)
    out["calls/final_T"] = view(image, lay.img_final_T, W * H, np.float32)

    gc, gd, go = (x.to(dev).contiguous() for x in synthetic.make_image_grads(W, H, 5))
    a.dL_dout_color = _p(gc)
    e = lambda *s: torch.zeros(*s, device=dev)
    for depth_grads in (True, False):
        a.dL_dout_depth, a.dL_dout_opacity = (_p(gd), _p(go)) if depth_grads else (None, None)
        tag = "calls/" + ("depth_grads" if depth_grads else "colour_only")
        gr = dict(means3D=e(N, 3), means2D=e(N, 3), opacities=e(N, 1), scales=e(N, 3), rotations=e(N, 4), colors=e(N, 3), tau=e(6))
        a.flags = 0
        a.dL_dmeans3D, a.dL_dmeans2D, a.dL_dopacities = _p(gr["means3D"]), _p(gr["means2D"]), _p(gr["opacities"])
        a.dL_dscales, a.dL_drotations, a.dL_dcolors, a.dL_dtau = _p(gr["scales"]), _p(gr["rotations"]), _p(gr["colors"]), _p(gr["tau"])
        _lib.check(L.lvdgs_backward(C.byref(a), stream), "lvdgs_backward")
        torch.cuda.synchronize()
        for k, v in gr.items():
            out[f"{tag}/full/{k}"] = v.cpu().numpy()
        tau = e(6)
        a.flags = _lib.FLAG_POSE_ONLY
        a.dL_dmeans3D = a.dL_dmeans2D = a.dL_dopacities = a.dL_dscales = a.dL_drotations = a.dL_dcolors = None
        a.dL_dtau = _p(tau)
        _lib.check(L.lvdgs_backward(C.byref(a), stream), "lvdgs_backward (pose only)")
        torch.cuda.synchronize()
        out[f"{tag}/pose_only/tau"] = tau.cpu().numpy()


def _fused_calls(g, out):
    """One iteration of a TrackingSession (lvdgs_forward_backward_fused_loss + lvdgs_tracking_tail): full / pose-only, monocular / RGB-D."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    import bench
    from lvdgs import _lib
    from lvdgs.camera_utils import Camera
    from lvdgs.fast_tracking import TrackingSession
    from lvdgs.gaussian_model import GaussianModel
    from lvdgs.graphics_utils import focal2fov, getProjectionMatrix2
    dev = torch.device("cuda", torch.cuda.current_device())
    fx = float(W)
    proj = getProjectionMatrix2(znear=0.01, zfar=100.0, fx=fx, fy=fx, cx=W / 2.0, cy=H / 2.0, W=W, H=H).transpose(0, 1).contiguous().to(dev)
    pipe = SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=False)
    lay = _lib.StateLayout()
    for monocular in (True, False):
        for full in (True, False):
            gen = torch.Generator().manual_seed(4242)
            image = torch.rand(3, H, W, generator=gen).to(dev)
            cam = Camera(1, image, None, (torch.rand(H, W, generator=gen) * 18 + 1).numpy(), torch.eye(4), proj, fx, fx, W / 2.0, H / 2.0,
                         focal2fov(fx, W), focal2fov(fx, H), H, W, device=dev)
            cam.grad_mask = (torch.rand(1, H, W, generator=gen) > 0.25).to(dev)
            with torch.no_grad():
                cam.exposure_a.fill_(0.03); cam.exposure_b.fill_(-0.02)
            model = GaussianModel.from_activated(g["means3D"], g["scales"], g["rotations"], g["opacities"], shs=g["shs"], sh_degree=0, device=dev)
            cfg = {k: (dict(v) if isinstance(v, dict) else v) for k, v in bench.CONFIG.items()}
            cfg["Training"]["monocular"] = monocular
            s = TrackingSession(cam, model, cfg, pipe, torch.zeros(3, device=dev), gaussian_gradients=full)
            assert s.pose_only == (not full)
            s.step()
            s.finish()
            tag = f"fused/{'mono' if monocular else 'rgbd'}/{'full' if full else 'pose_only'}"
            _lib.check(s.L.lvdgs_state_layout_query(N, s.cap, W, H, C.byref(lay)), "layout")
            nc = s.image[lay.img_n_contrib:lay.img_n_contrib + 4 * W * H].cpu().numpy().view(np.uint32)
            out[f"{tag}/n_contrib"] = nc.astype(np.uint16)
            for k, v in (("color", s.color), ("depth", s.depth), ("opacity", s.opacity), ("n_touched", s.n_touched), ("tau", s.d_tau),
                         ("loss_and_exposure", torch.cat([s.loss.reshape(1), s.d_a.reshape(1), s.d_b.reshape(1)]))):
                out[f"{tag}/{k}"] = v.cpu().numpy()
            if full:
                for k, v in (("means3D", s.d_m3), ("means2D", s.d_m2), ("opacities", s.d_op), ("scales", s.d_sc), ("rotations", s.d_rot), ("shs", s.d_sh)):
                    out[f"{tag}/{k}"] = v.cpu().numpy()
            del s, model


def collect():
    """Every result of every entry point on the scene: {name: numpy array}."""
    g = make_scene()
    out = {}
    _separate_calls(g, out)
    _fused_calls(g, out)
    return out


def digest(a):
    a = np.ascontiguousarray(a)
    return np.frombuffer(hashlib.sha256(a.tobytes()).digest(), np.uint8).copy()


def pack(results):
    """What the fixture holds of collect()'s dict: small arrays whole, large ones as the SHA-256 of their bytes (the comparison is
    bit for bit either way), every one with its shape and dtype."""
    packed = {}
    for k, v in results.items():
        v = np.ascontiguousarray(v)
        packed[k if v.nbytes <= WHOLE_LIMIT else "sha256:" + k] = v if v.nbytes <= WHOLE_LIMIT else digest(v)
        packed["meta:" + k] = np.array(f"{v.dtype.str} {v.shape}")
    return packed
