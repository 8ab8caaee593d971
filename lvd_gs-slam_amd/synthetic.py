"""Seeded synthetic scenes for parity tests and the benchmark.

The reference defines no synthetic input; this is the build's definition, generated on the CPU
with ``torch.Generator().manual_seed(seed)`` in float32 so that the CPU oracle and the GPU path
see identical bits.

* camera: pinhole fx = fy = W, cx = W/2, cy = H/2, znear 0.01, zfar 100
  (``utils/slam_frontend.py:1743-1748``); by default world == camera (R = I, T = 0),
  optionally a seeded rigid pose for the multi-keyframe cases;
* Gaussians: depth log-uniform [1, 50]; pixel uniform over [-0.1W, 1.1W] x [-0.1H, 1.1H];
  xyz by back-projection; pixel radius log-uniform [0.5, 8]; per-axis scale
  z*r/fx*U[0.7, 1.3]; unit quaternion from N(0,1)^4; opacity sigmoid(N(0, 1.5));
  colour rgb ~ U[0,1] (stored as the SH DC term (rgb - 0.5)/C0); SH degree 0.

Values are the *activated* quantities the rasterizer consumes (scale, not log-scale; opacity,
not logit), as ``render()`` passes them.
"""
import math
from types import SimpleNamespace

import torch

from .graphics_utils import focal2fov, getProjectionMatrix2
from .pose_utils import SE3_exp

SH_C0 = 0.28209479177387814


def make_camera(W, H, pose_seed=None, fx=None, fy=None, cx=None, cy=None, pose_scale=0.05):
    """Camera namespace with the attributes ``render()`` reads (float32 CPU tensors)."""
    fx = float(W) if fx is None else fx
    fy = float(W) if fy is None else fy
    cx = W / 2.0 if cx is None else cx
    cy = H / 2.0 if cy is None else cy
    w2c = torch.eye(4)
    if pose_seed is not None:
        g = torch.Generator().manual_seed(1000 + pose_seed)
        w2c = SE3_exp(torch.randn(6, generator=g) * pose_scale)
    proj = getProjectionMatrix2(znear=0.01, zfar=100.0, fx=fx, fy=fy, cx=cx, cy=cy, W=W, H=H).transpose(0, 1)
    view = w2c.transpose(0, 1).contiguous()
    cam = SimpleNamespace(
        image_width=W, image_height=H, fx=fx, fy=fy, cx=cx, cy=cy,
        FoVx=focal2fov(fx, W), FoVy=focal2fov(fy, H),
        R=w2c[:3, :3].contiguous(), T=w2c[:3, 3].contiguous(),
        world_view_transform=view, projection_matrix=proj.contiguous(),
        full_proj_transform=(view @ proj).contiguous(),
        camera_center=torch.linalg.inv(view)[3, :3].contiguous(),
        cam_rot_delta=torch.zeros(3), cam_trans_delta=torch.zeros(3),
    )
    cam.tanfovx = math.tan(cam.FoVx * 0.5)
    cam.tanfovy = math.tan(cam.FoVy * 0.5)
    return cam


def make_gaussians(N, W, H, seed=0, sh_degree=0, r_min=0.5, r_max=8.0, z_min=1.0, z_max=50.0):
    """dict of float32 CPU tensors: means3D (N,3), scales (N,3), rotations (N,4), opacities (N,1),
    shs (N,(deg+1)^2,3), colors (N,3)."""
    g = torch.Generator().manual_seed(seed)
    u = lambda *s: torch.rand(*s, generator=g)
    fx = float(W)
    z = torch.exp(u(N) * (math.log(z_max) - math.log(z_min)) + math.log(z_min))
    px = (u(N) * 1.2 - 0.1) * W
    py = (u(N) * 1.2 - 0.1) * H
    x = (px - W / 2.0) * z / fx
    y = (py - H / 2.0) * z / fx
    r = torch.exp(u(N) * (math.log(r_max) - math.log(r_min)) + math.log(r_min))
    scales = (z * r / fx)[:, None] * (0.7 + 0.6 * u(N, 3))
    q = torch.randn(N, 4, generator=g)
    q = q / q.norm(dim=1, keepdim=True)
    opac = torch.sigmoid(torch.randn(N, 1, generator=g) * 1.5)
    rgb = u(N, 3)
    K = (sh_degree + 1) ** 2
    shs = torch.zeros(N, K, 3)
    shs[:, 0] = (rgb - 0.5) / SH_C0
    if K > 1:
        shs[:, 1:] = torch.randn(N, K - 1, 3, generator=g) * 0.1
    return dict(means3D=torch.stack([x, y, z], 1).contiguous(), scales=scales.contiguous(), rotations=q.contiguous(),
                opacities=opac.contiguous(), shs=shs.contiguous(), colors=rgb.contiguous())


def make_surface_gaussians(N, W, H, seed=0, r_min=4.0, r_max=64.0, margin=0.1):
    """The regime real SLAM maps live in, which ``make_gaussians``' small random blobs never reach: opaque surfaces made
    of large, flat Gaussians.  Three slanted planes (depths around 3, 6 and 12, half of the Gaussians on the front one),
    footprints of r_min..r_max pixels (log-uniform, the in-plane sigma; a tenth of it along the normal), opacity
    sigmoid(N(2, 1)) ~ 0.88: tile lists of 500-2000 entries at ~100 Gaussians per 16x16 tile's worth of area, nearly
    every pixel saturating (transmittance below 1e-4) long before its list ends, rectangles of up to several hundred
    tiles.  Same dict as ``make_gaussians``.  ``margin``: how far past the frame of the camera at the origin the surfaces reach,
    in frame widths / heights (0.1, the workloads' value; the sequences of ``make_sequence`` move the camera and ask for more)."""
    g = torch.Generator().manual_seed(seed)
    u = lambda *s: torch.rand(*s, generator=g)
    fx = float(W)
    plane = torch.multinomial(torch.tensor([0.5, 0.3, 0.2]), N, replacement=True, generator=g)
    z0 = torch.tensor([3.0, 6.0, 12.0])[plane]
    slant = torch.tensor([[0.25, -0.1], [-0.2, 0.15], [0.1, 0.2]])[plane]
    span = 1.2 if margin == 0.1 else 1.0 + 2.0 * margin
    px = (u(N) * span - margin) * W
    py = (u(N) * span - margin) * H
    z = z0 * (1.0 + slant[:, 0] * (px / W - 0.5) + slant[:, 1] * (py / H - 0.5)) * (1.0 + 0.01 * torch.randn(N, generator=g))
    x = (px - W / 2.0) * z / fx
    y = (py - H / 2.0) * z / fx
    r = torch.exp(u(N) * (math.log(r_max) - math.log(r_min)) + math.log(r_min))
    s_in = (z * r / fx)[:, None] * (0.7 + 0.6 * u(N, 2))
    scales = torch.cat([s_in, 0.1 * s_in.mean(1, keepdim=True)], 1)      # thin along the (local) z axis
    q = torch.cat([torch.ones(N, 1), 0.15 * torch.randn(N, 3, generator=g)], 1)   # near the identity: the thin axis faces the camera
    q = q / q.norm(dim=1, keepdim=True)
    opac = torch.sigmoid(2.0 + torch.randn(N, 1, generator=g))
    rgb = u(N, 3)
    shs = ((rgb - 0.5) / SH_C0)[:, None, :].contiguous()
    return dict(means3D=torch.stack([x, y, z], 1).contiguous(), scales=scales.contiguous(), rotations=q.contiguous(),
                opacities=opac.contiguous(), shs=shs, colors=rgb.contiguous())


def make_workload_gaussians(name, seed=0):
    """The Gaussians of ``CONFIGS[name]`` (``kind``: "blobs", the default, or "surface")."""
    cfg = CONFIGS[name]
    make = make_surface_gaussians if cfg.get("kind") == "surface" else make_gaussians
    return make(cfg["N"], cfg["W"], cfg["H"], seed=seed)


def make_image_grads(W, H, seed=0):
    """Fixed seeded N(0,1) upstream gradients for (render, depth, opacity)."""
    g = torch.Generator().manual_seed(7000 + seed)
    return (torch.randn(3, H, W, generator=g), torch.randn(1, H, W, generator=g), torch.randn(1, H, W, generator=g))


CONFIGS = {
    # BASELINE.json configs[0..2]
    "cfg1_10k_640x480": dict(N=10_000, W=640, H=480),
    "cfg2_100k_640x480": dict(N=100_000, W=640, H=480),
    "cfg3_500k_1920x1080": dict(N=500_000, W=1920, H=1080),
    # KITTI-07 geometry (configs/mono/KITTI/07.yaml:8-18)
    "kitti07_geom": dict(N=200_000, W=1226, H=370, fx=707.0912, fy=707.0912, cx=601.8873, cy=183.1104),
    # the same pair density per tile as kitti07_geom on four times the area (diagnostic: is a 1848-tile frame slow per
    # pair because it leaves compute units idle?)
    "kitti07_x4": dict(N=800_000, W=2452, H=740, fx=1414.1824, fy=1414.1824, cx=1203.7746, cy=366.2208),
    # BASELINE.json configs[4] shape: 2 M Gaussians, waymo-sized frames (configs/mono/waymo/405841.yaml:15-16)
    "cfg5_2m_1920x1280": dict(N=2_000_000, W=1920, H=1280),
    # opaque surfaces of large flat Gaussians (make_surface_gaussians): lists of ~1000 entries per tile, saturating pixels
    "surface_100k_1920x1080": dict(N=100_000, W=1920, H=1080, kind="surface"),
    "surface_12k_640x480": dict(N=12_000, W=640, H=480, kind="surface"),
}


# ---------------------------------------------------------------------------------------------------------------------------
# Sequences: what FrontEnd.run reads from its dataset, frame by frame (reference utils/slam_frontend.py:1794-1797 ->
# utils/camera_utils.py Camera.init_from_dataset: ``dataset[idx] -> (image, depth, pose, mono_depth)`` and the intrinsics)
# ---------------------------------------------------------------------------------------------------------------------------
def dynamic_object_mask(H, W, seed):
    """A frame's ``static_mask`` (bool (H,W), True = static) as LVD-GS's front end makes it from GroundingDINO + SAM detections
    (utils/slam_frontend.py:1309-1329; the models are out of scope): two to four "vehicles" -- rectangles of 8-25 % of the image's
    width and 10-35 % of its height in the lower two thirds of the frame -- marked dynamic, seeded per frame."""
    m = torch.ones(H, W, dtype=torch.bool)
    for x0, y0, w, h in dynamic_object_rectangles(H, W, seed):
        m[y0:y0 + h, x0:x0 + w] = False
    return m


def dynamic_object_rectangles(H, W, seed):
    """The rectangles ``dynamic_object_mask`` marks, as (x0, y0, w, h) in its drawing order."""
    g = torch.Generator().manual_seed(7000 + seed)
    out = []
    for _ in range(2 + int(torch.randint(0, 3, (1,), generator=g))):
        w = int(W * (0.08 + 0.17 * float(torch.rand(1, generator=g)))); h = int(H * (0.10 + 0.25 * float(torch.rand(1, generator=g))))
        x0 = int(torch.randint(0, max(W - w, 1), (1,), generator=g)); y0 = H // 3 + int(torch.randint(0, max(H - H // 3 - h, 1), (1,), generator=g))
        out.append((x0, y0, w, h))
    return out


def vehicle_trajectory(n_frames, step=0.02, sway=0.15, yaw=0.03, period=40.0):
    """World-to-camera poses of a forward-moving camera: ``step`` along +z per frame with a sinusoidal lateral sway (amplitude
    ``sway``), a smaller vertical one and a yaw oscillation of ``yaw`` radians, period ``period`` frames; frame 0 at the identity
    (the front end adopts the first ground-truth pose, utils/slam_frontend.py:1718)."""
    poses = []
    for i in range(n_frames):
        ph = 2.0 * math.pi * i / period
        c2w = torch.eye(4)
        a = yaw * math.sin(ph)
        c2w[0, 0], c2w[0, 2], c2w[2, 0], c2w[2, 2] = math.cos(a), math.sin(a), -math.sin(a), math.cos(a)
        c2w[:3, 3] = torch.tensor([sway * (1.0 - math.cos(ph)) * 0.5, 0.2 * sway * math.sin(ph), step * i])
        poses.append(torch.linalg.inv(c2w))
    return poses


class SequenceDataset:
    """Frames held in memory with the interface ``Camera.init_from_dataset`` reads (reference utils/camera_utils.py:56-75):
    ``dataset[idx] -> (image (3,H,W) on the device, depth (H,W) numpy or None, ground-truth world-to-camera pose (4,4), mono
    depth (H,W) numpy float32)``, the intrinsics and ``device``.  ``static_mask(idx)``: the frame's static mask where the
    sequence carries dynamic objects (what the reference's ``dynamic_masker`` would return), else None."""

    def __init__(self, images, mono_depths, poses, W, H, fx, fy, cx, cy, device, depths=None, static_masks=None):
        self.images, self.mono_depths, self.poses, self.depths, self.static_masks = images, mono_depths, poses, depths, static_masks
        self.width, self.height, self.fx, self.fy, self.cx, self.cy, self.device = W, H, fx, fy, cx, cy, device
        self.fovx, self.fovy = focal2fov(fx, W), focal2fov(fy, H)
        self.dist_coeffs = None

    def __len__(self):
        return len(self.images)

    def __getitem__(self, idx):
        return (self.images[idx], None if self.depths is None else self.depths[idx], self.poses[idx].to(self.device), self.mono_depths[idx])

    def static_mask(self, idx):
        return None if self.static_masks is None else self.static_masks[idx]

    def to(self, device):
        """The same frames held on another device."""
        ds = SequenceDataset([t.to(device) for t in self.images], self.mono_depths, self.poses, self.width, self.height, self.fx, self.fy,
                             self.cx, self.cy, device, depths=self.depths,
                             static_masks=None if self.static_masks is None else [m.to(device) for m in self.static_masks])
        if hasattr(self, "dynamic_seeds"):
            ds.dynamic_seeds = self.dynamic_seeds
        return ds


def make_sequence(truth, render_fn, pipe, W, H, n_frames, device, fx=None, fy=None, cx=None, cy=None, seed=0, depth_noise=0.02,
                  image_noise=0.0, dynamic_objects=False, step=0.02, sway=0.15, yaw=0.03, period=40.0, camera_cls=None, mono_scale_drift=0.0,
                  metric_depth=False):
    """``n_frames`` frames of ``vehicle_trajectory`` through the map ``truth`` (a GaussianModel), rendered ONCE by ``render_fn``
    (the product's ``render`` on the GPU, the dense float64 renderer in the CPU tests): image = clamped render (+ seeded pixel
    noise), mono depth = expected depth of the opaque pixels x (1 + ``depth_noise`` N(0,1)) -- a metric depth predictor's output,
    what ``get_depth`` (the pointmap of MASt3R, which is out of scope) hands the reference's front end.  ``dynamic_objects``: every frame also carries two
    to four flat-coloured rectangles ("vehicles", ``dynamic_object_mask``, redrawn per frame: they move) painted over the image
    and marked dynamic in ``static_mask(idx)``.  ``mono_scale_drift``: frame i's mono depth is further multiplied by
    ``mono_scale_factor(i, mono_scale_drift)`` -- a monocular predictor's per-frame scale inconsistency, what the keyframe depth
    alignment (LVD-GS Algorithm 1) exists for; deterministic, no random draws (at 0 the dataset is bit-identical to one made without
    it).  The factors are kept as ``dataset.mono_scales``.  ``metric_depth``: the frames also carry the expected depth itself, without
    noise or drift and 0 where the map is not opaque, as ``dataset[idx][1]`` -- a ground-truth depth sensor, what ``SlamSequence.eval_mesh``
    fuses its ground-truth surface from (a monocular run reads no depth plane; no random draw is added or moved)."""
    if camera_cls is None:
        from .camera_utils import Camera as camera_cls
    fx = float(W) if fx is None else fx
    fy = float(W) if fy is None else fy
    cx = W / 2.0 if cx is None else cx
    cy = H / 2.0 if cy is None else cy
    proj = getProjectionMatrix2(znear=0.01, zfar=100.0, fx=fx, fy=fy, cx=cx, cy=cy, W=W, H=H).transpose(0, 1)
    bg = torch.zeros(3, device=device)
    gen = torch.Generator().manual_seed(9000 + seed)
    images, monos, masks, truths = [], [], [], []
    poses = vehicle_trajectory(n_frames, step, sway, yaw, period)
    for i, w2c in enumerate(poses):
        cam = camera_cls(i, torch.zeros(3, H, W, device=device), None, None, torch.eye(4), proj.to(device), fx, fy, cx, cy,
                         focal2fov(fx, W), focal2fov(fy, H), H, W, device=device)
        cam.update_RT(w2c[:3, :3].to(device), w2c[:3, 3].to(device))
        with torch.no_grad():
            pkg = render_fn(cam, truth, pipe, bg)
        img = pkg["render"].detach().float()
        if image_noise:
            img = img + image_noise * torch.randn(3, H, W, generator=gen).to(img.device)
        img = img.clamp(0.0, 1.0)
        opac = pkg["opacity"][0].detach().float()
        depth = torch.where(opac > 0.5, pkg["depth"][0].detach().float() / opac.clamp(min=1e-3), torch.zeros_like(opac))
        if metric_depth:
            truths.append(depth.cpu().numpy().astype("float32"))
        depth = depth * (1.0 + depth_noise * torch.randn(H, W, generator=gen).to(depth.device))
        if mono_scale_drift:
            depth = depth * mono_scale_factor(i, mono_scale_drift)
        if dynamic_objects:
            m = dynamic_object_mask(H, W, 100 * seed + i)
            colour = torch.rand(3, generator=gen)
            img = torch.where(m.to(img.device)[None], img, colour.to(img.device)[:, None, None].expand_as(img))
            masks.append(m.to(device))
        images.append(img.contiguous().to(device))
        monos.append(depth.cpu().numpy().astype("float32"))
    ds = SequenceDataset(images, monos, poses, W, H, fx, fy, cx, cy, device, depths=truths if metric_depth else None,
                         static_masks=masks if dynamic_objects else None)
    ds.mono_scales = [mono_scale_factor(i, mono_scale_drift) if mono_scale_drift else 1.0 for i in range(len(poses))]
    if dynamic_objects:
        ds.dynamic_seeds = [100 * seed + i for i in range(len(poses))]      # dynamic_object_rectangles' seeds (RectangleDetector)
    return ds


def mono_scale_factor(i, drift):
    """Frame i's mono depth scale under ``make_sequence(..., mono_scale_drift=drift)``: 1 + drift * sin(2 pi i / 11) -- a
    wander between 1 - drift and 1 + drift that never repeats within a short drive."""
    return 1.0 + drift * math.sin(2.0 * math.pi * i / 11.0)


class RectangleDetector:
    """A stand-in for BOTH networks behind ``dynamic_mask.DynamicMasker`` (GroundingDINO and SAM, out of scope) on a
    ``SequenceDataset`` made with ``dynamic_objects=True``: the rectangles ``dynamic_object_mask`` drew on a frame come back as pixel
    boxes (x0, y0, x0 + w, y0 + h) labelled "car" -- ``detect(image, frame_idx) -> (boxes (K, 4) float32 on the image's device,
    labels)``, the GroundingDINO seat -- and as one exact mask per rectangle -- ``segment(image, boxes) -> (K, H, W)`` bool, the SAM
    seat, for the frame ``detect`` was last asked about."""

    def __init__(self, dataset):
        if not hasattr(dataset, "dynamic_seeds"):
            raise ValueError("RectangleDetector needs a dataset made by make_sequence(dynamic_objects=True)")
        self.dataset, self.frame = dataset, None

    def rectangles(self, idx):
        return dynamic_object_rectangles(self.dataset.height, self.dataset.width, self.dataset.dynamic_seeds[idx])

    def detect(self, image, frame_idx):
        self.frame = int(frame_idx)
        rows = [[x0, y0, x0 + w, y0 + h] for x0, y0, w, h in self.rectangles(self.frame)]
        return torch.tensor(rows, dtype=torch.float32).reshape(-1, 4).to(image.device), ["car"] * len(rows)

    def segment(self, image, boxes):
        rects = self.rectangles(self.frame)
        masks = torch.zeros(len(rects), self.dataset.height, self.dataset.width, dtype=torch.bool)
        for m, (x0, y0, w, h) in zip(masks, rects):
            m[y0:y0 + h, x0:x0 + w] = True
        return masks.to(image.device)


class GroundTruthMatcher:
    """A stand-in for the whole matcher of ``init_pose.get_pose`` (MASt3R descriptors + ``fast_reciprocal_NNs(subsample_or_initxy1=8)``)
    that matches nothing: 2D-2D matches between a keyframe and a frame of a ``SequenceDataset`` made from the ground truth.  (Only the
    descriptor network is out of scope: ``WorldDescriptors`` below stands in for it alone, under ``init_pose.DescriptorMatcher``.)

    The stride-``stride`` grid of the keyframe at the matcher's raster; every grid point is carried into the new frame with the two
    ground-truth poses and the keyframe's mono depth at that pixel (points without depth are dropped), perturbed by Gaussian noise of
    ``noise_px`` raster pixels, and dropped when it leaves the frame.  A seeded share ``outlier_ratio`` of the matches -- and every match
    that lies on a dynamic rectangle in either frame: those objects move -- is replaced by a uniformly random pixel of the new frame.
    ``set_frames(keyframe_idx, frame_idx)`` says which pair the next call is about (``SlamSequence`` calls it); the call itself has the
    matcher's signature ``(img1, img2, model, (W1, H1)) -> (matches_im1 (M, 2) int32, matches_im2 (M, 2) float32)``, NumPy arrays."""

    def __init__(self, dataset, stride=8, noise_px=0.7, outlier_ratio=0.3, seed=0):
        self.dataset, self.stride, self.noise_px, self.outlier_ratio, self.seed = dataset, int(stride), float(noise_px), float(outlier_ratio), int(seed)
        self.pair = None

    def set_frames(self, keyframe_idx, frame_idx):
        self.pair = (int(keyframe_idx), int(frame_idx))

    def __call__(self, img1, img2, model, raster):
        import numpy as np
        if self.pair is None:
            raise RuntimeError("GroundTruthMatcher: set_frames(keyframe_idx, frame_idx) first")
        kf, cur = self.pair
        ds = self.dataset
        W1, H1 = raster
        sw, sh = W1 / ds.width, H1 / ds.height
        rng = np.random.default_rng([self.seed, kf, cur])
        gy, gx = np.meshgrid(np.arange(self.stride // 2, H1, self.stride), np.arange(self.stride // 2, W1, self.stride), indexing="ij")
        gx, gy = gx.ravel(), gy.ravel()
        # the full-size pixel under each grid point
        fx_, fy_ = np.minimum((gx / sw).round().astype(np.int64), ds.width - 1), np.minimum((gy / sh).round().astype(np.int64), ds.height - 1)
        Z = np.asarray(ds.mono_depths[kf], dtype=np.float64)[fy_, fx_]
        P = np.stack([(gx / sw - ds.cx) / ds.fx * Z, (gy / sh - ds.cy) / ds.fy * Z, Z], 1)
        T1, T2 = ds.poses[kf].double().cpu().numpy(), ds.poses[cur].double().cpu().numpy()
        rel = T2 @ np.linalg.inv(T1)
        X = P @ rel[:3, :3].T + rel[:3, 3]
        with np.errstate(all="ignore"):
            u = (ds.fx * X[:, 0] / X[:, 2] + ds.cx) * sw + self.noise_px * rng.normal(size=len(Z))
            v = (ds.fy * X[:, 1] / X[:, 2] + ds.cy) * sh + self.noise_px * rng.normal(size=len(Z))
            keep = (Z > 0) & np.isfinite(Z) & (X[:, 2] > 0) & (u >= 0) & (u <= W1 - 1) & (v >= 0) & (v <= H1 - 1)
        gx, gy, fx_, fy_, u, v = gx[keep], gy[keep], fx_[keep], fy_[keep], u[keep], v[keep]
        M = len(gx)
        bad = rng.random(M) < self.outlier_ratio
        m1s, m2s = ds.static_mask(kf), ds.static_mask(cur)
        if m1s is not None:
            bad |= ~m1s.cpu().numpy()[fy_, fx_]
        if m2s is not None:
            ux, vy = np.clip((u / sw).round().astype(np.int64), 0, ds.width - 1), np.clip((v / sh).round().astype(np.int64), 0, ds.height - 1)
            bad |= ~m2s.cpu().numpy()[vy, ux]
        u = np.where(bad, rng.uniform(0, W1 - 1, M), u)
        v = np.where(bad, rng.uniform(0, H1 - 1, M), v)
        return np.stack([gx, gy], 1).astype(np.int32), np.stack([u, v], 1).astype(np.float32)


class WorldDescriptors:
    """The stand-in for the descriptor network of the reference's matcher (MASt3R, out of scope): dense descriptor maps of a keyframe
    and a frame of a ``SequenceDataset`` at the matcher's raster, for ``init_pose.DescriptorMatcher`` to match.

    A raster pixel is back-projected with the frame's mono depth (the full-size pixel under it; ``smooth`` > 1: the mean of the valid
    depths in the ``smooth`` x ``smooth`` full-size pixels around it -- a network's descriptor sees a neighbourhood, not one pixel's
    depth noise) and the frame's true pose; the world point p goes through seeded random Fourier features cos(p . f_k + b_k), k < ``dim``
    (f_k ~ N(0, ``freq``^2) rad per world unit, b_k uniform), seeded N(0, ``noise``^2) is added per component (per frame: two frames see
    different noise) and the vector is unit-normalised.  Pixels without depth, and pixels on a dynamic rectangle of the frame's static
    mask -- those objects move -- get seeded random unit vectors: they match nothing consistently.  Everything is float32 tensor
    arithmetic on the dataset's device.  ``set_frames(keyframe_idx, frame_idx)`` says which pair the next call is about (``SlamSequence``
    calls it through the matcher); the call has the network's seat in ``DescriptorMatcher``: ``(img1, img2, model, (W1, H1)) -> (desc1,
    desc2)``, (H1, W1, dim) float32 tensors."""

    def __init__(self, dataset, dim=24, seed=0, noise=0.02, freq=8.0, smooth=5):
        self.dataset, self.dim, self.seed, self.noise, self.freq, self.smooth = dataset, int(dim), int(seed), float(noise), float(freq), int(smooth)
        g = torch.Generator().manual_seed(31000 + self.seed)
        self.f = (self.freq * torch.randn(3, self.dim, generator=g)).to(dataset.device)
        self.b = (2.0 * math.pi * torch.rand(self.dim, generator=g)).to(dataset.device)
        self.pair = None

    def set_frames(self, keyframe_idx, frame_idx):
        self.pair = (int(keyframe_idx), int(frame_idx))

    def describe(self, idx, raster):
        """The descriptor map of frame ``idx`` at ``raster`` = (W1, H1)."""
        ds, dev = self.dataset, self.dataset.device
        W1, H1 = raster
        sw, sh = W1 / ds.width, H1 / ds.height
        gx, gy = torch.arange(W1, device=dev, dtype=torch.float32), torch.arange(H1, device=dev, dtype=torch.float32)
        px = (gx / sw).round().clamp(max=ds.width - 1).long()
        py = (gy / sh).round().clamp(max=ds.height - 1).long()
        mono = torch.as_tensor(ds.mono_depths[idx], dtype=torch.float32, device=dev)
        valid = torch.isfinite(mono) & (mono > 0)
        mono = torch.where(valid, mono, torch.zeros_like(mono))
        if self.smooth > 1:
            box = lambda t: torch.nn.functional.avg_pool2d(t[None, None], self.smooth, stride=1, padding=self.smooth // 2, count_include_pad=True)[0, 0]
            mono = box(mono) / box(valid.float()).clamp(min=1e-6)
        Z = mono[py][:, px]
        ok = valid[py][:, px]
        m = ds.static_mask(idx)
        if m is not None:
            ok = ok & m.to(dev)[py][:, px]
        X = (gx[None, :] / sw - ds.cx) / ds.fx * Z
        Y = (gy[:, None] / sh - ds.cy) / ds.fy * Z
        T = ds.poses[idx].to(device=dev, dtype=torch.float32)
        P = (torch.stack([X, Y, Z], -1) - T[:3, 3]) @ T[:3, :3]      # world = R^T (camera - t)
        g = torch.Generator().manual_seed(32000 + 1000 * self.seed + int(idx))
        d = torch.cos(P @ self.f + self.b) + self.noise * torch.randn(H1, W1, self.dim, generator=g).to(dev)
        d = torch.where(ok[..., None], d, torch.randn(H1, W1, self.dim, generator=g).to(dev))
        return (d / d.norm(dim=-1, keepdim=True).clamp(min=1e-12)).contiguous()

    def __call__(self, img1, img2, model, raster):
        if self.pair is None:
            raise RuntimeError("WorldDescriptors: set_frames(keyframe_idx, frame_idx) first")
        return self.describe(self.pair[0], raster), self.describe(self.pair[1], raster)
