"""The fused seeding on the GPU (lvdgs_seed_points, lvdgs.seeding.seed_points, GaussianModel.seeding = "fused"): bit for bit the
NumPy oracle (tests/seeding_oracle.py), the edge counts, determinism, today's host path handed the same pixels, the model and the
toy sequence.  The rule's own properties and the ABI without a GPU: tests/test_seeding.py."""
import ctypes as C
import os
import random
import sys

import numpy as np
import pytest
import torch

import seeding_cases as cases
import seeding_oracle as oracle

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "tools"))
pytestmark = pytest.mark.gpu

EXPOSURE_A, EXPOSURE_B = 0.08, -0.0234
OPT = dict(position_lr_init=0.0016, position_lr_final=0.00016, position_lr_delay_mult=0.01, position_lr_max_steps=30000,
           feature_lr=0.0025, opacity_lr=0.05, scaling_lr=0.001, rotation_lr=0.001, percent_dense=0.01,
           densify_grad_threshold=0.0002, lambda_dssim=0.2)


def bits(t):
    a = t.detach().cpu().contiguous().numpy() if torch.is_tensor(t) else np.ascontiguousarray(t)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def fused(image, depth, ds, seed, want_median=False, gain=None, offset=None):
    from lvdgs.seeding import seed_points
    R, T = cases.pose()
    return seed_points(None if image is None else torch.from_numpy(image).cuda(), torch.from_numpy(depth).cuda(), cases.INTRINSICS,
                       torch.from_numpy(R).cuda(), torch.from_numpy(T).cuda(), ds, seed, gain=gain, offset=offset, want_median=want_median)


def same_as_oracle(got, want):
    assert (got.n_valid, got.n) == (want["n_valid"], want["n_keep"])
    assert np.array_equal(got.pixel.cpu().numpy(), want["pixel"].astype(np.int32))
    assert got.xyz.shape == (got.n, 3) and np.array_equal(bits(got.xyz), bits(want["xyz"]))
    if "rgb" in want:
        assert np.array_equal(bits(got.rgb), bits(want["rgb"])) and np.array_equal(bits(got.f_dc), bits(want["f_dc"]))
    if want["threshold"] is not None:
        assert got.threshold == want["threshold"]


@pytest.mark.parametrize("W,H,ds", [(W, H, ds) for (W, H), ds in zip(cases.SIZES, (4, 8, 32))])
def test_bits_against_the_oracle(W, H, ds):
    from lvdgs.seeding import call_seed
    seed = call_seed(0, W)
    depth, image = cases.depth_map(W, H), cases.image(W, H)
    a, b = torch.tensor([EXPOSURE_A], device="cuda"), torch.tensor([EXPOSURE_B], device="cuda")
    gain = torch.exp(a)
    got = fused(image, depth, ds, seed, gain=gain, offset=b)
    R, T = cases.pose()
    want = oracle.seed_points(image, depth, cases.INTRINSICS, R, T, 1.0 / ds, seed, gain=float(gain.cpu()), offset=float(b.cpu()))
    print(f"{W}x{H} ds {ds}: n_valid {got.n_valid} ({got.n_valid / (W * H):.3f}), n_keep {got.n}, threshold {got.threshold:#010x}")
    assert 0.55 < got.n_valid / (W * H) < 0.65 and got.n > 0
    assert np.isnan(got.median_depth) and got.median_bits == 0x7FC00000      # not asked for
    same_as_oracle(got, want)
    # today's statements (create_pcd_from_image) at those pixels
    image_ab = (torch.exp(a) * torch.from_numpy(image).cuda() + b).clamp(0.0, 1.0)
    rgb = (image_ab * 255).to(torch.uint8).to(torch.float32) / 255.0
    px = got.pixel.long()
    assert torch.equal(rgb.reshape(3, -1)[:, px].t().contiguous(), got.rgb)
    q = (got.rgb * 255).round()
    assert float(q.min()) == 0 and float(q.max()) == 255      # both clamps are in the selection
    # the median, on a depth map without NaN
    clean = cases.depth_map(W, H, specials=False)
    with_median = fused(None, clean, ds, seed, want_median=True)
    want_median = torch.from_numpy(clean).cuda().median()
    assert with_median.median_bits == int(bits(want_median.reshape(1))[0]) == int(bits(oracle.lower_median(clean).reshape(1))[0])
    assert with_median.rgb is None and with_median.f_dc is None
    same_as_oracle(with_median, oracle.seed_points(None, clean, cases.INTRINSICS, R, T, 1.0 / ds, seed))


@pytest.mark.parametrize("W,H,ds", [(W, H, ds) for (W, H), ds in zip(cases.SIZES, (4, 8, 32))])
def test_median_of_negative_markers_and_infinities(W, H, ds):
    """Every depth takes part in depth.median(): -1 markers, other negatives, both zeros and +inf go through the select's negative branch and
    across the sign in its bucket choice; here the median itself is negative."""
    depth = cases.marked_depth_map(W, H)
    got = fused(None, depth, ds, 80, want_median=True)
    want = oracle.lower_median(depth)
    assert want < 0 and want != -1.0 and np.isinf(depth).any() and (depth == -1.0).any()
    assert got.median_bits == int(bits(want.reshape(1))[0]) == int(bits(torch.from_numpy(depth).cuda().median().reshape(1))[0])
    R, T = cases.pose()
    same_as_oracle(got, oracle.seed_points(None, depth, cases.INTRINSICS, R, T, 1.0 / ds, 80))
    assert got.n > 0


def _sparse(W, H, n_valid, seed=4):
    d = np.zeros((H, W), np.float32)
    at = np.random.default_rng(seed).choice(W * H, size=n_valid, replace=False)
    d.reshape(-1)[at] = 3.0 + (np.arange(n_valid) % 90).astype(np.float32)      # all within the truncation
    return d


@pytest.mark.parametrize("n_valid,n_keep", [(0, 0), (7, 0), (8, 1), (9, 1), (23 * 37, 106)])
def test_edge_counts(n_valid, n_keep):
    W, H, ds, seed = 23, 37, 8, 77
    depth, image = _sparse(W, H, n_valid), cases.image(W, H)
    got = fused(image, depth, ds, seed)
    R, T = cases.pose()
    assert (got.n_valid, got.n) == (n_valid, n_keep) and got.xyz.shape == (n_keep, 3) and got.pixel.shape == (n_keep,)
    same_as_oracle(got, oracle.seed_points(image, depth, cases.INTRINSICS, R, T, 1.0 / ds, seed))
    if n_valid == W * H:      # all valid: n_keep is the capacity exactly (the host-side bound), every row of the buffers is written
        assert got.n == int(W * H * (1.0 / ds))


@pytest.mark.parametrize("ds", [1, 3])
def test_every_valid_pixel_and_a_downsample_that_is_no_power_of_two(ds):
    W, H, seed = 23, 37, 78
    depth, image = cases.depth_map(W, H), cases.image(W, H)
    got = fused(image, depth, ds, seed)
    R, T = cases.pose()
    same_as_oracle(got, oracle.seed_points(image, depth, cases.INTRINSICS, R, T, 1.0 / ds, seed))
    assert got.n == int(got.n_valid * (1.0 / ds))
    if ds == 1:      # everything valid, in raster order
        assert np.array_equal(got.pixel.cpu().numpy(), np.flatnonzero(oracle.valid_mask(depth)).astype(np.int32))


def test_no_image_leaves_the_colour_buffers_alone():
    from lvdgs import _lib
    W, H, ds, seed = 23, 37, 8, 79
    depth = torch.from_numpy(cases.depth_map(W, H)).cuda()
    R, T = (torch.from_numpy(x).cuda() for x in cases.pose())
    cap = int(W * H * (1.0 / ds))
    xyz = torch.zeros(cap, 3, device="cuda")
    rgb, f_dc = torch.full((cap, 3), 7.0, device="cuda"), torch.full((cap, 3), -7.0, device="cuda")
    L = _lib.lib()
    block = torch.zeros(_lib.SEED_HOST_BYTES, dtype=torch.uint8).pin_memory()
    scratch = _lib.device_bytes(L.lvdgs_seed_scratch_bytes(W, H), depth.device)
    fx, fy, cx, cy = cases.INTRINSICS
    a = _lib.SeedArgs(width=W, height=H, fx=fx, fy=fy, cx=cx, cy=cy, depth_trunc=100.0, want_median=0, inv_downsample=1.0 / ds, seed=seed,
                      seq=41, capacity=cap, image=None, gain=None, offset=None, depth=depth.data_ptr(), R=R.data_ptr(), T=T.data_ptr(),
                      xyz=xyz.data_ptr(), rgb=rgb.data_ptr(), f_dc=f_dc.data_ptr(), pixel=None, host_state=block.data_ptr(),
                      scratch=scratch.data_ptr(), scratch_bytes=scratch.numel())
    _lib.check(L.lvdgs_seed_points(C.byref(a), _lib.raw_stream(depth.device)), "lvdgs_seed_points")
    torch.cuda.current_stream().synchronize()
    w = block.numpy().view(np.int32)
    want = oracle.seed_points(None, depth.cpu().numpy(), cases.INTRINSICS, *cases.pose(), 1.0 / ds, seed)
    assert (int(w[_lib.SEED_SEQ]), int(w[_lib.SEED_N_VALID]), int(w[_lib.SEED_N_KEEP])) == (41, want["n_valid"], want["n_keep"])
    assert np.array_equal(bits(xyz[:want["n_keep"]]), bits(want["xyz"]))
    assert bool((rgb == 7.0).all()) and bool((f_dc == -7.0).all())


def test_two_calls_give_the_same_bytes_and_another_seed_another_set():
    W, H, ds = 96, 70, 8
    depth, image = cases.depth_map(W, H, specials=False), cases.image(W, H)
    a, b, c = fused(image, depth, ds, 1234, want_median=True), fused(image, depth, ds, 1234, want_median=True), fused(image, depth, ds, 1235)
    for name in ("xyz", "rgb", "f_dc", "pixel"):
        assert np.array_equal(bits(getattr(a, name)), bits(getattr(b, name))), name
    assert (a.n, a.n_valid, a.median_bits, a.threshold) == (b.n, b.n_valid, b.median_bits, b.threshold)
    assert c.n == a.n and not np.array_equal(c.pixel.cpu().numpy(), a.pixel.cpu().numpy())


# ---------------------------------------------------------------- the model
def _camera(W, H, image, intrinsics=None, pose=True):
    from lvdgs.camera_utils import Camera
    from lvdgs.graphics_utils import focal2fov, getProjectionMatrix2
    fx, fy, cx, cy = intrinsics or (float(W), float(W), W / 2.0, H / 2.0)
    proj = getProjectionMatrix2(znear=0.01, zfar=100.0, fx=fx, fy=fy, cx=cx, cy=cy, W=W, H=H).transpose(0, 1)
    cam = Camera(0, torch.from_numpy(image).cuda(), None, None, torch.eye(4), proj.cuda(), fx, fy, cx, cy, focal2fov(fx, W), focal2fov(fy, H),
                 H, W, device="cuda")
    if pose:
        R, T = cases.pose()
        cam.update_RT(torch.from_numpy(R).cuda(), torch.from_numpy(T).cuda())
    with torch.no_grad():
        cam.exposure_a.fill_(EXPOSURE_A)
        cam.exposure_b.fill_(EXPOSURE_B)
    return cam


def _model(seeding, ds=8, adaptive=True):
    from lvdgs.gaussian_model import GaussianModel
    cfg = {"Dataset": {"sensor_type": "depth", "pcd_downsample": ds, "pcd_downsample_init": ds, "point_size": 0.01, "adaptive_pointsize": adaptive}}
    m = GaussianModel(0, config=cfg)
    m.seeding = seeding
    m.init_lr(6.0)
    m.training_setup(OPT)
    return m


def test_against_todays_path_on_the_same_pixels():
    """1226 x 370, one seed per 64 valid pixels: the host statements handed the fused call's pixel list."""
    from lvdgs.simple_knn import distCUDA2
    W, H, ds = 1226, 370, 64
    depth_np, image = cases.depth_map(W, H, valid_share=0.8, specials=False), cases.image(W, H)
    cam = _camera(W, H, image, cases.INTRINSICS)
    m = _model("fused", ds)
    xyz, features, scales, rots, opacities = m.create_pcd_from_image(cam, init=False, depthmap=depth_np)
    assert m.seed_calls == 1
    colors = m.ply_input[1]
    from lvdgs.seeding import call_seed, seed_points
    depth = torch.from_numpy(depth_np).cuda()
    again = seed_points(cam.original_image, depth, (cam.fx, cam.fy, cam.cx, cam.cy), cam.R, cam.T, ds, call_seed(0, 0))
    assert torch.equal(again.xyz, xyz) and xyz.shape[0] == int(int(oracle.valid_mask(depth_np).sum()) * (1.0 / ds))
    # today's statements
    px = again.pixel.long()
    v, u = px // W, px % W
    z = depth[v, u]
    cam_pts = torch.stack(((u.float() - cam.cx) * z / cam.fx, (v.float() - cam.cy) * z / cam.fy, z), dim=1)
    R, T = cam.R.cuda().float(), cam.T.cuda().float()
    host_xyz = (cam_pts - T[None, :]) @ R
    # |ours - theirs| <= 8 * 2^-24 * sum_k |cam_k - T_k| |R_kj|: twice the bound of a three-term float32 sum of products (each product
    # one rounding, two additions), because the matmul's order of summation is not ours
    bound = 8 * 2.0 ** -24 * ((cam_pts - T[None, :]).double().abs() @ R.double().abs())
    err = (xyz.double() - host_xyz.double()).abs()
    print(f"xyz: max error {float(err.max()):.3e}, max error / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())
    image_ab = (torch.exp(cam.exposure_a.detach()) * cam.original_image + cam.exposure_b.detach()).clamp(0.0, 1.0)
    rgb = (image_ab * 255).to(torch.uint8).to(torch.float32) / 255.0
    assert torch.equal(rgb[:, v, u].t().contiguous(), colors)
    # the scales: today's statements on the same xyz, the median read the old way
    point_size = min(0.05, 0.01 * float(depth.median()))
    dist2 = torch.clamp_min(distCUDA2(xyz), 0.0000001) * point_size
    assert torch.equal(torch.log(torch.sqrt(dist2))[:, None].repeat(1, 3), scales)
    assert torch.equal(rots, torch.tensor([1.0, 0, 0, 0], device="cuda").repeat(xyz.shape[0], 1)) and bool((opacities == 0).all())
    assert torch.allclose(features[:, :, 0], (colors - 0.5) / 0.28209479177387814, rtol=1e-6, atol=1e-7)


def _keyframes(W, H, n):
    return [(_camera(W, H, cases.image(W, H, seed=10 + i)), cases.depth_map(W, H, seed=20 + i, specials=False)) for i in range(n)]


def test_two_fused_models_hold_the_same_bits():
    W, H = 160, 96
    frames = _keyframes(W, H, 3)
    models = [_model("fused"), _model("fused")]
    for m in models:
        for i, (cam, depth) in enumerate(frames):
            m.extend_from_pcd_seq(cam, kf_id=i, init=i == 0, depthmap=depth)
        assert m.seed_calls == 3
    a, b = models
    assert a.get_xyz.shape[0] > 0
    for pa, pb in zip(a.parameters(), b.parameters()):
        assert np.array_equal(bits(pa), bits(pb))
    assert torch.equal(a.unique_kfIDs, b.unique_kfIDs)


def test_extend_from_pcd_seq_in_fused_mode():
    W, H, ds = 160, 96, 8
    frames = _keyframes(W, H, 2)
    m, host = _model("fused", ds), _model("host", ds)
    counts = [int(int(oracle.valid_mask(d).sum()) * (1.0 / ds)) for _, d in frames]
    m.extend_from_pcd_seq(frames[0][0], kf_id=0, init=True, depthmap=frames[0][1])
    host.extend_from_pcd_seq(frames[0][0], kf_id=0, init=True, depthmap=frames[0][1])
    assert m.get_xyz.shape[0] == counts[0] == host.get_xyz.shape[0]      # the first seeding of a drive: the host mode's count
    # one optimiser step, so that there are Adam moments to extend
    for p in m.parameters():
        p.grad = torch.ones_like(p)
    m.optimizer.step()
    m.extend_from_pcd_seq(frames[1][0], kf_id=5, init=False, depthmap=frames[1][1])
    n0, n = counts[0], counts[0] + counts[1]
    assert m.get_xyz.shape[0] == n and all(p.shape[0] == n for p in m.parameters())
    assert m.unique_kfIDs.tolist() == [0] * n0 + [5] * counts[1] and m.n_obs.shape == (n,) and int(m.n_obs[n0:].sum()) == 0
    assert m.max_radii2D.shape == (n,) and m.denom.shape == (n, 1)
    for group in m.optimizer.param_groups:
        state = m.optimizer.state.get(group["params"][0])
        assert state or group["name"] == "f_rest", group["name"]      # (degree 0: f_rest has no elements)
        for key in ("exp_avg", "exp_avg_sq") if state else ():
            assert state[key].shape[0] == n and bool((state[key][n0:] == 0).all()), (group["name"], key)
            if state[key][:n0].numel():
                assert bool((state[key][:n0] != 0).any()), (group["name"], key)
    assert m.seed_calls == 2 and host.seed_calls == 0


# ---------------------------------------------------------------- the sequence
def test_toy_sequence_with_fused_seeding():
    import sequence_scene as ss
    from lvdgs.slam_sequence import SlamSequence
    cfg, ds, _, _, _ = ss.toy_sequence_on_cpu()
    ds = ds.to("cuda")
    runs = {}
    for mode in ("host", "fused"):
        torch.manual_seed(0)
        random.seed(0)
        seq = SlamSequence(cfg, ds, ss.empty_map(cfg, "cuda"), ss.PIPE, torch.zeros(3, device="cuda"), idle_map_iters=2, seeding=mode).run()
        assert seq.gaussians.seeding == mode and (seq.gaussians.seed_calls > 0) == (mode == "fused")
        runs[mode] = dict(seq=seq, ate=seq.eval_ate())
    h, f = runs["host"], runs["fused"]
    hc, fc = h["seq"].gaussian_counts, f["seq"].gaussian_counts
    print({k: (v["ate"], v["seq"].kf_indices) for k, v in runs.items()})
    # Frame 0 is the first keyframe.  Through the second keyframe's seeding the two drives go through the same events; after it they are
    # two drives: another subset of the same size is another map, and this toy sequence's keyframe test (kf_overlap 0.95 on 64 x 48 frames)
    # then picks other frames (measured: host [0, 4, 10, 14, 16], fused [0, 3, 12, 15]), so the number of idle mapping events between
    # later seedings differs by construction.
    assert len(h["seq"].kf_indices) >= 3 and len(f["seq"].kf_indices) >= 3
    k = [i for i, (e, _) in enumerate(hc) if e == "seed"][1] + 1
    assert [e for e, _ in fc[:k]] == [e for e, _ in hc[:k]], (fc[:k + 4], hc[:k + 4])
    assert [c for e, c in fc if e == "seed"][0] == [c for e, c in hc if e == "seed"][0]      # frame 0's seeding: the same count
    assert f["ate"] < 0.03, f["ate"]
