"""The pose initialisation without a GPU: the float64 oracle (tests/pnp_oracle.py -- the semantics of ``lvdgs_pnp_ransac``,
include/lvdgs.h) against ground truth on the seeded cases (tests/pnp_cases.py), the undistortion's round trip, the matcher's raster
sizes, the ctypes mirror against a compiled C probe, the exports' argument validation, and the ground-truth matcher with the oracle on
a trajectory several times faster than the default drive.  The HIP path is held against the oracle in tests/test_gpu_init_pose.py."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import pnp_cases as pc
import pnp_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lvdgs.h")

_solved = {}


def solved(name):
    if name not in _solved:
        c = pc.make_case(name)
        _solved[name] = (c, orc.solve(c["depth"], c["m1"], c["m2"], c["K"], c["dist"], **c["kw"]))
    return _solved[name]


# Twice the largest error the oracle shows over the ten seeds of a setting (degrees, units; translations are up to 1.5 units, 30-50 %
# of the matches are outliers).  Measured: rot1 0.0266 deg / 0.0075, rot5 0.0267 / 0.0230, rot10 0.0324 / 0.0118, rot20 0.2455 / 0.1792
# (seed 4: 455 matches survive the rotation, 266 of them inliers), waymo_distortion 0.0022 / 0.0016, zero_depth_holes 0.0146 / 0.0160,
# many_matches 0.0032 / 0.0016.
BOUNDS = {"rot1": (2 * 0.0266367894, 2 * 0.0074750833), "rot5": (2 * 0.0266950291, 2 * 0.0230094534), "rot10": (2 * 0.0324389131, 2 * 0.0117690999),
          "rot20": (2 * 0.2454678198, 2 * 0.1791522759), "waymo_distortion": (2 * 0.0021979122, 2 * 0.0015741083),
          "zero_depth_holes": (2 * 0.0146324346, 2 * 0.0160487413), "many_matches": (2 * 0.0032369663, 2 * 0.0015664661)}


@pytest.mark.parametrize("name", pc.RECOVERY)
def test_oracle_recovers_the_motion(name):
    c, o = solved(name)
    rot, trans = BOUNDS[name.split("_seed")[0]]
    assert o["status"] == orc.OK and o["reason"] == orc.FAIL_NONE and o["valid"] >= 6
    e_rot, e_trans = orc.pose_error(o["pose"], c["R"], c["t"])
    print(name, len(c["m1"]), o["valid"], o["hypothesis"], o["winner_count"], o["inliers"], e_rot, e_trans)
    assert e_rot <= rot and e_trans <= trans, (name, e_rot, e_trans)
    # the consensus is the matches that were carried by the motion, up to the few outliers that land within the threshold by chance
    truth = ~c["outlier"] & o["valid_mask"]
    assert int((o["inlier_mask"] & ~truth).sum()) <= 0.01 * len(truth) and int((truth & ~o["inlier_mask"]).sum()) <= 0.01 * len(truth)
    assert o["inliers"] == int(o["inlier_mask"].sum()) and o["counts"][o["hypothesis"]] == o["winner_count"] == o["counts"].max()
    R = o["pose"][:3, :3]
    assert np.allclose(R @ R.T, np.eye(3), atol=1e-12) and np.array_equal(o["pose"][3], [0, 0, 0, 1])


def test_the_cases_are_what_they_say():
    sizes = {n: len(pc.make_case(n)["m1"]) for n in pc.CASES}
    assert all(400 <= sizes[n] <= 1280 for n in pc.CASES if n.startswith("rot")), sizes      # (the grid holds 1280; large rotations push matches out of the frame)
    assert min(sizes[n] for n in pc.CASES if n.startswith("rot1_")) >= 1050
    assert sizes["many_matches"] > 16_000 and sizes["five_valid"] == 40
    c, o = solved("zero_depth_holes")
    assert 0.2 < 1.0 - o["valid"] / len(c["m1"]) < 0.4
    c, o = solved("waymo_distortion")
    assert c["dist"] == pc.WAYMO_DIST and c["depth"].shape == (336, 512)


@pytest.mark.parametrize("name,reason", [("five_valid", orc.FAIL_FEW_VALID), ("all_outliers", orc.FAIL_FEW_INLIERS)])
def test_oracle_refuses_the_failure_cases_with_the_exact_identity(name, reason):
    c, o = solved(name)
    assert o["status"] == orc.FAILED and o["reason"] == reason
    assert np.array_equal(o["pose"], np.eye(4)) and not o["inlier_mask"].any() and o["inliers"] == 0
    if name == "five_valid":
        assert o["valid"] == 5 and o["hypothesis"] == -1
    else:
        assert 3 <= o["winner_count"] < 6 and o["hypothesis"] >= 0      # (the three sample points always agree with their own pose)


def test_every_hypothesis_void_fails():
    c = pc.make_case("rot1_seed0")
    m2 = np.full_like(c["m2"], np.nan)         # no step on such a sample is finite
    o = orc.solve(c["depth"], c["m1"], m2, c["K"], c["dist"], **c["kw"])
    assert o["status"] == orc.FAILED and o["reason"] == orc.FAIL_ALL_VOID and (o["counts"] == -1).all() and np.array_equal(o["pose"], np.eye(4))


def test_fragile_matches_are_rare():
    """A match within 1e-6 px of the threshold under some hypothesis may be counted the other way by a computation that rounds
    otherwise; over all cases such matches stay under 0.1 % of (matches x hypotheses) (measured: 1 of 7.4 million)."""
    fragile = total = 0
    for name in pc.CASES:
        c, o = solved(name)
        fragile += int(o["fragile_counts"].sum()) + o["fragile_rounds"] + int(o["fragile_final"].sum())
        total += len(c["m1"]) * c["kw"]["hypotheses"]
    print("fragile", fragile, "of", total)
    assert fragile < 1e-3 * total


def test_the_sample_hash_is_the_one_the_header_states():
    assert [int(orc.mix32(x)) for x in (0, 1, 2, 0xDEADBEEF)] == [0, 1753845952, 3507691905, 3861431939]
    assert [int(orc.draw(s, h, d)) for s, h, d in ((0, 0, 0), (0, 1, 0), (7, 127, 95), (0xFFFFFFFF, 4095, 5))] == \
        [2488251732, 3330041933, 3471044460, 2122631651]
    text = open(HEADER).read()
    for word in ("0x7feb352d", "0x846ca68b", "0x9e3779b9"):
        assert word in text
    valid = np.ones(50, bool)
    valid[::2] = False
    S = orc.samples_of(3, 64, valid)
    assert (S >= 0).all() and valid[S].all() and all(len(set(row)) == 3 for row in S.tolist())
    assert (orc.samples_of(3, 8, np.zeros(50, bool)) == -1).all()


def test_undistortion_round_trip_at_the_waymo_coefficients():
    """Ten fixed-point steps, then the forward model: back on the pixel within 1e-6 px over the whole 1920 x 1280 frame (measured
    2.6e-8 px; five steps, cv2's default count, reach 7.8e-4 px; the distortion moves pixels by up to 28.9 px there)."""
    K = (2071.3932896281076, 2071.3932896281076, 952.3805527835524, 653.8669872813746)
    u, v = np.meshgrid(np.arange(0, 1920, 8.0), np.arange(0, 1280, 8.0))
    for Kc, uu, vv in ((K, u, v), (pc.WAYMO_K, u * 512 / 1920, v * 336 / 1280)):
        x, y = orc.undistort(uu, vv, Kc, pc.WAYMO_DIST)
        xd, yd = orc.distort(x, y, pc.WAYMO_DIST)
        err = np.hypot(xd * Kc[0] + Kc[2] - uu, yd * Kc[1] + Kc[3] - vv).max()
        moved = np.hypot(x * Kc[0] + Kc[2] - uu, y * Kc[1] + Kc[3] - vv).max()
        print("round trip", err, "moved", moved)
        assert err <= 1e-6 and moved > 5.0
    x, y = orc.undistort(u, v, K, (0, 0, 0, 0, 0))
    assert np.array_equal(x, (u - K[2]) / K[0]) and np.array_equal(y, (v - K[3]) / K[1])      # all zero: no distortion, exactly


@pytest.mark.parametrize("size,raster", [((1226, 370), (512, 144)), ((1920, 1080), (512, 288)), ((1920, 1280), (512, 336)), ((640, 480), (512, 384))])
def test_matcher_raster(size, raster):
    from lvdgs import init_pose
    assert init_pose.matcher_raster(*size) == raster


def test_pnp_constants_are_the_oracle_s():
    from lvdgs import _lib
    assert _lib.PNP_HOST_BYTES == 4 * _lib.PNP_STATE_WORDS + 12 * 8
    assert (_lib.PNP_OK, _lib.PNP_FAILED) == (orc.OK, orc.FAILED)
    assert (_lib.PNP_FAIL_NONE, _lib.PNP_FAIL_FEW_VALID, _lib.PNP_FAIL_ALL_VOID, _lib.PNP_FAIL_FEW_INLIERS, _lib.PNP_FAIL_SINGULAR) == \
        (orc.FAIL_NONE, orc.FAIL_FEW_VALID, orc.FAIL_ALL_VOID, orc.FAIL_FEW_INLIERS, orc.FAIL_SINGULAR)


def test_pnp_argument_validation_without_gpu():
    from lvdgs import _lib
    L = _lib.lib()
    assert L.lvdgs_pnp_ransac(None, None) == _lib.E_INVALID and b"NULL" in L.lvdgs_last_error()
    good = dict(width=512, height=144, num_matches=100, hypotheses=128, min_inliers=6, fx=295.0, fy=295.0, cx=256.0, cy=72.0, reproj_error=5.0)
    a = _lib.PnpArgs(**good)
    assert L.lvdgs_pnp_ransac(C.byref(a), None) == _lib.E_INVALID and b"NULL" in L.lvdgs_last_error()      # every pointer is NULL
    for field, value, word in (("hypotheses", 0, b"hypotheses"), ("hypotheses", -3, b"hypotheses"), ("hypotheses", _lib.PNP_MAX_HYPOTHESES + 1, b"hypotheses"),
                               ("num_matches", -1, b"num_matches"), ("width", 0, b"raster"), ("height", -2, b"raster"), ("reproj_error", 0.0, b"positive"),
                               ("fx", 0.0, b"positive")):
        a = _lib.PnpArgs(**{**good, field: value})
        for name in ("depth", "matches_im1", "matches_im2", "inlier_mask", "host_state", "scratch"):
            setattr(a, name, 256)      # (never dereferenced: every call here is refused before a launch)
        a.scratch_bytes = 1 << 30
        assert L.lvdgs_pnp_ransac(C.byref(a), None) == _lib.E_INVALID and word in L.lvdgs_last_error(), (field, L.lvdgs_last_error())
    a = _lib.PnpArgs(**good)
    for name in ("depth", "matches_im1", "matches_im2", "inlier_mask", "host_state", "scratch"):
        setattr(a, name, 256)
    a.scratch_bytes = L.lvdgs_pnp_scratch_bytes(100, 128) - 1
    assert L.lvdgs_pnp_ransac(C.byref(a), None) == _lib.E_INVALID and b"scratch too small" in L.lvdgs_last_error()
    # the scratch: a header, five float64 columns of the matches, a 128-byte record per hypothesis; nothing for nonsense sizes
    assert L.lvdgs_pnp_scratch_bytes(20_000, 512) % 256 == 0 and L.lvdgs_pnp_scratch_bytes(20_000, 512) >= 5 * 8 * 20_000 + 128 * 512
    assert L.lvdgs_pnp_scratch_bytes(-5, -5) == L.lvdgs_pnp_scratch_bytes(0, 0) > 0
    assert L.lvdgs_pnp_scratch_bytes(1000, 128) < L.lvdgs_pnp_scratch_bytes(1001, 128) + 256


def test_the_python_layer_names_what_is_missing():
    from lvdgs import _lib, init_pose
    from lvdgs.slam_sequence import SlamSequence
    with pytest.raises(TypeError, match="matcher"):
        init_pose.get_pose(None, None, None, None, None, None, None, None)
    with pytest.raises(TypeError, match="matcher"):
        SlamSequence(None, None, None, None, None, pose_init="pnp")
    with pytest.raises(ValueError, match="pose_init"):
        SlamSequence(None, None, None, None, None, pose_init="bogus")
    with pytest.raises(_lib.LvdgsError, match="no CPU path"):
        init_pose.pnp_ransac(torch.ones(8, 8), np.zeros((4, 2)), np.zeros((4, 2)), (8.0, 8.0, 4.0, 4.0))


# ------------------------------------------------------------------------------------ the ground-truth matcher with the oracle
FAST = dict(step=0.06, sway=0.3, yaw=0.09, period=40.0)      # inter-frame motion three times make_sequence's default (0.02, 0.15, 0.03)


def plane_dataset(n_frames=12, **trajectory):
    """A ``SequenceDataset`` without images: the cases' ground plane and wall seen from ``vehicle_trajectory`` at 512 x 160 (the
    matcher's raster of such frames is the frame itself), mono depth = true depth x 2 % noise."""
    from lvdgs import synthetic
    W, H = pc.W1, pc.H1
    fx, fy, cx, cy = pc.K
    poses = synthetic.vehicle_trajectory(n_frames, **trajectory)
    rng = np.random.default_rng(5)
    u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    rays = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], -1)
    monos = []
    for w2c in poses:
        c2w = np.linalg.inv(w2c.double().numpy())
        d, o = rays @ c2w[:3, :3].T, c2w[:3, 3]
        with np.errstate(divide="ignore", invalid="ignore"):
            s_ground = np.where(d[..., 1] > 1e-9, (pc.CAMERA_HEIGHT - o[1]) / d[..., 1], np.inf)       # world plane y = CAMERA_HEIGHT
            s_wall = np.where(d[..., 2] > 1e-9, (pc.WALL - o[2]) / d[..., 2], np.inf)                  # world plane z = WALL
        z = np.minimum(s_ground, s_wall)         # rays have unit camera z: the ray parameter is the depth
        monos.append((z * (1.0 + 0.02 * rng.normal(size=z.shape))).astype(np.float32))
    return synthetic.SequenceDataset([None] * n_frames, monos, poses, W, H, fx, fy, cx, cy, "cpu")


def test_ground_truth_matcher_carries_the_grid_with_the_true_motion():
    from lvdgs import init_pose, synthetic
    ds = plane_dataset(6, **FAST)
    assert init_pose.matcher_raster(ds.width, ds.height) == (ds.width, ds.height)
    m = synthetic.GroundTruthMatcher(ds, stride=8, noise_px=0.0, outlier_ratio=0.0, seed=1)
    with pytest.raises(RuntimeError, match="set_frames"):
        m(None, None, None, (ds.width, ds.height))
    m.set_frames(1, 4)
    m1, m2 = m(None, None, None, (ds.width, ds.height))
    assert m1.dtype == np.int32 and m2.dtype == np.float32 and m1.shape == m2.shape and 900 < len(m1) <= 1280
    assert ((m1 - 4) % 8 == 0).all() and (m2 >= 0).all() and (m2[:, 0] <= ds.width - 1).all() and (m2[:, 1] <= ds.height - 1).all()
    rel = ds.poses[4].double().numpy() @ np.linalg.inv(ds.poses[1].double().numpy())
    Z = ds.mono_depths[1][m1[:, 1], m1[:, 0]].astype(np.float64)
    P = np.stack([(m1[:, 0] - ds.cx) / ds.fx * Z, (m1[:, 1] - ds.cy) / ds.fy * Z, Z], 1) @ rel[:3, :3].T + rel[:3, 3]
    want = np.stack([ds.fx * P[:, 0] / P[:, 2] + ds.cx, ds.fy * P[:, 1] / P[:, 2] + ds.cy], 1)
    assert np.abs(m2 - want).max() < 1e-3
    # noise, the seeded share of outliers, the same matches for the same pair and seed
    n = synthetic.GroundTruthMatcher(ds, stride=8, noise_px=0.7, outlier_ratio=0.3, seed=1)
    n.set_frames(1, 4)
    a1, a2 = n(None, None, None, (ds.width, ds.height))
    b1, b2 = n(None, None, None, (ds.width, ds.height))
    assert np.array_equal(a1, b1) and np.array_equal(a2, b2)
    # (the noise can push a grid point over the frame's edge: compare the matches both calls kept)
    key = lambda g: g[:, 1].astype(np.int64) * 4096 + g[:, 0]
    _, ia, ib = np.intersect1d(key(a1), key(m1), return_indices=True)
    far = np.hypot(*(a2[ia] - m2[ib]).T) > 5.0
    assert 0.2 < far.mean() < 0.4


def test_on_a_fast_trajectory_the_estimate_beats_the_previous_pose_on_every_frame():
    """The drive of tests/test_gpu_init_pose.py, on the oracle alone: matches of ``GroundTruthMatcher`` (0.7 px noise, 30 % outliers)
    between a keyframe and the frames up to five behind it, depth = the keyframe's noisy mono depth.  The estimated motion composed with
    the keyframe's pose lies closer to the frame's true pose than the previous frame's true pose does -- by more than a factor of five."""
    from lvdgs import synthetic
    ds = plane_dataset(12, **FAST)
    matcher = synthetic.GroundTruthMatcher(ds, stride=8, noise_px=0.7, outlier_ratio=0.3, seed=0)
    centre = lambda T: -T[:3, :3].T @ T[:3, 3]
    worst = 0.0
    for kf in (0, 5):
        for cur in range(kf + 1, kf + 6):
            matcher.set_frames(kf, cur)
            m1, m2 = matcher(None, None, None, (ds.width, ds.height))
            o = orc.solve(ds.mono_depths[kf], m1, m2, pc.K, seed=cur)
            assert o["status"] == orc.OK and o["inliers"] > 0.5 * len(m1)
            T_kf, T_cur, T_prev = (ds.poses[i].double().numpy() for i in (kf, cur, cur - 1))
            e_pnp = np.linalg.norm(centre(o["pose"] @ T_kf) - centre(T_cur))
            e_prev = np.linalg.norm(centre(T_prev) - centre(T_cur))
            worst = max(worst, e_pnp / e_prev)
            assert e_pnp < 0.2 * e_prev, (kf, cur, e_pnp, e_prev)
    print("worst ratio", worst)
