"""The HIP reciprocal nearest-neighbour matcher (``lvdgs.init_pose.reciprocal_matches`` -> ``lvdgs_reciprocal_nn``) against the NumPy
float64 oracle (tests/recip_nn_oracle.py) on the seeded cases (tests/recip_nn_cases.py; tests/test_recip_nn.py shows on the oracle
alone what they ask): per-case parity up to the fragile seeds, one half round over every pixel, the tie rule, determinism, the
refusals of the C ABI, ``get_pose`` end to end on descriptor maps, and a drive started from those matches."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import pnp_oracle as pnp
import recip_nn_cases as rc
import recip_nn_oracle as orc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def hip(desc1, desc2, S, max_iter):
    """-> (flat pairs (M, 2), matches_im1, matches_im2 as returned, state words, per-seed state (seeds, 3) NumPy)."""
    from lvdgs import init_pose
    dev = torch.device("cuda", 0)
    d1 = desc1 if torch.is_tensor(desc1) else torch.tensor(desc1, device=dev)
    d2 = desc2 if torch.is_tensor(desc2) else torch.tensor(desc2, device=dev)
    m1, m2 = init_pose.reciprocal_matches(d1, d2, subsample=S, max_iter=max_iter, seed_state=True)
    lm = init_pose.last_match
    words = dict(seeds=lm.seeds, matches=lm.matches, unconverged=lm.unconverged, rounds=lm.rounds)
    return orc.flat_pairs(m1.cpu().numpy(), m2.cpu().numpy(), d1.shape[1], d2.shape[1]), m1, m2, words, lm.seed_state.cpu().numpy()


def check_against(o, pairs, m1, m2, words, seeds, shape1, shape2, what):
    """The parity rule: exact where the oracle has no fragile seed, else every non-fragile seed's end and the output up to the fragile ones."""
    dev = torch.device("cuda", 0)
    (H1, W1, _), (H2, W2, _) = shape1, shape2
    assert m1.device == dev and m2.device == dev and m1.dtype == torch.int32 and m2.dtype == torch.float32
    assert tuple(m1.shape) == tuple(m2.shape) == (words["matches"], 2) and m1.is_contiguous() and m2.is_contiguous()
    keys = pairs[:, 0] * (H2 * W2) + pairs[:, 1]
    assert (np.diff(keys) > 0).all(), what                                            # sorted by xy1 then xy2, distinct
    assert (pairs >= 0).all() and (pairs[:, 0] < H1 * W1).all() and (pairs[:, 1] < H2 * W2).all()
    assert seeds.shape == (o.seeds, 3) and words["seeds"] == o.seeds
    nf = int(o.fragile.sum())
    print(what, words, "oracle", dict(matches=len(o.pairs), unconverged=o.unconverged, rounds=o.rounds, fragile=nf))
    as_set = lambda p: set(map(tuple, np.asarray(p).tolist()))
    if nf == 0:
        assert words == dict(seeds=o.seeds, matches=len(o.pairs), unconverged=o.unconverged, rounds=o.rounds), what
        assert np.array_equal(pairs, o.pairs), what
        assert np.array_equal(seeds[:, 0], o.xy1) and np.array_equal(seeds[:, 1], o.xy2) and np.array_equal(seeds[:, 2] != 0, o.converged), what
        return
    keep = ~o.fragile
    assert np.array_equal(seeds[keep, 0], o.xy1[keep]) and np.array_equal(seeds[keep, 1], o.xy2[keep]), what
    assert np.array_equal(seeds[keep, 2] != 0, o.converged[keep]), what
    got = as_set(pairs)
    solid = as_set(np.stack([o.xy1, o.xy2], 1)[keep & o.converged]) - as_set(np.stack([o.xy1, o.xy2], 1)[o.fragile & o.converged])
    assert solid <= got, what                                                          # every oracle pair owned by non-fragile seeds alone
    from_fragile = as_set(seeds[o.fragile & (seeds[:, 2] != 0), :2])
    assert got <= as_set(o.pairs) | from_fragile, what                                 # every HIP pair: an oracle pair, or a fragile seed's
    assert got == as_set(seeds[seeds[:, 2] != 0, :2]), what                            # the output is the converged seeds' pairs, merged
    assert abs(words["matches"] - len(o.pairs)) <= nf and abs(words["unconverged"] - o.unconverged) <= nf, what


@pytest.mark.parametrize("name", list(rc.CASES))
def test_hip_matches_the_oracle(name):
    c = rc.case(name)
    check_against(c.oracle, *hip(c.desc1, c.desc2, c.S, c.max_iter), c.desc1.shape, c.desc2.shape, name)


@pytest.mark.parametrize("name", rc.PRIMITIVE)
def test_one_half_round_over_every_pixel(name):
    """subsample 1, one round: every pixel of map 1 is a query against map 2, and its winner one against map 1.  Exact wherever the
    margin is at least TAU."""
    c = rc.case(name)
    j, mj, i, mi = rc.half_round(name)
    _, _, _, words, seeds = hip(c.desc1, c.desc2, 1, 1)
    n = len(j)
    assert words["seeds"] == n == c.desc1.shape[0] * c.desc1.shape[1] and words["rounds"] == 1
    sure2 = mj >= orc.TAU
    sure1 = sure2 & (mi >= orc.TAU)
    print(name, "queries", n, "margin below TAU: forward", int((~sure2).sum()), "back", int((mi < orc.TAU).sum()),
          "differ forward", int((seeds[:, 1] != j).sum()), "back", int((seeds[:, 0] != i).sum()))
    assert sure2.mean() > 0.97
    assert np.array_equal(seeds[sure2, 1], j[sure2])
    assert np.array_equal(seeds[sure1, 0], i[sure1])
    assert np.array_equal(seeds[sure1, 2] != 0, (i == np.arange(n))[sure1])            # inactive after one round: mutual nearest neighbours
    assert words["unconverged"] == n - int((seeds[:, 2] != 0).sum())


def test_ties_go_to_the_lowest_index():
    c = rc.case("duplicate_rows")
    pairs, _, _, _, seeds = hip(c.desc1, c.desc2, c.S, c.max_iter)
    assert not set(pairs[:, 1].tolist()) & set(c.duplicates), "a copy at a higher index was returned"
    keep = ~c.oracle.fragile
    assert np.array_equal(seeds[keep, 1], c.oracle.xy2[keep]) and set(seeds[keep, 1].tolist()) & set(c.duplicates.values())
    # every row but the last of map 2 twice: the second half of the rows is a bit-identical copy of the first, at other places in the tiles
    D = c.desc2.shape[-1]
    flat = c.desc2.reshape(-1, D).copy()
    half = len(flat) // 2
    flat[half:2 * half] = flat[:half]
    twice = flat.reshape(c.desc2.shape)
    j, mj = orc.nearest(c.desc1.reshape(-1, D), flat)
    _, _, _, _, seeds = hip(c.desc1, twice, 1, 1)
    assert (j < half).sum() > 0.9 * len(j)
    assert ((seeds[:, 1] < half) | (seeds[:, 1] == 2 * half)).all()
    assert np.array_equal(seeds[mj >= orc.TAU, 1], j[mj >= orc.TAU])


def test_two_calls_are_bit_identical():
    for name in ("dense_s1_two_rounds", "shrunk_map2"):
        c, other = rc.case(name), rc.case("small_d16_s3")
        a = hip(c.desc1, c.desc2, c.S, c.max_iter)
        hip(other.desc1, other.desc2, other.S, other.max_iter)      # (another call in between leaves its own state in the scratch)
        b = hip(c.desc1, c.desc2, c.S, c.max_iter)
        assert a[1].cpu().numpy().tobytes() == b[1].cpu().numpy().tobytes() and a[2].cpu().numpy().tobytes() == b[2].cpu().numpy().tobytes(), name
        assert a[3] == b[3] and a[4].tobytes() == b[4].tobytes(), name


def test_c_abi_refusals_launch_nothing():
    """Every LVDGS_E_INVALID condition with real buffers behind the pointers: the call returns the status and its text, and neither the
    outputs nor the state words change."""
    from lvdgs import _lib
    dev = torch.device("cuda", 0)
    L = _lib.lib()
    c = rc.case("small_d24_s4")
    d1, d2 = torch.tensor(c.desc1, device=dev), torch.tensor(c.desc2, device=dev)
    # (room for the largest seed count a refused call names: it is refused, but nothing here relies on that for its memory)
    m1 = torch.full((16384, 2), -7, dtype=torch.int32, device=dev)
    m2 = torch.full((16384, 2), -7.0, dtype=torch.float32, device=dev)
    state = torch.full((_lib.RNN_STATE_WORDS,), -7, dtype=torch.int32).pin_memory()
    scratch = torch.zeros(max(L.lvdgs_recip_nn_scratch_bytes(53, 37, 4), L.lvdgs_recip_nn_scratch_bytes(128, 128, 1)), dtype=torch.uint8, device=dev)

    def make_args(**over):
        kw = dict(width1=53, height1=37, width2=67, height2=41, dim=24, subsample=4, max_iter=10, capacity=117, desc1=d1.data_ptr(),
                  desc2=d2.data_ptr(), matches_im1=m1.data_ptr(), matches_im2=m2.data_ptr(), seed_state=None, host_state=state.data_ptr(),
                  scratch=scratch.data_ptr(), scratch_bytes=L.lvdgs_recip_nn_scratch_bytes(53, 37, 4))
        kw.update(over)
        return _lib.RecipNnArgs(**kw)
    stream = _lib.raw_stream(dev)
    for what, a, word in rc.refusals(make_args):
        assert L.lvdgs_reciprocal_nn(None if a is None else C.byref(a), stream) == _lib.E_INVALID, what
        assert word in L.lvdgs_last_error(), (what, L.lvdgs_last_error())
    torch.cuda.synchronize(dev)
    assert (state == -7).all() and bool((m1 == -7).all()) and bool((m2 == -7.0).all()) and not bool(scratch.any())
    # the same block without a fault in it runs
    assert L.lvdgs_reciprocal_nn(C.byref(make_args()), stream) == _lib.OK
    torch.cuda.synchronize(dev)
    assert state[0] == _lib.RNN_OK and state[1] == 117 and state[2] == len(c.oracle.pairs)
    with pytest.raises(_lib.LvdgsError, match="subsample"):
        from lvdgs import init_pose
        init_pose.reciprocal_matches(d1, d2, subsample=0)


# ----------------------------------------------------------------------------------------------- get_pose and the sequence
FAST = dict(step=0.06, sway=0.3, yaw=0.09, period=40.0)      # the fast trajectory of tests/test_gpu_init_pose.py


def rotation_angle_deg(Ra, Rb):
    return float(np.degrees(2.0 * np.arcsin(min(1.0, np.linalg.norm(Ra - Rb) / (2.0 * np.sqrt(2.0))))))


def test_get_pose_end_to_end_on_descriptor_maps():
    """The setup of test_get_pose_end_to_end_on_a_rendered_map with ``DescriptorMatcher(WorldDescriptors(ds))`` in the matcher's place:
    the matches are the oracle's on the same descriptor maps up to the fragile seeds, and the pose is no further from the true motion
    than the float64 PnP oracle's on the same matches and depth, plus that oracle's sensitivity to its summation order x 1000 (the pose
    tolerance rule of tests/test_gpu_init_pose.py), three times as there."""
    import sequence as tool
    from lvdgs import init_pose, synthetic
    from lvdgs.camera_utils import Camera
    from lvdgs.graphics_utils import getProjectionMatrix2
    dev = torch.device("cuda", 0)
    cfg, ds, truth = tool.kitti_sequence(dev, frames=8, scale=0.5, cadence="short", masks=True, trajectory=FAST)
    proj = getProjectionMatrix2(znear=0.01, zfar=100.0, fx=ds.fx, fy=ds.fy, cx=ds.cx, cy=ds.cy, W=ds.width, H=ds.height).transpose(0, 1).to(dev)
    kf = 2
    vp = Camera.init_from_dataset(ds, kf, proj)
    vp.update_RT(vp.R_gt, vp.T_gt)
    bg = torch.zeros(3, device=dev)
    seen = []

    class Recording(init_pose.DescriptorMatcher):
        def __call__(self, img1, img2, model, raster):
            d1, d2 = self.describe(img1, img2, model, raster)
            m1, m2 = init_pose.reciprocal_matches(d1, d2, subsample=self.subsample, max_iter=self.max_iter, seed_state=True)
            lm = init_pose.last_match
            seen.append((d1, d2, m1, m2, dict(seeds=lm.seeds, matches=lm.matches, unconverged=lm.unconverged, rounds=lm.rounds), lm.seed_state.cpu().numpy()))
            return m1, m2
    matcher = Recording(synthetic.WorldDescriptors(ds))
    W1, H1 = init_pose.matcher_raster(ds.width, ds.height)
    assert (W1, H1) == (512, 144)
    K1 = (ds.fx * W1 / ds.width, ds.fy * H1 / ds.height, ds.cx * W1 / ds.width, ds.cy * H1 / ds.height)
    results, spread = [], 0.0
    for cur in range(kf + 1, 8):
        matcher.set_frames(kf, cur)
        pose, depth = init_pose.get_pose(ds.images[kf], ds.images[cur], None, ds.dist_coeffs, vp, truth, tool.PIPE, bg, matcher=matcher, seed=cur)
        lc = init_pose.last_call
        assert lc.status == pnp.OK and pose.dtype == np.float64 and pose.shape == (4, 4)
        d1, d2, m1, m2, words, seeds = seen[-1]
        assert tuple(d1.shape) == tuple(d2.shape) == (H1, W1, 24) and m1.device == dev and m2.device == dev
        o = orc.reciprocal_nn(d1.cpu().numpy(), d2.cpu().numpy(), 8, 10)
        pairs = orc.flat_pairs(m1.cpu().numpy(), m2.cpu().numpy(), W1, W1)
        check_against(o, pairs, m1, m2, words, seeds, d1.shape, d2.shape, f"frame {cur}")
        m1n, m2n, dn = m1.cpu().numpy(), m2.cpu().numpy(), depth[0].cpu().numpy()
        po = pnp.solve(dn, m1n, m2n, K1, seed=cur)
        assert po["status"] == pnp.OK
        for k in range(2):
            perm = np.random.default_rng(100 + k).permutation(len(m1n))
            spread = max(spread, float(np.abs(pnp.solve(dn, m1n, m2n, K1, seed=cur, sum_order=perm)["pose"] - po["pose"]).max()))
        rel = ds.poses[cur].double().numpy() @ np.linalg.inv(ds.poses[kf].double().numpy())
        e_hip = (rotation_angle_deg(pose[:3, :3], rel[:3, :3]), float(np.linalg.norm(pose[:3, 3] - rel[:3, 3])))
        e_orc = (rotation_angle_deg(po["pose"][:3, :3], rel[:3, :3]), float(np.linalg.norm(po["pose"][:3, 3] - rel[:3, 3])))
        print("frame", cur, words, "inliers", lc.inliers, "oracle", po["inliers"], "error hip", e_hip, "oracle", e_orc, "motion", float(np.linalg.norm(rel[:3, 3])))
        assert lc.inliers >= 6
        results.append((e_hip, e_orc))
    tol = 1000.0 * spread
    print("oracle pose spread under permuted summation", spread, "-> pose tolerance", tol)
    assert 0.0 < spread < 1e-12
    for e_hip, e_orc in results:
        assert e_hip[0] <= e_orc[0] + np.degrees(3.0 * tol) and e_hip[1] <= e_orc[1] + 3.0 * tol, (e_hip, e_orc)


def test_a_drive_started_from_descriptor_matches():
    """Twelve half-size frames of the fast trajectory, every tracked frame started from PnP on the matches of the descriptor matcher:
    every frame is estimated with at least 6 inliers, and the end ATE stays in the band of tests/test_gpu_sequence.py (25 % + 1e-3)
    against the same drive on ``GroundTruthMatcher``'s matches."""
    import sequence as tool
    dev = torch.device("cuda", 0)
    drive = dict(frames=12, scale=0.5, cadence="short", idle=0, refine=0, masks=True, window_size=5, trajectory=FAST, pose_init="pnp")
    rg, _ = tool.run_sequence(dev, **drive)
    rd, sd = tool.run_sequence(dev, **drive, matcher="descriptors")
    for name, r in (("ground truth", rg), ("descriptors", rd)):
        print(name, {k: r[k] for k in ("keyframes", "tracking_iterations", "ate_rmse", "pose_error_unaligned_mean", "pose_error_unaligned_max")})
        for rec in r["pose_init"]:
            print("   ", rec)
    from lvdgs import init_pose
    assert isinstance(sd.matcher, init_pose.DescriptorMatcher) and init_pose.last_match.seeds == 1152
    assert [r["frame"] for r in rd["pose_init"]] == list(range(1, 12))
    assert all(r["estimated"] and r["inliers"] >= 6 for r in rd["pose_init"]), rd["pose_init"]
    assert rd["ate_rmse"] <= rg["ate_rmse"] + 0.25 * max(rd["ate_rmse"], rg["ate_rmse"]) + 1e-3, (rd["ate_rmse"], rg["ate_rmse"])
