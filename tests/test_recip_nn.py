"""Reciprocal nearest-neighbour matching without a GPU: the NumPy float64 oracle (tests/recip_nn_oracle.py) on the seeded cases
(tests/recip_nn_cases.py) has the properties the GPU tests lean on -- few fragile seeds, several rounds, unconverged seeds, merged
duplicates, mutual nearest neighbours, matches on the warp -- so that a GPU test cannot hide behind a case that asks nothing; the
refusals of ``init_pose.reciprocal_matches`` and of the C ABI that launch nothing;
``DescriptorMatcher`` and ``synthetic.WorldDescriptors`` on the CPU."""
import ctypes as C

import numpy as np
import pytest
import torch

import recip_nn_cases as rc
import recip_nn_oracle as orc
from lvdgs import _lib, init_pose, synthetic


def test_tau_is_just_above_the_rounding_of_two_scores():
    assert 2 * _lib.RNN_MAX_DIM * 2.0 ** -24 < orc.TAU < 1.5 * 2 * _lib.RNN_MAX_DIM * 2.0 ** -24


@pytest.mark.parametrize("name", list(rc.CASES))
def test_oracle_on_the_cases(name):
    c = rc.case(name)
    o = c.oracle
    (H1, W1, D), (H2, W2, _) = c.desc1.shape, c.desc2.shape
    assert (H1, W1, H2, W2, D, c.S, c.max_iter) == rc.CASES[name]
    assert o.seeds == len(range(c.S // 2, H1, c.S)) * len(range(c.S // 2, W1, c.S))
    assert o.seeds % 64 != 0 or name in ("dense_s1", "dense_s1_two_rounds", "raster_144x512")      # (6144 and 1152 seeds: whole waves, the others not)
    assert np.allclose(np.linalg.norm(c.desc1, axis=-1), 1.0, atol=1e-6) and np.allclose(np.linalg.norm(c.desc2, axis=-1), 1.0, atol=1e-6)
    print(name, "seeds", o.seeds, "active after each round", o.active_after, "matches", len(o.pairs), "unconverged", o.unconverged,
          "fragile", int(o.fragile.sum()))
    assert o.fragile.sum() <= 0.03 * o.seeds
    assert o.unconverged == o.seeds - int(o.converged.sum()) and (o.unconverged == 0 or o.rounds == c.max_iter)
    # sorted and distinct
    keys = o.pairs[:, 0] * (H2 * W2) + o.pairs[:, 1]
    assert len(o.pairs) > 0 and (np.diff(keys) > 0).all()
    assert o.matches_im1.dtype == np.int32 and o.matches_im2.dtype == np.float32
    assert np.array_equal(orc.flat_pairs(o.matches_im1, o.matches_im2, W1, W2), o.pairs)
    # every pair is a mutual nearest neighbour under brute force (float64, no chunks, no margins)
    A, B = c.desc1.reshape(-1, D).astype(np.float64), c.desc2.reshape(-1, D).astype(np.float64)
    assert np.array_equal((A[o.pairs[:, 0]] @ B.T).argmax(1), o.pairs[:, 1])
    assert np.array_equal((B[o.pairs[:, 1]] @ A.T).argmax(1), o.pairs[:, 0])
    # the matches lie on the warp (those it carries inside map 2: the others have nothing to match)
    pred = rc.warp(o.matches_im1.astype(np.float64))
    inside = (pred[:, 0] >= 0) & (pred[:, 0] <= W2 - 1) & (pred[:, 1] >= 0) & (pred[:, 1] <= H2 - 1)
    assert inside.sum() > 0.5 * len(o.pairs)
    assert np.median(np.linalg.norm(pred - o.matches_im2, axis=1)[inside]) < 1.0


def test_the_cases_ask_something():
    runs = {n: rc.case(n).oracle for n in rc.SMALL}
    assert max(o.rounds for o in runs.values()) >= 3
    assert any(o.unconverged > 0 for o in runs.values())
    assert any(int(o.converged.sum()) > len(o.pairs) for o in runs.values())      # merged duplicates
    assert any(o.fragile.any() for o in runs.values()) and any(not o.fragile.any() for o in runs.values())
    assert runs["small_d16_s3_one_round"].rounds == 1 and runs["dense_s1_two_rounds"].unconverged > 0
    dup = rc.case("duplicate_rows")
    D = dup.desc2.shape[-1]
    flat = dup.desc2.reshape(-1, D)
    assert len(dup.duplicates) > 50 and all(k > v and flat[k].tobytes() == flat[v].tobytes() for k, v in dup.duplicates.items())
    # the originals win: no copy is ever returned, and the winners are among the originals
    assert not set(dup.oracle.pairs[:, 1].tolist()) & set(dup.duplicates) and set(dup.oracle.pairs[:, 1].tolist()) & set(dup.duplicates.values())


def test_reciprocal_matches_refusals_without_gpu():
    a, b = torch.zeros(8, 8, 4), torch.zeros(6, 9, 4)
    with pytest.raises(_lib.LvdgsError, match="no CPU path"):
        init_pose.reciprocal_matches(a, b)
    with pytest.raises(_lib.LvdgsError, match="no CPU path"):
        init_pose.reciprocal_matches(a.numpy(), b.numpy())
    with pytest.raises(ValueError, match=r"\(H, W, D\)"):
        init_pose.reciprocal_matches(a[0], b)
    with pytest.raises(ValueError, match=r"\(H, W, D\)"):
        init_pose.reciprocal_matches(a, b[None])
    with pytest.raises(ValueError, match="descriptor size"):
        init_pose.reciprocal_matches(a, torch.zeros(6, 9, 5))
    with pytest.raises(ValueError, match="empty"):
        init_pose.reciprocal_matches(a, torch.zeros(0, 9, 4))
    assert init_pose.last_match.seeds == 0 and init_pose.last_match.seed_state is None


def test_descriptor_matcher_calls_describe_and_forwards_set_frames():
    calls = []

    class Describe:
        def set_frames(self, kf, cur):
            calls.append(("set_frames", kf, cur))

        def __call__(self, img1, img2, model, raster):
            calls.append(("describe", img1, img2, model, raster))
            return torch.zeros(8, 8, 4), torch.zeros(8, 8, 4)
    m = init_pose.DescriptorMatcher(Describe(), subsample=4, max_iter=3)
    m.set_frames(2, 5)
    with pytest.raises(_lib.LvdgsError, match="no CPU path"):      # it got as far as the matching
        m("a", "b", None, (8, 8))
    assert calls == [("set_frames", 2, 5), ("describe", "a", "b", None, (8, 8))] and (m.subsample, m.max_iter) == (4, 3)
    init_pose.DescriptorMatcher(lambda *a: None).set_frames(0, 1)      # a describe without set_frames: nothing to forward
    with pytest.raises(TypeError, match="DescriptorMatcher"):
        init_pose.get_pose(None, None, None, None, None, None, None, None)


def test_world_descriptors_on_the_cpu():
    """Two frames of a fronto-parallel plane: unit vectors, deterministic, the same world point the same descriptor up to the noise, and
    random vectors where there is no depth or a dynamic object."""
    W, H = 64, 40
    poses = synthetic.vehicle_trajectory(2, step=0.2, sway=0.0, yaw=0.0)
    mono = [np.full((H, W), 5.0, dtype=np.float32), np.full((H, W), 5.0 - 0.2, dtype=np.float32)]
    mono[0][:4, :4] = 0.0
    masks = [torch.ones(H, W, dtype=torch.bool), torch.ones(H, W, dtype=torch.bool)]
    masks[0][30:, 50:] = False
    ds = synthetic.SequenceDataset([torch.zeros(3, H, W)] * 2, mono, poses, W, H, 50.0, 50.0, W / 2, H / 2, torch.device("cpu"), static_masks=masks)
    wd = synthetic.WorldDescriptors(ds, dim=24, seed=1, noise=0.0, smooth=1)
    with pytest.raises(RuntimeError, match="set_frames"):
        wd(None, None, None, (W, H))
    wd.set_frames(0, 1)
    d1, d2 = wd(None, None, None, (W, H))
    assert d1.shape == d2.shape == (H, W, 24) and d1.dtype == torch.float32 and d1.is_contiguous()
    assert torch.allclose(d1.norm(dim=-1), torch.ones(H, W), atol=1e-5)
    e1, _ = wd(None, None, None, (W, H))
    assert torch.equal(d1, e1)
    # the plane's point under pixel (x, y) of frame 0 is seen at ((x - cx) 5 / 4.8 + cx, ...) in frame 1: at the principal point, the same pixel
    assert torch.allclose(d1[H // 2, W // 2], d2[H // 2, W // 2], atol=1e-4)
    assert (d1[10, 10] @ d2[10, 10]) < 0.999
    # against the same frame with depth everywhere and nothing dynamic: the same vectors up to the noise, unrelated ones where there was no depth / a dynamic object
    full = synthetic.SequenceDataset(ds.images, [np.full((H, W), 5.0, dtype=np.float32), mono[1]], poses, W, H, 50.0, 50.0, W / 2, H / 2, torch.device("cpu"))
    noisy = synthetic.WorldDescriptors(ds, dim=24, seed=1, noise=0.05, smooth=3).describe(0, (W, H))
    clean = synthetic.WorldDescriptors(full, dim=24, seed=1, noise=0.0, smooth=3).describe(0, (W, H))
    cos = (noisy * clean).sum(-1)
    assert cos[8:28, 8:48].min() > 0.95 and cos[:3, :3].max() < 0.9 and cos[32:, 52:].max() < 0.9


def test_recip_nn_limits_hold_the_matcher_s_sizes():
    assert _lib.RNN_MAX_DIM >= 64 and _lib.RNN_MAX_SEEDS >= 8192


def fake_args(**over):
    """A block that passes every check (its pointers are never dereferenced: every call here is refused before a launch)."""
    L = _lib.lib()
    kw = dict(width1=53, height1=37, width2=67, height2=41, dim=24, subsample=4, max_iter=10, capacity=117, desc1=256, desc2=512,
              matches_im1=768, matches_im2=1024, seed_state=None, host_state=1280, scratch=1536,
              scratch_bytes=L.lvdgs_recip_nn_scratch_bytes(53, 37, 4))
    kw.update(over)
    return _lib.RecipNnArgs(**kw)


def test_c_abi_refusals_launch_nothing():
    """Every LVDGS_E_INVALID condition, on a machine without a GPU: none of them can have reached a launch."""
    L = _lib.lib()
    for what, a, word in rc.refusals(fake_args):
        assert L.lvdgs_reciprocal_nn(None if a is None else C.byref(a), None) == _lib.E_INVALID, what
        assert word in L.lvdgs_last_error(), (what, L.lvdgs_last_error())
    assert L.lvdgs_recip_nn_scratch_bytes(53, 37, 4) % 256 == 0 and L.lvdgs_recip_nn_scratch_bytes(53, 37, 4) >= 117 * 36
    assert L.lvdgs_recip_nn_scratch_bytes(512, 160, 8) > L.lvdgs_recip_nn_scratch_bytes(53, 37, 4)
    assert L.lvdgs_recip_nn_scratch_bytes(0, 37, 4) == 0 and L.lvdgs_recip_nn_scratch_bytes(53, 37, 0) == 0
