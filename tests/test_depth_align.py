"""CPU checks of the keyframe depth alignment (LVD-GS Algorithm 1, ``lvdgs.depth_utils.process_depth`` / ``lvdgs_depth_align``):
the float64 oracle (tests/depth_align_oracle.py) against what the reference's own ``process_depth`` computed on the golden cases,
argument validation, and the sequence's opt-in wiring on the toy CPU harness with the oracle
as the aligner."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import depth_align_cases as dc
import depth_align_oracle as orc
from lvdgs import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "depth_align.npz")


def golden():
    g = np.load(GOLDEN)
    return g, json.loads(str(g["meta"]))


def ulps(a, b):
    a, b = np.float32(a), np.float32(b)
    return abs(int(a.view(np.int32)) - int(b.view(np.int32)))


@pytest.mark.parametrize("name", sorted(dc.CASES))
def test_oracle_matches_the_reference_on_the_golden_cases(name):
    g, meta = golden()
    r, m, kw, remedy = dc.make_case(name)
    assert dc.sha256(r, m) == meta[name]["input_sha256"], "the case generator changed: regenerate tests/golden/depth_align.npz"
    stand_in = dc.RecordedRemedy(remedy)
    out = orc.align(r, m, scale_remedy=stand_in, **kw)
    num_accurate, patch_num, remedy_calls = (int(x) for x in g[name + "/ints"])
    assert ulps(out["scale"], g[name + "/scale"]) <= 2, (out["scale"], g[name + "/scale"])
    assert out["num_accurate"] == num_accurate and out["patch_num"] == patch_num
    assert len(out["remedies"]) == remedy_calls == stand_in.calls
    want = np.unpackbits(g[name + "/error_mask"], count=r.size).reshape(r.shape).astype(bool)
    keep = ~out["fragile"]
    assert np.array_equal(out["error_mask"][keep], want[keep]), int((out["error_mask"] != want)[keep].sum())


def test_golden_cases_cover_the_branches():
    """Every branch the issue lists is in the fixture: clipped edge patches, a patch of 16 on a non-multiple size, zeros / NaNs,
    convergence at the top of iteration 1, the remedy at k = 2 and at k = 3, no accurate pixel at all."""
    g, meta = golden()
    shape = lambda n: meta[n]["shape"]   # noqa: E731
    assert shape("kitti_clipped_edges") == [370, 1226] and 1226 % 10 == 6
    assert meta["odd_size_patch16"]["kwargs"]["patch_size"] == 16 and all(v % 16 for v in shape("odd_size_patch16"))
    r, m, kw, rem = dc.make_case("converges_at_k1")
    assert orc.align(r, m, **kw)["iterations"] == 1
    assert orc.align(*dc.make_case("remedy_at_k2")[:2], scale_remedy=dc.RecordedRemedy([2.47]))["remedies"] == [2]
    r, m, kw, rem = dc.make_case("remedy_at_k3")
    assert orc.align(r, m, scale_remedy=dc.RecordedRemedy(rem), **kw)["remedies"] == [2, 3]
    assert int(g["no_accurate_pixel/ints"][0]) == 0 and float(g["no_accurate_pixel/scale"]) == 1.0
    assert sum(len(g[k].tobytes()) for k in g.files) < 2 * 2 ** 20


def test_oracle_without_remedy_keeps_the_scale():
    """No remedy: the scale stays 1, so the top-of-iteration test (which never stops at s == 1) lets iteration 3 run and take the
    remedy branch again."""
    r, m, kw, _ = dc.make_case("remedy_at_k2")
    out = orc.align(r, m, **kw)
    assert out["remedies"] == [2, 3] and out["iterations"] == 4 and out["scale"] == np.float32(1.0)


def test_depth_align_argument_validation_without_gpu():
    L = _lib.lib()
    assert L.lvdgs_depth_align(None, None) == _lib.E_INVALID
    a = _lib.DepthAlignArgs(width=1226, height=370, patch_size=10, max_iter=4)
    assert L.lvdgs_depth_align(C.byref(a), None) == _lib.E_INVALID and b"NULL" in L.lvdgs_last_error()
    for p in (0, -3, _lib.DEPTH_ALIGN_MAX_PATCH + 1):
        a.patch_size = p
        assert L.lvdgs_depth_align(C.byref(a), None) == _lib.E_INVALID and b"patch_size" in L.lvdgs_last_error()
    a.patch_size, a.width = 10, 0
    assert L.lvdgs_depth_align(C.byref(a), None) == _lib.E_INVALID and b"image size" in L.lvdgs_last_error()
    a.width, a.max_iter = 1226, -1
    assert L.lvdgs_depth_align(C.byref(a), None) == _lib.E_INVALID
    a.max_iter = 4
    for f in ("render_depth", "mono_depth", "final_depth", "error_mask", "host_state", "scratch"):
        setattr(a, f, 256)          # (never dereferenced: every call here is rejected before a launch)
    a.scratch_bytes = L.lvdgs_depth_align_scratch_bytes(1226, 370, 10) - 1
    assert L.lvdgs_depth_align(C.byref(a), None) == _lib.E_INVALID and b"scratch" in L.lvdgs_last_error()
    assert L.lvdgs_depth_align_resume(None, 1.0, None) == _lib.E_INVALID
    s10, s4 = L.lvdgs_depth_align_scratch_bytes(1226, 370, 10), L.lvdgs_depth_align_scratch_bytes(1226, 370, 4)
    assert s10 % 256 == 0 and s4 > s10 >= 4551 // 4 * 24


def oracle_aligner(calls):
    """process_depth's signature over the oracle (the CPU stand-in for the HIP call); records what it was given."""
    def fn(render_depth, mono_depth, last_depth=None, im1=None, im2=None, model=None, scale_remedy=None, **kw):
        r = render_depth.detach().cpu().numpy() if torch.is_tensor(render_depth) else np.asarray(render_depth)
        m = np.array(mono_depth, np.float32)
        remedy = None if scale_remedy is None else (lambda: scale_remedy(im1, im2, last_depth, mono_depth, model))
        out = orc.align(r, m, scale_remedy=remedy, **kw)
        calls.append(dict(r=r, m=m, out=out, kw=kw))
        return out["final_depth"], out["scale"], out["error_mask"], out["num_accurate"]
    return fn


def test_sequence_patch_align_wiring_on_the_cpu_harness():
    """SlamSequence(keyframe_depth="patch_align") on the toy CPU harness with the oracle as the aligner: every keyframe after the
    first is aligned against the tracking render's depth; the keyframe's mono depth is rescaled on the viewpoint (a new array), the
    seeded depth is the aligner's, zero outside the valid pixels; the scale remedy receives the previous keyframe's mono depth and
    image; the per-keyframe log and the step's time are in the summary."""
    import random

    import sequence_scene as ss
    from lvdgs import simple_knn
    from lvdgs.slam_sequence import SlamSequence
    torch.manual_seed(0)
    random.seed(0)
    cfg, ds, hooks, knn, _ = ss.toy_sequence_on_cpu(n_frames=9)
    for im in ds.images:      # a black corner (outside the valid pixels, as the black borders of rectified frames), so that the zeroing shows
        im[:, :3, :6] = 0.0
    calls, remedy_args, seeded = [], [], {}

    def remedy(im1, im2, last_depth, mono_depth, model):
        remedy_args.append((im1, im2, last_depth, mono_depth))
        return None

    real_knn, simple_knn.distCUDA2 = simple_knn.distCUDA2, knn
    try:
        # min_accurate_pixels_ratio 1: never enough accurate pixels, epsilon 0: never converged, so both remedy branches are taken at every keyframe
        seq = SlamSequence(cfg, ds, ss.empty_map(cfg, "cpu"), ss.PIPE, torch.zeros(3), keyframe_depth="patch_align",
                           depth_align_fn=oracle_aligner(calls), scale_remedy=remedy,
                           depth_align_params=dict(patch_size=8, min_accurate_pixels_ratio=1.0, epsilon=0.0), **hooks)
        orig = seq.add_new_keyframe

        def record(idx, render_pkg=None, init=False):
            before = np.array(seq.cameras[idx].mono_depth, copy=True)
            d = orig(idx, render_pkg=render_pkg, init=init)
            seeded[idx] = (np.array(d, copy=True), before)
            return d
        seq.add_new_keyframe = record
        seq.run()
    finally:
        simple_knn.distCUDA2 = real_knn
    kfs = seq.kf_indices
    assert len(kfs) >= 2 and len(calls) == len(kfs) - 1 == len(seq.depth_align_log)
    thr = cfg["Training"]["rgb_boundary_threshold"]
    # the first keyframe: the mono path
    valid0 = (seq.cameras[0].original_image.sum(0) > thr).numpy()
    np.testing.assert_array_equal(seeded[0][0], np.where(valid0, ds.mono_depths[0], 0.0).astype(np.float32))
    for j, idx in enumerate(kfs[1:]):
        c, vp, rec = calls[j], seq.cameras[idx], seq.depth_align_log[j]
        depth, mono_before = seeded[idx]
        np.testing.assert_array_equal(c["m"], mono_before)
        assert c["kw"] == dict(patch_size=8, min_accurate_pixels_ratio=1.0, epsilon=0.0)
        scale = c["out"]["scale"]
        assert vp.mono_depth is not mono_before and vp.mono_depth.dtype == np.float32
        np.testing.assert_array_equal(vp.mono_depth, (mono_before * np.float32(scale)).astype(np.float32))
        valid = (vp.original_image.sum(0) > thr).numpy()
        assert (~valid).any()
        np.testing.assert_array_equal(depth, np.where(valid, c["out"]["final_depth"], 0.0).astype(np.float32))
        assert rec["frame"] == idx and rec["scale_factor"] == float(scale) and rec["remedy_fired"]
        assert rec["num_accurate_pixels"] == c["out"]["num_accurate"]
        assert rec["error_pixel_share"] == pytest.approx(float(c["out"]["error_mask"].mean()))
    # two remedy calls per aligned keyframe (k = 2 and k = 3), each with the PREVIOUS keyframe's mono depth and image
    assert len(remedy_args) == 2 * (len(kfs) - 1)
    for j, idx in enumerate(kfs[1:]):
        prev = seq.cameras[kfs[j]]
        for im1, im2, last_depth, mono in remedy_args[2 * j: 2 * j + 2]:
            assert im1 is prev.original_image and im2 is seq.cameras[idx].original_image
            assert last_depth is prev.mono_depth or np.array_equal(last_depth, prev.mono_depth)
    s = seq.summary()
    assert s["depth_align"] == seq.depth_align_log and s["seconds"]["depth_align"] > 0.0


def test_sequence_default_is_unchanged_and_bad_choice_is_refused():
    import sequence_scene as ss
    from lvdgs.slam_sequence import SlamSequence
    cfg, ds, hooks, _, _ = ss.toy_sequence_on_cpu(n_frames=2)
    seq = SlamSequence(cfg, ds, ss.empty_map(cfg, "cpu"), ss.PIPE, torch.zeros(3), **hooks)
    assert seq.keyframe_depth == seq.default_keyframe_depth and "depth_align" not in seq.seconds
    assert "depth_align" not in seq.summary()
    with pytest.raises(ValueError):
        SlamSequence(cfg, ds, ss.empty_map(cfg, "cpu"), ss.PIPE, torch.zeros(3), keyframe_depth="median", **hooks)


def test_mono_scale_drift_is_deterministic_and_off_by_default():
    """make_sequence(mono_scale_drift=d) multiplies frame i's mono depth by 1 + d sin(2 pi i / 11) and draws nothing extra: the
    images are the same, the mono depths are the drift-free ones times the factor."""
    import sequence_scene as ss
    from lvdgs import synthetic
    t = ss.TOY
    hooks, _, _ = ss.cpu_hooks()
    truth = ss.truth_model(t["W"], t["H"], 120, t["r_min"], t["r_max"], t["margin"], "cpu")
    mk = lambda d: synthetic.make_sequence(truth, hooks["render_fn"], ss.PIPE, t["W"], t["H"], 3, "cpu", seed=3, depth_noise=0.01,  # noqa: E731
                                           mono_scale_drift=d)
    a, b = mk(0.0), mk(0.2)
    assert a.mono_scales == [1.0, 1.0, 1.0]
    for i in range(3):
        assert torch.equal(a.images[i], b.images[i])
        f = synthetic.mono_scale_factor(i, 0.2)
        assert b.mono_scales[i] == f
        np.testing.assert_allclose(b.mono_depths[i], a.mono_depths[i] * f, rtol=1e-6)
