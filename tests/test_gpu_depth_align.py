"""The HIP keyframe depth alignment (``lvdgs.depth_utils.process_depth`` -> ``lvdgs_depth_align``, LVD-GS Algorithm 1) against the
reference's own results (tests/golden/depth_align.npz) and the float64 oracle (tests/depth_align_oracle.py), on the golden cases and
40 seeded random ones; determinism, NumPy vs tensor inputs, argument errors; and a KITTI-geometry drive whose mono depth drifts in
scale from frame to frame, aligned by the sequence's opt-in ``keyframe_depth="patch_align"``."""
import json
import os

import numpy as np
import pytest
import torch

import depth_align_cases as dc
import depth_align_oracle as orc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ulps(a, b):
    return abs(int(np.float32(a).view(np.int32)) - int(np.float32(b).view(np.int32)))


def hip(r, m, kw, remedy):
    from lvdgs import depth_utils
    stand_in = dc.RecordedRemedy(remedy) if remedy else None
    out = depth_utils.process_depth(r, m, None, None, None, None, scale_remedy=stand_in, **kw)
    rec = depth_utils.last_call
    return out, rec, (stand_in.calls if stand_in else 0)


def check_against_oracle(r, m, kw, remedy, what):
    (final, scale, mask, num_acc), rec, _ = hip(r, m, kw, remedy)
    o = orc.align(r, m, scale_remedy=dc.RecordedRemedy(remedy) if remedy else None, **kw)
    assert isinstance(final, np.ndarray) and final.dtype == np.float32 and mask.dtype == bool and isinstance(scale, np.float32)
    assert ulps(scale, o["scale"]) <= 2, (what, scale, o["scale"])
    nfrag = int(o["fragile"].sum())
    assert abs(num_acc - o["num_accurate"]) <= nfrag, (what, num_acc, o["num_accurate"], nfrag)
    if o["fragile_patches"] == 0:
        assert rec.patch_num == o["patch_num"], what
    assert [k for k, _ in rec.remedies] == o["remedies"], what
    keep = ~o["fragile"]
    assert np.array_equal(mask[keep], o["error_mask"][keep]), (what, int((mask != o["error_mask"])[keep].sum()))
    # the fill, as NumPy forms it, at the scale the kernel found
    ms = m * np.float32(scale)
    np.testing.assert_array_equal(final, np.where(mask, ms, r))
    return o


@pytest.mark.parametrize("name", sorted(dc.CASES))
def test_hip_matches_the_reference_and_the_oracle_on_the_golden_cases(name):
    g = np.load(os.path.join(ROOT, "tests", "golden", "depth_align.npz"))
    meta = json.loads(str(g["meta"]))[name]
    r, m, kw, remedy = dc.make_case(name)
    assert dc.sha256(r, m) == meta["input_sha256"]
    o = check_against_oracle(r, m, kw, remedy, name)
    (final, scale, mask, num_acc), rec, calls = hip(r, m, kw, remedy)
    num_accurate, patch_num, remedy_calls = (int(x) for x in g[name + "/ints"])
    assert ulps(scale, g[name + "/scale"]) <= 2, (scale, g[name + "/scale"])
    assert num_acc == num_accurate and rec.patch_num == patch_num and calls == remedy_calls
    want = np.unpackbits(g[name + "/error_mask"], count=r.size).reshape(r.shape).astype(bool)
    keep = ~o["fragile"]
    assert np.array_equal(mask[keep], want[keep])


@pytest.mark.parametrize("seed", range(40))
def test_hip_matches_the_oracle_on_random_cases(seed):
    r, m, kw, remedy = dc.random_case(seed)
    o = check_against_oracle(r, m, kw, remedy, seed)
    if seed % 4 in (1, 2):
        assert o["remedies"] == ([2] if seed % 4 == 1 else [2, 3])


def test_two_calls_are_bit_identical_and_numpy_equals_tensor_inputs():
    from lvdgs import depth_utils
    r, m, kw, _ = dc.make_case("kitti_clipped_edges")
    a = depth_utils.process_depth(r, m, **kw)
    b = depth_utils.process_depth(r, m, **kw)
    assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[2], b[2]) and a[1].tobytes() == b[1].tobytes() and a[3] == b[3]
    dev = torch.device("cuda", 0)
    rt, mt = torch.from_numpy(r).to(dev)[None], torch.from_numpy(m).to(dev)     # (1, H, W) render depth, as the renderer returns it
    t = depth_utils.process_depth(rt, mt, **kw)
    assert t[0].device == dev and t[0].dtype == torch.float32 and t[2].dtype == torch.bool and t[2].device == dev
    assert t[0].cpu().numpy().tobytes() == a[0].tobytes() and np.array_equal(t[2].cpu().numpy(), a[2])
    assert np.float32(t[1]) == a[1] and t[3] == a[3]


def test_remedy_branches_are_exposed_and_without_a_remedy_the_scale_is_kept():
    from lvdgs import _lib, depth_utils
    r, m, kw, _ = dc.make_case("remedy_at_k2")
    final, scale, mask, n = depth_utils.process_depth(r, m, **kw)
    assert depth_utils.last_call.remedy_fired and depth_utils.last_call.remedies == [(2, None), (3, None)]
    assert scale == np.float32(1.0) and depth_utils.last_call.status == _lib.DEPTH_ALIGN_EXHAUSTED
    seen = []
    depth_utils.process_depth(r, m, "last", "im1", "im2", "model", scale_remedy=lambda *a: seen.append(a) or 2.47, **kw)
    assert len(seen) == 1 and seen[0][:3] == ("im1", "im2", "last") and seen[0][3] is m and seen[0][4] == "model"
    assert depth_utils.last_call.remedies == [(2, 2.47)]
    r, m, kw, _ = dc.make_case("converges_at_k1")
    depth_utils.process_depth(r, m, **kw)
    assert not depth_utils.last_call.remedy_fired and depth_utils.last_call.status == _lib.DEPTH_ALIGN_CONVERGED
    assert depth_utils.last_call.iteration == 0
    final, scale, mask, n = depth_utils.process_depth(r, m, max_iter=0, **kw)
    assert scale == np.float32(1.0) and n == 0 and depth_utils.last_call.patch_num == 0


def test_invalid_arguments_are_refused():
    import ctypes as C

    from lvdgs import _lib, depth_utils
    r, m, kw, _ = dc.make_case("zeros_in_render")
    for p in (0, _lib.DEPTH_ALIGN_MAX_PATCH + 1):
        with pytest.raises(_lib.LvdgsError, match=r"\(1\).*patch_size"):
            depth_utils.process_depth(r, m, patch_size=p)
    with pytest.raises(ValueError):
        depth_utils.process_depth(r, m[:-1])
    with pytest.raises(_lib.LvdgsError):
        depth_utils.process_depth(torch.from_numpy(r), torch.from_numpy(m))     # CPU tensors: no CPU path
    L = _lib.lib()
    a = _lib.DepthAlignArgs(width=250, height=120, patch_size=10, max_iter=4)
    assert L.lvdgs_depth_align(C.byref(a), None) == _lib.E_INVALID
    a.width = -1
    assert L.lvdgs_depth_align(C.byref(a), None) == _lib.E_INVALID


# ----------------------------------------------------------------------------------------------- the sequence
DRIFT = 0.15


@pytest.fixture(scope="module")
def drives():
    """The same 40-frame KITTI-geometry drive (half size, short cadence, no dynamic objects) with a mono depth whose scale wanders by
    +-15 % from frame to frame, seeded from the mono depth (default) and from Algorithm 1's alignment; the seeded depth of every
    keyframe and the true depth at its ground-truth pose."""
    import random
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import sequence as tool
    from lvdgs.gaussian_renderer import render
    from lvdgs.slam_sequence import SlamSequence
    dev = torch.device("cuda", 0)
    out = {}
    for mode in ("mono", "patch_align"):
        torch.manual_seed(0)
        random.seed(0)
        cfg, ds, truth = tool.kitti_sequence(dev, frames=40, scale=0.5, cadence="short", masks=False, mono_scale_drift=DRIFT, window_size=4)
        seq = SlamSequence(cfg, ds, tool.empty_map(cfg, dev), tool.PIPE, torch.zeros(3, device=dev), idle_map_iters=2,
                           keyframe_depth=None if mode == "mono" else "patch_align")
        seeded, orig = {}, seq.add_new_keyframe

        def record(idx, render_pkg=None, init=False, orig=orig, seeded=seeded):
            d = orig(idx, render_pkg=render_pkg, init=init)
            seeded[idx] = torch.as_tensor(np.asarray(d) if not torch.is_tensor(d) else d).float().to(dev)
            return d
        seq.add_new_keyframe = record
        seq.run()
        true_depth = {}
        for idx in seq.kf_indices:
            vp = seq.cameras[idx]
            R, T = vp.R.clone(), vp.T.clone()
            vp.update_RT(vp.R_gt, vp.T_gt)
            with torch.no_grad():
                pkg = render(vp, truth, tool.PIPE, torch.zeros(3, device=dev))
            vp.update_RT(R, T)
            op = pkg["opacity"][0]
            true_depth[idx] = torch.where(op > 0.5, pkg["depth"][0] / op.clamp(min=1e-3), torch.zeros_like(op))
        out[mode] = dict(seq=seq, ds=ds, seeded=seeded, truth=true_depth, summary=seq.summary())
    return out


def test_patch_align_recovers_the_per_keyframe_mono_scale(drives):
    """Frame i's mono depth is its true depth times f_i = 1 + 0.15 sin(2 pi i / 11) (times 2 % pixel noise); the map is seeded from
    frame 0's, so the factor Algorithm 1 finds for keyframe i should be c * f_0 / f_i: factor * f_i / f_0 ~ c, the same c for every
    keyframe.  c is the map's own depth level against frame 0's surface depth: the rendered depth is the alpha-blended sum T alpha d
    (as upstream's), below the surface wherever the accumulated opacity is below one -- 0.86-0.90 on this short drive.  What the
    algorithm has to remove is the per-keyframe drift, up to +-15 %: the ratios lie within +-4 % of their median (observed +-2.5 %:
    the map's opacity and pose errors vary from view to view; the 2 % pixel noise averages out over the thousands of accurate pixels)."""
    d = drives["patch_align"]
    log, ds = d["summary"]["depth_align"], d["ds"]
    assert len(log) == len(d["seq"].kf_indices) - 1 >= 3
    f0 = ds.mono_scales[0]
    ratios = [rec["scale_factor"] * ds.mono_scales[rec["frame"]] / f0 for rec in log]
    c = float(np.median(ratios))
    assert 0.75 < c < 1.05, ratios
    assert all(abs(x / c - 1.0) < 0.04 for x in ratios), ratios
    drifts = [ds.mono_scales[rec["frame"]] for rec in log]
    assert max(drifts) / min(drifts) > 1.1       # the drive does drift between its keyframes
    assert sum(rec["remedy_fired"] for rec in log) <= len(log) // 2   # (a keyframe with little overlap may still take the remedy branch)
    assert d["summary"]["seconds"]["depth_align"] > 0.0


def test_patch_align_seeds_closer_to_the_truth_than_the_mono_default(drives):
    """The depth every keyframe after the first seeds from, against its true surface depth, up to ONE scale for the whole drive (a
    monocular map's scale is free; what matters is that the keyframes agree with one another): the median relative error per keyframe,
    averaged over the keyframes, after the best common factor.  The mono default carries each keyframe's drift into the map."""
    def err(mode):
        d = drives[mode]
        pairs = []
        for idx in d["seq"].kf_indices[1:]:
            s, t = d["seeded"][idx], d["truth"][idx]
            ok = (s > 0) & (t > 0)
            pairs.append((s[ok].double(), t[ok].double()))
        c = float(torch.cat([t / s for s, t in pairs]).median())
        return float(np.mean([float(((c * s - t).abs() / t).median()) for s, t in pairs]))
    mono, aligned = err("mono"), err("patch_align")
    assert aligned < mono, (aligned, mono)
