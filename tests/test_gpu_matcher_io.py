"""The HIP matcher I/O (``lvdgs_format_image`` behind ``init_pose.format_image`` / ``torch_images_to_dust3r_format``;
``lvdgs_match_depth_scale`` behind ``depth_utils.scale_from_matches`` / ``find_scale`` / ``MatchScaleRemedy``) against the NumPy
restatements tests/test_matcher_io.py holds to PIL and to their definitions: bit-exact formatting, the scale to the adjacent float32
with the valid count exact, determinism, the refusals of the C ABI, and the remedy branch of the keyframe depth alignment end to end --
``process_depth`` on the remedy cases, ``get_depth`` / ``NetworkDescribe`` on a stand-in network, and a drive whose every keyframe
takes the remedy."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import depth_align_cases as dc
import depth_align_oracle as dao
import image_format_oracle as fmt
import match_scale_oracle as mso
import matcher_io_cases as mc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
DEV = torch.device("cuda", 0)
CASE_KINDS = [(n, k) for n in mc.FORMAT_CASES for k in mc.KINDS]


def ulps(a, b):
    return abs(int(np.float32(a).view(np.int32)) - int(np.float32(b).view(np.int32)))


# ----------------------------------------------------------------------------------------------- the image formatting
@pytest.mark.parametrize("name,kind", CASE_KINDS)
def test_hip_format_is_bit_exact(name, kind):
    from lvdgs import init_pose
    W, H, size, raster = mc.FORMAT_CASES[name]
    img = mc.image(name, kind)
    want_q, want = fmt.format_image(img, size)
    t = torch.from_numpy(img).to(DEV)
    q = init_pose.format_image(t, size, quantised=True)
    out = init_pose.format_image(t, size)
    assert (out.shape[3], out.shape[2]) == init_pose.matcher_raster(W, H, size) == raster
    assert out.device == DEV and out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (1, 3, raster[1], raster[0])
    assert q.device == DEV and q.dtype == torch.uint8 and q.is_contiguous() and tuple(q.shape) == (raster[1], raster[0], 3)
    qn = q.cpu().numpy()
    print(name, kind, "bytes that differ", int((qn != want_q).sum()), "of", qn.size)
    assert np.array_equal(qn, want_q)
    assert out.cpu().numpy().tobytes() == want.tobytes()


def test_format_two_calls_are_bit_identical_across_the_table_cache():
    from lvdgs import init_pose
    a_img = torch.from_numpy(mc.image("lanczos_ratio_1p2", "noise")).to(DEV)
    b_img = torch.from_numpy(mc.image("odd_crop_offset", "noise")).to(DEV)
    a = init_pose.format_image(a_img, 512).cpu().numpy().tobytes()
    other = init_pose.format_image(b_img, 90).cpu().numpy().tobytes()       # another size's tables and a smaller use of the scratch
    init_pose.format_image(a_img, 128)                                       # the same image at another size
    assert init_pose.format_image(a_img, 512).cpu().numpy().tobytes() == a
    assert init_pose.format_image(b_img, 90).cpu().numpy().tobytes() == other
    assert len([k for k in init_pose._format_tables if k[1:3] == (613, 185)]) == 2


def test_format_refusals_and_the_dict_list():
    from lvdgs import _lib, init_pose
    img = torch.from_numpy(mc.image("lanczos_ratio_1p2", "smooth")).to(DEV)
    with pytest.raises(_lib.LvdgsError, match="224"):
        init_pose.format_image(img, 224)
    with pytest.raises(_lib.LvdgsError):
        init_pose.format_image(img.cpu(), 512)
    with pytest.raises(ValueError):
        init_pose.format_image(img[0], 512)
    other = torch.from_numpy(mc.image("lanczos_ratio_1p2", "noise")).to(DEV)
    views = init_pose.torch_images_to_dust3r_format([img, other], size=512)
    assert [v["idx"] for v in views] == [0, 1] and [v["instance"] for v in views] == ["0", "1"]
    for v, src in zip(views, (img, other)):
        assert set(v) == {"img", "true_shape", "idx", "instance"}
        assert v["true_shape"].dtype == np.int32 and v["true_shape"].tolist() == [[144, 512]]
        assert v["img"].device == DEV and tuple(v["img"].shape) == (1, 3, 144, 512)
        assert v["img"].cpu().numpy().tobytes() == fmt.format_image(src.cpu().numpy(), 512)[1].tobytes()


# ----------------------------------------------------------------------------------------------- the scale
def hip_scale(m1, m2, d1, d2, raster=mc.RASTER, tensors=True):
    from lvdgs import depth_utils
    if tensors:
        m1, m2 = torch.from_numpy(m1).to(DEV), torch.from_numpy(m2).to(DEV)
    s = depth_utils.scale_from_matches(m1, m2, d1, d2, raster)
    ls = depth_utils.last_scale
    return s, dict(status=ls.status, matches=ls.matches, valid=ls.valid, sum1=ls.sum1, sum2=ls.sum2)


def check_scale(m1, m2, d1, d2, what, raster=mc.RASTER):
    o = mso.match_scale(m1, m2, d1, d2, raster)
    s, words = hip_scale(m1, m2, d1, d2, raster)
    print(what, "hip", s, words, "oracle", o["scale"], o["valid"], o["sum1"], o["sum2"])
    assert words["matches"] == len(m1) and words["valid"] == o["valid"] and words["status"] == o["status"], what
    if o["scale"] is None:
        assert s is None and words["sum1"] == 0.0 and words["sum2"] == 0.0, what
        return o
    assert isinstance(s, float) and ulps(s, o["scale"]) <= 1, (what, s, o["scale"])
    assert abs(words["sum1"] - o["sum1"]) <= 1e-11 * o["sum1"] and abs(words["sum2"] - o["sum2"]) <= 1e-11 * o["sum2"], what
    return o


@pytest.mark.parametrize("with_holes", [False, True])
@pytest.mark.parametrize("M", mc.M_SWEEP)
def test_hip_scale_matches_the_oracle(M, with_holes):
    o = check_scale(*mc.sweep_case(M, with_holes), (M, with_holes))
    if M >= 63:
        assert (o["valid"] == M) if not with_holes else (0 < o["valid"] < 0.9 * M)


def test_hip_scale_borders_known_scales_and_no_valid():
    from lvdgs import _lib, depth_utils
    d1, d2 = mc.depth_map(185, 613, 1), mc.depth_map(90, 300, 2)
    m1, m2, inside = mc.border_matches()
    o = check_scale(m1, m2, d1, d2, "borders")
    assert o["valid"] == int(inside.sum())
    check_scale(m1, m2, mc.depth_map(30, 100, 3), mc.depth_map(20, 70, 4), "borders, upsizing")       # both corners clamp
    assert check_scale(m1[~inside], m2[~inside], d1, d2, "outside only")["scale"] is None
    assert depth_utils.last_scale.status == _lib.MATCH_SCALE_NO_VALID
    assert check_scale(*mc.grid_matches(), np.zeros_like(d1), d2, "zero map")["scale"] is None
    for shape in ((185, 613), (30, 100)):
        a, b = mc.scaled_pair(*shape, 1.37)
        s, words = hip_scale(*mc.grid_matches(), a, b)
        assert words["valid"] == 1152 and ulps(s, np.float32(1.37)) <= 1, (shape, s)
    # NumPy matches, a (1, H, W) tensor map: the same call
    g1, g2 = mc.grid_matches(jitter=2.0, seed=1)
    want, _ = hip_scale(g1, g2, d1, d2)
    got, _ = hip_scale(g1, g2, torch.from_numpy(d1).to(DEV)[None], d2, tensors=False)
    assert got == want


def test_scale_two_calls_are_bit_identical():
    m1, m2, d1, d2 = mc.sweep_case(8192, True)
    a = hip_scale(m1, m2, d1, d2)
    hip_scale(*mc.sweep_case(65, False))
    b = hip_scale(m1, m2, d1, d2)
    assert a == b and np.float64(a[1]["sum1"]).tobytes() == np.float64(b[1]["sum1"]).tobytes()


# ----------------------------------------------------------------------------------------------- the C ABI
def test_c_abi_refusals_launch_nothing():
    """Every LVDGS_E_INVALID condition of both entry points with real buffers behind the pointers: the call returns the status and its
    text, and neither the outputs nor the state words change."""
    from lvdgs import _lib, init_pose
    L = _lib.lib()
    stream = _lib.raw_stream(DEV)
    W, H, size = 200, 75, 90
    img = torch.from_numpy(mc.image("odd_crop_offset", "noise")).to(DEV)
    p, tx, ty = init_pose._format_plan(DEV, W, H, size)
    out = torch.full((3, p.out_height, p.out_width), -7.0, dtype=torch.float32, device=DEV)
    q = torch.full((p.out_height, p.out_width, 3), 7, dtype=torch.uint8, device=DEV)
    scratch = torch.zeros(max(L.lvdgs_format_scratch_bytes(W, H, size), 1 << 20), dtype=torch.uint8, device=DEV)

    def fmt_args(**over):
        kw = dict(width=W, height=H, size=size, image=img.data_ptr(), table_x=tx.data_ptr(), table_y=ty.data_ptr(), out=out.data_ptr(),
                  quantised=q.data_ptr(), scratch=scratch.data_ptr(), scratch_bytes=L.lvdgs_format_scratch_bytes(W, H, size))
        kw.update(over)
        return _lib.FormatImageArgs(**kw)
    for what, a, word in mc.format_refusals(fmt_args):
        assert L.lvdgs_format_image(None if a is None else C.byref(a), stream) == _lib.E_INVALID, what
        assert word in L.lvdgs_last_error(), (what, L.lvdgs_last_error())
    torch.cuda.synchronize(DEV)
    assert bool((out == -7.0).all()) and bool((q == 7).all()) and not bool(scratch.any())
    assert L.lvdgs_format_image(C.byref(fmt_args()), stream) == _lib.OK      # the same block without a fault in it runs
    torch.cuda.synchronize(DEV)
    want_q, want = fmt.format_image(img.cpu().numpy(), size)
    assert np.array_equal(q.cpu().numpy(), want_q) and out.cpu().numpy().tobytes() == want.tobytes()

    m1n, m2n, d1n, d2n = mc.sweep_case(64, False)
    m1, m2, d1, d2 = (torch.from_numpy(x).to(DEV) for x in (m1n, m2n, d1n, d2n))
    state = torch.full((_lib.MATCH_SCALE_HOST_BYTES // 4,), -7, dtype=torch.int32).pin_memory()

    def scale_args(**over):
        kw = dict(num_matches=64, raster_width=512, raster_height=144, width1=613, height1=185, width2=300, height2=90,
                  matches_im1=m1.data_ptr(), matches_im2=m2.data_ptr(), depth1=d1.data_ptr(), depth2=d2.data_ptr(), host_state=state.data_ptr())
        kw.update(over)
        return _lib.MatchScaleArgs(**kw)
    for what, a, word in mc.scale_refusals(scale_args):
        assert L.lvdgs_match_depth_scale(None if a is None else C.byref(a), stream) == _lib.E_INVALID, what
        assert word in L.lvdgs_last_error(), (what, L.lvdgs_last_error())
    torch.cuda.synchronize(DEV)
    assert (state == -7).all()
    assert L.lvdgs_match_depth_scale(C.byref(scale_args()), stream) == _lib.OK
    torch.cuda.synchronize(DEV)
    o = mso.match_scale(m1n, m2n, d1n, d2n, mc.RASTER)
    assert state[0] == _lib.MATCH_SCALE_OK and state[1] == 64 and state[2] == o["valid"]
    assert ulps(state[3:4].numpy().view(np.float32)[0], o["scale"]) <= 1
    # no matches: the pointers may be NULL, and the call reports NO_VALID
    assert L.lvdgs_match_depth_scale(C.byref(scale_args(num_matches=0, matches_im1=None, matches_im2=None)), stream) == _lib.OK
    torch.cuda.synchronize(DEV)
    assert state[0] == _lib.MATCH_SCALE_NO_VALID and state[1] == 0 and state[2] == 0


# ----------------------------------------------------------------------------------------------- end to end
class GridMatcher:
    """A fixed-grid stand-in for the matcher: the seeds' grid of the raster it is given, map-2 pixels jittered, as device tensors."""

    def __init__(self):
        self.rasters = []

    def __call__(self, im1, im2, model, raster):
        self.rasters.append(raster)
        m1, m2 = mc.grid_matches(raster, stride=8, seed=11, jitter=2.5)
        return torch.from_numpy(m1).to(DEV), torch.from_numpy(m2).to(DEV)


@pytest.mark.parametrize("name,factor,want_ks", [("remedy_at_k2", 2.47, [2]), ("remedy_at_k3", 0.55, [2, 3])])
def test_process_depth_takes_its_remedy_from_the_matches(name, factor, want_ks):
    """``process_depth`` on the remedy cases with ``MatchScaleRemedy`` on a stand-in matcher: the previous keyframe's depth is this one's
    mono depth x ``factor`` at half the size, so the remedy's scale is about ``factor`` -- one that lets the alignment go on (2.47) or
    sends it to the remedy again (0.55).  The scales are the scale oracle's on the same matches and maps, and the result is the
    depth-align oracle's when it is fed those scales."""
    from lvdgs import depth_utils, init_pose
    r, m, kw, _ = dc.make_case(name)
    H, W = r.shape
    last = np.ascontiguousarray(m[::2, ::2] * np.float32(factor))
    im1 = torch.zeros((3, H, W), device=DEV)
    matcher = GridMatcher()
    remedy = depth_utils.MatchScaleRemedy(matcher, record=True)
    final, scale, mask, num_acc = depth_utils.process_depth(r, m, last, im1, im1, None, scale_remedy=remedy, **kw)
    rec = depth_utils.last_call
    raster = init_pose.matcher_raster(W, H)
    assert matcher.rasters == [raster] * len(want_ks) and [k for k, _ in rec.remedies] == want_ks and rec.remedy_fired
    scales = []
    for (k, given), call in zip(rec.remedies, remedy.calls):
        assert call["depth1"] is last and call["depth2"] is m and call["raster"] == raster and call["matches_im1"].device == DEV
        o = mso.match_scale(call["matches_im1"].cpu().numpy(), call["matches_im2"].cpu().numpy(), last, m, raster)
        print(name, "k", k, "remedy", given, "oracle", o["scale"], "valid", o["valid"])
        assert given == call["scale"] and ulps(given, o["scale"]) <= 1 and abs(given / factor - 1.0) < 0.05
        scales.append(given)
    o = dao.align(r, m, scale_remedy=dc.RecordedRemedy(scales), **kw)
    assert o["remedies"] == want_ks
    assert ulps(scale, o["scale"]) <= 2, (scale, o["scale"])
    assert abs(num_acc - o["num_accurate"]) <= int(o["fragile"].sum())
    keep = ~o["fragile"]
    assert np.array_equal(mask[keep], o["error_mask"][keep])
    np.testing.assert_array_equal(final, np.where(mask, m * np.float32(scale), r))


class StandInNetwork:
    """``infer`` of ``NetworkDescribe`` / ``get_depth``: checks that its views are the formatted frames, returns seeded maps."""

    def __init__(self, frames, D=16):
        self.frames, self.D, self.calls = frames, D, 0

    def __call__(self, view1, view2, model):
        self.calls += 1
        preds = []
        for k, (view, frame) in enumerate(zip((view1, view2), self.frames)):
            want = fmt.format_image(frame, 512)[1]
            assert view["img"].device == DEV and view["img"].cpu().numpy().tobytes() == want.tobytes()
            H1, W1 = view["true_shape"][0]
            g = torch.Generator().manual_seed(70 + k)
            preds.append(dict(desc=torch.randn((1, H1, W1, self.D), generator=g).to(DEV), pts3d=(torch.rand((1, H1, W1, 3), generator=g) * 20 + 1).to(DEV)))
        return preds[0], preds[1]


def test_get_depth_and_network_describe_on_a_stand_in_network():
    from lvdgs import init_pose
    frames = [mc.image("lanczos_ratio_1p2", "smooth"), mc.image("lanczos_ratio_1p2", "noise")]
    img1, img2 = (torch.from_numpy(f).to(DEV) for f in frames)
    net = StandInNetwork(frames)
    raster = init_pose.matcher_raster(613, 185)
    d1, d2 = init_pose.NetworkDescribe(net)(img1, img2, "model", raster)
    assert tuple(d1.shape) == tuple(d2.shape) == (144, 512, 16) and d1.device == DEV
    g = torch.Generator().manual_seed(70)
    assert torch.equal(d1.cpu(), torch.randn((1, 144, 512, 16), generator=g)[0])
    with pytest.raises(ValueError, match="descriptors"):
        init_pose.NetworkDescribe(net)(img1, img2, "model", (512, 160))
    m1, m2 = init_pose.DescriptorMatcher(init_pose.NetworkDescribe(net))(img1, img2, "model", raster)
    assert m1.device == DEV and m1.shape == m2.shape and m1.shape[0] > 0
    z = init_pose.get_depth(img1, img2, "model", infer=net)
    assert z.device == DEV and z.dtype == torch.float32 and tuple(z.shape) == (185, 613) and z.is_contiguous()
    g = torch.Generator().manual_seed(70)
    torch.randn((1, 144, 512, 16), generator=g)
    pts = (torch.rand((1, 144, 512, 3), generator=g) * 20 + 1).numpy()
    assert np.array_equal(z.cpu().numpy(), mso.nearest_resize(pts[0, :, :, 2], 613, 185))
    with pytest.raises(TypeError):
        init_pose.get_depth(img1, img2, "model")
    assert net.calls == 4


FAST = dict(step=0.06, sway=0.3, yaw=0.09, period=40.0)      # the fast trajectory of tests/test_gpu_init_pose.py


def test_a_drive_whose_keyframes_all_take_the_remedy():
    """Twelve half-size frames, short cadence, Algorithm 1 with a bar no keyframe can pass (min_accurate_pixels_ratio 1.1): every
    keyframe after the first goes through the remedy, which is ``find_scale`` on the descriptor matcher's matches -- a finite scale,
    the scale oracle's on the recorded matches and depth maps.  Without ``scale_remedy`` the same constructor arguments leave the
    stand-in in place, and a drive with default arguments touches none of this.

    ``epsilon=0.0`` goes with the ratio.  The bar is looked at in iterations 2 and 3 only, and the loop's own exit (|scale - previous
    scale| < epsilon at the top of an iteration, utils/depth_utils.py:77 of the reference) comes first: this drive's mono depth is
    consistent with its map, so iteration 0 finds the scale (0.980 and 0.969 on the two keyframes), iteration 1 finds it again, and
    with the default epsilon of 0.01 the loop ends at the top of iteration 2 on both -- the bar is never looked at and nothing fires,
    here as in the reference.  With epsilon 0 that exit cannot be taken (no difference is < 0), every keyframe reaches iteration 2,
    and the ratio does what it is there for."""
    import sequence as tool
    from lvdgs import depth_utils, init_pose
    from lvdgs.slam_sequence import SlamSequence
    drive = dict(frames=12, scale=0.5, cadence="short", idle=0, refine=0, masks=True, window_size=5, trajectory=FAST)

    def start_recording(event, seq):
        if seq.scale_remedy is not None and seq.scale_remedy.calls is None:
            seq.scale_remedy.calls = []
    rec, seq = tool.run_sequence(DEV, **drive, keyframe_depth="patch_align", scale_remedy="matches", matcher="descriptors",
                                 depth_align_params=dict(min_accurate_pixels_ratio=1.1, epsilon=0.0), on_event=start_recording)
    assert isinstance(seq.scale_remedy, depth_utils.MatchScaleRemedy) and isinstance(seq.scale_remedy.matcher, init_pose.DescriptorMatcher)
    log, calls = rec["depth_align"], seq.scale_remedy.calls
    print(log)
    assert len(log) == len(seq.kf_indices) - 1 >= 2 and all(r["remedy_fired"] for r in log)
    assert len(log) <= len(calls) <= 2 * len(log)
    raster = init_pose.matcher_raster(seq.dataset.width, seq.dataset.height)
    for call in calls:
        assert call["raster"] == raster == (512, 144) and call["matches_im1"].device == DEV
        o = mso.match_scale(call["matches_im1"].cpu().numpy(), call["matches_im2"].cpu().numpy(), call["depth1"], call["depth2"], raster)
        print("matches", o["matches"], "valid", o["valid"], "scale", call["scale"], "oracle", o["scale"])
        assert o["valid"] > 100 and np.isfinite(call["scale"]) and ulps(call["scale"], o["scale"]) <= 1
    assert all(np.isfinite(r["scale_factor"]) and r["scale_factor"] > 0 for r in log)
    with pytest.raises(TypeError, match="matcher"):
        SlamSequence(seq.config, seq.dataset, tool.empty_map(seq.config, DEV), tool.PIPE, torch.zeros(3, device=DEV), keyframe_depth="patch_align",
                     scale_remedy="matches")
    depth_utils.last_scale.status = "untouched"
    tables = dict(init_pose._format_tables)
    rec0, seq0 = tool.run_sequence(DEV, **drive)
    assert seq0.scale_remedy is None and depth_utils.last_scale.status == "untouched" and init_pose._format_tables == tables
    assert "depth_align" not in rec0 and rec0["frames"] == 12
