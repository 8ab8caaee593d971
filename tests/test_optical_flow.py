"""The optical-flow specification without a GPU: the float64 NumPy statement of the header's text (tests/optical_flow_oracle.py) checked
against what Farneback's method promises, ``lvdgs.optical_flow.farneback_torch`` against it, ``MotionFallback(fused=False)`` in the
masker's seat against the recorded reference sequences (tests/golden/motion_fallback.npz), and every refusal of the two entry points
(all happen before any launch)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import optical_flow_cases as cases
import optical_flow_oracle as oracle
from lvdgs import _lib
from lvdgs import dynamic_mask as dm
from lvdgs import optical_flow as of

# the median endpoint error of the float64 oracle on scene (a) -- recorded in DESIGN.md section 4p; the tests assert at twice these
RECORDED_MEDIAN_EPE = {(64, 48): 0.0341, (130, 70): 0.0214, (261, 259): 0.0153}


def test_level_counts_and_sizes():
    sizes = lambda W, H: [(lv["w"], lv["h"]) for lv in oracle.pyramid(W, H, 0.5, 3)]
    assert sizes(64, 48) == [(64, 48)]
    assert sizes(130, 70) == [(65, 35), (130, 70)]
    assert sizes(261, 259) == [(33, 32), (65, 65), (130, 130), (261, 259)]      # both half-to-even roundings: 130.5 -> 130, 129.5 -> 130
    assert sizes(9, 7) == [(9, 7)]
    assert [lv["ksize"] for lv in oracle.pyramid(261, 259, 0.5, 3)] == [19, 9, 3, 3]
    assert [lv["sigma"] for lv in oracle.pyramid(261, 259, 0.5, 3)] == [3.5, 1.5, 0.5, 0.0]
    assert len(oracle.pyramid(1226, 370, 0.5, 3)) == 4 and len(oracle.pyramid(1226, 370, 0.5, 0)) == 1
    for W, H in cases.SIZES + ((1226, 370),):
        assert of.pyramid(W, H, 0.5, 3) == oracle.pyramid(W, H, 0.5, 3)


@pytest.mark.parametrize("n,sigma", [(5, 1.2), (7, 1.5)])
def test_the_expansion_returns_the_coefficients_of_a_quadratic_image(n, sigma):
    W, H = 40, 33
    x, y = cases.grid(W, H)
    c0, cx, cy, cxx, cyy, cxy = 3.0, -0.7, 0.45, 0.031, -0.022, 0.017
    img = c0 + cx * x + cy * y + cxx * x * x + cyy * y * y + cxy * x * y
    want = np.stack([cy + 2 * cyy * y + cxy * x, cx + 2 * cxx * x + cxy * y, np.full_like(x, cyy), np.full_like(x, cxx), np.full_like(x, cxy)], axis=2)
    R = oracle.poly_exp(img, n, sigma, np.float64)
    inner = (slice(n, H - n), slice(n, W - n))
    assert np.abs(R[inner] - want[inner]).max() < 1e-11      # (values up to 60: 1e-15 relative leaves room)
    Rt = of._poly_exp(torch.from_numpy(img), n, sigma).numpy()
    assert np.abs(Rt - R).max() < 1e-11


@pytest.mark.parametrize("W,H", cases.SIZES[:3])
def test_a_whole_frame_shift_is_recovered_with_its_sign(W, H):
    f1, f2 = cases.whole_shift(W, H)
    shift = np.array(cases.SHIFT_A)
    for flow in (oracle.farneback(f1, f2), of.farneback_torch(torch.from_numpy(f1), torch.from_numpy(f2)).numpy().astype(np.float64)):
        epe = np.sqrt(((flow - shift) ** 2).sum(-1))
        print(f"{W}x{H}: median endpoint error {np.median(epe):.4f} px")
        assert np.median(epe) <= 2 * RECORDED_MEDIAN_EPE[W, H]
        assert abs(np.median(flow[..., 0]) - shift[0]) < 0.05 and abs(np.median(flow[..., 1]) - shift[1]) < 0.05      # +d gives +d
    back = oracle.farneback(f2, f1)
    assert abs(np.median(back[..., 0]) + shift[0]) < 0.05 and abs(np.median(back[..., 1]) + shift[1]) < 0.05


@pytest.mark.parametrize("W,H", cases.SIZES)
@pytest.mark.parametrize("kind", ["a", "b"])
def test_farneback_torch_against_the_oracle(kind, W, H):
    """Float32 PyTorch statements against the float64 oracle, within 16 x the oracle's own float32 - float64 distance."""
    f1, f2 = (cases.whole_shift if kind == "a" else cases.moving_rectangle)(W, H)[:2]
    f64, levels = oracle.farneback(f1, f2, np.float64, return_levels=True)
    f32 = oracle.farneback(f1, f2, np.float32)
    got, got_levels = of.farneback_torch(torch.from_numpy(f1), torch.from_numpy(f2), return_levels=True)
    tol = 16 * np.abs(f32 - f64).max()
    assert got_levels == levels and got.dtype is torch.float32 and np.abs(got.numpy() - f64).max() <= tol
    wide = of.farneback_torch(torch.from_numpy(f1), torch.from_numpy(f2), dtype=torch.float64)
    assert np.abs(wide.numpy() - f64).max() <= 1e-9


def test_the_oracles_mask_on_the_moving_rectangle():
    """What the GPU test relies on, from the oracle alone: few pixels near the threshold, no flip in float32, the rectangle covered."""
    for W, H in ((130, 70), (261, 259)):
        f1, f2, inside = cases.moving_rectangle(W, H)
        moving, mask, magnitude, _ = oracle.motion_mask(f1, f2)
        moving32, mask32, _, _ = oracle.motion_mask(f1, f2, dtype=np.float32)
        near = np.abs(magnitude - 3.0) < 1e-3
        print(f"{W}x{H}: {100 * near.mean():.4f} % near the threshold, {100 * mask[inside].mean():.1f} % of the rectangle covered")
        assert near.mean() <= 0.0003 and np.array_equal(moving, moving32) and np.array_equal(mask, mask32)
        assert mask[inside].mean() >= 0.98


def test_grey_is_the_quantised_integer_grey():
    rng = np.random.default_rng(3)
    image = rng.uniform(-0.1, 1.1, (3, 37, 53)).astype(np.float32)
    image[:, 0, :4] = np.array([0.0, 1.0, 254.999 / 255, 0.5], np.float32)
    q = np.clip(image * np.float32(255), 0, 255).astype(np.uint8).astype(np.int64)
    want = ((4899 * q[0] + 9617 * q[1] + 1868 * q[2] + 8192) >> 14).astype(np.uint8)
    assert np.array_equal(oracle.grey_of(image), want) and np.array_equal(of.grey_torch(torch.from_numpy(image)).numpy(), want)
    g = rng.integers(0, 256, (20, 30)).astype(np.uint8)
    assert np.array_equal(oracle.grey_of(cases.as_image(g)), g)


# ---------------------------------------------------------------- the masker's seat against the reference's own calls
def replay(frames, W, H, conservative, fused, device):
    """The recorded sequence through DynamicMasker with MotionFallback in its seat -> per frame (dynamic mask, a frame is stored)."""
    x0, y0, x1, y1 = conservative
    scripted = torch.zeros((H, W), dtype=torch.bool, device=device)
    scripted[y0:y1, x0:x1] = True
    early = lambda image, idx: dm._dilate(dm._dilate(scripted, 9), 9)      # _fallback_detection :644-647 around the scripted heuristic
    by_idx = {fr["frame_idx"]: fr for fr in frames}

    def detect(image, idx):
        fr = by_idx[idx]
        return (torch.from_numpy(fr["boxes"]), fr["labels"]) if fr["has_boxes"] else (None, [])

    fallback = of.MotionFallback(early=early, fused=fused)
    masker = dm.DynamicMasker(detect, fallback=fallback, fused=fused)
    out = []
    for fr in frames:
        image = torch.from_numpy(cases.image_of(fr["image"])).to(device)
        got = masker.detect_and_segment(image, fr["frame_idx"])
        out.append((got.dynamic_mask.cpu().numpy(), fallback._stored if fused else fallback.prev_frame is not None))
    return out


def test_motion_fallback_replays_the_reference_sequences():
    W, H, conservative, seqs = cases.golden()
    kinds = [fr["kind"] for frames in seqs for fr in frames]
    assert {"boxes", "early", "motion", "none"} <= set(kinds)
    assert any(a["kind"] == b["kind"] == "motion" for frames in seqs for a, b in zip(frames, frames[1:]))      # consecutive fallbacks
    for s, frames in enumerate(seqs):
        stored = False
        for f, (fr, (mask, has)) in enumerate(zip(frames, replay(frames, W, H, conservative, False, "cpu"))):
            stored = stored or fr["stored"]
            assert np.array_equal(mask, fr["dynamic"] == 1), (s, f, fr["kind"])
            assert has == stored, (s, f)
            assert (fr["kind"] == "none") == (not fr["has_boxes"] and fr["frame_idx"] >= 5 and not has)


def test_the_fallback_branch_never_advances_the_stored_frame_unless_asked():
    W, H, _, seqs = cases.golden()
    frames = seqs[0]
    images = [torch.from_numpy(cases.image_of(fr["image"])) for fr in frames]
    plain, advancing = of.MotionFallback(fused=False), of.MotionFallback(fused=False, advance_on_fallback=True)
    for fb in (plain, advancing):
        assert fb(images[0], 7) is None      # nothing stored
    assert plain.prev_frame is None and np.array_equal(advancing.prev_frame.numpy(), oracle.grey_of(images[0].numpy()))
    plain.observe(images[0])
    a1, a2 = plain(images[1], 8), plain(images[2], 9)
    b1, b2 = advancing(images[1], 8), advancing(images[2], 9)
    assert np.array_equal(plain.prev_frame.numpy(), oracle.grey_of(images[0].numpy()))
    assert np.array_equal(advancing.prev_frame.numpy(), oracle.grey_of(images[2].numpy()))
    assert torch.equal(a1, b1) and not torch.equal(a2, b2)
    assert plain(images[1], 3) is None and plain(images[1], None) is not None      # early frames go to the (empty) early seat
    assert of.MotionFallback(fused=False, early=lambda image, idx: "early")(images[1], 4) == "early"


def test_existing_seats_behave_as_before():
    calls = []
    detect = lambda image, idx: (torch.tensor([[2.0, 2.0, 20.0, 20.0]]), ["person"]) if idx != 2 else (None, [])
    image = torch.zeros((3, 32, 48))
    for fallback in (None, lambda image, idx: calls.append(idx)):
        masker = dm.DynamicMasker(detect, fallback=fallback, fused=False)
        sums = [int(masker.detect_and_segment(image, idx).dynamic_mask.sum()) for idx in range(4)]
        assert sums == [324, 324, 0, 324]
    assert calls == [2]


# ---------------------------------------------------------------- refusals: before any launch, so without a GPU
GOOD = dict(pyr_scale=0.5, levels=3, winsize=15, iterations=3, poly_n=5, poly_sigma=1.2)
FAKE = 256      # a pointer that is never dereferenced: every call below is refused


def flow_args(W=64, H=48, scratch_bytes=None, **changed):
    L = _lib.lib()
    pointers = {k: changed.pop(k, FAKE) for k in ("prev", "next", "flow", "scratch")}
    nbytes = L.lvdgs_farneback_scratch_bytes(W, H) if scratch_bytes is None else scratch_bytes
    return _lib.FarnebackArgs(width=W, height=H, params=_lib.FarnebackParams(**dict(GOOD, **changed)), scratch_bytes=nbytes, **pointers)


def mask_args(W=64, H=48, mode=_lib.MOTION_MASK, dilate_kernel=7, state_bytes=None, scratch_bytes=None, **changed):
    L = _lib.lib()
    pointers = {k: changed.pop(k, FAKE) for k in ("image", "mask", "info", "state", "scratch")}
    return _lib.MotionMaskArgs(width=W, height=H, mode=mode, dilate_kernel=dilate_kernel, params=_lib.FarnebackParams(**dict(GOOD, **changed)),
                               motion_threshold=3.0, state_bytes=L.lvdgs_motion_mask_state_bytes(W, H) if state_bytes is None else state_bytes,
                               scratch_bytes=L.lvdgs_motion_mask_scratch_bytes(W, H) if scratch_bytes is None else scratch_bytes, **pointers)


RANGE = [dict(W=0), dict(H=0), dict(W=16385), dict(H=16385), dict(pyr_scale=0.0), dict(pyr_scale=1.0), dict(pyr_scale=math.nan), dict(levels=-1),
         dict(levels=9), dict(iterations=0), dict(iterations=11), dict(poly_sigma=0.0), dict(poly_sigma=math.nan), dict(poly_sigma=math.inf),
         dict(W=16384, H=16384, levels=8)]      # the last: level 8 would blur with 639 taps
INVALID = [dict(winsize=14), dict(winsize=1), dict(winsize=33), dict(poly_n=6), dict(poly_n=3)]


def test_every_refusal_of_the_flow():
    L = _lib.lib()
    call = lambda a: L.lvdgs_farneback_flow(C.byref(a), None)
    assert L.lvdgs_farneback_flow(None, None) == _lib.E_INVALID and b"NULL" in L.lvdgs_last_error()
    for kw in RANGE:
        assert call(flow_args(scratch_bytes=1 << 40, **kw)) == _lib.E_RANGE, kw
    for kw in INVALID:
        assert call(flow_args(**kw)) == _lib.E_INVALID, kw
    for name in ("prev", "next", "flow", "scratch"):
        assert call(flow_args(**{name: None})) == _lib.E_INVALID and b"NULL" in L.lvdgs_last_error(), name
    assert call(flow_args(scratch_bytes=L.lvdgs_farneback_scratch_bytes(64, 48) - 1)) == _lib.E_INVALID and b"too small" in L.lvdgs_last_error()
    assert b"639 taps" in (call(flow_args(scratch_bytes=1 << 40, **RANGE[-1])), L.lvdgs_last_error())[1]
    for W, H in ((0, 5), (5, 0), (16385, 5), (5, 16385), (-1, -1)):
        assert L.lvdgs_farneback_scratch_bytes(W, H) == 0 and L.lvdgs_motion_mask_scratch_bytes(W, H) == 0 and L.lvdgs_motion_mask_state_bytes(W, H) == 0
    assert L.lvdgs_farneback_scratch_bytes(1226, 370) % 256 == 0 and L.lvdgs_farneback_scratch_bytes(1226, 370) >= 24 * 4 * 1226 * 370
    assert L.lvdgs_motion_mask_scratch_bytes(1226, 370) > L.lvdgs_farneback_scratch_bytes(1226, 370)
    assert L.lvdgs_motion_mask_state_bytes(1226, 370) >= 1226 * 370


def test_every_refusal_of_the_motion_mask():
    L = _lib.lib()
    call = lambda a: L.lvdgs_motion_mask(C.byref(a), None)
    assert L.lvdgs_motion_mask(None, None) == _lib.E_INVALID and b"NULL" in L.lvdgs_last_error()
    for kw in RANGE:
        assert call(mask_args(state_bytes=1 << 40, scratch_bytes=1 << 40, **kw)) == _lib.E_RANGE, kw
    for kw in INVALID:
        assert call(mask_args(**kw)) == _lib.E_INVALID, kw
    for mode in (0, _lib.MOTION_OBSERVE | _lib.MOTION_MASK, _lib.MOTION_ADVANCE, _lib.MOTION_OBSERVE | _lib.MOTION_ADVANCE, 7, 8):
        assert call(mask_args(mode=mode)) == _lib.E_INVALID and b"mode" in L.lvdgs_last_error(), mode
    for k in (0, 2, 17, -3):
        assert call(mask_args(dilate_kernel=k)) == _lib.E_INVALID and b"dilate_kernel" in L.lvdgs_last_error(), k
    for mode in (_lib.MOTION_MASK, _lib.MOTION_MASK | _lib.MOTION_ADVANCE, _lib.MOTION_OBSERVE):
        for name in ("image", "state"):
            assert call(mask_args(mode=mode, **{name: None})) == _lib.E_INVALID and b"NULL" in L.lvdgs_last_error(), (mode, name)
        assert call(mask_args(mode=mode, state_bytes=L.lvdgs_motion_mask_state_bytes(64, 48) - 1)) == _lib.E_INVALID and b"state too small" in L.lvdgs_last_error()
    for name in ("mask", "info", "scratch"):
        assert call(mask_args(**{name: None})) == _lib.E_INVALID and b"NULL" in L.lvdgs_last_error(), name
    assert call(mask_args(scratch_bytes=L.lvdgs_motion_mask_scratch_bytes(64, 48) - 1)) == _lib.E_INVALID and b"scratch too small" in L.lvdgs_last_error()


def test_the_python_layer_refuses_what_it_cannot_pass_on():
    with pytest.raises(TypeError):
        of.farneback_torch(torch.zeros((8, 8), dtype=torch.uint8), torch.zeros((8, 8), dtype=torch.uint8), flags=0)
    with pytest.raises(TypeError):
        of.MotionFallback(window=3)
    with pytest.raises(ValueError):
        of.MotionFallback(dilate_kernel=4)
    with pytest.raises(_lib.LvdgsError):
        of.farneback(torch.zeros((8, 8), dtype=torch.uint8), torch.zeros((8, 8), dtype=torch.uint8))      # CPU tensors: there is no CPU path
    with pytest.raises(_lib.LvdgsError):
        of.MotionFallback()(torch.zeros((3, 8, 8)), 9)
    assert set(_lib.MOTION_INFO) == {"has_prev", "levels", "moving_pixels", "mask_pixels"} and len(_lib.MOTION_INFO) <= _lib.MOTION_INFO_WORDS


def test_reset_clears_the_stored_frame_too():
    fallback = of.MotionFallback(fused=False)
    masker = dm.DynamicMasker(lambda image, idx: (torch.tensor([[2.0, 2.0, 20.0, 20.0]]), ["person"]), fallback=fallback, fused=False)
    image = torch.zeros((3, 32, 48))
    masker.detect_and_segment(image, 0)
    assert fallback.prev_frame is None      # a first frame is not shown to the seat
    masker.detect_and_segment(image, 1)
    assert fallback.prev_frame is not None
    masker.reset()
    assert fallback.prev_frame is None and not masker.first_frame_processed
