"""lvdgs_farneback_flow and lvdgs_motion_mask on the GPU (lvdgs.optical_flow) against the float64 NumPy statement of the header's text
(tests/optical_flow_oracle.py) on the scenes of tests/optical_flow_cases.py.

The flow's tolerance is computed here, per case, from the oracle alone: 16 x the largest difference between the oracle run in
float32 and in float64 (3e-6 .. 1e-5 px on these scenes) -- the margin is there because the device may order a sum differently; it is
not taken from the device code.  Masks, counts, state and repeatability are compared exactly."""
import functools

import numpy as np
import pytest
import torch

import optical_flow_cases as cases
import optical_flow_oracle as oracle

pytestmark = pytest.mark.gpu
DEV = "cuda"
THRESHOLD, NEAR = 3.0, 1e-3
MASK_SIZES = ((130, 70), (261, 259))
VARIANTS = {      # beyond the reference's parameters: the update kernel's short tiles (winsize > 23), the wider expansion, other scales
    "wide": dict(winsize=31, poly_n=7, iterations=2),
    "narrow": dict(winsize=3, iterations=1, pyr_scale=0.7, levels=2),
    "flat": dict(levels=0, poly_sigma=1.5),
}


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def scene(kind, W, H):
    if kind == "a":
        return cases.whole_shift(W, H) + (None,)
    return cases.moving_rectangle(W, H)


@functools.lru_cache(maxsize=None)
def reference(kind, W, H, variant=None):
    """-> (the float64 flow, the tolerance, the levels)."""
    f1, f2, _ = scene(kind, W, H)
    params = VARIANTS[variant] if variant else {}
    f64, levels = oracle.farneback(f1, f2, np.float64, return_levels=True, **params)
    f32 = oracle.farneback(f1, f2, np.float32, **params)
    for a in (f64, f32):
        a.setflags(write=False)
    return f64, 16.0 * float(np.abs(f32.astype(np.float64) - f64).max()), levels


def check_flow(kind, W, H, variant=None):
    from lvdgs import optical_flow as of
    f1, f2, _ = scene(kind, W, H)
    want, tol, _ = reference(kind, W, H, variant)
    got = of.farneback(up(f1), up(f2), **(VARIANTS[variant] if variant else {})).cpu().numpy()
    assert got.shape == want.shape and got.dtype == np.float32 and np.isfinite(got).all()
    err = float(np.abs(got.astype(np.float64) - want).max())
    print(f"flow {kind} {W}x{H} {variant}: max |device - float64 oracle| = {err:.3e} px, tolerance {tol:.3e} px")
    assert err <= tol, (kind, W, H, variant, err, tol)


@pytest.mark.parametrize("W,H", cases.SIZES)
@pytest.mark.parametrize("kind", ["a", "b"])
def test_flow_matches_the_float64_oracle(kind, W, H):
    check_flow(kind, W, H)


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_flow_with_other_parameters(variant):
    check_flow("a", 130, 70, variant)


def test_whole_frame_shift_is_recovered_with_its_sign():
    from lvdgs import optical_flow as of
    f1, f2, _ = scene("a", 261, 259)
    flow = of.farneback(up(f1), up(f2)).cpu().numpy()
    epe = np.sqrt(((flow - np.array(cases.SHIFT_A, np.float32)) ** 2).sum(-1))
    assert np.median(epe) < 0.05 and np.sign(np.median(flow[..., 0])) == 1 and np.sign(np.median(flow[..., 1])) == -1


@functools.lru_cache(maxsize=None)
def mask_reference(W, H):
    f1, f2, inside = scene("b", W, H)
    moving, mask, magnitude, _ = oracle.motion_mask(f1, f2, THRESHOLD, 7)
    return moving, mask, magnitude, inside


def run_mask(W, H, *, mode=None, state=None, observe=True, want_flow=True, dilate_kernel=7):
    """OBSERVE of scene (b)'s first frame into a fresh state (or the given one), then one MASK call on its second."""
    from lvdgs import _lib
    from lvdgs import optical_flow as of
    f1, f2, _ = scene("b", W, H)
    state = of.MotionState(W, H, DEV) if state is None else state
    if observe:
        assert of.motion_mask(up(cases.as_image(f1)), state, _lib.MOTION_OBSERVE) is None
    mask, info, flow = of.motion_mask(up(cases.as_image(f2)), state, mode, motion_threshold=THRESHOLD, dilate_kernel=dilate_kernel, want_flow=want_flow)
    return state, mask, info, flow


@pytest.mark.parametrize("W,H", MASK_SIZES)
def test_motion_mask_matches_the_oracle(W, H):
    from lvdgs import _lib
    moving, mask, magnitude, inside = mask_reference(W, H)
    _, got, info, flow = run_mask(W, H)
    got, info, flow = got.cpu().numpy(), info.cpu().numpy(), flow.cpu().numpy()
    want_flow, tol, levels = reference("b", W, H)
    assert float(np.abs(flow.astype(np.float64) - want_flow).max()) <= tol      # the grey plane went through the image and back
    near = np.abs(magnitude - THRESHOLD) < NEAR
    print(f"mask {W}x{H}: {100 * near.mean():.4f} % of the pixels within {NEAR} of the threshold")
    assert near.mean() <= 0.005
    got_moving = np.sqrt(flow[..., 0] * flow[..., 0] + flow[..., 1] * flow[..., 1]) > np.float32(THRESHOLD)      # float32, as written
    assert np.array_equal(got_moving[~near], moving[~near])
    assert np.array_equal(got, oracle.dilate(got_moving, 7))      # the device's threshold and dilation on its own flow: exact
    if np.array_equal(got_moving, moving):
        assert np.array_equal(got, mask)
    cover = got[inside].mean()
    print(f"mask {W}x{H}: covers {100 * cover:.1f} % of the moved rectangle")
    assert cover >= 0.95
    named = dict(zip(_lib.MOTION_INFO, info.tolist()))
    assert named == dict(has_prev=1, levels=levels, moving_pixels=int(got_moving.sum()), mask_pixels=int(got.sum())) and not info[4:].any()


def test_equal_inputs_and_state_give_equal_bytes():
    a, b = run_mask(130, 70), run_mask(130, 70)
    for x, y in zip(a[1:], b[1:]):
        assert torch.equal(x, y)
    assert torch.equal(a[0].block, b[0].block)


def test_mask_leaves_the_state_advance_and_observe_change_it():
    from lvdgs import _lib
    W, H = 130, 70
    f1, f2, _ = scene("b", W, H)
    state, mask, _, _ = run_mask(W, H)
    before = state.block.clone()
    assert np.array_equal(state.stored(), f1)
    _, again, _, _ = run_mask(W, H, state=state, observe=False)
    assert torch.equal(state.block, before) and torch.equal(again, mask)
    _, advanced, info, _ = run_mask(W, H, state=state, observe=False, mode=_lib.MOTION_MASK | _lib.MOTION_ADVANCE, want_flow=False)
    assert torch.equal(advanced, mask) and np.array_equal(state.stored(), f2)
    _, still, info, _ = run_mask(W, H, state=state, observe=False)      # the second frame against itself: nothing moves
    assert not still.any() and info.cpu().tolist()[:4] == [1, 2, 0, 0]
    run_mask(W, H, state=state)                                         # OBSERVE puts the first frame back
    assert np.array_equal(state.stored(), f1)


def test_a_zeroed_state_or_one_of_another_size_gives_an_empty_mask():
    from lvdgs import optical_flow as of
    W, H = 130, 70
    state, mask, info, _ = run_mask(W, H, observe=False)
    assert not mask.any() and info.cpu().tolist() == [0, 2, 0, 0, 0, 0, 0, 0] and state.stored() is None
    assert not state.block.any()
    state, _, _, _ = run_mask(W, H)
    state.block[:4] = torch.tensor(list(np.array([W + 1], np.int32).tobytes()), dtype=torch.uint8, device=DEV)      # a header of 131 x 70
    _, mask, info, _ = run_mask(W, H, state=state, observe=False)
    assert not mask.any() and info.cpu().tolist()[:4] == [0, 2, 0, 0]
    assert isinstance(state, of.MotionState)


def test_dilation_kernels_and_widths_around_the_word():
    """The threshold's ballots and the dilation at widths that are no multiple of 64, kernels 1 and 15."""
    for (W, H), k in (((64, 48), 1), ((130, 70), 15), ((261, 259), 3)):
        _, got, _, flow = run_mask(W, H, dilate_kernel=k)
        flow = flow.cpu().numpy()
        moving = np.sqrt(flow[..., 0] * flow[..., 0] + flow[..., 1] * flow[..., 1]) > np.float32(THRESHOLD)
        assert np.array_equal(got.cpu().numpy(), oracle.dilate(moving, k)), (W, H, k)


def scripted_sequence(W, H, n=9):
    """Frames of scene (b)'s kind with the rectangle moving on, and which of them have boxes."""
    bg, fg = cases.texture(5), cases.texture(6)
    x, y = cases.grid(W, H)
    x0, y0, x1, y1 = cases.rectangle_of(W, H)
    frames = []
    for i in range(n):
        sx, sy = 4.0 * i, 1.5 * i
        inside = (x - sx >= x0) & (x - sx < x1) & (y - sy >= y0) & (y - sy < y1)
        frames.append(cases.as_image(cases.to_bytes(np.where(inside, fg(x - sx, y - sy), bg(x - 0.25 * i, y)))))
    boxes = {0: True, 1: True, 3: True, 6: True}      # frames 2, 4, 5, 7, 8 fall back: 2 and 4 early, 5 and 7, 8 by motion
    return frames, boxes


def test_the_masker_with_the_fused_fallback_equals_the_pytorch_statements():
    from lvdgs import dynamic_mask as dm
    from lvdgs import optical_flow as of
    W, H = 130, 70
    frames, boxes = scripted_sequence(W, H)
    box = torch.tensor([[10.0, 12.0, 40.0, 50.0]])

    def masker(fused, **kw):
        detect = lambda image, idx: (box.to(image.device), ["person"]) if boxes.get(idx) else (None, [])
        return dm.DynamicMasker(detect, fallback=of.MotionFallback(fused=fused, **kw), fused=fused)

    for kw in ({}, dict(advance_on_fallback=True)):
        a, b = masker(True, **kw), masker(False, **kw)
        moved = 0
        for idx, frame in enumerate(frames):
            image = up(frame)
            got, want = a.detect_and_segment(image, idx), b.detect_and_segment(image, idx)
            assert torch.equal(got.dynamic_mask, want.dynamic_mask), (kw, idx)
            if not boxes.get(idx) and idx >= 5:
                moved += int(got.dynamic_mask.sum())
        assert moved > 0


def test_the_fused_masker_replays_the_reference_sequences():
    """tests/golden/motion_fallback.npz -- the reference's own detect_and_segment with its fallback -- through the fused masker with the
    fused fallback in its seat: the masks of every frame, boxes or not."""
    from test_optical_flow import replay
    W, H, conservative, seqs = cases.golden()
    for s, frames in enumerate(seqs):
        for f, (fr, (mask, _)) in enumerate(zip(frames, replay(frames, W, H, conservative, True, DEV))):
            assert np.array_equal(mask, fr["dynamic"] == 1), (s, f, fr["kind"])
