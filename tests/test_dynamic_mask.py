"""The dynamic-mask assembly without a GPU: the NumPy oracle (tests/dynamic_mask_oracle.py) against what the reference's own
detect_and_segment / _temporal_consistency / _expand_dynamic_mask produced (tests/golden/dynamic_mask.npz), the PyTorch chain of
lvdgs.dynamic_mask.DynamicMasker(fused=False) against the oracle, the C ABI (every refusal), and a toy drive of
SlamSequence(dynamic_masks="detections") on the CPU harness.  Every comparison is exact."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

import dynamic_mask_cases as cases
import dynamic_mask_oracle as oracle

INFO = {k: i for i, k in enumerate(oracle.INFO)}


def replay_oracle(frames, W, H):
    """The oracle's ``Masker`` over a recorded sequence -> per frame (its output with the keyframe's expansion, the history after)."""
    m = oracle.Masker()
    out = []
    for fr in frames:
        image = np.ones((3, H, W), np.float32)
        got = m.frame(W, H, fr["frame_idx"], fr["boxes"], fr["labels"], fr["sam"], expand_kernel=fr["expand_kernel"], image=image)
        out.append((got, [h.copy() for h in m.history]))
    return out


def test_oracle_equals_the_reference_on_every_recorded_frame():
    W, H, seqs = cases.golden()
    assert len(seqs) == 4 and all(len(s) == 8 for s in seqs)
    lengths = set()
    for s, frames in enumerate(seqs):
        for f, (fr, (got, hist)) in enumerate(zip(frames, replay_oracle(frames, W, H))):
            what = (s, f)
            assert np.array_equal(got["dynamic"], fr["dynamic"]), what
            assert np.array_equal(got["static"], 1 - fr["dynamic"]), what
            assert np.array_equal(got["expanded_dynamic"], fr["expanded"]), what
            info = got["info"]
            assert info[INFO["filtered"]] == fr["filtered"] and info[INFO["history"]] == fr["history"] == len(hist), what
            # the reference dilates when a vehicle was detected and the mask is not empty
            assert bool(info[INFO["vehicle_detected"]] and info[INFO["dynamic_pixels"]] > 0) == bool(fr["dilated"]), what
            assert info[INFO["use_sam_result"]] == int(fr["sam"].any()), what
            lengths.add((fr["history"], fr["filtered"]))
    # the recorded cases the kernel's paths need: a first frame by the index and one by the flag, SAM and box frames, an empty SAM
    # union, non-vehicle-only frames, dropped boxes, histories of every length and the drop of the oldest entry
    assert {(n, 1) for n in (1, 2, 3, 4, 5)} <= lengths
    assert seqs[2][0]["frame_idx"] == 3 and seqs[2][0]["first"] == 1 and seqs[0][0]["first"] == 1 and seqs[0][1]["first"] == 0
    assert any(len(fr["sam"]) and not fr["sam"].any() for fr in seqs[1]) and any(not fr["dilated"] for fr in seqs[1])
    assert [fr["history"] for fr in seqs[0]][-3:] == [5, 5, 5]


@pytest.mark.parametrize("k", [5, 7, 9])
def test_oracle_dilation_is_the_maximum_filter(k):
    import scipy.ndimage
    rng = np.random.default_rng(k)
    for W, H, p in ((1, 1, 0.5), (3, 17, 0.2), (40, 23, 0.02), (65, 9, 0.05), (12, 12, 0.0)):
        m = (rng.random((H, W)) < p).astype(np.uint8)
        want = scipy.ndimage.maximum_filter(m, size=(k, k), mode="constant", cval=0)
        assert np.array_equal(oracle.dilate(m, k), want), (W, H)


def test_box_widening_truncation_identity():
    """int(w * 0.1) == w // 10 and int(w * 0.15) == 3 * w // 20 for every extent the clamps allow (the float64 product is the definition)."""
    w = np.arange(0, 4097, dtype=np.int64)
    assert np.array_equal((w.astype(np.float64) * 0.1).astype(np.int64), w // 10)
    assert np.array_equal((w.astype(np.float64) * 0.15).astype(np.int64), 3 * w // 20)
    assert all(int(int(v) * 0.1) == v // 10 and int(int(v) * 0.15) == 3 * v // 20 for v in w[::7])


def test_majority_is_the_median_of_the_history():
    """More than n / 2 of n entries == np.median(...).astype(uint8) for n = 3, 4, 5; an even n with a tie gives 0."""
    rng = np.random.default_rng(0)
    for n in (3, 4, 5):
        stack = (rng.random((n, 6, 50)) < 0.5).astype(np.uint8)
        assert np.array_equal((2 * stack.sum(0) > n).astype(np.uint8), np.median(stack, axis=0).astype(np.uint8))


def to_torch(fr, device="cpu"):
    return torch.from_numpy(fr["boxes"]).to(device), torch.from_numpy(np.ascontiguousarray(fr["sam"])).to(device)


def check_masks(got, want, what):
    """A ``DynamicMasks`` against the oracle's dict: every mask it holds, the depth, the named info words."""
    pairs = (("dynamic_mask", "dynamic"), ("static_mask", "static"), ("expanded_dynamic_mask", "expanded_dynamic"),
             ("expanded_static_mask", "expanded_static"), ("valid_rgb", "valid_rgb"), ("depth", "depth"))
    for name, key in pairs:
        t = getattr(got, name)
        if want[key] is None:
            assert t is None, (what, name)
        elif t is not None:
            a = t.cpu().numpy()
            assert a.dtype == (np.float32 if name == "depth" else np.bool_), (what, name)
            assert np.array_equal(a.view(np.uint8) if name != "depth" else a.view(np.uint32),
                                  want[key] if name != "depth" else want[key].view(np.uint32)), (what, name)
    assert got.info.cpu().tolist()[:len(oracle.INFO)] == want["info"], (what, got.info.cpu().tolist(), want["info"])
    assert got.info.cpu().tolist()[len(oracle.INFO):] == [0] * (16 - len(oracle.INFO)), what


def test_torch_chain_equals_the_oracle_on_the_recorded_sequences():
    from lvdgs.dynamic_mask import DynamicMasker
    W, H, seqs = cases.golden()
    for s, frames in enumerate(seqs):
        cur = {}
        masker = DynamicMasker(lambda image, idx: (cur["boxes"], cur["labels"]), lambda image, boxes: cur["sam"], fused=False)
        image = torch.ones(3, H, W)
        for f, (fr, (want, hist)) in enumerate(zip(frames, replay_oracle(frames, W, H))):
            cur["boxes"], cur["sam"] = to_torch(fr)
            cur["labels"] = fr["labels"]
            got = masker.detect_and_segment(image, fr["frame_idx"], expand_kernel=fr["expand_kernel"])
            check_masks(got, want, (s, f))
            assert len(masker.mask_history) == len(hist) and all(np.array_equal(a.numpy(), b) for a, b in zip(masker.mask_history, hist)), (s, f)


@pytest.mark.parametrize("box_format", ["xyxy", "cxcywh"])
def test_torch_chain_equals_the_oracle_on_random_frames(box_format):
    """Random frames through one masker and one oracle state: box and SAM frames mixed, a frame without boxes (the fallback branch:
    mask as it is, history untouched), a reset in the middle."""
    from lvdgs.dynamic_mask import DynamicMasker
    W, H = 67, 21
    cur = {}
    fallback = torch.zeros(H, W, dtype=torch.bool)
    fallback[3:9, 60:] = True
    masker = DynamicMasker(lambda image, idx: (cur["boxes"], cur["labels"]), lambda image, boxes: cur["sam"], lambda image, idx: cur["fallback"],
                           fused=False, box_format=box_format, history_length=4)
    ref = oracle.Masker(history_length=4)
    plan = [(6, 0), (5, 0), (0, 0), (4, 2), (7, 0), (3, 0), (0, 0), (9, 0), (2, 1), (8, 0), (300, 0), (1, 0)]
    for n, (nb, ns) in enumerate(plan):
        if n == 7:
            masker.reset()
            ref.reset()
        c = cases.random_frame(n, W, H, nb, ns, box_format, empty_sam=n == 8)
        cur.update(boxes=torch.from_numpy(c["boxes"]), labels=c["labels"], sam=torch.from_numpy(c["sam"]), fallback=fallback if n == 2 else None)
        k = (9, 7, 0, 15)[n % 4]
        frame_idx = n + 1 if n != 7 else 0
        got = masker.detect_and_segment(torch.from_numpy(c["image"]), frame_idx, expand_kernel=k, rgb_boundary_threshold=0.3,
                                        depth=torch.from_numpy(c["depth"]))
        want = ref.frame(W, H, frame_idx, c["boxes"], c["labels"], c["sam"], fallback=None if n != 2 else fallback.numpy(), box_format=box_format,
                         expand_kernel=k, image=c["image"], threshold=0.3, depth=c["depth"])
        check_masks(got, want, (box_format, n))
        assert masker.first_frame_processed and len(masker.mask_history) == len(ref.history)
    assert len(ref.history) >= 3      # the majority ran


def test_info_names_are_the_oracle_s():
    from lvdgs import _lib
    assert _lib.DYNAMIC_MASK_INFO == oracle.INFO


def test_every_refusal_without_a_gpu():
    """Each is refused before any launch (the pointers are never dereferenced), with its message."""
    from lvdgs import _lib
    L = _lib.lib()
    p = 4096      # a non-NULL address nobody reads

    def good():
        return _lib.DynamicMaskArgs(width=96, height=70, first_frame=0, box_format=0, num_boxes=2, boxes=p, vehicle=p, num_sam_masks=1,
                                    sam_masks=p, history_length=5, vehicle_kernel_first=7, vehicle_kernel=5, expand_kernel=9, image=p,
                                    rgb_boundary_threshold=0.01, depth_in=p, depth_out=p, static_mask=p, dynamic_mask=p, expanded_dynamic=p,
                                    expanded_static=p, valid_rgb=p, info=p, state=p, state_bytes=L.lvdgs_dynamic_mask_state_bytes(96, 70, 5),
                                    scratch=p, scratch_bytes=L.lvdgs_dynamic_mask_scratch_bytes(96, 70))

    def refused(status, message, **change):
        a = good()
        for k, v in change.items():
            setattr(a, k, v)
        assert L.lvdgs_dynamic_mask(C.byref(a), None) == status, change
        assert message in L.lvdgs_last_error(), (change, L.lvdgs_last_error())

    assert L.lvdgs_dynamic_mask(None, None) == _lib.E_INVALID and b"args is NULL" in L.lvdgs_last_error()
    for name in ("state", "scratch", "info"):
        refused(_lib.E_INVALID, b"state / scratch / info is NULL", **{name: None})
    refused(_lib.E_INVALID, b"boxes is NULL", boxes=None)
    refused(_lib.E_INVALID, b"sam_masks is NULL", sam_masks=None)
    refused(_lib.E_INVALID, b"image is NULL", image=None)
    refused(_lib.E_INVALID, b"depth_out without depth_in", depth_in=None)
    refused(_lib.E_INVALID, b"box_format 2", box_format=2)
    refused(_lib.E_INVALID, b"box_format -1", box_format=-1)
    for change in (dict(vehicle_kernel=4), dict(vehicle_kernel_first=17), dict(vehicle_kernel=0), dict(vehicle_kernel_first=-3)):
        refused(_lib.E_INVALID, b"vehicle kernels", **change)
    for k in (8, 17, -1):
        refused(_lib.E_INVALID, b"expand_kernel", expand_kernel=k)
    refused(_lib.E_INVALID, b"state too small", state_bytes=L.lvdgs_dynamic_mask_state_bytes(96, 70, 5) - 1)
    refused(_lib.E_INVALID, b"state too small", history_length=6)
    refused(_lib.E_INVALID, b"scratch too small", scratch_bytes=L.lvdgs_dynamic_mask_scratch_bytes(96, 70) - 1)
    refused(_lib.E_RANGE, b"image size", width=0)
    refused(_lib.E_RANGE, b"image size", height=-2)
    refused(_lib.E_RANGE, b"image size", width=65536, height=32768)      # 2^31 pixels
    refused(_lib.E_RANGE, b"negative", num_boxes=-1)
    refused(_lib.E_RANGE, b"negative", num_sam_masks=-1)
    refused(_lib.E_RANGE, b"history_length 0", history_length=0)
    refused(_lib.E_RANGE, b"history_length 9", history_length=9)
    # the size queries: 0 for what the call refuses, else the header + the ring's bit planes / two bit planes
    assert L.lvdgs_dynamic_mask_state_bytes(0, 70, 5) == L.lvdgs_dynamic_mask_state_bytes(96, 70, 9) == L.lvdgs_dynamic_mask_scratch_bytes(96, 0) == 0
    assert L.lvdgs_dynamic_mask_state_bytes(65, 3, 2) == 256 + 256 and L.lvdgs_dynamic_mask_scratch_bytes(65, 3) == 2 * 256
    assert L.lvdgs_dynamic_mask_state_bytes(1226, 370, 5) >= 256 + 5 * 370 * 20 * 8


def test_masker_and_sequence_argument_checks():
    from lvdgs import _lib
    from lvdgs.dynamic_mask import DynamicMasker
    from lvdgs.slam_sequence import SlamSequence
    with pytest.raises(ValueError):
        DynamicMasker(None, box_format="xywh")
    with pytest.raises(ValueError):
        DynamicMasker(None, history_length=9)
    with pytest.raises(_lib.LvdgsError):      # no quiet fall-back to PyTorch: the fused path needs the GPU
        DynamicMasker(lambda image, idx: (torch.zeros(1, 4), ["car"])).detect_and_segment(torch.zeros(3, 4, 4), 0)
    with pytest.raises(TypeError):
        SlamSequence(None, None, None, None, None, dynamic_masks="detections")
    with pytest.raises(ValueError):
        SlamSequence(None, None, None, None, None, dynamic_masks="bogus")


def test_rectangle_detector_returns_the_datasets_rectangles():
    from lvdgs import synthetic
    H, W = 48, 64
    for seed in (3, 304, 1207):
        rects = synthetic.dynamic_object_rectangles(H, W, seed)
        m = torch.ones(H, W, dtype=torch.bool)
        for x0, y0, w, h in rects:
            m[y0:y0 + h, x0:x0 + w] = False
        assert 2 <= len(rects) <= 4 and torch.equal(m, synthetic.dynamic_object_mask(H, W, seed))


def test_toy_drive_with_detections_on_the_cpu_harness():
    """SlamSequence(dynamic_masks="detections") with the PyTorch chain behind the masker runs to the end; every keyframe carries the
    masks the oracle makes of the stand-in detector's output, call by call (a tracked frame is one call, a keyframe one more)."""
    import sequence_scene as ss
    from lvdgs import simple_knn, synthetic
    from lvdgs.dynamic_mask import DynamicMasker
    from lvdgs.slam_sequence import SlamSequence
    torch.manual_seed(0)
    random.seed(0)
    cfg, ds, hooks, knn, _ = ss.toy_sequence_on_cpu(dynamic_objects=True, n_frames=4)
    cfg["Training"]["kf_overlap"] = 1.01      # every frame kf_interval after the last keyframe becomes one: frames 0 and 2
    det = synthetic.RectangleDetector(ds)
    masker = DynamicMasker(det.detect, det.segment, fused=False)
    real_knn, simple_knn.distCUDA2 = simple_knn.distCUDA2, knn
    try:
        seq = SlamSequence(cfg, ds, ss.empty_map(cfg, "cpu"), ss.PIPE, torch.zeros(3), dynamic_masks="detections", masker=masker, **hooks).run()
    finally:
        simple_knn.distCUDA2 = real_knn
    assert seq.counts["frames"] == len(ds) and len(seq.kf_indices) >= 2 and seq.kf_indices[0] == 0
    W, H, thr = ds.width, ds.height, cfg["Training"]["rgb_boundary_threshold"]
    ref = oracle.Masker()
    for idx in range(len(ds)):
        boxes, labels = det.detect(ds[idx][0], idx)
        sam = det.segment(ds[idx][0], boxes).numpy()
        image = ds[idx][0].numpy()
        want = None
        if idx > 0:
            want = ref.frame(W, H, idx, boxes.numpy(), labels, sam)
        if idx in seq.kf_indices:
            want = ref.frame(W, H, idx, boxes.numpy(), labels, sam, expand_kernel=9 if idx == 0 else 7, image=image, threshold=thr)
            vp = seq.cameras[idx]
            assert np.array_equal(vp.static_mask.numpy(), want["static"] == 1) and np.array_equal(vp.dynamic_mask.numpy(), want["dynamic"] == 1), idx
            assert np.array_equal(vp.expanded_dynamic_mask.numpy(), want["expanded_dynamic"] == 1), idx
            assert np.array_equal(vp.expanded_static_mask.numpy(), want["expanded_static"] == 1), idx
            assert 0 < want["info"][INFO["dynamic_pixels"]] < want["info"][INFO["expanded_pixels"]] < W * H, idx
    assert masker.last.info.tolist()[:len(oracle.INFO)] == want["info"]
