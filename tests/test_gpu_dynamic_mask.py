"""lvdgs_dynamic_mask on the GPU (lvdgs.dynamic_mask) against the NumPy oracle (tests/dynamic_mask_oracle.py), against the recorded
reference sequences (tests/golden/dynamic_mask.npz) and against the PyTorch statements it replaces on the same device tensors.
Every comparison is exact: output bytes, info words, the history's entries."""
import random

import numpy as np
import pytest
import torch

import dynamic_mask_cases as cases
import dynamic_mask_oracle as oracle
from test_dynamic_mask import check_masks, replay_oracle

pytestmark = pytest.mark.gpu
DEV = "cuda"
INFO = {k: i for i, k in enumerate(oracle.INFO)}


def up(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def call(W, H, history, ref_history, first, case, *, box_format="xyxy", expand_kernel=0, threshold=0.3, depth=True, outputs=None,
         vehicle_kernels=(7, 5)):
    """One library call on uploaded inputs and the oracle's call on the same; compared; -> (DynamicMasks, the oracle's dict)."""
    from lvdgs import dynamic_mask as dm
    vehicle = np.array([oracle.is_vehicle(s) for s in case["labels"]], np.uint8)
    got = dm.assemble(W, H, up(case["boxes"]), up(vehicle) if len(vehicle) else None, up(case["sam"]) if len(case["sam"]) else None,
                      first_frame=first, history=history, box_format=box_format, vehicle_kernels=vehicle_kernels, expand_kernel=expand_kernel,
                      image=up(case["image"]), rgb_boundary_threshold=threshold, depth=up(case["depth"]) if depth else None,
                      outputs=dm.OUTPUTS if outputs is None else outputs)
    want = oracle.assemble(W, H, first, case["boxes"], vehicle, case["sam"], ref_history, box_format=box_format,
                           history_length=history.history_length, vehicle_kernels=vehicle_kernels, expand_kernel=expand_kernel,
                           image=case["image"], threshold=threshold, depth=case["depth"] if depth else None)
    what = (W, H, first, box_format, expand_kernel, len(case["boxes"]), len(case["sam"]))
    check_masks(got, want, what)
    entries = history.entries()
    assert len(entries) == len(ref_history) and all(np.array_equal(a, b) for a, b in zip(entries, ref_history)), what
    return got, want


def test_recorded_sequences_replayed_with_one_persistent_state():
    from lvdgs import dynamic_mask as dm
    W, H, seqs = cases.golden()
    image = np.ones((3, H, W), np.float32)
    for s, frames in enumerate(seqs):
        history, ref_history = dm.MaskHistory(W, H, 5, DEV), []
        processed = False
        for f, (fr, (ref, _)) in enumerate(zip(frames, replay_oracle(frames, W, H))):
            first = fr["frame_idx"] == 0 or not processed
            processed = True
            assert first == bool(fr["first"])
            case = dict(boxes=fr["boxes"], labels=fr["labels"], sam=fr["sam"], image=image, depth=None)
            got, want = call(W, H, history, ref_history, first, case, expand_kernel=fr["expand_kernel"], depth=False)
            assert want["info"] == ref["info"], (s, f)
            # ... and the reference's own bytes
            assert np.array_equal(got.dynamic_mask.cpu().numpy(), fr["dynamic"] == 1), (s, f)
            assert np.array_equal(got.expanded_dynamic_mask.cpu().numpy(), fr["expanded"] == 1), (s, f)
            assert got.info_dict()["history"] == fr["history"] and got.info_dict()["filtered"] == fr["filtered"], (s, f)


@pytest.mark.parametrize("W", cases.SHAPE_WIDTHS)
def test_word_boundary_and_degenerate_shapes(W):
    """Widths around the 64-pixel word, heights down to one row; 0, 1 and 300 boxes, 0, 1 and 7 SAM masks, both box formats, a kernel
    wider than the image, every output omitted in turn, the history filling up to its majority."""
    from lvdgs import dynamic_mask as dm
    plan = [  # (boxes, SAM masks, empty SAM, format, first, expand kernel, depth)
        (300, 0, False, "xyxy", True, 15, True), (1, 0, False, "cxcywh", False, 9, False), (0, 0, False, "xyxy", False, 0, False),
        (5, 1, False, "xyxy", False, 7, True), (7, 7, True, "cxcywh", False, 5, True), (3, 0, False, "xyxy", False, 7, True),
        (300, 0, False, "cxcywh", False, 9, True), (4, 7, False, "xyxy", True, 0, False)]
    for H in cases.SHAPE_HEIGHTS:
        history, ref_history = dm.MaskHistory(W, H, 3, DEV), []
        for n, (nb, ns, empty, fmt, first, k, depth) in enumerate(plan):
            case = cases.random_frame(n, W, H, nb, ns, fmt, empty_sam=empty)
            outputs = tuple(o for j, o in enumerate(dm.OUTPUTS) if j != n % (len(dm.OUTPUTS) + 1))
            got, _ = call(W, H, history, ref_history, first, case, box_format=fmt, expand_kernel=k, depth=depth, outputs=outputs,
                          vehicle_kernels=(15, 5) if n == 0 else (7, 5))
            omitted = [o for o in dm.OUTPUTS if o not in outputs]
            assert all(getattr(got, o) is None for o in omitted)
        assert len(ref_history) == 3      # at least four appends into a ring of three: the oldest dropped, the majority taken


@pytest.mark.parametrize("W,H", [(1226, 370), (1920, 1280)])
def test_full_size_frame(W, H):
    from lvdgs import dynamic_mask as dm
    history, ref_history = dm.MaskHistory(W, H, 5, DEV), []
    for n, (nb, ns, first, k) in enumerate([(12, 0, True, 9), (9, 3, False, 7), (14, 0, False, 7)]):
        call(W, H, history, ref_history, first, cases.random_frame(n, W, H, nb, ns), expand_kernel=k)
    # a smaller frame after a larger one, on the scratch the larger one left
    w, h = 129, 37
    call(w, h, dm.MaskHistory(w, h, 5, DEV), [], True, cases.random_frame(3, w, h, 6, 0), expand_kernel=9)


def test_two_calls_on_equal_state_give_equal_bytes():
    from lvdgs import dynamic_mask as dm
    W, H = 200, 37
    history, ref_history = dm.MaskHistory(W, H, 5, DEV), []
    for n in range(3):
        call(W, H, history, ref_history, False, cases.random_frame(n, W, H, 6, 0))
    case = cases.random_frame(9, W, H, 8, 0)
    runs = []
    for _ in range(2):
        h = dm.MaskHistory(W, H, 5, DEV)
        h.block.copy_(history.block)
        got, _ = call(W, H, h, [a.copy() for a in ref_history], False, case, expand_kernel=7)
        runs.append([getattr(got, o).cpu().numpy() for o in dm.OUTPUTS] + [got.depth.cpu().numpy().view(np.uint32), got.info.cpu().numpy(),
                                                                         h.block.cpu().numpy()])
    assert all(np.array_equal(a, b) for a, b in zip(*runs))
    assert not np.array_equal(runs[0][-1], history.block.cpu().numpy())      # (the call did move the state on)


def scripted_maskers(cur, **kw):
    from lvdgs.dynamic_mask import DynamicMasker
    seats = (lambda image, idx: (cur["boxes"], cur["labels"]), lambda image, boxes: cur["sam"], lambda image, idx: cur["fallback"])
    return DynamicMasker(*seats, fused=True, **kw), DynamicMasker(*seats, fused=False, **kw)


def test_twelve_frames_with_a_reset_fused_equals_the_torch_chain_and_the_oracle():
    """SAM and box frames mixed, a frame without boxes (the fallback branch), ``reset()`` in the middle: the masker with the library
    behind it, the masker with the PyTorch chain on the same device tensors, and the oracle agree on every frame."""
    W, H = 129, 37
    cur = {}
    fused, chain = scripted_maskers(cur)
    ref = oracle.Masker()
    fallback = torch.zeros(H, W, dtype=torch.bool, device=DEV)
    fallback[5:20, 100:] = True
    plan = [(6, 0), (5, 0), (0, 0), (4, 2), (7, 0), (3, 0), (9, 0), (2, 1), (8, 0), (6, 0), (0, 0), (5, 0)]
    for n, (nb, ns) in enumerate(plan):
        if n == 6:
            for m in (fused, chain, ref):
                m.reset()
        c = cases.random_frame(40 + n, W, H, nb, ns, empty_sam=n == 7)
        cur.update(boxes=up(c["boxes"]), labels=c["labels"], sam=up(c["sam"]), fallback=fallback if n == 2 else None)
        k = (9, 7, 0)[n % 3]
        frame_idx = 0 if n == 6 else n + 1
        kw = dict(expand_kernel=k, rgb_boundary_threshold=0.3, depth=up(c["depth"]))
        a = fused.detect_and_segment(up(c["image"]), frame_idx, **kw)
        b = chain.detect_and_segment(up(c["image"]), frame_idx, **kw)
        want = ref.frame(W, H, frame_idx, c["boxes"], c["labels"], c["sam"], fallback=fallback.cpu().numpy() if n == 2 else None, expand_kernel=k,
                         image=c["image"], threshold=0.3, depth=c["depth"])
        check_masks(a, want, ("fused", n))
        check_masks(b, want, ("chain", n))
        entries = fused._history.entries()
        assert len(entries) == len(ref.history) == len(chain.mask_history), n
        assert all(np.array_equal(x, y) and np.array_equal(x, z.cpu().numpy()) for x, y, z in zip(entries, ref.history, chain.mask_history)), n
    assert len(ref.history) == 4      # frames 7, 8, 9 and 11 after the reset: the majority ran


@pytest.mark.parametrize("k", [5, 7, 9])
def test_against_the_pytorch_statements_on_the_same_tensors(k):
    """``expand_dynamic_mask``, ``valid_rgb`` and the masked depth as SlamSequence.add_new_keyframe states them, on the device tensors
    the call read (image values are multiples of 1 / 256: their channel sums are exact in any order)."""
    from lvdgs import dynamic_mask as dm
    from lvdgs.slam_sequence import expand_dynamic_mask
    W, H, thr = 333, 75, 0.3
    c = cases.random_frame(k, W, H, 0, 3)
    sam, image, depth = up(c["sam"]), up(c["image"]), up(c["depth"])
    got = dm.assemble(W, H, None, None, sam, first_frame=True, history=dm.MaskHistory(W, H, 5, DEV), expand_kernel=k, image=image,
                      rgb_boundary_threshold=thr, depth=depth)
    dynamic = (sam != 0).any(dim=0)
    grown = expand_dynamic_mask(dynamic, k)
    valid = (image.sum(dim=0) > thr) & ~grown
    masked = depth.clone()
    masked[~valid] = 0
    assert int(dynamic.sum()) > 0 and int(grown.sum()) > int(dynamic.sum())
    assert torch.equal(got.dynamic_mask, dynamic) and torch.equal(got.static_mask, ~dynamic)
    assert torch.equal(got.expanded_dynamic_mask, grown) and torch.equal(got.expanded_static_mask, ~grown)
    assert torch.equal(got.valid_rgb, valid) and torch.equal(got.depth, masked)
    info = got.info_dict()
    assert info["expanded_pixels"] == int(grown.sum()) and info["valid_pixels"] == int(valid.sum()) and info["depth_pixels"] == int((masked > 0).sum())
    # vehicle dilation: the same statement at the vehicle kernel's size
    box = torch.tensor([[40.0, 20.0, 90.0, 50.0]], device=DEV)
    got = dm.assemble(W, H, box, [True], sam, first_frame=False, history=dm.MaskHistory(W, H, 5, DEV), vehicle_kernels=(7, k))
    assert torch.equal(got.dynamic_mask, expand_dynamic_mask(dynamic, k))


def test_toy_drive_with_detections_fused_equals_the_torch_chain():
    """The toy drive of tests/sequence_scene.py on the HIP path with dynamic_masks="detections": the library behind the masker and the
    PyTorch chain behind it give identical masks on every keyframe, an identical window log and map size."""
    import sequence_scene as ss
    from lvdgs import synthetic
    from lvdgs.dynamic_mask import DynamicMasker
    from lvdgs.slam_sequence import SlamSequence
    cfg, ds, _, _, _ = ss.toy_sequence_on_cpu(dynamic_objects=True, n_frames=8)
    cfg["Training"]["kf_overlap"] = 1.01      # while the window fills, every frame kf_interval after the last keyframe becomes one
    ds = ds.to(DEV)
    runs = []
    for fused in (True, False):
        torch.manual_seed(0)
        random.seed(0)
        det = synthetic.RectangleDetector(ds)
        masker = DynamicMasker(det.detect, det.segment, fused=fused)
        runs.append(SlamSequence(cfg, ds, ss.empty_map(cfg, DEV), ss.PIPE, torch.zeros(3, device=DEV), idle_map_iters=2, dynamic_masks="detections",
                                 masker=masker).run())
    a, b = runs
    assert a.kf_indices == b.kf_indices and len(a.kf_indices) >= 2 and a.window_log == b.window_log and a.frame_log == b.frame_log
    assert a.gaussian_counts == b.gaussian_counts and a._n() == b._n() > 0
    for i in a.kf_indices:
        for name in ("static_mask", "dynamic_mask", "expanded_dynamic_mask", "expanded_static_mask"):
            x, y = getattr(a.cameras[i], name), getattr(b.cameras[i], name)
            assert x.dtype is torch.bool and torch.equal(x, y), (i, name)
        assert 0 < int(a.cameras[i].dynamic_mask.sum()) < int(a.cameras[i].expanded_dynamic_mask.sum())
    assert a.masker.last.info.tolist() == b.masker.last.info.tolist()
