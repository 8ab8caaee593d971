"""lvdgs_edge_mask and lvdgs_frame_summary on the GPU (lvdgs.frame_stats) against the NumPy oracle (tests/frame_stats_oracle.py) and
against the PyTorch statements they replace on the same device tensors -- bit for bit: the medians are exact order statistics, the
counts integer sums, the edge arithmetic fixed by include/lvdgs.h.  Then the decisions of keyframe_utils and a whole toy drive with
the fused switches on: nothing may move."""
import os
import random
import sys

import numpy as np
import pytest
import torch

import frame_stats_cases as cases
import frame_stats_oracle as oracle

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "tools"))
pytestmark = pytest.mark.gpu
DEV = "cuda"


def bits(x):
    return np.asarray(x, dtype=np.float32).reshape(-1).view(np.uint32)


def summarise(depth, opacity, touched=None, rows=(), mask=None, count_mask=None):
    """(FrameSummary, the pinned block's bytes) of NumPy inputs uploaded to the device."""
    from lvdgs import frame_stats
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    touched = np.zeros(0, np.int32) if touched is None else touched
    pkg = dict(depth=up(depth), opacity=up(opacity), n_touched=up(touched.astype(np.int32)))
    fs = frame_stats.frame_summary(pkg, [up(r) for r in rows], mask=up(mask), count_mask=up(count_mask))
    block = frame_stats._summary.blocks[torch.device(DEV, torch.cuda.current_device()).index].numpy().copy()
    return fs, block, pkg


def check_selection(d, o, mask=None):
    from lvdgs.slam_utils import get_median_depth
    fs, block, pkg = summarise(d, o, mask=mask)
    want = oracle.summary(d, o, np.zeros(0, np.int32), [], mask=mask)
    torch_median = get_median_depth(pkg["depth"], pkg["opacity"], None if mask is None else torch.from_numpy(mask).to(DEV)).cpu().numpy()
    what = (d.size, want["selected"])
    assert fs.selected == want["selected"], what
    if want["selected"] == 0:
        assert fs.median_bits == 0x7fc00000 and np.isnan(fs.median_depth) and np.isnan(torch_median), what
    else:
        assert fs.median_bits == bits(want["median"])[0] == bits(torch_median)[0], (what, fs.median_depth, want["median"], torch_median)
    return block


@pytest.mark.parametrize("pattern", cases.SELECT_PATTERNS)
def test_median_depth_bits(pattern):
    """Every size and opacity selection, largest first so that every call after the first finds a used scratch behind it."""
    for n in sorted(cases.SELECT_SIZES, reverse=True):
        d = cases.depths(pattern, n)
        for kind in cases.OPACITY_KINDS:
            a = check_selection(d, cases.opacities(kind, n))
            b = check_selection(d, cases.opacities(kind, n))
            assert np.array_equal(a[4:], b[4:]), (pattern, n, kind)      # two calls: the same bytes (but for the sequence word)


def test_median_depth_of_a_frame_with_a_mask_then_of_a_small_one():
    H, W = 370, 1226
    rng = np.random.default_rng(4)
    d = rng.uniform(0.5, 80.0, H * W).astype(np.float32)
    d[rng.random(H * W) < 0.3] = 0.0                              # unrendered pixels
    o = np.where(rng.random(H * W) < 0.8, 0.99, 0.5).astype(np.float32)
    check_selection(d, o)
    check_selection(d, o, mask=rng.random(H * W) < 0.5)
    check_selection(d[:3], o[:3])                                   # a smaller input on the same scratch: no stale histogram
    check_selection(d, None)                                        # no opacity: depth > 0 alone
    big = np.full(H * W, 3.5, np.float32)                           # one bucket holds every pixel: counts beyond 65 535
    check_selection(big, np.ones(H * W, np.float32))


@pytest.mark.parametrize("N", cases.COVIS_SIZES)
def test_covisibility_counts(N):
    from lvdgs import frame_stats
    from lvdgs.keyframe_utils import covisibility
    d, o = cases.depths("random", 257), cases.opacities("all", 257)
    for n_rows in cases.COVIS_ROWS:
        for cur_kind in ("random", "true", "false"):
            touched = (cases.visibility(cur_kind, N, seed=1) * 2).astype(np.int32)
            kinds = ["false", "true", "random"]
            rows = [cases.visibility(kinds[r % 3], N, seed=10 + r) for r in range(n_rows)]
            cmask = cases.visibility("random", 257, seed=3)
            fs, _, pkg = summarise(d, o, touched, rows, count_mask=cmask)
            want = oracle.summary(d, o, touched, rows, count_mask=cmask)
            assert fs.visible == want["visible"] and fs.mask_count == want["mask_count"] and len(fs.covis) == n_rows
            cur = pkg["n_touched"] > 0
            for r, row in enumerate(rows):
                assert fs.covis[r] == covisibility(cur, torch.from_numpy(row).to(DEV).long()) == \
                    (want["rows"][r][0], want["rows"][r][1], want["visible"], want["rows"][r][2]), (N, n_rows, r)
            assert fs.mask_share == float(torch.from_numpy(cmask).to(DEV).float().mean())
    # int64 rows (what the loops store), more rows than one call takes, and a row of another length, which takes the PyTorch path
    if N:
        touched = (cases.visibility("random", N, seed=1) * 2).astype(np.int32)
        pkg = dict(depth=torch.from_numpy(d).to(DEV), opacity=torch.from_numpy(o).to(DEV), n_touched=torch.from_numpy(touched).to(DEV))
        rows = {100 + r: torch.from_numpy(cases.visibility("random", N, seed=50 + r)).to(DEV).long() for r in range(19)}
        rows["cpu"] = torch.from_numpy(cases.visibility("random", N, seed=99)).long()
        fs = frame_stats.frame_summary(pkg, rows)
        assert list(fs.covis) == list(rows)
        for k, row in rows.items():
            assert fs.covis[k] == covisibility((pkg["n_touched"] > 0).to(row.device), row), k


def test_mask_share_is_the_device_mean():
    """``is_keyframe`` compares float(mask.float().mean()) with 0.3: the share made from the count is that number, on the bar too."""
    from lvdgs import frame_stats
    for n, count in ((370 * 1226, 136086), (370 * 1226, 136085), (1920 * 1080, 622080), (257, 77), (10, 3)):
        m = torch.zeros(n, dtype=torch.bool, device=DEV)
        m[:count] = True
        assert frame_stats.mean_of_mask(count, n) == float(m.float().mean()), (n, count)


def edge(img, thr, kind):
    from lvdgs import frame_stats
    out = frame_stats.edge_mask_call(torch.from_numpy(img).to(DEV), thr, kind, loss_mask=True, magnitude=True, stats=True)
    return {k: getattr(out, k).cpu().numpy() for k in ("mask", "loss_mask", "magnitude", "stats")}


@pytest.mark.parametrize("H,W", ((2, 2), (2, 37)) + cases.MEDIAN_SIZES)
def test_edge_mask_whole_image(H, W):
    img = cases.image(H, W)
    want = oracle.edge_mask_median(img, cases.EDGE_THRESHOLD)
    got, again = edge(img, cases.EDGE_THRESHOLD, "kitti"), edge(img, cases.EDGE_THRESHOLD, "kitti")
    assert np.array_equal(bits(got["magnitude"]), bits(want["mag"]))
    assert np.array_equal(bits(got["stats"]), bits([want["median"], want["cut"]]))
    assert got["mask"].dtype == bool and np.array_equal(got["mask"][0], want["mask"])
    assert np.array_equal(got["loss_mask"], want["mask"].reshape(-1).astype(np.uint8))
    for k in got:
        assert np.array_equal(got[k], again[k]), k


def test_edge_mask_of_a_black_image():
    got = edge(np.zeros((3, 64, 64), np.float32), cases.EDGE_THRESHOLD, "kitti")
    assert np.array_equal(bits(got["stats"]), [0, 0]) and not got["mask"].any() and not got["magnitude"].any()


@pytest.mark.parametrize("H,W", ((32, 32),) + cases.BLOCK_SIZES)
@pytest.mark.parametrize("thr,gain", [(1.1, 1.0), (0.5, 1.0), (1.1, 40.0)])
def test_edge_mask_block_rule(H, W, thr, gain):
    img = cases.image(H, W, gain=gain)
    want = oracle.edge_mask_blocks(img, thr)
    got = edge(img, thr, "replica")
    assert np.array_equal(bits(got["magnitude"]), bits(want["mag"]))
    assert np.array_equal(bits(got["stats"][:, 0]), bits(want["medians"])) and np.array_equal(bits(got["stats"][:, 1]), bits(want["cuts"]))
    assert got["mask"].dtype == np.float32 and np.array_equal(bits(got["mask"]), bits(want["mask"]))
    assert np.array_equal(got["loss_mask"], (want["mask"] != 0).reshape(-1).astype(np.uint8))
    if gain > 1.0 and min(H, W) > 32:
        assert (want["cuts"] >= 1.0).any() and (want["cuts"] < 1.0).any()


def test_loss_form_mask_gives_the_loss_of_the_bool_mask():
    from lvdgs import frame_stats
    from lvdgs.fused_loss import photometric_loss
    H, W = 64, 64
    gt = torch.from_numpy(cases.image(H, W)).to(DEV)
    render = torch.from_numpy(cases.image(H, W, seed=1)).to(DEV)
    opacity = torch.full((1, H, W), 0.9, device=DEV)
    out = frame_stats.edge_mask_call(gt, cases.EDGE_THRESHOLD, "kitti", loss_mask=True)
    assert out.mask.data_ptr() % 16 == 0      # the bool mask's own storage is what the loss kernel reads: no conversion, no copy
    losses = [photometric_loss(render, gt, opacity=opacity, grad_mask=m, weight_by_opacity=True) for m in (out.mask, out.loss_mask)]
    assert float(losses[0]) > 0 and np.array_equal(bits(losses[0].cpu().numpy()), bits(losses[1].cpu().numpy()))


def test_keyframe_decisions_from_the_kernel_counts(golden_dir):
    """is_keyframe / add_to_window on the loop fixture's recorded visibilities and poses: with ``covis=`` from the kernel they
    return what they return without it."""
    import json
    from loop_scene import build_scene, loop_config
    from lvdgs import frame_stats
    from lvdgs.keyframe_utils import add_to_window, is_keyframe
    gold = np.load(os.path.join(golden_dir, "loops.npz"), allow_pickle=True)
    cfg = loop_config()
    torch.manual_seed(2)
    sc = build_scene("cpu")
    cameras = {i: c for i, c in enumerate(sc["cameras"])}
    cam = sc["track_camera"]
    cam.update_RT(torch.from_numpy(gold["track_end_R"]).float(), torch.from_numpy(gold["track_end_T"]).float())
    cameras[7] = cam
    cur_vis = torch.from_numpy(gold["kf_cur_visibility"]).bool()
    occ = {i: torch.from_numpy(gold[f"kf_occ_{i}"]).long() for i in range(7)}
    occ_thin = dict(occ)
    occ_thin[4] = occ[4] * (torch.arange(occ[4].numel()) % 7 == 0).long()
    median_depth = float(gold["track_median_depth"])
    pkg = dict(depth=torch.ones(16, device=DEV), opacity=torch.ones(16, device=DEV), n_touched=cur_vis.to(DEV).int())
    covis = {name: frame_stats.frame_summary(pkg, {i: v.to(DEV) for i, v in table.items()}).covis for name, table in (("full", occ), ("thin", occ_thin))}
    got = [is_keyframe(cfg, cameras, 7, last, None, None, median_depth, covis=covis["full"]) for last in range(7)]
    assert got == [is_keyframe(cfg, cameras, 7, last, cur_vis, occ, median_depth) for last in range(7)] == gold["kf_is_keyframe"].tolist()
    for scale in (0.25, 4.0, 16.0):
        assert [is_keyframe(cfg, cameras, 7, last, None, None, median_depth * scale, covis=covis["full"]) for last in range(7)] == \
            [is_keyframe(cfg, cameras, 7, last, cur_vis, occ, median_depth * scale) for last in range(7)]
    for c in json.loads(str(gold["kf_windows_json"])):
        table, name = (occ_thin, "thin") if c["thinned"] else (occ, "full")
        with_counts = add_to_window(cfg, cameras, 7, None, None, c["window"], initialized=c["initialized"], covis=covis[name])
        assert with_counts == add_to_window(cfg, cameras, 7, cur_vis, table, c["window"], initialized=c["initialized"])
        assert (list(with_counts[0]), with_counts[1]) == (c["new_window"], c["removed"]), c


@pytest.fixture(scope="module")
def toy_drives():
    """The toy drive of tests/sequence_scene.py on the HIP path: with the defaults, with frame_stats="fused", and with both switches."""
    import sequence_scene as ss
    from lvdgs.camera_utils import Camera
    from lvdgs.slam_sequence import SlamSequence
    cfg, ds, _, _, _ = ss.toy_sequence_on_cpu()
    ds = ds.to(DEV)
    runs = {}
    for name, kw in (("torch", {}), ("stats", dict(frame_stats="fused")), ("both", dict(frame_stats="fused", edge_mask="fused"))):
        masks = {}

        class Recording(Camera):
            @staticmethod
            def init_from_dataset(dataset, idx, projection_matrix):
                cam = Camera.init_from_dataset(dataset, idx, projection_matrix)
                cam.__class__ = Recording
                return cam

            def compute_grad_mask(self, config, fused=False, _masks=masks):
                super().compute_grad_mask(config, fused=fused)
                _masks[self.uid] = (bool(fused), self.grad_mask.clone())

        torch.manual_seed(0)
        random.seed(0)
        seq = SlamSequence(cfg, ds, ss.empty_map(cfg, DEV), ss.PIPE, torch.zeros(3, device=DEV), idle_map_iters=2, camera_cls=Recording, **kw).run()
        runs[name] = (seq, masks)
    return cfg, ds, runs


def test_drive_with_fused_frame_stats_is_the_same_drive(toy_drives):
    _, _, runs = toy_drives
    a, b = runs["torch"][0], runs["stats"][0]
    assert len(a.frame_log) == len(a.dataset) - 1 and any(f["keyframe"] for f in a.frame_log) and not all(f["keyframe"] for f in a.frame_log)
    assert b.frame_log == a.frame_log      # tracking iterations, median depth, covisibility, visible, the decision: every frame
    assert b.window_log == a.window_log and b.kf_indices == a.kf_indices and len(a.kf_indices) >= 3
    pa, pb = a.gaussians._params_by_name(), b.gaussians._params_by_name()
    assert list(pa) == list(pb)
    for k in pa:
        assert torch.equal(pa[k], pb[k]), k
    for i in a.cameras:
        assert torch.equal(a.cameras[i].R, b.cameras[i].R) and torch.equal(a.cameras[i].T, b.cameras[i].T), i


def test_drive_with_the_fused_edge_mask(toy_drives):
    cfg, ds, runs = toy_drives
    seq, masks = runs["both"]
    thr = cfg["Training"]["edge_threshold"]
    assert sorted(masks) == list(range(len(ds)))
    for i, (fused, m) in masks.items():
        want = oracle.edge_mask_median(ds[i][0].cpu().numpy(), thr)["mask"]
        assert fused and m.dtype is torch.bool and np.array_equal(m.cpu().numpy()[0], want), i
    assert all(not fused for fused, _ in runs["torch"][1].values())
    assert seq.kf_indices == runs["torch"][0].kf_indices and len(seq.frame_log) == len(ds) - 1
