#!/usr/bin/env python3
"""The loops as a system: a synthetic drive through an opaque-surface scene at KITTI-07's geometry, from an EMPTY map --
initialize_map on frame 0, then per frame track_frame -> keyframe test -> seeding -> masked map_window bursts with densification /
pruning / opacity resets at the reference's cadence -> pruning pass, the back end's free-running iterations between frames, and at
the end ATE (Umeyama), PSNR before / after a colour refinement (lvdgs.slam_sequence.SlamSequence; reference utils/slam_frontend.py:1740-1899,
utils/slam_backend.py:485-609, utils/eval_utils_0806.py:33-306).

    python tools/sequence.py [--frames 60] [--scale 1.0] [--cadence reference|short] [--no-fused] [--idle 10] [--refine 500] [--no-masks] [--pose-init previous|pnp] [--scale-remedy keep|matches]
    python tools/sequence.py --config YAML [--dataset-path DIR] [--ingest host|fused] [--prefetch N] [--planes host|device]     # the frames of a directory instead (lvdgs.dataset.load_dataset)

Prints one JSON object (bench.py's config.side.sequence_kitti07_geom is the same record).  `--cadence reference`: the iteration
counts and densification schedule of configs/mono/KITTI/base_config.yaml as they are; `short`: every burst a fifth of it (the GPU
test's schedule).  The first three tracked frames of a reference-cadence run are the map's slowest (the map is one keyframe old)."""
import argparse
import copy
import json
import os
import random
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import lvdgs  # noqa: E402,F401
from lvdgs import synthetic  # noqa: E402
from lvdgs.gaussian_renderer import render  # noqa: E402
from lvdgs.slam_sequence import SlamSequence  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
PIPE = SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=False)


def sequence_config(W, H, **training):
    """The merged KITTI-07 config (tests/golden/config_07.json: ``load_config("configs/mono/KITTI/07.yaml")`` of the reference, captured by
    tests/golden/make_golden.py) with ``training`` laid over its Training block and the frame size set."""
    training = dict(training)
    cfg = copy.deepcopy(json.load(open(os.path.join(GOLDEN, "config_07.json"))))
    cfg["Training"]["monocular"] = cfg["Dataset"]["sensor_type"] == "monocular"   # (set by the absent slam.py entry point)
    lr = training.pop("lr", None)
    cfg["Training"].update(training)
    if lr:
        cfg["Training"]["lr"].update(lr)
    cfg["Dataset"]["Calibration"].update(width=W, height=H)
    cfg["Results"].update(save_results=False, use_gui=False)
    return cfg


def truth_model(W, H, n_true, r_min, r_max, margin, device, seed=11):
    from lvdgs.gaussian_model import GaussianModel
    g = synthetic.make_surface_gaussians(n_true, W, H, seed=seed, r_min=r_min, r_max=r_max, margin=margin)
    return GaussianModel.from_activated(g["means3D"], g["scales"], g["rotations"], g["opacities"], shs=g["shs"], device=device)


def empty_map(cfg, device):
    from lvdgs.gaussian_model import GaussianModel
    m = GaussianModel(cfg["model_params"]["sh_degree"], config=cfg, device=device)
    m.init_lr(cfg["opt_params"]["init_lr"])
    m.training_setup(cfg["opt_params"])
    return m


SHORT = dict(init_itr_num=210, init_gaussian_update=20, init_gaussian_reset=100, tracking_itr_num=40, mapping_itr_num=30,
             mapping_itr_nosingle=10, initial_ba_itr_num=60, gaussian_update_every=30, gaussian_update_offset=10, gaussian_reset=401)


# frame geometries: KITTI-07 (configs/mono/KITTI/07.yaml:8-18) and the waymo segment of BASELINE configs[4]'s size (configs/mono/waymo/405841.yaml:5-16,
# whose Training block also runs 30 mapping iterations per keyframe instead of 10)
GEOMETRY = {"kitti07": dict(W=1226, H=370, fx=707.0912, cx=601.8873, cy=183.1104, training={}),
            "waymo": dict(W=1920, H=1280, fx=2066.697564417299, cx=950.5512774150723, cy=641.1870541472169, training={"mapping_itr_nosingle": 30})}


def kitti_sequence(dev, frames=60, scale=1.0, cadence="reference", masks=True, n_true=None, seed=0, training=None, window_size=None, geometry="kitti07",
                   pcd_downsample=None, mono_scale_drift=0.0, trajectory=None, metric_depth=False):
    """(config, dataset, true map): a frame geometry of ``GEOMETRY`` (x ``scale``), the merged KITTI-07 config with the chosen cadence.
    ``trajectory``: ``synthetic.vehicle_trajectory``'s parameters (step, sway, yaw, period) laid over the default drive's."""
    geo = GEOMETRY[geometry]
    W, H = int(round(geo["W"] * scale)), int(round(geo["H"] * scale))
    fx = fy = geo["fx"] * scale
    cx, cy = geo["cx"] * scale, geo["cy"] * scale
    tr = dict(SHORT) if cadence == "short" else {}
    tr.update(geo["training"])
    if window_size is not None:
        tr.update(window_size=window_size, pose_window=min(3, window_size - 1))
    tr.update(training or {})
    cfg = sequence_config(W, H, **tr)
    cfg["Dataset"]["Calibration"].update(fx=fx, fy=fy, cx=cx, cy=cy)
    if pcd_downsample is not None:   # (init, later keyframes): seeds per keyframe = valid pixels / this (configs/mono/KITTI/base_config.yaml:13-14: 32, 64)
        cfg["Dataset"].update(pcd_downsample_init=int(pcd_downsample[0]), pcd_downsample=int(pcd_downsample[1]))
    n_true = int(600_000 * scale * scale * (W * H) / (1226.0 * scale * 370.0 * scale) * (707.0912 / geo["fx"]) ** 2) if n_true is None and geometry != "kitti07" else n_true
    n_true = int(600_000 * scale * scale) if n_true is None else n_true
    # opaque surfaces of 1.5..16-pixel footprints (x scale) -- texture at the scale of a few pixels, which is what keeps a SLAM map's
    # Gaussians small and many (the 4..64-pixel footprints of the surface WORKLOADS render to a blur that a few hundred large Gaussians
    # reproduce: the map then prunes itself down to them) -- reaching 0.9 frame widths past the first frame's edges: the camera's field
    # of view is wider than the generator's (fx < W) and the camera moves
    truth = truth_model(W, H, n_true, 1.5 * scale, 16.0 * scale, 0.9, dev, seed=11 + seed)
    ds = synthetic.make_sequence(truth, render, PIPE, W, H, frames, dev, fx=fx, fy=fy, cx=cx, cy=cy, seed=seed, depth_noise=0.02,
                                 image_noise=0.01, dynamic_objects=masks, mono_scale_drift=mono_scale_drift, metric_depth=metric_depth,
                                 **{**dict(step=0.02, sway=0.15, yaw=0.03, period=40.0), **(trajectory or {})})
    return cfg, ds, truth


def directory_sequence(dev, config_path, dataset_path=None, ingest="host", cadence="reference", training=None, window_size=None, planes="host"):
    """(config, dataset): the settings of ``config_path`` (lvdgs.config_utils.load_config) and the dataset they name
    (lvdgs.dataset.load_dataset: KITTI, waymo, dl3dv, replica or tum files on disk; ``dataset_path`` replaces the YAML's).  ``cadence``
    "reference" leaves the Training block as the file has it, "short" lays ``SHORT`` over it; ``training`` / ``window_size`` as in
    ``kitti_sequence``."""
    from lvdgs.config_utils import load_config
    from lvdgs.dataset import load_dataset
    cfg = load_config(config_path)
    cfg["Training"]["monocular"] = cfg["Dataset"]["sensor_type"] == "monocular"   # (set by the absent slam.py entry point)
    tr = dict(SHORT) if cadence == "short" else {}
    if window_size is not None:
        tr.update(window_size=window_size, pose_window=min(3, window_size - 1))
    tr.update(training or {})
    lr = tr.pop("lr", None)
    cfg["Training"].update(tr)
    if lr:
        cfg["Training"]["lr"].update(lr)
    cfg.setdefault("Results", {}).update(save_results=False, use_gui=False)
    if dataset_path is not None:
        cfg["Dataset"]["dataset_path"] = dataset_path
    return cfg, load_dataset(None, None, cfg, device=dev, ingest=ingest, planes=planes)


def run_sequence(dev, frames=60, scale=1.0, cadence="reference", fused="auto", idle=10, refine=500, masks=True, seed=0, training=None,
                 window_size=None, on_event=None, geometry="kitti07", pcd_downsample=None, mono_scale_drift=0.0, trajectory=None,
                 config_path=None, dataset_path=None, ingest="host", eval_mode="host", planes="host", metric_depth=False, **sequence_kwargs):
    torch.manual_seed(seed)
    random.seed(seed)
    if config_path is not None:      # frames from a directory: at most ``frames`` of them
        cfg, ds = directory_sequence(dev, config_path, dataset_path, ingest, cadence, training, window_size, planes)
        masks, geometry = False, cfg["Dataset"]["type"]
        ds.num_imgs = min(len(ds), frames)
    else:
        cfg, ds, truth = kitti_sequence(dev, frames, scale, cadence, masks, seed=seed, training=training, window_size=window_size, geometry=geometry,
                                        pcd_downsample=pcd_downsample, mono_scale_drift=mono_scale_drift, trajectory=trajectory,
                                        metric_depth=metric_depth)
        del truth
    m = empty_map(cfg, dev)
    if sequence_kwargs.get("matcher") == "descriptors":      # descriptor maps matched on the device (the network's stand-in: synthetic.WorldDescriptors)
        from lvdgs import init_pose
        sequence_kwargs["matcher"] = init_pose.DescriptorMatcher(synthetic.WorldDescriptors(ds, seed=seed))
    if (sequence_kwargs.get("pose_init") == "pnp" or sequence_kwargs.get("scale_remedy") == "matches") and sequence_kwargs.get("matcher") is None:
        sequence_kwargs["matcher"] = synthetic.GroundTruthMatcher(ds, stride=8, noise_px=0.7, outlier_ratio=0.3, seed=seed)
    if sequence_kwargs.get("dynamic_masks") == "detections" and sequence_kwargs.get("masker") is None:
        # the masks assembled from detections (dynamic_mask.DynamicMasker) of the stand-in for the two networks: the dataset's rectangles
        from lvdgs.dynamic_mask import DynamicMasker
        det = synthetic.RectangleDetector(ds)
        sequence_kwargs["masker"] = DynamicMasker(det.detect, det.segment, fused=sequence_kwargs.pop("fused_masks", True))
    seq = SlamSequence(cfg, ds, m, PIPE, torch.zeros(3, device=dev), fused=fused, idle_map_iters=idle, on_event=on_event, **sequence_kwargs)
    seq.run()
    out = seq.summary()
    out["ate_rmse"] = seq.eval_ate()
    eval_fused = eval_mode == "fused"      # one FrameEvaluator over the evaluation loop, one read at its end
    t_eval = time.perf_counter()
    before = seq.eval_rendering(fused=eval_fused)
    out["eval_rendering_seconds"] = round(time.perf_counter() - t_eval, 4)
    out["psnr_before_refinement"], out["ssim_before_refinement"] = before.get("psnr"), before.get("ssim")
    out["psnr_static_before_refinement"] = before.get("psnr_static")
    if refine:
        seq.refine(refine)
        t_eval = time.perf_counter()
        after = seq.eval_rendering(fused=eval_fused)
        out["eval_rendering_seconds_after_refinement"] = round(time.perf_counter() - t_eval, 4)
        out["psnr"], out["ssim"], out["psnr_static"] = after.get("psnr"), after.get("ssim"), after.get("psnr_static")
        s = seq.seconds["refinement"]
        out["refinement_ms_per_iteration"] = round(1e3 * s / refine, 4)
    err = seq.pose_errors()
    out["pose_error_unaligned_mean"], out["pose_error_unaligned_max"] = sum(err.values()) / len(err), max(err.values())
    out["trajectory_length"] = float(sum(float(torch.linalg.inv(torch.as_tensor(ds.poses[i + 1]))[:3, 3].sub(torch.linalg.inv(torch.as_tensor(ds.poses[i]))[:3, 3]).norm())
                                         for i in range(len(ds) - 1)))
    out["window_log"] = seq.window_log
    out["batched_window_runs"] = int(getattr(getattr(seq.backend, "_lvdgs_window_batch", None), "runs", 0))
    out.update(geometry=geometry, width=ds.width, height=ds.height, cadence=cadence, fused=fused, idle_map_iters=idle, keyframes_carry_static_mask=masks)
    if config_path is not None:
        out.update(config=config_path, ingest=ingest)
        if planes != "host" or sequence_kwargs.get("prefetch"):
            out.update(planes=planes, prefetch=int(sequence_kwargs.get("prefetch") or 0))
    if mono_scale_drift or sequence_kwargs.get("keyframe_depth") is not None:
        out.update(mono_scale_drift=mono_scale_drift, keyframe_depth=sequence_kwargs.get("keyframe_depth") or "mono")
    return out, seq


def png16(plane):
    """An (H, W) uint16 array as the bytes of a 16-bit grey PNG."""
    import struct
    import zlib

    import numpy as np
    h, w = plane.shape
    rows = np.concatenate([np.zeros((h, 1), np.uint8), plane.astype(">u2").view(np.uint8).reshape(h, 2 * w)], axis=1)      # filter 0 per row

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)
    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 16, 0, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(rows.tobytes(), 6))
            + chunk(b"IEND", b""))


def write_depth_planes(directory, planes, fmt):
    """``SlamSequence.last_eval_depths`` -- (the estimate's planes, the ground truth's), one per evaluated frame -- into ``directory``."""
    import numpy as np
    os.makedirs(directory, exist_ok=True)
    written = 0
    for name, group in zip(("est", "gt"), planes):
        for k, plane in enumerate(group):
            d = plane.detach().cpu().numpy()
            path = os.path.join(directory, f"{name}_{k:04d}.{fmt}")
            if fmt == "npy":
                np.save(path, d)
            else:
                with open(path, "wb") as fh:
                    fh.write(png16(np.clip(np.rint(d.astype(np.float64) * 1000.0), 0, 65535).astype(np.uint16)))
            written += 1
    return dict(directory=directory, format=fmt, files=written)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--cadence", choices=["reference", "short"], default="reference")
    ap.add_argument("--no-fused", action="store_true")
    ap.add_argument("--idle", type=int, default=10)
    ap.add_argument("--refine", type=int, default=500)
    ap.add_argument("--no-masks", action="store_true")
    ap.add_argument("--window-size", type=int, default=None)
    ap.add_argument("--geometry", choices=sorted(GEOMETRY), default="kitti07")
    ap.add_argument("--pcd-downsample", type=int, nargs=2, default=None, metavar=("INIT", "KEYFRAME"),
                    help="seed one Gaussian per INIT valid pixels of frame 0 and per KEYFRAME of every later keyframe (the config's 32 / 64): smaller = a larger map")
    ap.add_argument("--seed", type=int, default=0, help="scene, trajectory noise, dynamic objects and the loops' random draws")
    ap.add_argument("--keyframe-depth", choices=["mono", "patch_align"], default="mono",
                    help="seed later keyframes from the mono depth (default) or from LVD-GS Algorithm 1's alignment to the rendered depth")
    ap.add_argument("--mono-scale-drift", type=float, default=0.0, help="per-frame scale wander of the synthetic mono depth (synthetic.mono_scale_factor)")
    ap.add_argument("--pose-init", choices=["previous", "pnp"], default=None,
                    help="log every tracked frame's initial pose (summary key pose_init); pnp: start it from init_pose.get_pose with synthetic.GroundTruthMatcher")
    ap.add_argument("--matcher", choices=["ground_truth", "descriptors"], default="ground_truth",
                    help="with --pose-init pnp: matches made from the ground truth (default), or synthetic.WorldDescriptors' maps matched by init_pose.reciprocal_matches")
    ap.add_argument("--scale-remedy", choices=["keep", "matches"], default="keep",
                    help="with --keyframe-depth patch_align: keep the current scale when Algorithm 1's remedy branch fires (default), or take "
                         "depth_utils.find_scale's on the matches of --matcher (ground_truth: synthetic.GroundTruthMatcher)")
    ap.add_argument("--frame-stats", choices=["torch", "fused"], default="torch",
                    help="what a tracked frame reads after its loop (median depth, covisibility counts): PyTorch statements with a host wait "
                         "per count (default), or one frame_stats.frame_summary call and one wait")
    ap.add_argument("--edge-mask", choices=["torch", "fused"], default="torch",
                    help="Camera.compute_grad_mask's PyTorch statements (default) or one frame_stats.edge_mask call")
    ap.add_argument("--dynamic-masks", choices=["dataset", "detections"], default="dataset",
                    help="the frames' static masks: the dataset's finished ones (default), or assembled on the device from the boxes and masks of "
                         "synthetic.RectangleDetector by dynamic_mask.DynamicMasker (lvdgs_dynamic_mask)")
    ap.add_argument("--seeding", choices=["host", "fused"], default="host",
                    help="a keyframe's new Gaussians: GaussianModel's PyTorch statements and host draw (default), or one seeding.seed_points "
                         "call and one wait (lvdgs_seed_points; another subsample of the same size)")
    ap.add_argument("--map-edit", choices=["host", "fused"], default="host",
                    help="prune_points, densify_and_prune and the pruning pass: GaussianModel's PyTorch statements (default), or one map_edit plan, "
                         "one wait and one launch each (lvdgs_map_edit_plan / lvdgs_map_edit_apply)")
    ap.add_argument("--eval", choices=["host", "fused"], default="host", dest="eval_mode",
                    help="eval_rendering's per-frame block: frame_metrics' PyTorch statements with their host waits (default), or one "
                         "lvdgs_frame_eval call per frame and one read of the table at the end (eval_utils.FrameEvaluator)")
    ap.add_argument("--config", default=None, metavar="YAML",
                    help="run on the dataset this settings file names (lvdgs.config_utils.load_config + lvdgs.dataset.load_dataset) instead of the "
                         "synthetic drive; --frames caps the frames read, --cadence short lays the short schedule over the file's Training block")
    ap.add_argument("--dataset-path", default=None, metavar="DIR", help="with --config: the directory of the frames, instead of the file's dataset_path")
    ap.add_argument("--ingest", choices=["host", "fused"], default="host",
                    help="with --config: undistort and convert a decoded frame in NumPy and upload float32 (default), or upload its bytes and make "
                         "one lvdgs_ingest_frame call (the same bits)")
    ap.add_argument("--prefetch", type=int, default=0, metavar="N",
                    help="with --config: read N frames ahead of the loops on worker threads (lvdgs.dataset.FramePrefetcher); the same frames")
    ap.add_argument("--planes", choices=["host", "device"], default="host",
                    help="with --config --ingest fused: device makes the float32 depth planes on the GPU (lvdgs_ingest_depth) and the loops "
                         "take them without another upload")
    ap.add_argument("--mesh", default=None, metavar="PATH",
                    help="after the run: fuse the keyframes' rendered depth into a TSDF volume on the device (SlamSequence.fuse_mesh, "
                         "lvdgs_tsdf_integrate / lvdgs_tsdf_mesh) and write the mesh as a binary PLY")
    ap.add_argument("--mesh-voxel", type=float, default=None, metavar="SIZE",
                    help="with --mesh / --mesh-eval: the voxel size (default: 1/192 of the longest side of the opaque Gaussians' extent)")
    ap.add_argument("--mesh-volume", choices=("dense", "blocks"), default="dense",
                    help="with --mesh / --mesh-eval: 'blocks' fuses the rendered depth into a block-sparse volume (tsdf_blocks.TsdfBlockVolume): only "
                         "the blocks near a surface are stored and the voxel size asked for is the one used")
    ap.add_argument("--mesh-eval", action="store_true",
                    help="after the run: the fused mesh scored against a mesh fused from the dataset's depth at the ground-truth poses "
                         "(SlamSequence.eval_mesh, lvdgs_mesh_sample / lvdgs_cloud_distance): accuracy, completion, F-score; needs no --mesh PATH")
    ap.add_argument("--mesh-samples", type=int, default=200_000, metavar="N", help="with --mesh-eval: samples per mesh")
    ap.add_argument("--mesh-gt", default=None, metavar="PATH",
                    help="with --mesh-eval: a ground-truth mesh (a binary PLY in the ground-truth poses' world frame, mesh_eval.load_mesh_ply) in "
                         "place of the one fused from the dataset's depth")
    ap.add_argument("--mesh-cull", choices=("frustum", "visible", "occlusion"), default=None,
                    help="with --mesh-eval: cull both meshes to what the evaluated frames observed before scoring (mesh_eval.cull_mesh, "
                         "lvdgs_mesh_visibility / lvdgs_mesh_cull): 'frustum' -- inside some frame's image --, 'visible' -- the ground truth also "
                         "not behind the frames' dataset depth --, 'occlusion' -- each mesh against the depth rendered from itself "
                         "(lvdgs_mesh_depth), which needs no dataset depth")
    ap.add_argument("--mesh-depth-l1", action="store_true",
                    help="with --mesh-eval: both final meshes rendered at the evaluated frames (mesh_eval.render_depth) and the mean absolute "
                         "difference of the two depths over the pixels both cover: the protocol's 'Depth L1'")
    ap.add_argument("--mesh-depth-out", default=None, metavar="DIR",
                    help="with --mesh-eval: the depth planes rendered from both final meshes at the evaluated frames, written to DIR as "
                         "est_NNNN / gt_NNNN in --mesh-depth-format")
    ap.add_argument("--mesh-depth-format", choices=("png", "npy"), default="png",
                    help="with --mesh-depth-out: 'png' -- 16-bit grey, millimetres, saturated at 65535 --, 'npy' -- the float32 plane as it is")
    ap.add_argument("--verbose", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    t0 = time.perf_counter()
    ev = (lambda e, s: print(f"  frame {s.counts['frames']:3d} {e:16s} N = {s._n()}", file=sys.stderr)) if a.verbose else None
    out, seq = run_sequence(dev, a.frames, a.scale, a.cadence, False if a.no_fused else "auto", a.idle, a.refine, not a.no_masks, seed=a.seed,
                          window_size=a.window_size, on_event=ev, geometry=a.geometry, pcd_downsample=a.pcd_downsample,
                          mono_scale_drift=a.mono_scale_drift, eval_mode=a.eval_mode, metric_depth=a.mesh_eval, **({"keyframe_depth": "patch_align"} if a.keyframe_depth == "patch_align" else {}),
                          **({"pose_init": a.pose_init} if a.pose_init else {}), **({"matcher": "descriptors"} if a.matcher == "descriptors" else {}),
                          **({"scale_remedy": "matches"} if a.scale_remedy == "matches" else {}),
                          **({"frame_stats": "fused"} if a.frame_stats == "fused" else {}), **({"edge_mask": "fused"} if a.edge_mask == "fused" else {}),
                          **({"dynamic_masks": "detections"} if a.dynamic_masks == "detections" else {}),
                          **({"seeding": "fused"} if a.seeding == "fused" else {}), **({"map_edit": "fused"} if a.map_edit == "fused" else {}),
                          **({"config_path": a.config, "dataset_path": a.dataset_path, "ingest": a.ingest, "planes": a.planes} if a.config else {}),
                          **({"prefetch": a.prefetch} if a.config and a.prefetch else {}))
    out.update(frame_stats=a.frame_stats, edge_mask=a.edge_mask, dynamic_masks=a.dynamic_masks, seeding=a.seeding, map_edit=a.map_edit, eval=a.eval_mode)
    for rec in out.get("pose_init", []):
        print("  frame {frame:3d} kf {keyframe:3d} inliers {inl:>5} init error {e:.4f} ({r:.3f} deg; previous pose {p:.4f}) tracking iterations {it}".format(
            frame=rec["frame"], keyframe=rec["keyframe"], inl=rec.get("inliers", "-"), e=rec["init_translation_error"], r=rec["init_rotation_error_deg"],
            p=rec["previous_translation_error"], it=rec["tracking_iterations"]), file=sys.stderr)
    voxel = a.mesh_voxel
    if (a.mesh or a.mesh_eval) and voxel is None:
        g = seq.frontend_gaussians
        xyz = g.get_xyz.detach()
        opaque = g.get_opacity.detach().reshape(-1) >= 0.5
        points = xyz[opaque] if bool(opaque.any()) else xyz
        voxel = float((points.max(0).values - points.min(0).values).max()) / 192.0
    if a.mesh:
        from lvdgs.tsdf import save_mesh_ply
        t_mesh = time.perf_counter()
        mesh, record = seq.fuse_mesh(voxel, volume=a.mesh_volume)
        record["fuse_mesh_seconds"] = round(time.perf_counter() - t_mesh, 4)
        save_mesh_ply(a.mesh, mesh)
        out["mesh"] = dict(record, path=a.mesh, file_bytes=os.path.getsize(a.mesh))
    if a.mesh_eval:
        t_eval = time.perf_counter()
        want_depth = a.mesh_depth_l1 or a.mesh_depth_out is not None
        score, record = seq.eval_mesh(voxel, n_samples=a.mesh_samples, volume=a.mesh_volume, gt_mesh=a.mesh_gt, cull=a.mesh_cull, depth_l1=want_depth)
        out["mesh_eval"] = dict(score, record=record, eval_mesh_seconds=round(time.perf_counter() - t_eval, 4))
        if a.mesh_cull:
            print("  mesh cull {how}: estimate {eb} -> {ea} faces, ground truth {gb} -> {ga} faces".format(
                how=a.mesh_cull, eb=record["est"]["faces_before"], ea=record["est"]["faces"], gb=record["gt"]["faces_before"], ga=record["gt"]["faces"]),
                file=sys.stderr)
        if want_depth:
            print(f"  depth L1 {record['depth_l1']:.5f} over {record['depth_l1_pixels']} pixels", file=sys.stderr)
        if a.mesh_depth_out is not None:
            out["mesh_eval"]["depth_planes"] = write_depth_planes(a.mesh_depth_out, seq.last_eval_depths, a.mesh_depth_format)
        if a.mesh_cull:      # the same meshes scored whole, beside the culled score
            whole, _ = seq.eval_mesh(voxel, n_samples=a.mesh_samples, volume=a.mesh_volume, gt_mesh=a.mesh_gt)
            out["mesh_eval"]["without_cull"] = {k: whole[k] for k in ("accuracy", "completion", "completion_ratio", "precision", "recall", "fscore")}
    out["seed"] = a.seed
    out["tool_seconds"] = round(time.perf_counter() - t0, 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
