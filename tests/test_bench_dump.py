"""``bench.py --dump-outputs DIR``: what the last timed step computed, written as DIR/<name>.npy (float32 / float64, at most
64 MB in all; a fixed seeded sample of rows / pixels of the large arrays), so that two builds run with the same arguments can be
compared output for output.  The CPU tests check the sampling and the files on stand-in tensors; the GPU test runs the benchmark
twice and checks that the same arguments give the same outputs."""
import json
import os
import shutil
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import lvdgs  # noqa: E402,F401


def _entries(N, H, W):
    g = torch.Generator().manual_seed(3)
    return [("color", torch.rand(3, H, W, generator=g), "image"), ("depth", torch.rand(1, H, W, generator=g), "image"),
            ("radii", torch.randint(0, 50, (N,), generator=g, dtype=torch.int32), "gaussian"),
            ("grad_means3D", torch.randn(N, 3, generator=g), "gaussian"), ("grad_shs", torch.randn(N, 1, 3, generator=g), "gaussian"),
            ("features_rest", torch.zeros(N, 0, 3), "gaussian"), ("skipped", None, "small"),
            ("loss", torch.tensor(0.25), "small"), ("R", torch.eye(3, dtype=torch.float64), "small")]


def _file_bytes(d):
    return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


def test_small_outputs_are_written_whole(tmp_path):
    N, H, W = 1000, 12, 16
    ent = _entries(N, H, W)
    info = bench.write_outputs(str(tmp_path), bench.snapshot_outputs(ent, N, H, W, torch.device("cpu")))
    names = sorted(p[:-4] for p in os.listdir(tmp_path))
    assert names == sorted(["color", "depth", "radii", "grad_means3D", "grad_shs", "loss", "R"])   # empty and None entries: no file
    assert info["files"] == len(names) and info["bytes"] == _file_bytes(tmp_path)
    src = {n: t for n, t, _ in ent if t is not None}
    for n in names:
        a = np.load(tmp_path / (n + ".npy"))
        assert a.dtype == (np.float64 if n in ("radii", "R") else np.float32), n
        assert np.array_equal(a, src[n].numpy().astype(a.dtype)), n


@pytest.mark.parametrize("limit, pixels_sampled", [(20_000, False), (6_000, True)])
def test_large_outputs_are_a_fixed_seeded_sample_sized_to_the_limit(tmp_path, limit, pixels_sampled):
    N, H, W = 1000, 12, 16
    ent = _entries(N, H, W)
    dirs = [tmp_path / "a", tmp_path / "b"]
    for d in dirs:
        info = bench.write_outputs(str(d), bench.snapshot_outputs(ent, N, H, W, torch.device("cpu"), limit=limit))
        assert info["bytes"] == _file_bytes(d) <= limit
    rows = np.load(dirs[0] / "gaussian_rows.npy")
    assert rows.dtype == np.float64 and 0 < len(rows) < N and len(np.unique(rows)) == len(rows) and rows.max() < N
    r = rows.astype(np.int64)
    src = {n: t.numpy() for n, t, _ in ent if t is not None}
    assert np.array_equal(np.load(dirs[0] / "grad_means3D.npy"), src["grad_means3D"][r])
    assert np.array_equal(np.load(dirs[0] / "radii.npy"), src["radii"][r].astype(np.float64))
    if pixels_sampled:
        pix = np.load(dirs[0] / "pixel_index.npy")
        assert 0 < len(pix) < H * W and len(np.unique(pix)) == len(pix) and pix.max() < H * W
        assert np.array_equal(np.load(dirs[0] / "color.npy"), src["color"].reshape(3, -1)[:, pix.astype(np.int64)])
    else:   # the images fit beside a sample of the Gaussians: written whole
        assert not (dirs[0] / "pixel_index.npy").exists()
        assert np.array_equal(np.load(dirs[0] / "color.npy"), src["color"])
    assert np.array_equal(np.load(dirs[0] / "loss.npy"), src["loss"])
    for f in os.listdir(dirs[0]):   # the same inputs, the same sample
        assert np.array_equal(np.load(dirs[0] / f), np.load(dirs[1] / f)), f
    with pytest.raises(ValueError):   # not even the whole small arrays fit
        bench.snapshot_outputs(ent, N, H, W, torch.device("cpu"), limit=500)


def _stand_ins(path, N, H, W):
    """Zero tensors of the shapes each timed path of bench.py hands bench.dump_entries at sh_degree 0 with the full backward."""
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt)
    cam = SimpleNamespace(cam_rot_delta=z(3), cam_trans_delta=z(3), exposure_a=z(1), exposure_b=z(1))
    if path == "tracking":
        sess = SimpleNamespace(color=z(3, H, W), depth=z(1, H, W), opacity=z(1, H, W), radii=z(N, dt=torch.int32), n_touched=z(N, dt=torch.int32),
                               loss=z(()), d_m3=z(N, 3), d_m2=z(N, 3), d_op=z(N, 1), d_sc=z(N, 3), d_rot=z(N, 4), d_sh=z(N, 1, 3), d_tau=z(6),
                               d_a=z(1), d_b=z(1), R=z(3, 3), T=z(3), view=z(4, 4), proj=z(4, 4), campos=z(3))
        return bench.dump_entries(cam, session=sess)
    if path == "tracking-autograd":
        params = [SimpleNamespace(grad=g) for g in (z(N, 3), z(N, 1, 3), z(N, 0, 3), z(N, 3), z(N, 4), z(N, 1))]
        pose = [SimpleNamespace(grad=g) for g in (z(3), z(3), z(1), z(1))]
        last = {"pkg": {"render": z(3, H, W), "depth": z(1, H, W), "opacity": z(1, H, W), "radii": z(N, dt=torch.int32)}, "loss": z(())}
        return bench.dump_entries(cam, last=last, params=params, pose_params=pose)
    m = SimpleNamespace(_xyz=z(N, 3), _features_dc=z(N, 1, 3), _features_rest=z(N, 0, 3), _scaling=z(N, 3), _rotation=z(N, 4), _opacity=z(N, 1),
                        max_radii2D=z(N), xyz_gradient_accum=z(N, 1), denom=z(N, 1))
    window = list(range(12, 4, -1))
    vps = {k: SimpleNamespace(R=z(3, 3), T=z(3), exposure_a=z(1), exposure_b=z(1)) for k in window}
    return bench.dump_entries(cam, backend=SimpleNamespace(gaussians=m, viewpoints=vps), window=window)


@pytest.mark.parametrize("path", ["tracking", "tracking-autograd", "mapping"])
def test_every_workload_dumps_within_the_limit(tmp_path, path):
    """The benchmark's workloads at their real sizes, up to 2M Gaussians at 1920x1280: the dump always fits, sampled where it must be."""
    from lvdgs import synthetic
    for name, cfg in synthetic.CONFIGS.items():
        N, W, H = cfg["N"], cfg["W"], cfg["H"]
        d = tmp_path / name
        info = bench.write_outputs(str(d), bench.snapshot_outputs(_stand_ins(path, N, H, W), N, H, W, torch.device("cpu")))
        assert info["bytes"] == _file_bytes(d) <= bench.DUMP_LIMIT_BYTES, name
        files = set(os.listdir(d))
        assert ("xyz.npy" if path == "mapping" else "color.npy") in files, name
        if name == "cfg5_2m_1920x1280":   # 2M Gaussians cannot be written whole on any path
            assert "gaussian_rows.npy" in files, name
        shutil.rmtree(d)


def _run_bench(out_dir, extra=()):
    env = dict(os.environ, LVDGS_BENCH_WORKLOAD="kitti07_geom")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "2", "--no-side", "--no-cpu-baseline",
           "--dump-outputs", str(out_dir), *extra]
    res = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [(), ("--step", "mapping")], ids=["tracking", "mapping"])
def test_bench_dumps_the_same_outputs_for_the_same_arguments(tmp_path, extra):
    outs = [_run_bench(tmp_path / k, extra) for k in ("a", "b")]
    for out in outs:
        assert out["steps"] == 4 and out["ms_per_step"] > 0
        assert out["dump_outputs"]["bytes"] <= 64_000_000 and out["dump_outputs"]["files"] == len(os.listdir(out["dump_outputs"]["dir"]))
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == sorted(os.listdir(tmp_path / "b"))
    want = {"color.npy", "radii.npy", "grad_means3D.npy", "grad_tau.npy"} if not extra else {"xyz.npy", "opacity.npy", "kf12_R.npy"}
    assert want <= set(files), files
    assert "gaussian_rows.npy" not in files and "pixel_index.npy" not in files   # 200k Gaussians at 1226x370 fit whole
    assert np.load(tmp_path / "a" / ("xyz.npy" if extra else "radii.npy")).shape[0] == 200_000
    for f in files:
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all(), f
        assert np.array_equal(a, b), f
