"""``bench.py --gpus 1``: a plain run times the headline alone -- set-up, warm-up, the K steps, the line -- and leaves every extra
measurement null; ``--full`` adds them (here with ``--no-side --no-cpu-baseline``, which keep the run short: the steady-state block,
the per-kernel times and the autograd-API rate still run)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run_bench(extra=()):
    env = dict(os.environ, LVDGS_BENCH_WORKLOAD="kitti07_geom")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "2", *extra]
    res = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]
    return json.loads(lines[0])


def _check_headline(out):
    assert out["n_gpus"] == 1 and out["steps"] == 4 and out["warmup"] == 2 and out["unit"] == "iters/s"
    assert out["higher_is_better"] is True and out["dtype"] == "f32"
    assert out["value"] > 0 and abs(out["value"] - 1e3 / out["ms_per_step"]) <= 1e-2 * out["value"]
    assert out["config"]["pairs"] > 0 and out["config"]["visible"] > 0


def test_plain_run_prints_the_headline_alone():
    out = _run_bench()
    _check_headline(out)
    assert out["full"] is False
    for k in ("steady_state", "roofline", "cpu_baseline", "kernels_us_per_step", "scaling_anchor_value"):
        assert out[k] is None, k
    for k in ("side", "autograd_api_iters_per_s", "pose_only_iters_per_s", "mapping_window_views_per_s"):
        assert out["config"][k] is None, k
    assert "sequence_kitti07_geom_summary" not in out


def test_full_run_adds_the_extra_measurements():
    out = _run_bench(("--full", "--no-side", "--no-cpu-baseline"))
    _check_headline(out)
    assert out["full"] is True
    ss = out["steady_state"]
    assert ss["steps"] == 4 and ss["value"] > 0 and ss["kernels_us_per_step"] == out["kernels_us_per_step"]
    assert out["kernels_us_per_step"] and all(v >= 0 for v in out["kernels_us_per_step"].values())
    assert out["config"]["autograd_api_iters_per_s"] > 0
    assert out["cpu_baseline"] is None and out["config"]["side"] is None   # (the two --no-* switches)
