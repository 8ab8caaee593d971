#!/usr/bin/env python3
"""Wall time per call of the keyframe depth alignment (``lvdgs.depth_utils.process_depth`` on device tensors: max_iter + 1 launches
and one host wait; with the remedy, a second enqueue and wait) at KITTI's 1226 x 370 and waymo's 1920 x 1280, in the converging case
and in the remedy case (a scale-remedy stand-in that returns a fixed scale), measured with device events around the whole call; the
kernels' own time from the library's per-launch event timing.  Next to it, when the reference checkout is given (``--reference DIR``),
the reference's NumPy ``process_depth`` on the host (loaded as tests/golden/make_depth_align_golden.py does).  One JSON line per case.

    python tools/depth_align_bench.py [--reps 50] [--reference /path/to/reference]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import lvdgs  # noqa: E402,F401
from lvdgs import _lib, depth_utils  # noqa: E402
import depth_align_cases as dc  # noqa: E402

SIZES = {"kitti": (370, 1226), "waymo": (1280, 1920)}
CASES = {"converging": (1.15, None), "remedy": (2.5, 2.47)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--reference", default=None, help="reference checkout: also time its NumPy process_depth on the host")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    ref = None
    if a.reference and os.path.isdir(a.reference):
        os.environ["LVDGS_REFERENCE"] = a.reference
        sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
        import make_depth_align_golden as mk
        mk.REF = a.reference
        ref = mk.load_reference()
    for size, (H, W) in SIZES.items():
        for case, (true_scale, remedy_scale) in CASES.items():
            r, m = dc.depth_pair(H, W, 1, true_scale)
            rt, mt = torch.from_numpy(r).to(dev), torch.from_numpy(m).to(dev)
            remedy = None if remedy_scale is None else (lambda *args, s=remedy_scale: s)
            for _ in range(3):
                depth_utils.process_depth(rt, mt, scale_remedy=remedy)
            _lib.profile_reset()
            _lib.profile_enable(True)
            depth_utils.process_depth(rt, mt, scale_remedy=remedy)
            kernels = _lib.profile_read()
            _lib.profile_enable(False)
            times = []
            for _ in range(a.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                out = depth_utils.process_depth(rt, mt, scale_remedy=remedy)
                e1.record()
                e1.synchronize()
                times.append(e0.elapsed_time(e1))
            rec = depth_utils.last_call
            line = dict(size=size, width=W, height=H, case=case, reps=a.reps, ms_median=round(float(np.median(times)), 4),
                        ms_min=round(float(np.min(times)), 4), ms_max=round(float(np.max(times)), 4),
                        scale=float(out[1]), num_accurate=int(out[3]), patch_num=rec.patch_num, last_iteration=rec.iteration,
                        remedies=[k for k, _ in rec.remedies],
                        kernels_us={k: dict(launches=n, us_per_launch=round(1e3 * t / max(n, 1), 2)) for k, (n, t) in kernels.items()})
            if ref is not None:
                ref.find_scale = dc.RecordedRemedy([remedy_scale] if remedy_scale else [])
                import contextlib
                import io
                t0 = time.perf_counter()
                with contextlib.redirect_stdout(io.StringIO()):
                    ref.process_depth(r, m, None, None, None, None)
                line["reference_numpy_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
