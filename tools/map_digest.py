#!/usr/bin/env python3
"""One sha256 over everything a fixed schedule of ``backend_map.map_window`` calls leaves behind on the toy window of
tests/loop_scene.py (keyframe 4 carries a static mask): two calls of ``iters=3`` (densifications at iterations 2 and 6, the
opacity reset at 5), the pruning pass on the full window, one more iteration.  Equal digests at two commits = the loop computes
the same bits.  usage: python tools/map_digest.py [--device cpu|cuda] [--world N] [--sharded] [--unfused]
(cpu: the dense renderer and the float64 loss statements; several ranks: gloo, on the one device)"""
import argparse
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "oracle"), ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402
import torch.multiprocessing as mp  # noqa: E402


def run(device, world, sharded, fused, aux_group=None):
    import lvdgs  # noqa: F401
    from dense_render import dense_render
    from loop_scene import backend_namespace, build_scene, cpu_view_loss, loop_config
    from lvdgs import backend_map as bm
    cfg = loop_config()
    sc = build_scene(device)
    be = backend_namespace(sc, cfg)
    be.initialized, be.shard_optimizer, be.shard_aux_group = True, sharded, aux_group
    be.viewpoints.update(enumerate(sc["cameras"]))
    window = be.current_window = sc["window"]
    be.keyframe_optimizers = sc["make_keyframe_optimizer"](be.viewpoints, window, cfg)
    kw = dict(render_fn=dense_render, view_loss_fn=cpu_view_loss, bands_ok=True) if device == "cpu" else dict(fused=fused)
    stats = {}
    for call in (dict(iters=3), dict(iters=3), dict(prune=True), dict(iters=1)):
        # (the loss of a pruning pass stays local to its rank, like its gradients: not recorded)
        bm.map_window(be, window, stats=None if call.get("prune") else stats, **kw, **call)
    G = be.gaussians
    out = dict(G._params_by_name())
    for gp in G.optimizer.param_groups:
        st = G.optimizer.state.get(gp["params"][0], {})
        out["m_" + gp["name"]], out["v_" + gp["name"]] = st.get("exp_avg"), st.get("exp_avg_sq")
    out.update(max_radii2D=G.max_radii2D, accum=G.xyz_gradient_accum, denom=G.denom, n_obs=G.n_obs)
    for i, cam in enumerate(sc["cameras"]):
        out.update({f"R{i}": cam.R, f"T{i}": cam.T, f"exp_a{i}": cam.exposure_a, f"exp_b{i}": cam.exposure_b})
    out.update({f"occ{kf}": be.occ_aware_visibility[kf] for kf in window})
    out["losses"] = torch.cat([l.reshape(1).float().cpu() for l in stats["losses"]])
    h = hashlib.sha256()
    for k in sorted(out):
        h.update(k.encode())
        if out[k] is not None:
            h.update(np.ascontiguousarray(out[k].detach().cpu().numpy()).tobytes())
    return h.hexdigest()


def worker(rank, a, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=a.world)
    try:
        torch.manual_seed(100 + rank)   # the ranks' global generators differ on purpose: nothing may depend on them
        q.put((rank, run(a.device, a.world, a.sharded, not a.unfused, dist.new_group() if a.world >= 4 else None)))
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", default="cpu", choices=("cpu", "cuda"))
    ap.add_argument("--world", type=int, default=1)
    ap.add_argument("--sharded", action="store_true")
    ap.add_argument("--unfused", action="store_true")
    a = ap.parse_args()
    if a.world == 1:
        torch.manual_seed(7)
        digests = {run(a.device, 1, False, not a.unfused)}
    else:
        ctx = mp.get_context("spawn")
        q = ctx.Queue()
        procs = [ctx.Process(target=worker, args=(r, a, 29000 + os.getpid() % 2000, q)) for r in range(a.world)]
        for p in procs:
            p.start()
        digests = {q.get(timeout=900)[1] for _ in procs}
        for p in procs:
            p.join(timeout=120)
    assert len(digests) == 1, f"the ranks ended differently: {sorted(digests)}"
    print(f"device={a.device} world={a.world} sharded={a.sharded} fused={not a.unfused}: {digests.pop()}")
