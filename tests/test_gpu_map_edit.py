"""Map edit on the GPU: the plan against the provenance oracle bit for bit, apply's bytes, the split children against a float64
restatement, a fused model against a host model through a sequence of edits, the pruning pass, the one wait, the toy sequence."""
import functools
import random
import types

import numpy as np
import pytest
import torch

import map_edit_cases as cases
import map_edit_oracle as orc
from lvdgs import _lib

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -24
DEV = "cuda:0"


@functools.lru_cache(maxsize=None)
def _case(kind, n, S, degree=0):
    return cases.make_case(kind, n, S, degree)


@functools.lru_cache(maxsize=None)
def _oracle(kind, n, S):
    c = _case(kind, n, S)
    return orc.densify_and_prune(c["scaling"], c["opacity"], c["max_radii2D"], c["grad_accum"], c["denom"], c["max_grad"], c["min_opacity"],
                                 c["extent"], c["max_screen_size"], c["percent_dense"])


def _gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _plan_densify(c):
    from lvdgs import map_edit
    return map_edit.plan_densify(_gpu(c["grad_accum"]), _gpu(c["denom"]), _gpu(c["scaling"]), _gpu(c["opacity"]), c["max_grad"],
                                 c["percent_dense"] * c["extent"], c["min_opacity"], c["max_screen_size"], 0.1 * c["extent"])


def _check_plan(p, o):
    counts = ("n_out", "n_keep", "n_clone", "n_split_sel", "n_pruned_final")
    assert tuple(getattr(p, k) for k in counts) == tuple(int(o[k]) for k in counts), ([getattr(p, k) for k in counts], [o[k] for k in counts])
    assert np.array_equal(p.src.cpu().numpy(), o["src"]) and np.array_equal(p.src_cpu.numpy(), o["src"])
    assert np.array_equal(p.kind.cpu().numpy(), o["kind"]) and np.array_equal(p.noise_row.cpu().numpy(), o["noise_row"])


# ---------------------------------------------------------------- 1. the plan
@pytest.mark.parametrize("kind,n,S", [(k, n, S) for k in cases.KINDS for n in cases.SIZES for S in (3, 1)] +
                         [("mixed", cases.LONG_SPANS, 3), ("mixed", cases.LONG_SPANS, 1)])
def test_densify_plan_is_the_oracles(kind, n, S):
    _check_plan(_plan_densify(_case(kind, n, S)), _oracle(kind, n, S))


@pytest.mark.parametrize("n", cases.SIZES + (cases.LONG_SPANS,))
def test_prune_plans_are_the_oracles(n):
    from lvdgs import map_edit
    rng = np.random.default_rng(n)
    for share in (0.0, 0.05, 0.5, 1.0):
        mask = rng.random(n) < share if share < 1.0 else np.ones(n, dtype=bool)
        _check_plan(map_edit.plan_prune(n, DEV, _gpu(mask)), orc.prune_points(n, mask))
    kf = rng.integers(0, 12, n).astype(np.int32)
    window = [11, 9, 7, 6, 4, 3, 2, 0]
    for rows, dtype in ((8, np.bool_), (16, np.int64), (1, np.uint8), (0, np.bool_)):
        vis = [(rng.random(n) < 0.35).astype(dtype) for _ in range(rows)]
        for mode, initialized in (("odometry", True), ("slam", True), ("slam", False)):
            o, n_obs = orc.pruning_pass(vis, kf, mode, 3, window, initialized)
            prune_num, min_kf = (2, map_edit.INT32_MIN) if mode == "odometry" else (3, sorted(window, reverse=True)[2] if initialized else 0)
            p = map_edit.plan_prune(n, DEV, vis_rows=[_gpu(v) for v in vis], kf_id=_gpu(kf), prune_num=prune_num, min_kf_id=min_kf)
            _check_plan(p, o)
            assert np.array_equal(p.n_obs.cpu().numpy(), n_obs) and np.array_equal(p.n_obs_cpu.numpy(), n_obs[o["src"]])


# ---------------------------------------------------------------- 2. apply
WIDTHS = ((torch.uint8, ()), (torch.float32, ()), (torch.float32, (3,)), (torch.float32, (4,)), (torch.float32, (45,)), (torch.uint8, (7,)),
          (torch.int64, ()))      # 1, 4, 12, 16, 180, 7 and 8 bytes per row


@pytest.mark.parametrize("n", (65, 1025, 70_001))
def test_apply_moves_every_byte(n):
    from lvdgs import map_edit
    c, o = _case("mixed", n, 3), _oracle("mixed", n, 3)
    p = _plan_densify(c)
    _check_plan(p, o)
    g = torch.Generator().manual_seed(n)
    spare = 5
    ins, outs, cols, want = [], [], [], []
    for new_rows in (map_edit.COPY, map_edit.ZERO):
        for dtype, tail in WIDTHS:
            t = torch.randint(1, 250, (n,) + tail, generator=g).to(dtype)
            ins.append(t)
            outs.append(torch.full((p.n_out + spare,) + tail, 77, dtype=dtype, device=DEV))
            cols.append((t.to(DEV), outs[-1], new_rows))
            want.append(orc.materialise(t.numpy(), o["src"], o["kind"], zero_new=new_rows == map_edit.ZERO))
    # a 4-byte row at an odd address: the byte path
    odd_in, odd_out = torch.randint(1, 250, (4 * n + 1,), generator=g).to(torch.uint8), torch.full((4 * (p.n_out + spare) + 1,), 77, dtype=torch.uint8, device=DEV)
    cols.append((odd_in.to(DEV)[1:].view(n, 4), odd_out[1:].view(-1, 4), map_edit.COPY))
    untouched = torch.full((p.n_out + spare, 3), 77.0, device=DEV)       # never passed
    map_edit.apply(p, cols)
    for k, (out, w) in enumerate(zip(outs, want)):
        got = out.cpu().numpy()
        assert np.array_equal(got[:p.n_out], w), k
        assert (got[p.n_out:] == 77).all(), k                                # rows beyond n_out are not written
    assert np.array_equal(odd_out.cpu().numpy()[1:].reshape(-1, 4)[:p.n_out], odd_in.numpy()[1:].reshape(n, 4)[o["src"]])
    assert int(odd_out[0]) == 77 and bool((odd_out[1 + 4 * p.n_out:] == 77).all()) and bool((untouched == 77.0).all())


# ---------------------------------------------------------------- 3. the split children
def _children_reference(c, o, noise):
    """float64: (xyz, raw scale) of the rows of kind SPLIT0 / SPLIT1 and the a-priori bounds of a float32 evaluation of either statement.

    xyz_j = sum_k R_jk v_k + p_j with v_k = noise_k exp(s_k), R from q / |q|.  First-order bounds, eps = 2^-24 (half an ulp, relative):
      * q / |q|: the squared norm is four products and three additions, (1 + eps)^4; its root halves that and rounds, 3 eps; the division
        rounds, so a component carries at most 4 eps.  A product of two components carries 9 eps; x y - r z and its like: at most
        9 eps (|x y| + |r z|) + eps <= 5 eps (|x y| + |r z| <= 1/2), doubled exactly: 10 eps.  1 - 2 (y y + z z): 10 eps for the sum (<= 1),
        doubled, and the subtraction's rounding: 21 eps.  |dR_jk| <= 21 eps for every entry.
      * v_k: expf to one ulp (2 eps, the accuracy the device library documents for expf and logf; PyTorch's exp on the GPU calls the
        same function) and the product's rounding: 3 eps, relative.
      * the sum: each product rounds (eps), two additions among the three terms and the addition of p_j round: at most 3 eps of
        A_j + |p_j|, A_j = sum_k |R_jk| |v_k|, whatever the order of summation (the host statement's bmm has its own).
      => |err_j| <= eps (21 sum_k |v_k| + (3 + 1 + 3) A_j + 3 |p_j|)
    raw scale = log(exp(s) / 1.6): expf 2 eps, the constant 1.6 in float32 1 eps, the division 1 eps (a multiplication by a rounded
    reciprocal, as PyTorch divides by a scalar on the GPU: 2 eps) -- at most 5 eps relative in the logarithm's argument, which is 5 eps
    absolute in its value --, logf to one ulp, 2 eps |s'|:   |err| <= eps (5 + 2 |s'|).
    The fused path is allowed exactly these bounds, factor 1: it evaluates the same expressions with the same roundings counted above,
    in another order.  The host statement's own error is measured against the same bounds below, as the check of the derivation."""
    child = o["kind"] >= orc.SPLIT0
    src = o["src"][child]
    q = c["rotation"][src].astype(np.float64)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    r, x, y, z = q.T
    R = np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y)], -1),
                  np.stack([2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x)], -1),
                  np.stack([2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], -1)], 1)
    s = np.broadcast_to(c["scaling"][src].astype(np.float64), (src.size, 3))
    v = noise.astype(np.float64)[o["noise_row"][child]] * np.exp(s)
    p = c["xyz"][src].astype(np.float64)
    xyz = np.einsum("njk,nk->nj", R, v) + p
    A = np.einsum("njk,nk->nj", np.abs(R), np.abs(v))
    xyz_bound = EPS * (21 * np.abs(v).sum(1, keepdims=True) + 7 * A + 3 * np.abs(p))
    s_child = np.log(np.exp(c["scaling"][src].astype(np.float64)) / 1.6)
    return child, xyz, xyz_bound, s_child, EPS * (5 + 2 * np.abs(s_child))


def test_split_children_against_float64():
    from lvdgs import map_edit
    from lvdgs.gaussian_model import build_rotation
    n = 70_001
    c, o = _case("mixed", n, 3), _oracle("mixed", n, 3)
    p = _plan_densify(c)
    noise = torch.randn((2 * p.n_split_sel, 3), generator=torch.Generator().manual_seed(5))
    xyz, scaling, rotation = _gpu(c["xyz"]), _gpu(c["scaling"]), _gpu(c["rotation"])
    out_xyz, out_s = torch.empty(p.n_out, 3, device=DEV), torch.empty(p.n_out, 3, device=DEV)
    map_edit.apply(p, [(xyz, out_xyz, map_edit.XYZ), (scaling, out_s, map_edit.SCALE)], noise=noise.to(DEV), scaling=scaling, rotation=rotation)
    child, ref_xyz, b_xyz, ref_s, b_s = _children_reference(c, o, noise.numpy())
    assert child.sum() > 1000
    # everything but the children: the source's bytes
    assert np.array_equal(out_xyz.cpu().numpy()[~child], c["xyz"][o["src"][~child]]) and np.array_equal(out_s.cpu().numpy()[~child], c["scaling"][o["src"][~child]])
    # the host statements (gaussian_model.py, densify_and_split) on the same rows, in float32 on the GPU
    idx = _gpu(o["src"][child])
    samples = noise.to(DEV)[_gpu(o["noise_row"][child])] * torch.exp(scaling[idx])
    host_xyz = torch.bmm(build_rotation(rotation[idx]), samples.unsqueeze(-1)).squeeze(-1) + xyz[idx]
    host_s = torch.log(torch.exp(scaling[idx]) / (0.8 * 2))
    for name, got, host, ref, bound in (("xyz", out_xyz, host_xyz, ref_xyz, b_xyz), ("scale", out_s, host_s, ref_s, b_s)):
        e_fused = np.abs(got.cpu().numpy()[child].astype(np.float64) - ref)
        e_host = np.abs(host.cpu().numpy().astype(np.float64) - ref)
        print(f"{name}: fused max error {e_fused.max():.3e}, max error / bound {(e_fused / bound).max():.3f}; "
              f"host statement max error {e_host.max():.3e}, max error / bound {(e_host / bound).max():.3f}")
        assert (e_host <= bound).all(), name         # the derivation holds for the statement it was made for
        assert (e_fused <= bound).all(), name


def test_isotropic_children():
    """S = 1: one scale serves the three axes (the host statements cannot split such a map: the float64 restatement alone)."""
    from lvdgs import map_edit
    n = 1025
    c, o = _case("all_split", n, 1), _oracle("all_split", n, 1)
    p = _plan_densify(c)
    noise = torch.randn((2 * p.n_split_sel, 3), generator=torch.Generator().manual_seed(6))
    xyz, scaling, rotation = _gpu(c["xyz"]), _gpu(c["scaling"]), _gpu(c["rotation"])
    out_xyz, out_s = torch.empty(p.n_out, 3, device=DEV), torch.empty(p.n_out, 1, device=DEV)
    map_edit.apply(p, [(xyz, out_xyz, map_edit.XYZ), (scaling, out_s, map_edit.SCALE)], noise=noise.to(DEV), scaling=scaling, rotation=rotation)
    child, ref_xyz, b_xyz, ref_s, b_s = _children_reference(c, o, noise.numpy())
    assert child.all() and p.n_out == o["n_out"] and p.n_split_sel == n and p.n_out > n      # (children of faint sources are pruned)
    assert (np.abs(out_xyz.cpu().numpy().astype(np.float64) - ref_xyz) <= b_xyz).all()
    assert (np.abs(out_s.cpu().numpy().astype(np.float64) - ref_s) <= b_s).all()


# ---------------------------------------------------------------- 4. the model
def _bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.contiguous().view(torch.uint8).numpy() if a.numel() else a.numpy(),
                                                                        b.contiguous().view(torch.uint8).numpy() if b.numel() else b.numpy())


def _compare_models(host, fused, loose_rows, xyz_tol, s_tol, what):
    """Every tensor bit-identical, but for xyz / scaling in ``loose_rows`` (bool per row), held to the tolerances (per element)."""
    h, f = cases.model_tensors(host), cases.model_tensors(fused)
    assert h.keys() == f.keys() and h["xyz"].shape[0] == f["xyz"].shape[0], what
    loose = torch.from_numpy(loose_rows)
    for name in h:
        if name in ("xyz", "scaling"):
            assert _bits_equal(h[name][~loose], f[name][~loose]), (what, name)
            err = (h[name][loose].double() - f[name][loose].double()).abs().numpy()
            tol = xyz_tol if name == "xyz" else s_tol
            print(f"{what}: {name} of {int(loose.sum())} loose rows: max difference {err.max() if err.size else 0.0:.3e}, "
                  f"max difference / tolerance {(err / tol).max() if err.size else 0.0:.3f}")
            assert (err <= tol).all(), (what, name)
        else:
            assert _bits_equal(h[name], f[name]), (what, name)


def _state_np(m):
    return dict(scaling=m._scaling.detach().cpu().numpy(), opacity=m._opacity.detach().cpu().numpy(), rotation=m._rotation.detach().cpu().numpy(),
                xyz=m._xyz.detach().cpu().numpy(), grad_accum=m.xyz_gradient_accum.cpu().numpy(), denom=m.denom.cpu().numpy(),
                max_radii2D=m.max_radii2D.cpu().numpy())


def test_fused_model_follows_the_host_model():
    n = 70_001
    c = _case("mixed", n, 3)
    host, fused = cases.build_model(c, DEV, "host"), cases.build_model(c, DEV, "fused")
    for m in (host, fused):
        m.generator = torch.Generator().manual_seed(21)
    args = (c["max_grad"], c["min_opacity"], c["extent"], c["max_screen_size"])
    # ---- event 1
    o1 = _oracle("mixed", n, 3)
    noise1 = torch.randn((2 * o1["n_split_sel"], 3), generator=torch.Generator().manual_seed(21)).numpy()
    for m in (host, fused):
        m.densify_and_prune(*args)
    child, _, b_xyz, _, b_s = _children_reference(c, o1, noise1)
    n1 = o1["n_out"]
    assert host._xyz.shape[0] == fused._xyz.shape[0] == n1
    xyz_tol, s_tol = np.zeros((n1, 3)), np.zeros((n1, 3))
    xyz_tol[child], s_tol[child] = 2 * b_xyz, 2 * b_s         # both within the bound of the float64 value: twice it between them
    _compare_models(host, fused, child, xyz_tol[child], s_tol[child], "after the first densification")
    # ---- a prune
    mask = np.random.default_rng(1).random(n1) < 0.05
    for m in (host, fused):
        m.prune_points(torch.from_numpy(mask).to(DEV))
    keep = ~mask
    loose, xyz_tol, s_tol = child[keep], xyz_tol[keep], s_tol[keep]
    n2 = int(keep.sum())
    assert host._xyz.shape[0] == fused._xyz.shape[0] == n2
    _compare_models(host, fused, loose, xyz_tol[loose], s_tol[loose], "after prune_points")
    # ---- an optimiser step on gradients that do not depend on the parameters
    g = torch.Generator().manual_seed(3)
    for pa, pb in zip(host.parameters(), fused.parameters()):
        grad = (torch.rand(pa.shape, generator=g) - 0.5).to(DEV)
        pa.grad, pb.grad = grad, grad.clone()
    for m in (host, fused):
        m.optimizer.step()
        m.optimizer.zero_grad(set_to_none=True)
    # the update is the same number on both sides (same gradients, same moments); subtracting it rounds once: 2 eps |p| between them
    xyz_tol = xyz_tol + 4 * EPS * np.abs(host._xyz.detach().cpu().numpy())
    s_tol = s_tol + 4 * EPS * np.abs(host._scaling.detach().cpu().numpy())
    _compare_models(host, fused, loose, xyz_tol[loose], s_tol[loose], "after the optimiser step")
    # ---- event 2: statistics drawn once; rows that differ between the models take no part in the selection (they are kept or pruned)
    rng = np.random.default_rng(4)
    denom2 = rng.integers(0, 5, n2).astype(np.float32)
    accum2 = (np.exp(rng.uniform(np.log(1e-5), np.log(1e-2), n2)).astype(np.float32) * denom2).astype(np.float32)
    accum2[loose] = 0.0
    for m in (host, fused):
        m.xyz_gradient_accum, m.denom = _gpu(accum2.reshape(-1, 1)), _gpu(denom2.reshape(-1, 1))
    # the state is chosen so that no activated value of EITHER model sits on a threshold: entries that do are moved, alike in both
    bad_s = np.zeros((n2, 3), dtype=bool)
    bad_o = np.zeros((n2, 1), dtype=bool)
    for m in (host, fused):
        st = _state_np(m)
        vs, vo = cases.gap_violations(st["scaling"], st["opacity"], c)
        bad_s |= vs
        bad_o |= vo
    with torch.no_grad():
        for m in (host, fused):
            m._scaling.data += _gpu(bad_s.astype(np.float32)) * 0.001
            m._opacity.data += _gpu(bad_o.astype(np.float32)) * 0.001
    states = [_state_np(m) for m in (host, fused)]
    for st in states:
        cases.assert_gaps(st["scaling"], st["opacity"], c)
    o2 = [orc.densify_and_prune(st["scaling"], st["opacity"], st["max_radii2D"], st["grad_accum"], st["denom"], c["max_grad"], c["min_opacity"],
                                c["extent"], c["max_screen_size"], c["percent_dense"]) for st in states]
    assert all(np.array_equal(o2[0][k], o2[1][k]) for k in ("src", "kind", "noise_row"))      # with the gaps, both models decide alike
    o2 = o2[0]
    assert (o2["kind"] >= orc.SPLIT0).sum() > 100 and (o2["kind"] == orc.CLONE).sum() > 100
    gen_state = host.generator.get_state()
    assert torch.equal(gen_state, fused.generator.get_state())
    noise2 = torch.randn((2 * o2["n_split_sel"], 3), generator=_generator_from(gen_state)).numpy()
    for m in (host, fused):
        m.densify_and_prune(*args)
    case2 = dict(rotation=states[0]["rotation"], scaling=states[0]["scaling"], xyz=states[0]["xyz"])
    child2, _, b_xyz2, _, b_s2 = _children_reference(case2, o2, noise2)
    n3 = o2["n_out"]
    assert host._xyz.shape[0] == fused._xyz.shape[0] == n3
    assert not loose[o2["src"][child2]].any()                     # no child of a row that differed
    loose3 = loose[o2["src"]] | child2
    xyz_tol3, s_tol3 = xyz_tol[o2["src"]], s_tol[o2["src"]] + 4 * EPS * np.abs(states[0]["scaling"][o2["src"]])      # (the moved entries were rounded once more)
    xyz_tol3[child2], s_tol3[child2] = 2 * b_xyz2, 2 * b_s2
    _compare_models(host, fused, loose3, xyz_tol3[loose3], s_tol3[loose3], "after the second densification")
    assert torch.equal(host.generator.get_state(), fused.generator.get_state())
    assert torch.equal(host.unique_kfIDs, fused.unique_kfIDs) and torch.equal(host.n_obs, fused.n_obs)


def _generator_from(state):
    g = torch.Generator()
    g.set_state(state)
    return g


# ---------------------------------------------------------------- 5. the pruning pass
@pytest.mark.parametrize("prune_mode,initialized", [("slam", True), ("slam", False), ("odometry", True), ("odometry", False)])
def test_pruning_pass(prune_mode, initialized):
    from lvdgs import backend_map
    n = 70_001
    c = _case("mixed", n, 3)
    window = [11, 9, 8, 6, 5, 3, 2, 0]
    rng = np.random.default_rng(7)
    touched = (rng.random((8, n)) < 0.3)
    results = []
    for mode in ("host", "fused"):
        G = cases.build_model(c, DEV, mode)
        flags = _gpu(touched.astype(np.uint8)).long()           # as map_window leaves them: rows of one int64 tensor
        backend = types.SimpleNamespace(occ_aware_visibility={k: flags[i] for i, k in enumerate(window)}, initialized=initialized, monocular=True)
        ctx = types.SimpleNamespace(backend=backend, G=G, sharder=None, n_window=8, window=list(window),
                                    cfg={"Training": {"window_size": 8, "prune_mode": prune_mode, "prune_num": 2}})
        waits = _count_waits(lambda: backend_map._pruning_pass(ctx))
        assert backend.initialized and waits == (1 if mode == "fused" else 0)
        results.append((G, backend))
    (hG, hb), (fG, fb) = results
    o, n_obs = orc.pruning_pass(list(touched), c["kf_ids"], prune_mode, 2, window, initialized)
    assert 0 < o["n_out"] < n and hG._xyz.shape[0] == fG._xyz.shape[0] == o["n_out"]
    _compare_models(hG, fG, np.zeros(o["n_out"], dtype=bool), 0.0, 0.0, "the pruning pass")
    assert np.array_equal(fG.n_obs.numpy(), n_obs[o["src"]]) and fG.n_obs.dtype == hG.n_obs.dtype
    assert np.array_equal(fG.unique_kfIDs.numpy(), c["kf_ids"][o["src"]])
    for k in window:
        assert hb.occ_aware_visibility[k].dtype == fb.occ_aware_visibility[k].dtype and torch.equal(hb.occ_aware_visibility[k], fb.occ_aware_visibility[k]), k
        assert np.array_equal(fb.occ_aware_visibility[k].cpu().numpy(), touched[window.index(k)][o["src"]].astype(np.int64))


# ---------------------------------------------------------------- 6. one wait, the same bytes twice
def _count_waits(fn):
    from lvdgs import map_edit
    calls, real = [], map_edit._plan.wait
    map_edit._plan.wait = lambda device: (calls.append(device), real(device))[1]
    try:
        fn()
    finally:
        del map_edit._plan.wait
    return len(calls)


def test_one_wait_and_the_same_bytes_twice():
    n = 1025
    c = _case("mixed", n, 3, 3)
    models = [cases.build_model(c, DEV, "fused") for _ in range(2)]
    for m in models:
        m.generator = torch.Generator().manual_seed(9)
        assert _count_waits(lambda: m.densify_and_prune(c["max_grad"], c["min_opacity"], c["extent"], c["max_screen_size"])) == 1
        assert _count_waits(lambda: m.prune_points(torch.zeros(m._xyz.shape[0], dtype=torch.bool, device=DEV))) == 1
    a, b = (cases.model_tensors(m) for m in models)
    o = orc.densify_and_prune(c["scaling"], c["opacity"], c["max_radii2D"], c["grad_accum"], c["denom"], c["max_grad"], c["min_opacity"],
                              c["extent"], c["max_screen_size"], c["percent_dense"])
    assert a["xyz"].shape[0] == o["n_out"] and a["f_rest"].shape == (o["n_out"], 15, 3)
    for name in a:
        assert _bits_equal(a[name], b[name]), name
    # degree 3: f_rest rows of 180 bytes and their moments travelled too
    assert np.array_equal(a["f_rest"].numpy(), c["f_rest"][o["src"]])
    assert np.array_equal(a["exp_avg_f_rest"].numpy(), orc.materialise(c["exp_avg_f_rest"], o["src"], o["kind"], zero_new=True))


# ---------------------------------------------------------------- 7. the sequence
def test_toy_sequence_with_fused_map_edits():
    import sequence_scene as ss
    from lvdgs.slam_sequence import SlamSequence
    cfg, ds, _, _, _ = ss.toy_sequence_on_cpu()
    ds = ds.to("cuda")
    runs = {}
    for mode in ("host", "fused"):
        torch.manual_seed(0)
        random.seed(0)
        seq = SlamSequence(cfg, ds, ss.empty_map(cfg, "cuda"), ss.PIPE, torch.zeros(3, device="cuda"), idle_map_iters=2, map_edit=mode).run()
        assert seq.gaussians.map_edit == mode
        runs[mode] = dict(seq=seq, ate=seq.eval_ate())
    h, f = runs["host"], runs["fused"]
    hc, fc = h["seq"].gaussian_counts, f["seq"].gaussian_counts
    print({k: (v["ate"], v["seq"].kf_indices, v["seq"].gaussian_counts[:12]) for k, v in runs.items()})
    # Up to and including the first densification the two drives go through the same events with the same map sizes; from then on split
    # children differ in their last bits and the drives are two drives.
    k = [i for i, (e, _) in enumerate(hc) if e == "densify"][0] + 1
    assert fc[:k] == hc[:k], (fc[:k + 4], hc[:k + 4])
    assert f["ate"] < 0.03, f["ate"]
