"""The float64 oracles of the loss / Adam / isotropic / statistics kernels (step_oracle.py), pinned without a GPU:

* against float64 ``torch.autograd`` / ``torch.optim.Adam`` on the statements the reference runs (step_oracle.torch_*);
* against the fixtures the reference itself wrote (tests/golden/loss_tracking.npz, loss_mapping.npz);
* the cases' conditions (step_cases.py);
* the a-priori error bounds (step_oracle.*_bounds, derived in test_gpu_step_kernels.py) applied to the float32 PyTorch statements on
  the CPU: an independent float32 evaluation of the same mathematics has to fit them, or the derivation is wrong.
"""
import functools
import os

import numpy as np
import pytest

import step_cases as cases
import step_oracle as orc

EPS = orc.EPS
f32, f64 = np.float32, np.float64
CPU_LOSS_SIZES = cases.LOSS_SIZES[:7] + ((516, 512),)       # 513 x 513 adds nothing to a CPU statement that knows no 16-byte path


def ratio(err, bound):
    """max over the elements of err / bound, 0 / 0 = 0 (an exact result where an exact result is due), x / 0 = inf."""
    err, bound = np.abs(np.asarray(err, f64)), np.asarray(bound, f64) + np.zeros_like(err)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0, 0.0, err / bound)
    return float(q.max()) if q.size else 0.0


@functools.lru_cache(maxsize=None)
def _loss(W, H, config):
    c = cases.loss_case(W, H, config)
    return c, orc.photometric(**cases.loss_oracle_args(c))


# ---------------------------------------------------------------- the oracles against float64 autograd / Adam
@pytest.mark.parametrize("config", list(cases.LOSS_CONFIGS))
@pytest.mark.parametrize("W,H", CPU_LOSS_SIZES[:7])
def test_photometric_oracle_is_float64_autograd_of_the_statement(W, H, config):
    import torch
    c, o = _loss(W, H, config)
    t = orc.torch_photometric(torch.float64, **cases.loss_oracle_args(c))
    np.testing.assert_allclose(o["value"], t["value"], rtol=1e-13, atol=0)
    for k in ("d_image", "d_depth", "d_opacity"):
        np.testing.assert_allclose(o[k], t[k], rtol=1e-12, atol=0, err_msg=k)
        assert np.array_equal(o[k] == 0, t[k] == 0), k
    np.testing.assert_allclose([o["d_a"], o["d_b"]], [t["d_a"], t["d_b"]], rtol=1e-11, atol=1e-18)


GOLDEN_LOSSES = (   # fixture, entry, the header's configuration of it
    ("loss_tracking", "mono", dict(weight_rgb=1.0, weight_by_opacity=1, mask=True, depth=False)),
    ("loss_tracking", "mono_depthloss", dict(weight_rgb=1.0, weight_by_opacity=1, mask=True, depth=False)),
    ("loss_tracking", "rgbd", dict(weight_rgb=0.98, weight_depth=0.02, weight_by_opacity=1, depth_needs_opaque=1, mask=True, depth=True)),
    ("loss_mapping", "mono_nodepth", dict(weight_rgb=1.0, depth=False)),
    ("loss_mapping", "mono_monodepth", dict(weight_rgb=0.98, weight_depth=0.02, depth=True)),
    ("loss_mapping", "rgbd", dict(weight_rgb=0.98, weight_depth=0.02, depth=True)),
    ("loss_mapping", "init", dict(weight_rgb=0.98, weight_depth=0.02, depth=True, exposure=False)),
)


@pytest.mark.parametrize("fixture,entry,cfg", GOLDEN_LOSSES)
def test_photometric_oracle_against_the_reference_fixtures(golden_dir, fixture, entry, cfg):
    """What the reference's own get_loss_tracking / get_loss_mapping + autograd gave in float32 (tests/golden/make_golden.py)."""
    g = np.load(os.path.join(golden_dir, fixture + ".npz"))
    cfg = dict(cfg)
    has_mask, has_depth, has_exp = cfg.pop("mask", False), cfg.pop("depth"), cfg.pop("exposure", True)
    P = g["image"][0].size
    o = orc.photometric(g["image"].reshape(3, P), g["gt"].reshape(3, P), depth=g["depth"].reshape(P) if has_depth else None,
                        gt_depth=g["mono_depth"].reshape(P) if has_depth else None, opacity=g["opacity"].reshape(P),
                        grad_mask=g["grad_mask"].reshape(P).astype(np.uint8) if has_mask else None,
                        exposure_a=g["exposure_a"][0] if has_exp else None, exposure_b=g["exposure_b"][0] if has_exp else None, rgb_thr=0.01, **cfg)
    np.testing.assert_allclose(o["value"], g[entry + ".loss"], rtol=1e-6)
    np.testing.assert_allclose(o["d_image"], g[entry + ".d_image"].reshape(3, P), rtol=1e-5, atol=1e-12)
    np.testing.assert_allclose(o["d_depth"], g[entry + ".d_depth"].reshape(P), rtol=1e-5, atol=1e-12)
    np.testing.assert_allclose(o["d_opacity"], g[entry + ".d_opacity"].reshape(P), rtol=1e-5, atol=1e-10)
    if has_exp:
        np.testing.assert_allclose([o["d_a"], o["d_b"]], [g[entry + ".d_a"][0], g[entry + ".d_b"][0]], rtol=1e-5)


@pytest.mark.parametrize("n", cases.ISO_SIZES)
def test_isotropic_oracle_is_float64_autograd_of_the_statement(n):
    import torch
    c = cases.iso_case(n)
    value, grad, ex = orc.isotropic(c["raw"], c["weight"], c["grad_in"])
    tv, tg = orc.torch_isotropic(torch.float64, c["raw"], c["weight"], c["grad_in"])
    np.testing.assert_allclose(value, tv, rtol=1e-13, atol=0)
    np.testing.assert_allclose(grad, tg, rtol=1e-12, atol=1e-22)
    if n:
        assert np.array_equal(grad[ex["equal"]], c["grad_in"][ex["equal"]].astype(f64))     # bit-equal rows: nothing is added
    assert orc.isotropic(c["raw"], c["weight"], None)[1] is None


@pytest.mark.parametrize("name", cases.ADAM_LISTS)
def test_adam_oracle_is_float64_torch_adam(name):
    """With the scalars left unrounded the oracle IS torch.optim.Adam's single-tensor step in float64; the header's rounding of the six
    scalars to float32 then moves nothing by more than a few 2^-24 relative."""
    import torch
    for t in cases.adam_list(name):
        n, o = t["numel"], t["offset"]
        args = [t[k][o:o + n] for k in ("param", "grad", "exp_avg", "exp_avg_sq")] + [t["step"], t["lr"], cases.ADAM_BETA1, cases.ADAM_BETA2, cases.ADAM_EPS]
        p1, m1, v1, _ = orc.adam(*args, round_scalars=False)
        tp, tm, tv = orc.torch_adam(torch.float64, *args)
        rp, rm, rv, ex = orc.adam(*args)
        assert (np.abs(m1 - tm) <= 1e-15 * ex["m_terms"]).all()            # (the lerp cancels: relative to its operands)
        np.testing.assert_allclose(v1, tv, rtol=1e-14, atol=0)
        assert (np.abs(p1 - tp) <= 1e-15 * np.abs(p1) + 1e-13 * np.abs(ex["update"])).all()
        assert (np.abs(rm - m1) <= 2 * EPS * ex["m_terms"]).all() and (np.abs(rv - v1) <= 2 * EPS * v1).all()
        assert (np.abs(rp - p1) <= 8 * EPS * np.abs(ex["update"]) + np.abs(ex["step_size"] / ex["denom"]) * 2 * EPS * ex["m_terms"]).all()
        assert np.array_equal(rp[t["still"]], args[0][t["still"]].astype(f64))              # zero gradient, zero moments: unmoved


def _stats_reference(c, views):
    """The statistics of ``views`` in PyTorch statements (slam_backend.py:311-315, :350-357, float64) -- the oracle's counterpart."""
    import torch
    rmax = torch.from_numpy(c["radii_max0"].astype(np.int64))
    vis_count = torch.from_numpy(c["vis_count0"].astype(f64))
    touched = []
    for v in views:
        radii = torch.from_numpy(v["radii"].astype(np.int64))
        vis = radii > 0
        rmax[vis] = torch.max(rmax[vis], radii[vis])
        vis_count[vis] += 1
        touched.append((torch.from_numpy(v["n_touched"]) > 0).long().numpy())
    return rmax.numpy(), orc.torch_norm_sum(torch.float64, c["norm_sum0"], views), vis_count.numpy(), touched


@pytest.mark.parametrize("n", cases.STATS_SIZES)
def test_statistics_oracle_is_the_backends_bookkeeping(n):
    c = cases.stats_case(n)
    st = dict(radii_max=c["radii_max0"], norm_sum=c["norm_sum0"].astype(f64), vis_count=c["vis_count0"].astype(f64))
    touched = []
    for v in c["views"]:
        st, tr, _ = orc.view_stats(v["radii"], v["n_touched"], v["grad"], st)
        touched.append(tr)
    rmax, norm, cnt, tch = _stats_reference(c, c["views"])
    assert np.array_equal(st["radii_max"], rmax) and np.array_equal(st["vis_count"], cnt)
    np.testing.assert_allclose(st["norm_sum"], norm, rtol=1e-14, atol=0)
    assert all(np.array_equal(a, b) for a, b in zip(touched, tch))
    assert np.isfinite(st["norm_sum"]).all() and (st["norm_sum"] < 1e3).all()                # the 1e30 column was never read
    # split: the xy of the visible rows, zero elsewhere; NULL pointers leave their accumulator alone
    v = c["views"][0]
    st2, tr, split = orc.view_stats(v["radii"], None, v["grad"], dict(radii_max=c["radii_max0"], norm_sum=None, vis_count=None), use_split=True)
    assert tr is None and st2["norm_sum"] is None and st2["vis_count"] is None
    assert np.array_equal(split, np.where((v["radii"] > 0)[:, None], v["grad"][:, :2].astype(f64), 0.0))
    _, _, none = orc.view_stats(v["radii"], None, None, dict(radii_max=c["radii_max0"], norm_sum=None, vis_count=None), use_split=True)
    assert not none.any()
    # the way into the model
    for n_split in (0, 1, 3):
        planes = np.stack([orc.view_stats(w["radii"], None, w["grad"], st2, use_split=True)[2] for w in c["views"][:n_split]]) if n_split else np.zeros((0, n, 2))
        mr, acc, den, _ = orc.map_stats_apply(st["radii_max"], st["norm_sum"].astype(f32), st["vis_count"], planes, c["max_radii2D0"], c["grad_accum0"], c["denom0"])
        want = c["grad_accum0"].astype(f64) + st["norm_sum"].astype(f32).astype(f64) + sum(np.hypot(p[:, 0], p[:, 1]) for p in planes)
        np.testing.assert_allclose(acc, want, rtol=1e-14, atol=0)
        assert np.array_equal(mr, np.maximum(c["max_radii2D0"].astype(f64), st["radii_max"])) and np.array_equal(den, c["denom0"] + st["vis_count"])


# ---------------------------------------------------------------- the cases
def test_loss_cases_hold_their_conditions_and_their_placed_rows():
    seen = set()
    for W, H in cases.LOSS_SIZES:
        for config in cases.LOSS_CONFIGS:
            c = cases.loss_case(W, H, config)          # asserts its conditions on the way out
            cases.assert_loss_conditions(c)
            seen.update(name for name, _ in c["placed"])
            if W * H >= 22:
                assert {name for name, _ in c["placed"]} == set(cases.PLACED)
                assert any(p >= c["P"] - len(cases.PLACED) for _, p in c["placed"])             # ... once more in the last lanes
    assert seen == set(cases.PLACED)
    assert sorted(W * H for W, H in cases.LOSS_SIZES)[:7] == [1, 3, 4, 5, 1023, 1024, 1025]
    tiny = {name for W, H in cases.LOSS_SIZES[:4] for config in cases.LOSS_CONFIGS for name, _ in cases.loss_case(W, H, config)["placed"]}
    assert tiny == set(cases.PLACED)                       # the 1- to 5-pixel images see every placed row between them
    c = cases.loss_case(33, 31, "no_exposure")
    p = dict(c["placed"])["i_eq_g"]
    o = orc.photometric(**cases.loss_oracle_args(c))
    assert not o["d_image"][:, p].any() and o["d_opacity"][p] == 0.0          # residual exactly zero: sign(0) = 0
    # the placed pairs decide differently, one float apart
    c = cases.loss_case(33, 31, "tracking_rgbd")
    o, pl = orc.photometric(**cases.loss_oracle_args(c)), dict(c["placed"])
    assert not o["d_image"][:, pl["g_tie"]].any() and o["d_image"][:, pl["g_in"]].all()
    assert o["d_depth"][pl["z_tie"]] == 0 and o["d_depth"][pl["z_in"]] != 0 and o["d_depth"][pl["o_tie"]] == 0 and o["d_depth"][pl["o_in"]] != 0
    assert not o["d_image"][:, pl["mask0"]].any() and all(o["d_image"][:, pl[k]].all() for k in ("mask1", "mask2", "mask255"))


def test_isotropic_adam_and_statistics_cases_hold_their_conditions():
    for n in cases.ISO_SIZES:
        assert cases.iso_condition(cases.iso_case(n)["raw"]).all()
    for name in cases.ADAM_LISTS:
        for t in cases.adam_list(name):
            n, o = t["numel"], t["offset"]
            assert all(t[k].size == o + n + cases.ADAM_GUARD and (t[k][o + n:] == cases.ADAM_GUARD_VALUE).all() for k in ("param", "grad", "exp_avg", "exp_avg_sq"))
            g = t["grad"][o:o + n]
            assert not g[t["still"]].any() and not t["exp_avg"][o:o + n][t["still"]].any() and not t["exp_avg_sq"][o:o + n][t["still"]].any()
    eight = cases.adam_list("eight")
    assert len(eight) == 8 and eight[3]["numel"] == 0 and len({t["step"] for t in eight}) >= 4 and len({t["lr"] for t in eight}) == 8
    assert cases.adam_list("unaligned")[0]["offset"] == 1 and cases.adam_list("unaligned")[0]["numel"] % 4 == 0
    for n in cases.STATS_SIZES:
        c = cases.stats_case(n)
        assert len(c["views"]) == 13 and all((v["grad"][:, 2] == cases.UNREAD).all() for v in c["views"])


# ---------------------------------------------------------------- the bounds, held by the float32 PyTorch statements on the CPU
@pytest.mark.parametrize("config", list(cases.LOSS_CONFIGS))
@pytest.mark.parametrize("W,H", CPU_LOSS_SIZES)
def test_float32_statement_of_the_loss_fits_the_bounds(W, H, config):
    import torch
    c, o = _loss(W, H, config)
    t = orc.torch_photometric(torch.float32, **cases.loss_oracle_args(c))
    b = orc.photometric_bounds(o)
    worst = {k: ratio(t[k] - o[k], b[k]) for k in ("value", "d_a", "d_b", "d_image", "d_depth", "d_opacity")}
    print(f"loss {W}x{H} {config}: achieved/allowed " + " ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst
    for k in ("d_image", "d_depth", "d_opacity"):
        assert not t[k][o[k] == 0].any(), k


@pytest.mark.parametrize("n", cases.ISO_SIZES)
def test_float32_statement_of_the_isotropic_term_fits_the_bounds(n):
    import torch
    c = cases.iso_case(n)
    value, grad, ex = orc.isotropic(c["raw"], c["weight"], c["grad_in"])
    tv, tg = orc.torch_isotropic(torch.float32, c["raw"], c["weight"], c["grad_in"])
    bv, bg = orc.isotropic_bounds(ex, n, c["grad_in"])
    rv, rg = ratio(tv - value, bv), ratio(tg - grad, bg) if n else 0.0
    print(f"isotropic n={n}: achieved/allowed value {rv:.3f} grad {rg:.3f}")
    assert rv <= 1.0 and rg <= 1.0


@pytest.mark.parametrize("name", cases.ADAM_LISTS)
def test_float32_torch_adam_fits_the_bounds(name):
    import torch
    for t in cases.adam_list(name):
        n, o = t["numel"], t["offset"]
        args = [t[k][o:o + n] for k in ("param", "grad", "exp_avg", "exp_avg_sq")] + [t["step"], t["lr"], cases.ADAM_BETA1, cases.ADAM_BETA2, cases.ADAM_EPS]
        p1, m1, v1, ex = orc.adam(*args)
        tp, tm, tv = orc.torch_adam(torch.float32, *args)
        bp, bm, bv = orc.adam_bounds(p1, m1, v1, ex)
        r = (ratio(tp - p1, bp), ratio(tm - m1, bm), ratio(tv - v1, bv))
        print(f"adam {name} numel={n} step={t['step']}: achieved/allowed param {r[0]:.3f} exp_avg {r[1]:.3f} exp_avg_sq {r[2]:.3f}")
        assert max(r) <= 1.0, r
        assert np.array_equal(tp[t["still"]], args[0][t["still"]].astype(f64))


@pytest.mark.parametrize("n", cases.STATS_SIZES)
def test_float32_statement_of_norm_sum_fits_the_bound(n):
    import torch
    c = cases.stats_case(n)
    st = dict(radii_max=c["radii_max0"], norm_sum=c["norm_sum0"].astype(f64), vis_count=None)
    for v in c["views"]:
        st, _, _ = orc.view_stats(v["radii"], None, v["grad"], st)
    got = orc.torch_norm_sum(torch.float32, c["norm_sum0"], c["views"])
    r = ratio(got - st["norm_sum"], EPS * st["norm_err"]) if n else 0.0
    print(f"norm_sum n={n}: achieved/allowed {r:.3f}")
    assert r <= 1.0
