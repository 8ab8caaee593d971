"""The four small kernel families of a tracking / mapping iteration -- photometric loss, the map's Adam step, the isotropic regulariser,
the per-view statistics and their way into the model -- through the raw C ABI against float64 oracles (step_oracle.py) on seeded cases
whose decisions do not hang on a rounding (step_cases.py).  Integers, flags, counts and copied floats are exact; every float32 result
is held to 1 x an a-priori bound, eps = 2^-24 (half an ulp, relative: one rounding of + - * / sqrt; expf 2 eps).  The same bounds are
held by the float32 PyTorch statements on the CPU in test_step_oracle.py, which is the check of these derivations:

LOSS.  r_c = (e^a I_c + b) m - G_c m, m in {0, 1}.  e^a carries 2 eps, the product 1, the two additions 1 each:
  |err r_c| <= 5 eps A_c,  A_c = m (|e^a I_c| + |b| + |G_c|).  The cases keep |r_c| >= 2^-18 A_c, so sign(r_c) is the oracle's.
  * d_image = (w/(3P) g) omega sign e^a: 3P, the division and g (3), omega (1), e^a (1 + 2): <= 8 eps |ref|.  d_depth: 3 <= 8 eps |ref|.
  * d_opacity = W_r sum_c |r_c| is NOT relative to its value -- r_c cancels.  3 eps for W_r, 1 for the product, 2 for the sum and the
    residuals' own error: <= 8 eps |ref| + 5 eps |W_r| sum_c A_c.  (The issue's 8 eps |ref| alone holds for d_image and d_depth only.)
  * value: a term omega sum_c |r_c| errs by <= 5 eps omega sum A + 3 eps omega sum |r| <= 8 eps omega sum_c A_c; the final
    s / (3 P) * w + depth part adds 4: r = 12 on sum|t| = sum omega A (the operands, since the residual cancels), n = 3P; the depth sum:
    r = 1 + 4 on sum |D k - Z k|, n = P.  d_a: terms q e^a I, r = 3 + 1 + 3 + 3 = 10; d_b: r = 3 + 1 + 2 = 6; n = 3P.
  Summed results are allowed max(4 x the error of the float32 PyTorch statement on the CPU, (ceil(log2 n) + 8 + r) eps sum|t|).
  Gradients are exactly 0 where the oracle's are.
ADAM.  exp_avg' = m + w1 (g - m): <= 3 eps (|m| + |w1 g| + |w1 m|) =: E_m.  exp_avg_sq' (all terms positive, 4 roundings): <= 4 eps v'.
  The update u = step_size m' / (sqrt(v') / bc2 + eps): sqrt(v') 2 + 1, the division 1, + eps 1, m' / denom 1, step_size 1: 7 eps |u|, and
  p - u rounds: eps |p'|.  But m' itself cancels, so its error is not relative to it: + |step_size / denom| E_m on top of the issue's
  eps |p'| + 8 eps |u|.
ISOTROPIC.  Gradient term = scale (g_k - mean g) s_k, |g_k - mean g| <= 4/3: scale 2, the mean and the difference 2, two products 2, expf 2,
  and grad_in + term rounds once: <= eps (|grad_in| + 12 scale s_k)  (9 roundings x 4/3; the issue's 8 scale s_k leaves the 4/3 out).
  Bit-equal rows: exactly grad_in.  Value: per row <= 11 eps sum_k s_k, the final product with scale 3: r = 14 on sum s, n = 3N.
STATISTICS.  norm_sum: <= eps (3 t_v + |S_v|) per added view (t_v > 0).  xyz_gradient_accum: the same per split plane plus eps |accum'|.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import step_cases as cases
import step_oracle as orc
from lvdgs import _lib

pytestmark = pytest.mark.gpu
EPS = orc.EPS
DEV = "cuda:0"
f32, f64 = np.float32, np.float64
GUARD, SENT = 8, -77.25          # floats behind every output, and what they (and every output) hold before a call


def ratio(err, bound):
    err, bound = np.abs(np.asarray(err, f64)), np.asarray(bound, f64) + np.zeros_like(err)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0, 0.0, err / bound)
    return float(q.max()) if q.size else 0.0


def report(kernel, what, **ratios):
    print(f"RATIO {kernel} [{what}] achieved/allowed " + " ".join(f"{k} {v:.4f}" for k, v in ratios.items()))
    assert all(v <= 1.0 for v in ratios.values()), (kernel, what, ratios)


def _stream():
    return _lib.raw_stream(torch.device(DEV))


class Buf:
    """``lead`` elements, the data, GUARD elements on the device; ``ptr`` addresses the data."""

    def __init__(self, data=None, n=None, dtype=np.float32, lead=0, fill=None):
        n = int(np.asarray(data).size if data is not None else n)
        fill = fill if fill is not None else (SENT if dtype is np.float32 else 99 if dtype is np.uint8 else -7)
        host = np.full(lead + n + GUARD, fill, dtype)
        if data is not None:
            host[lead:lead + n] = np.asarray(data, dtype).reshape(-1)
        self.n, self.lead, self.fill, self.t = n, lead, dtype(fill), torch.from_numpy(host).to(DEV)
        self.ptr = C.c_void_p(self.t.data_ptr() + lead * host.itemsize)

    def get(self):
        """The data; asserts that nothing before or behind it was written."""
        h = self.t.cpu().numpy()
        assert (h[:self.lead] == self.fill).all() and (h[self.lead + self.n:] == self.fill).all(), "wrote outside its buffer"
        return h[self.lead:self.lead + self.n].copy()

    def untouched(self):
        return bool((self.t.cpu().numpy() == self.fill).all())


# ================================================================================================ photometric loss
@functools.lru_cache(maxsize=None)
def _loss_reference(W, H, config):
    """The case, the oracle, the bounds and the float32 CPU statement's own error on the summed results -- computed once."""
    c = cases.loss_case(W, H, config)
    args = cases.loss_oracle_args(c)
    o = orc.photometric(**args)
    t = orc.torch_photometric(torch.float32, **args)
    b = orc.photometric_bounds(o)
    for k in ("value", "d_a", "d_b"):
        b[k] = max(b[k], 4.0 * abs(t[k] - o[k]))
    return c, o, b


def _loss_outputs(P, lead):
    return dict(loss=Buf(n=1), d_image=Buf(n=3 * P, lead=lead), d_depth=Buf(n=P, lead=lead), d_opacity=Buf(n=P, lead=lead), d_a=Buf(n=1), d_b=Buf(n=1))


def _run_loss(c, lead=0):
    """forward, backward, value_and_grad (twice) on the case -> {entry: {output: array or None where NULL was passed}}."""
    L, cfg, P = _lib.lib(), c["cfg"], c["P"]
    plane = lambda a, dtype=np.float32: None if a is None else Buf(a, dtype=dtype, lead=lead)
    inp = dict(image=plane(c["image"]), gt_image=plane(c["gt_image"]), depth=plane(c["depth"]), gt_depth=plane(c["gt_depth"]), opacity=plane(c["opacity"]),
               grad_mask=plane(c["grad_mask"], np.uint8), exposure_a=None if c["exposure_a"] is None else Buf([c["exposure_a"]]),
               exposure_b=None if c["exposure_b"] is None else Buf([c["exposure_b"]]))
    if lead:
        assert all(b.ptr.value % 16 == 4 for k, b in inp.items() if b is not None and k not in ("grad_mask", "exposure_a", "exposure_b"))
        assert inp["grad_mask"] is None or inp["grad_mask"].ptr.value % 4 == 1
    g_given = Buf([c["grad_loss"] if c["grad_loss"] is not None else 1.0])
    scratch = _lib.device_bytes(L.lvdgs_loss_scratch_bytes(c["W"], c["H"]), DEV)
    results = {}
    for entry in ("forward", "backward", "value_and_grad", "value_and_grad_again"):
        out = _loss_outputs(P, lead)
        la = _lib.LossArgs()
        la.width, la.height = c["W"], c["H"]
        for k, b in inp.items():
            setattr(la, k, None if b is None else b.ptr)
        la.rgb_boundary_threshold, la.weight_rgb, la.weight_depth = c["rgb_thr"], cfg["weight_rgb"], cfg["weight_depth"]
        la.weight_by_opacity, la.depth_needs_opaque = cfg["weight_by_opacity"], cfg["depth_needs_opaque"]
        la.scratch, la.scratch_bytes = C.c_void_p(scratch.data_ptr()), scratch.numel()
        passed = {"loss", "d_image"} | ({"d_depth", "d_opacity", "d_a", "d_b"} if cfg["optional_outputs"] else set())
        la.loss, la.d_image = out["loss"].ptr, out["d_image"].ptr
        if cfg["optional_outputs"]:
            la.d_depth, la.d_opacity, la.d_exposure_a, la.d_exposure_b = out["d_depth"].ptr, out["d_opacity"].ptr, out["d_a"].ptr, out["d_b"].ptr
        # backward needs the device scalar; value_and_grad takes NULL for 1 where the case has none
        la.grad_loss = g_given.ptr if (entry == "backward" or c["grad_loss"] is not None) else None
        fn = getattr(L, "lvdgs_photometric_loss_" + entry.replace("_again", ""))
        _lib.check(fn(C.byref(la), _stream()), entry)
        torch.cuda.synchronize()
        written = {"forward": {"loss"}, "backward": passed - {"loss"}}.get(entry, passed)
        res = {}
        for k, b in out.items():
            if k in written:
                res[k] = b.get()               # (asserts the guards: nothing behind P, nothing before the plane)
            else:
                assert b.untouched(), f"{entry} wrote {k}"         # NULL, or not this entry point's to write
                res[k] = None
        results[entry] = res
    return results


def _check_loss(c, o, b, res, what):
    fwd, bwd, vag, again = (res[k] for k in ("forward", "backward", "value_and_grad", "value_and_grad_again"))
    for k, v in vag.items():                  # one pass = the two passes, and the same bits every time
        two = fwd[k] if k == "loss" else bwd[k]
        assert (v is None) == (two is None) and (v is None or (np.array_equal(v.view(np.int32), two.view(np.int32)) and np.array_equal(v.view(np.int32), again[k].view(np.int32)))), k
    ratios = dict(value=ratio(vag["loss"][0] - o["value"], b["value"]), d_image=ratio(vag["d_image"].reshape(3, -1) - o["d_image"], b["d_image"]))
    assert not vag["d_image"].reshape(3, -1)[o["d_image"] == 0].any()
    for k, ok in (("d_depth", "d_depth"), ("d_opacity", "d_opacity")):
        if vag[k] is not None:
            ratios[k] = ratio(vag[k] - o[ok], b[ok])
            assert not vag[k][o[ok] == 0].any(), k
    for k in ("d_a", "d_b"):
        if vag[k] is not None:
            ratios[k] = ratio(vag[k][0] - o[k], b[k])
    report("photometric", what, **ratios)


@pytest.mark.parametrize("config", list(cases.LOSS_CONFIGS))
@pytest.mark.parametrize("W,H", cases.LOSS_SIZES)
def test_photometric_loss_against_the_oracle(W, H, config):
    c, o, b = _loss_reference(W, H, config)
    _check_loss(c, o, b, _run_loss(c), f"{W}x{H} {config}")


@pytest.mark.parametrize("config", ("tracking_rgbd", "mapping_rgbd", "no_optional_outputs"))
@pytest.mark.parametrize("W,H", ((2, 2), (32, 32), (516, 512)))
def test_photometric_loss_on_planes_one_float_into_their_buffers(W, H, config):
    """P % 4 == 0 and every plane at an address that is 4 modulo 16 (the mask: 1 modulo 4): lvdgs_loss_args promises no alignment, so
    the same oracle holds -- and the elements before and behind every output plane stay as they were."""
    c, o, b = _loss_reference(W, H, config)
    _check_loss(c, o, b, _run_loss(c, lead=1), f"{W}x{H} {config} unaligned")


# ================================================================================================ isotropic regulariser
def _run_iso(c, with_grad=True, short=0):
    L, n = _lib.lib(), c["n"]
    raw, grad, loss = Buf(c["raw"]), Buf(c["grad_in"]), Buf(n=1)
    nbytes = L.lvdgs_isotropic_scratch_bytes(n)
    scratch = _lib.device_bytes(nbytes, DEV)
    status = L.lvdgs_isotropic_reg(n, raw.ptr if n else None, grad.ptr if with_grad else None, c["weight"], C.c_void_p(scratch.data_ptr()), nbytes - short,
                                   loss.ptr, _stream())
    torch.cuda.synchronize()
    return status, loss, grad


@pytest.mark.parametrize("n", cases.ISO_SIZES)
def test_isotropic_reg_against_the_oracle(n):
    import torch as _t
    c = cases.iso_case(n)
    value, grad, ex = orc.isotropic(c["raw"], c["weight"], c["grad_in"])
    status, loss, out = _run_iso(c)
    assert status == _lib.OK
    got_v, got_g = loss.get()[0], out.get().reshape(-1, 3)
    if n == 0:
        assert got_v == 0.0 and not np.signbit(got_v)
        return
    bv, bg = orc.isotropic_bounds(ex, n, c["grad_in"])
    bv = max(bv, 4.0 * abs(orc.torch_isotropic(_t.float32, c["raw"], c["weight"], None)[0] - value))
    report("isotropic", f"n={n}", value=ratio(got_v - value, bv), grad=ratio(got_g - grad, bg))
    assert np.array_equal(got_g[ex["equal"]].view(np.int32), c["grad_in"][ex["equal"]].view(np.int32))      # bit-equal scales: gradient exactly 0
    # the same bits again; grad = NULL: the same value, nothing written
    status2, loss2, out2 = _run_iso(c)
    assert status2 == _lib.OK and loss2.get()[0].tobytes() == got_v.tobytes() and np.array_equal(out2.get().view(np.int32), out.get().view(np.int32))
    status3, loss3, out3 = _run_iso(c, with_grad=False)
    assert status3 == _lib.OK and loss3.get()[0].tobytes() == got_v.tobytes() and np.array_equal(out3.get(), c["grad_in"].reshape(-1))
    # scratch one byte short: refused, nothing written
    status4, loss4, out4 = _run_iso(c, short=1)
    assert status4 == _lib.E_INVALID and loss4.untouched() and np.array_equal(out4.get(), c["grad_in"].reshape(-1))


# ================================================================================================ Adam
@pytest.mark.parametrize("name", cases.ADAM_LISTS)
def test_adam_step_against_the_oracle(name):
    L = _lib.lib()
    tensors = cases.adam_list(name)
    arr = (_lib.AdamTensor * len(tensors))()
    bufs = []
    for k, t in enumerate(tensors):
        b = {key: torch.from_numpy(t[key].copy()).to(DEV) for key in ("param", "grad", "exp_avg", "exp_avg_sq")}
        bufs.append(b)
        for key in b:
            setattr(arr[k], key, C.c_void_p(b[key].data_ptr() + 4 * t["offset"]))
        if t["offset"]:
            assert all((b[key].data_ptr() + 4 * t["offset"]) % 16 == 4 for key in b)
        arr[k].numel, arr[k].step, arr[k].lr = t["numel"], t["step"], t["lr"]
    _lib.check(L.lvdgs_adam_step(arr, len(tensors), cases.ADAM_BETA1, cases.ADAM_BETA2, cases.ADAM_EPS, _stream()), "lvdgs_adam_step")
    torch.cuda.synchronize()
    worst = dict(param=0.0, exp_avg=0.0, exp_avg_sq=0.0)
    for t, b in zip(tensors, bufs):
        n, o = t["numel"], t["offset"]
        sl = slice(o, o + n)
        got = {key: b[key].cpu().numpy() for key in b}
        for key in got:                                   # the guards behind numel and the float before an offset view
            assert (got[key][o + n:] == cases.ADAM_GUARD_VALUE).all() and (got[key][:o] == cases.ADAM_GUARD_VALUE).all(), (key, n)
        assert np.array_equal(got["grad"], t["grad"])
        p1, m1, v1, ex = orc.adam(t["param"][sl], t["grad"][sl], t["exp_avg"][sl], t["exp_avg_sq"][sl], t["step"], t["lr"], cases.ADAM_BETA1,
                                  cases.ADAM_BETA2, cases.ADAM_EPS)
        bp, bm, bv = orc.adam_bounds(p1, m1, v1, ex)
        for key, ref, bound in (("param", p1, bp), ("exp_avg", m1, bm), ("exp_avg_sq", v1, bv)):
            worst[key] = max(worst[key], ratio(got[key][sl] - ref, bound))
        still = t["still"]
        assert np.array_equal(got["param"][sl][still].view(np.int32), t["param"][sl][still].view(np.int32))      # zero gradient, zero moments: unmoved
        assert not got["exp_avg"][sl][still].any() and not got["exp_avg_sq"][sl][still].any()
    report("adam", name, **worst)


# ================================================================================================ statistics
def _acc(c):
    return dict(radii_max=Buf(c["radii_max0"], dtype=np.int32, fill=-7), norm_sum=Buf(c["norm_sum0"]), vis_count=Buf(c["vis_count0"]))


@functools.lru_cache(maxsize=None)
def _stats_reference(n):
    c = cases.stats_case(n)
    st = dict(radii_max=c["radii_max0"], norm_sum=c["norm_sum0"].astype(f64), vis_count=c["vis_count0"].astype(f64))
    touched = []
    for v in c["views"]:
        st, tr, _ = orc.view_stats(v["radii"], v["n_touched"], v["grad"], st)
        touched.append(tr)
    return c, st, touched


def _view_buffers(c):
    return [dict(radii=Buf(v["radii"], dtype=np.int32, fill=-7), n_touched=Buf(v["n_touched"], dtype=np.int32, fill=-7), grad=Buf(v["grad"]),
                 touched=Buf(n=c["n"], dtype=np.uint8, fill=99)) for v in c["views"]]


def _stats_by_view_stats(c, views):
    """lvdgs_view_stats, view after view -> (accumulators, per-view touched rows) as host arrays."""
    L, n, acc = _lib.lib(), c["n"], _acc(c)
    for vb in views:
        _lib.check(L.lvdgs_view_stats(n, vb["radii"].ptr, vb["n_touched"].ptr, vb["grad"].ptr, acc["radii_max"].ptr, acc["norm_sum"].ptr,
                                      acc["vis_count"].ptr, vb["touched"].ptr, None, _stream()), "lvdgs_view_stats")
    torch.cuda.synchronize()
    return {k: b.get() for k, b in acc.items()}, [vb["touched"].get() for vb in views]


@pytest.mark.parametrize("n", cases.STATS_SIZES)
def test_view_stats_over_thirteen_views_and_map_stats_apply(n):
    L = _lib.lib()
    c, st, touched = _stats_reference(n)
    views = _view_buffers(c)
    acc, rows = _stats_by_view_stats(c, views)
    assert np.array_equal(acc["radii_max"], st["radii_max"]) and np.array_equal(acc["vis_count"], st["vis_count"])
    assert all(np.array_equal(a, b) for a, b in zip(rows, touched))
    report("view_stats", f"n={n} 13 views", norm_sum=ratio(acc["norm_sum"] - st["norm_sum"], EPS * st["norm_err"]) if n else 0.0)
    # split planes: the xy of the visible rows, byte for byte
    planes, spare = Buf(n=3 * n * 2), Buf(c["radii_max0"], dtype=np.int32)
    for k in range(3):
        vb = views[k]
        _lib.check(L.lvdgs_view_stats(n, vb["radii"].ptr, None, vb["grad"].ptr, spare.ptr, None, None, None,
                                      C.c_void_p(planes.ptr.value + 8 * n * k), _stream()), "lvdgs_view_stats (split)")
    torch.cuda.synchronize()
    host_planes = planes.get().reshape(3, n, 2)
    want = np.stack([np.where((v["radii"] > 0)[:, None], v["grad"][:, :2], f32(0)) for v in c["views"][:3]]) if n else host_planes
    assert np.array_equal(host_planes.view(np.int32), want.astype(f32).view(np.int32))
    # ... and the statistics' way into the model
    for n_split in (0, 1, 3):
        model = dict(max_radii2D=Buf(c["max_radii2D0"]), grad_accum=Buf(c["grad_accum0"]), denom=Buf(c["denom0"]))
        inputs = [Buf(acc["radii_max"], dtype=np.int32), Buf(acc["norm_sum"]), Buf(acc["vis_count"])]
        _lib.check(L.lvdgs_map_stats_apply(n, inputs[0].ptr, inputs[1].ptr, inputs[2].ptr, planes.ptr if n_split else None, n_split, model["max_radii2D"].ptr,
                                           model["grad_accum"].ptr, model["denom"].ptr, _stream()), "lvdgs_map_stats_apply")
        torch.cuda.synchronize()
        mr, ga, dn, err = orc.map_stats_apply(acc["radii_max"], acc["norm_sum"], acc["vis_count"], host_planes[:n_split], c["max_radii2D0"], c["grad_accum0"], c["denom0"])
        assert np.array_equal(model["max_radii2D"].get(), mr) and np.array_equal(model["denom"].get(), dn)
        report("map_stats_apply", f"n={n} n_split={n_split}", grad_accum=ratio(model["grad_accum"].get() - ga, EPS * err) if n else 0.0)


@pytest.mark.parametrize("n", cases.STATS_SIZES)
def test_view_stats_with_every_allowed_null(n):
    """viewspace_grad, vis_count, touched_row present or NULL, split_xy (norm_sum NULL) or norm_sum: two views each."""
    L = _lib.lib()
    c = cases.stats_case(n, views=2)
    worst = 0.0
    for combo in range(16):
        has_grad, has_cnt, has_row, split = (bool(combo >> k & 1) for k in range(4))
        views, acc = _view_buffers(c), _acc(c)
        st = dict(radii_max=c["radii_max0"], norm_sum=None if split else c["norm_sum0"].astype(f64), vis_count=c["vis_count0"].astype(f64) if has_cnt else None)
        xy = Buf(n=2 * n)
        for v, vb in zip(c["views"], views):
            _lib.check(L.lvdgs_view_stats(n, vb["radii"].ptr, vb["n_touched"].ptr if has_row else None, vb["grad"].ptr if has_grad else None,
                                          acc["radii_max"].ptr, None if split else acc["norm_sum"].ptr, acc["vis_count"].ptr if has_cnt else None,
                                          vb["touched"].ptr if has_row else None, xy.ptr if split else None, _stream()), "lvdgs_view_stats")
            torch.cuda.synchronize()
            st, tr, sp = orc.view_stats(v["radii"], v["n_touched"] if has_row else None, v["grad"] if has_grad else None, st, use_split=split)
            if has_row:
                assert np.array_equal(vb["touched"].get(), tr), combo
            else:
                assert vb["touched"].untouched(), combo
            if split:
                assert np.array_equal(xy.get().view(np.int32), sp.astype(f32).reshape(-1).view(np.int32)), combo
        assert np.array_equal(acc["radii_max"].get(), st["radii_max"]), combo
        if has_cnt:
            assert np.array_equal(acc["vis_count"].get(), st["vis_count"]), combo
        else:
            assert np.array_equal(acc["vis_count"].get(), c["vis_count0"]), combo
        if split or not has_grad:
            assert np.array_equal(acc["norm_sum"].get(), c["norm_sum0"]) and (split or xy.untouched()), combo
        elif n:
            worst = max(worst, ratio(acc["norm_sum"].get() - st["norm_sum"], EPS * st["norm_err"]))
    report("view_stats", f"n={n} NULL combinations", norm_sum=worst)


def _tail_args(c, vb, scratch):
    a = _lib.Args()
    a.image_height, a.image_width, a.num_gaussians, a.num_rendered = 16, 16, c["n"], 0
    a.scratch, a.scratch_bytes = (C.c_void_p(scratch.data_ptr()), scratch.numel()) if c["n"] else (None, 0)
    a.radii, a.n_touched, a.dL_dmeans2D = vb["radii"].ptr, vb["n_touched"].ptr, vb["grad"].ptr
    return a


@pytest.mark.parametrize("n", cases.STATS_SIZES)
def test_map_view_tails_take_the_statistics_of_view_stats(n):
    """loss = NULL, num_rendered = 0, a zero-filled scratch: the statistics half of lvdgs_map_view_tail (view after view) and of
    lvdgs_map_view_tail_batch (13 views: a launch of 12 and one of 1) has the bits of lvdgs_view_stats -- itself held to the oracle
    above -- and the pose gradient of nothing is exactly 0."""
    L = _lib.lib()
    c, _, _ = _stats_reference(n)
    want_acc, want_rows = _stats_by_view_stats(c, _view_buffers(c))
    scratch = torch.zeros(max(int(L.lvdgs_backward_scratch_bytes(n, 0)), 256), dtype=torch.uint8, device=DEV)
    for batched in (False, True):
        views, acc = _view_buffers(c), _acc(c)
        taus = [Buf(n=6) for _ in views]
        args = [_tail_args(c, vb, scratch) for vb in views]
        sas = [_lib.ViewStatsArgs() for _ in views]
        for sa, vb in zip(sas, views):
            sa.radii_max, sa.norm_sum, sa.vis_count, sa.touched_row, sa.split_xy = acc["radii_max"].ptr, acc["norm_sum"].ptr, acc["vis_count"].ptr, vb["touched"].ptr, None
        if batched:
            k = len(views)
            _lib.check(L.lvdgs_map_view_tail_batch(None, (C.POINTER(_lib.Args) * k)(*[C.pointer(a) for a in args]), (C.c_void_p * k)(*[t.ptr.value for t in taus]),
                                                   (C.POINTER(_lib.ViewStatsArgs) * k)(*[C.pointer(sa) for sa in sas]), k, _stream()), "lvdgs_map_view_tail_batch")
        else:
            for a, sa, t in zip(args, sas, taus):
                _lib.check(L.lvdgs_map_view_tail(None, C.byref(a), t.ptr, C.byref(sa), _stream()), "lvdgs_map_view_tail")
        torch.cuda.synchronize()
        for key in acc:
            assert acc[key].get().tobytes() == want_acc[key].tobytes(), (batched, key)
        assert all(np.array_equal(vb["touched"].get(), w) for vb, w in zip(views, want_rows)), batched
        for t in taus:
            tau = t.get()
            assert not tau.any() and not np.signbit(tau).any(), batched
