"""Float64 NumPy statement of the patch-based scale alignment (LVD-GS Algorithm 1; the semantics of ``lvdgs_depth_align``,
include/lvdgs.h), vectorised over the patches: the image is padded to whole patches and viewed as (rows of patches, p, columns of
patches, p), so every patch statistic is one reduction over axes 1 and 3 with the padding masked out.

``align(r, m, ...)`` returns a dict: final_depth (float32), scale (np.float32), error_mask (bool), num_accurate, patch_num (passing
patches of the last iteration run), remedies ([k, ...]), iterations (the iterations run) and ``fragile`` (bool map) / ``fragile_patches``
(count): the pixels and patches some decision of which lay within ``tie`` (relative) of its threshold in any iteration run, or in the
fill -- where a float32 computation, or one that sums in another order, may decide the other way."""
import numpy as np

F32 = np.float32


def _patches(x, p, fill=0.0):
    """(H, W) -> (npy, p, npx, p) view of x padded with `fill` to whole patches."""
    H, W = x.shape
    npy, npx = -(-H // p), -(-W // p)
    out = np.full((npy * p, npx * p), fill, dtype=x.dtype)
    out[:H, :W] = x
    return out.reshape(npy, p, npx, p)


def _unpatch(x, H, W):
    npy, p, npx, _ = x.shape
    return x.reshape(npy * p, npx * p)[:H, :W]


def _near(lhs, rhs, tie):
    """Is the comparison lhs < rhs within `tie` (relative to |rhs|) of flipping?"""
    with np.errstate(invalid="ignore"):
        return np.abs(lhs - rhs) <= tie * np.abs(rhs)


def top_stop(s, s_prev, eps):
    """Top of an iteration: |s - s_prev| < eps in float32 (eps rounded to float32), unless s is still 1."""
    return bool(np.abs(F32(s) - F32(s_prev)) < F32(eps)) and F32(s) != F32(1.0)


def iteration(r, m, s, p, mean_thr, std_thr, err_thr, tie=1e-6):
    """One pass over the patches at scale s -> (accurate mask, passing patches, fragile pixel mask, fragile patch count)."""
    H, W = r.shape
    ms = (m.astype(F32) * F32(s)).astype(np.float64)          # the float32 product NumPy forms
    R, M = _patches(r.astype(np.float64), p), _patches(ms, p)
    valid = _patches(np.ones((H, W), bool), p, False)
    n = valid.sum(axis=(1, 3), keepdims=True).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        mr = np.where(valid, R, 0.0).sum(axis=(1, 3), keepdims=True) / n
        mm = np.where(valid, M, 0.0).sum(axis=(1, 3), keepdims=True) / n
        sr = np.sqrt(np.where(valid, (R - mr) ** 2, 0.0).sum(axis=(1, 3), keepdims=True) / n)
        sm = np.sqrt(np.where(valid, (M - mm) ** 2, 0.0).sum(axis=(1, 3), keepdims=True) / n)
        lhs1, rhs1 = np.abs(mr - mm), mean_thr * mm
        lhs2, rhs2 = np.abs(sr - sm), std_thr * sm
        passing = (lhs1 < rhs1) & (lhs2 < rhs2)
        frag_patch = (_near(lhs1, rhs1, tie) & (lhs2 < rhs2)) | (_near(lhs2, rhs2, tie) & (lhs1 < rhs1)) | \
            (_near(lhs1, rhs1, tie) & _near(lhs2, rhs2, tie))
        d = np.abs((R - mr) / (sr + 1e-6) - (M - mm) / (sm + 1e-6))
        acc = passing & valid & (d < err_thr)
        frag = valid & ((frag_patch & (d < err_thr + tie * err_thr)) | (passing & _near(d, err_thr, tie)))
    return _unpatch(acc, H, W), int(passing.sum()), _unpatch(frag, H, W), int(frag_patch.sum())


def fill(r, m, s, final_thr, tie=1e-6):
    """The fill step in float32, as NumPy forms it -> (final depth, error mask, fragile mask)."""
    r32, ms = r.astype(F32), m.astype(F32) * F32(s)
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.abs(r32 - ms) / (ms + F32(1e-8))
        err = (rel > F32(final_thr)) | (r32 == 0)
        rel64 = np.abs(r32.astype(np.float64) - ms.astype(np.float64)) / (ms.astype(np.float64) + 1e-8)
        frag = (r32 != 0) & _near(rel64, np.float64(F32(final_thr)), tie)
    return np.where(err, ms, r32).astype(F32), err, frag


def align(r, m, patch_size=10, mean_threshold=0.25, std_threshold=0.3, error_threshold=0.1, final_error_threshold=0.15, max_iter=4,
          epsilon=0.01, min_accurate_pixels_ratio=0.01, scale_remedy=None, tie=1e-6):
    """The algorithm; ``scale_remedy()`` -> the remedy's scale (no remedy, or None from it: keep the current scale)."""
    r = np.asarray(r, F32)
    if r.ndim == 3:
        r = r[0]
    m = np.asarray(m, F32)
    H, W = r.shape
    min_acc = int(min_accurate_pixels_ratio * H * W)
    s, s_prev = F32(1.0), F32(0.0)
    num_accurate, patch_num, remedies, iterations = 0, 0, [], 0
    fragile, fragile_patches = np.zeros((H, W), bool), 0
    for k in range(max_iter):
        if top_stop(s, s_prev, epsilon):
            break
        s_prev = s
        acc, patch_num, frag, fp = iteration(r, m, s, patch_size, mean_threshold, std_threshold, error_threshold, tie)
        iterations += 1
        fragile |= frag
        fragile_patches += fp
        count = int(acc.sum())
        if count < min_acc and k in (2, 3):
            num_accurate = count
            remedies.append(k)
            given = None if scale_remedy is None else scale_remedy()
            if given is not None:
                s = F32(given)
            if k == 3:
                break
            continue
        num_accurate = 0
        if count > 0 and (k < 2 or count >= min_acc):
            s = F32(r[acc].astype(np.float64).mean() / m[acc].astype(np.float64).mean())
            num_accurate = count
    final, err, frag = fill(r, m, s, final_error_threshold, tie)
    fragile |= frag
    return dict(final_depth=final, scale=s, error_mask=err, num_accurate=num_accurate, patch_num=patch_num, remedies=remedies,
                iterations=iterations, fragile=fragile, fragile_patches=fragile_patches)
