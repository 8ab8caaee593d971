"""NumPy float64 restatement of the reciprocal nearest-neighbour matching of include/lvdgs.h (``lvdgs_reciprocal_nn``).

Besides the merged output it keeps every seed's final ``(xy1, xy2, converged)`` and whether the seed is FRAGILE: some query on its
trajectory had a margin -- best score minus the best score below it -- under ``TAU``.  TAU: a float32 dot product of two unit
vectors of D <= 64 terms errs by at most D * 2^-24 <= 3.8e-6, two scores compared can so differ by 7.6e-6 from rounding alone, and TAU
sits just above that.  Rows that score EXACTLY the best in float64 (bit-identical rows of a map) are the tie rule's business -- the
lowest flat index wins, here as in the kernel -- and do not count as a margin.
"""
from types import SimpleNamespace

import numpy as np

TAU = 1e-5


def seed_grid(H1, W1, S):
    """Ascending flat indices of the seed grid y, x = S//2, S//2 + S, ... of an (H1, W1) map."""
    ys, xs = np.arange(S // 2, H1, S), np.arange(S // 2, W1, S)
    return (xs[None, :] + W1 * ys[:, None]).reshape(-1).astype(np.int64)


def nearest(Q, DB, chunk=256):
    """For every row of Q (n, D): the arg-max over DB (N, D) of the dot product (lowest index among equals) and its margin."""
    Q, DB = np.asarray(Q, dtype=np.float64), np.asarray(DB, dtype=np.float64)
    idx, margin = np.empty(len(Q), dtype=np.int64), np.empty(len(Q), dtype=np.float64)
    for lo in range(0, len(Q), chunk):
        s = Q[lo:lo + chunk] @ DB.T
        i = s.argmax(axis=1)
        best = s[np.arange(len(i)), i]
        below = np.where(s < best[:, None], s, -np.inf).max(axis=1)
        idx[lo:lo + chunk], margin[lo:lo + chunk] = i, best - below
    return idx, margin


def reciprocal_nn(desc1, desc2, subsample=8, max_iter=10, tau=TAU):
    """-> namespace: ``seeds``; per seed ``xy1``, ``xy2`` (flat indices), ``converged``, ``fragile``; ``active_after`` (seeds still
    active after each round run), ``rounds``; ``unconverged``; ``pairs`` (M, 2) the distinct flat pairs of the converged seeds, sorted;
    ``matches_im1`` (M, 2) int32 and ``matches_im2`` (M, 2) float32 pixel coordinates (x, y)."""
    H1, W1, D = desc1.shape
    H2, W2, _ = desc2.shape
    A, B = np.asarray(desc1, dtype=np.float64).reshape(-1, D), np.asarray(desc2, dtype=np.float64).reshape(-1, D)
    xy1 = seed_grid(H1, W1, subsample)
    n = len(xy1)
    xy2 = np.full(n, -1, dtype=np.int64)
    old1, old2 = xy1.copy(), xy2.copy()
    active, fragile = np.ones(n, dtype=bool), np.zeros(n, dtype=bool)
    active_after = []
    for _ in range(max_iter):
        if not active.any():
            break
        a = np.nonzero(active)[0]
        j, m = nearest(A[xy1[a]], B)
        xy2[a] = j
        fragile[a] |= m < tau
        active[a[j == old2[a]]] = False
        a = np.nonzero(active)[0]
        if len(a):
            i, m = nearest(B[xy2[a]], A)
            xy1[a] = i
            fragile[a] |= m < tau
            active[a[i == old1[a]]] = False
        old1, old2 = xy1.copy(), xy2.copy()
        active_after.append(int(active.sum()))
    conv = ~active
    pairs = np.unique(np.stack([xy1[conv], xy2[conv]], 1), axis=0) if conv.any() else np.zeros((0, 2), dtype=np.int64)
    return SimpleNamespace(seeds=n, xy1=xy1, xy2=xy2, converged=conv, fragile=fragile, active_after=active_after, rounds=len(active_after),
                           unconverged=int(active.sum()), pairs=pairs,
                           matches_im1=np.stack([pairs[:, 0] % W1, pairs[:, 0] // W1], 1).astype(np.int32),
                           matches_im2=np.stack([pairs[:, 1] % W2, pairs[:, 1] // W2], 1).astype(np.float32))


def flat_pairs(matches_im1, matches_im2, W1, W2):
    """(M, 2) flat index pairs of an output in pixel coordinates."""
    m1, m2 = np.asarray(matches_im1).astype(np.int64).reshape(-1, 2), np.asarray(matches_im2).astype(np.int64).reshape(-1, 2)
    return np.stack([m1[:, 0] + W1 * m1[:, 1], m2[:, 0] + W2 * m2[:, 1]], 1)
