"""Restatement of the bin index of pgd_points_locate (csrc/pgd_locate.hip: index_grid, bin_of, index_range, the count / fill pair) in
numpy float64, operation by operation in the library's order, so that the bins per axis, bin_ptr and the set of cells in every bin
come out identically: the boxes are comparisons, hi - lo, K * that, lo - m and hi + m are one rounding each (numpy fuses nothing),
(x - o) * inv, floor and the clamp likewise; the grid rule uses math.pow and round (half to even), as the host code uses pow and
nearbyint.  Nothing is taken from the library."""
import math

import numpy as np

INDEX_TOL = 2.0 ** -10        # LOC_INDEX_TOL
INDEX_SLACK = 2.0 ** -20      # LOC_INDEX_SLACK
TARGET = {2: 8, 3: 48}        # cells per bin the grid aims at
CAP = 16                      # entries per cell beyond which the grid is coarsened


def cell_boxes(X, cells):
    """lo, hi (nc, D) over the first D + 1 record entries."""
    X = np.asarray(X, dtype=np.float64).reshape(len(X), -1)
    D = X.shape[1]
    V = X[np.asarray(cells)[:, :D + 1]]
    return V.min(axis=1), V.max(axis=1)


def grid(nc, o, top, target):
    """(n (3,) int, L (3,)): bins per axis and extents, before any coarsening."""
    D = len(o)
    L = np.zeros(3)
    for a in range(D):
        ext = top[a] - o[a]
        L[a] = ext if (ext > 0.0 and math.isfinite(ext)) else 0.0
    n = [1, 1, 1]
    live = [a for a in range(3) if L[a] > 0.0]
    if live:
        prod = 1.0
        for a in live:
            prod *= L[a]
        s = math.pow((float(nc) / float(target)) / prod, 1.0 / len(live))
        for a in live:
            f = float(round(L[a] * s))
            f = f if f >= 1.0 else 1.0
            n[a] = int(min(f, 1073741824.0))
    while float(n[0]) * n[1] * n[2] >= 2147483647.0:
        n = [max(1, k // 2) for k in n]
    return np.array(n, dtype=np.int64), L


def inverse_steps(n, L):
    return np.array([float(n[a]) / L[a] if L[a] > 0.0 else 0.0 for a in range(3)])


def bin_of(x, o, inv, n):
    """clamp(floor((x - o) * inv), 0, n - 1) as an integer; a NaN gives 0."""
    with np.errstate(invalid="ignore", over="ignore"):
        f = np.floor((np.asarray(x, dtype=np.float64) - o) * inv)
    f = np.where(f >= 0.0, f, 0.0)
    f = np.where(f <= float(n - 1), f, float(n - 1))
    return f.astype(np.int64)


def ranges(lo, hi, o, inv, n):
    """r0, r1 (nc, 3): the bins per axis of the inflated boxes (0, 0 on a missing axis)."""
    nc, D = lo.shape
    K = (D + 1) * (INDEX_TOL + INDEX_SLACK)
    r0, r1 = np.zeros((nc, 3), dtype=np.int64), np.zeros((nc, 3), dtype=np.int64)
    for a in range(D):
        d = hi[:, a] - lo[:, a]
        m = K * d
        r0[:, a] = bin_of(lo[:, a] - m, o[a], inv[a], int(n[a]))
        r1[:, a] = bin_of(hi[:, a] + m, o[a], inv[a], int(n[a]))
    return r0, r1


def build(X, cells, target=0):
    """The index as a dict: o, inv (3,), n (3,) int64, bin_ptr (bins + 1,) int64, lists (one ascending array of cells per bin), entries,
    longest."""
    lo, hi = cell_boxes(X, cells)
    nc, D = lo.shape
    o3 = np.zeros(3)
    o3[:D] = lo.min(axis=0)
    n, L = grid(nc, lo.min(axis=0), hi.max(axis=0), target if target > 0 else TARGET[D])
    while True:
        inv = inverse_steps(n, L)
        r0, r1 = ranges(lo, hi, o3, inv, n)
        total = int(np.prod(np.maximum(r1 - r0 + 1, 0), axis=1).sum())
        if total <= CAP * nc and total <= 2 ** 31 - 1:
            break
        assert n.max() > 1
        n = np.maximum(n // 2, 1)
    bins = int(n[0] * n[1] * n[2])
    lists = [[] for _ in range(bins)]
    for e in range(nc):
        for bz in range(r0[e, 2], r1[e, 2] + 1):
            for by in range(r0[e, 1], r1[e, 1] + 1):
                for bx in range(r0[e, 0], r1[e, 0] + 1):
                    lists[bx + n[0] * (by + n[1] * bz)].append(e)
    lists = [np.array(sorted(l), dtype=np.int64) for l in lists]
    counts = np.array([len(l) for l in lists], dtype=np.int64)
    bin_ptr = np.concatenate([[0], np.cumsum(counts)])
    assert bin_ptr[-1] == total
    return dict(o=o3, inv=inv, n=n, bin_ptr=bin_ptr, lists=lists, entries=total, longest=int(counts.max()) if bins else 0)


def point_bins(index, pts):
    """The bin of every point (P,)."""
    pts = np.asarray(pts, dtype=np.float64)
    pts = pts.reshape(len(pts), -1)
    q = np.zeros((len(pts), 3), dtype=np.int64)
    for a in range(pts.shape[1]):
        q[:, a] = bin_of(pts[:, a], index["o"][a], index["inv"][a], int(index["n"][a]))
    n = index["n"]
    return q[:, 0] + n[0] * (q[:, 1] + n[1] * q[:, 2])


def candidates(index, pts):
    """Per point the ascending array of the cells of its bin."""
    return [index["lists"][b] for b in point_bins(index, pts)]
