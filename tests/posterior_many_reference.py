"""Restatements behind ``pgd_grid_posterior_many`` and ``PGD.sensor_posterior_many`` in ``np.longdouble``, on top of
``tests/posterior_reference.py`` (its ``coefficients``, ``posterior_exact`` and ``posterior_bounds`` with the ``tau`` argument), with
the derived rounding bound of the expanded misfit.  u = 2^-53 throughout.

The code under test never forms a residual.  For data set j with the data vectors y_i, i in I_j (one vector, or the first j + 1 of
them with ``accumulate``), it is handed u_j = sum_i y_i, alpha_j = |I_j| and beta_j = sum_i |y_i|^2, all formed on the host in
double, and evaluates
    chi2[j, s] = beta_j - 2 u_j . p_s + alpha_j |p_s|^2,   p_s = a c(s).
``chi2_many_exact`` is the difference form sum_{i in I_j} sum_p (y_ip - p_ps)^2 in longdouble from the data themselves.

``chi2_many_bound``.  Let A_p = sum_k |a_pk| |c_k(s)| (B_p of ``posterior_reference`` for data 0: the bound of |p_ps|), n_j = |I_j|,
U_jp = sum_{i in I_j} |y_ip| (= |u_jp| for one vector) and
    scale[j, s] = beta_j + 2 sum_p U_jp A_p + alpha_j sum_p A_p^2,
the sum of the absolute values of everything that is added.  The expanded form cancels: its error is in terms of this scale, not
of chi2.
  * c_k: D roundings; p_ps: Kp terms (k padded as the matrix-unit kernel pads it) in any order, fused or not:
    |d p_ps| <= (Kp + D) u A_p, as in ``chi2_bound``.
  * pp = |p_s|^2: Mp squares (m padded to whole tiles of 16) in one chain and two shuffles, every term passes at most Mp + 2
    roundings, and d(p^2) <= 2 |p| |dp|:  |d pp| <= (2 (Kp + D) + Mp + 2) u sum_p A_p^2.
  * u_jp: a running sum of n_j terms, n_j - 1 roundings: |d u_jp| <= (n_j - 1) u U_jp.  -2 u is exact.
  * beta_j: m squares summed (m + 1 roundings per term) and n_j - 1 further additions: |d beta_j| <= (m + n_j) u beta_j.
    alpha_j = n_j is exact.
  * the second product adds Mp + 4 terms (Mp products u p, then pp alpha, 1 beta and two zeros), products exact inside the fused
    operations, in any order: every term passes at most Mp + 4 roundings.
  To first order
    |fl(chi2) - chi2| <= [ ((Kp + D) + (n_j - 1) + (Mp + 4)) 2 sum U A  +  (2 (Kp + D) + 2 Mp + 6) alpha sum A^2
                           +  (m + n_j + Mp + 4) beta ] u
                      <= (2 (Kp + D) + 2 Mp + m + n_j + 6) u scale;
  + 4 holds the second-order terms as in ``chi2_bound``.  The longdouble restatement adds (2 (k + D + 1) + m + n_j + 2) 2^-64 of
  the same scale.  A misfit of exactly 0 (data generated at a grid node) is met within it.

The sums of e = w exp(-(chi2 - shift) / 2) are held to ``posterior_bounds`` with the SAME double ``shift`` (the code's own minimum)
on both sides and tau[s] = bound[j, s] + bound[j, argmin]: the bound of the misfit plus that of the shift itself.
"""
import math

import numpy as np

from tests import posterior_reference as R

LD = R.LD
U53 = R.U53


def data_sets(Y, accumulate=False):
    """(u, alpha, beta) as the frontend forms them on the host, in double, from the whitened data Y (N, m)."""
    Y = np.ascontiguousarray(Y, dtype=np.float64)
    y2 = np.einsum("np,np->n", Y, Y)
    if accumulate:
        return np.cumsum(Y, axis=0), np.arange(1, Y.shape[0] + 1, dtype=np.float64), np.cumsum(y2)
    return Y, np.ones(Y.shape[0]), y2


def chi2_many_exact(a, Y, tables, accumulate=False):
    """(chi2 (N, S) longdouble in the difference form, scale (N, S) float) for the data vectors Y (N, m)."""
    a, Y = np.asarray(a, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    C = R.coefficients(tables)
    P = a.astype(LD) @ C                                          # (m, S)
    A = (np.abs(a).astype(LD) @ np.abs(C)).astype(np.float64)     # (m, S)
    N, m = Y.shape
    chi2 = np.zeros((N, P.shape[1]), dtype=LD)
    for p in range(m):
        r = Y[:, p].astype(LD)[:, None] - P[p][None, :]
        chi2 += r * r
    absY, y2 = np.abs(Y), (Y.astype(LD) ** 2).sum(axis=1).astype(np.float64)
    alpha = np.ones(N)
    if accumulate:
        chi2, absY, y2, alpha = np.cumsum(chi2, axis=0), np.cumsum(absY, axis=0), np.cumsum(y2), np.arange(1.0, N + 1)
    scale = y2[:, None] + 2.0 * (absY @ A) + alpha[:, None] * (A * A).sum(axis=0)[None, :]
    return chi2, scale


def chi2_many_bound(k, m, ndim, scale, accumulate=False):
    scale = np.asarray(scale, dtype=np.float64)
    nj = np.arange(1.0, scale.shape[0] + 1)[:, None] if accumulate else 1.0
    return ((2 * (R.kpad(k) + ndim) + 2 * R.mpad(m) + m + nj + 10) * R.U53 + (2 * (k + ndim + 1) + m + nj + 2) * R.U64) * scale


def gap(chi2x):
    """Per data set the exact runner-up gap: the second smallest exact misfit minus the smallest."""
    part = np.partition(np.asarray(chi2x, dtype=np.float64), 1, axis=1) if chi2x.shape[1] > 1 else None
    return np.full(chi2x.shape[0], np.inf) if part is None else part[:, 1] - part[:, 0]


def check(out, chi2x, bound, weights, abscissae=None):
    """The outputs of one call (dict of ``Context.grid_posterior_many`` / ``grid_posterior_many_numpy``) against the restatement:
    asserts the argmin rule and returns the largest error / bound ratio per quantity."""
    nd, S = chi2x.shape
    D = len(weights)
    worst = {"shift": 0.0, "Z": 0.0, "sum_e2": 0.0, "theta1": 0.0, "theta2": 0.0}
    for j in range(nd):
        arg, shift = int(out["argmin"][j]), float(out["chi2_min"][j])
        assert 0 <= arg < S
        best = int(np.argmin(chi2x[j]))
        # the expanded form may pick another sample when two misfits lie within the bound, but never a worse one than that
        assert float(chi2x[j, arg] - chi2x[j, best]) <= 2.0 * max(bound[j, arg], bound[j, best])
        worst["shift"] = max(worst["shift"], abs(float(shift - chi2x[j, arg])) / bound[j, arg])
        ex = R.posterior_exact(chi2x[j], shift, None, weights, abscissae)
        bd = R.posterior_bounds(ex, chi2x[j].astype(np.float64), shift, bound[j] + bound[j, arg], D)
        for key in ("Z", "sum_e2") + (("theta1", "theta2") if abscissae is not None else ()):
            err = np.abs(np.asarray(out[key][j]) - ex[key]).astype(np.float64)
            b = np.asarray(bd[key], dtype=np.float64)
            assert np.all((b > 0.0) | (err == 0.0)), key
            worst[key] = max(worst[key], float((err / np.where(b > 0.0, b, 1.0)).max()))
        if abscissae is not None:
            assert np.array_equal(out["theta2"][j], out["theta2"][j].T)
    return worst


# ---- a PosteriorManyResult of the frontend against the restatement (both routes)
def ratio_bound(q, dN, dZ, Z):
    """A quotient q = N / Z of two sums within dN and dZ of their exact values, two roundings of its own."""
    return (np.asarray(dN) + np.abs(q) * dZ) / (Z - dZ) + 2 * U53 * np.abs(q)


def moments(res, j, chi2x, bound, tables):
    """(mean, its bound, Z's relative bound) of data set j of a result from the restatement."""
    shape = R.shape_of(tables)
    arg = int(np.ravel_multi_index(tuple(res.map_index[j]), shape))
    ex = R.posterior_exact(chi2x[j], float(res.shift[j]), None, res.weights, res.grids)
    bd = R.posterior_bounds(ex, chi2x[j].astype(np.float64), float(res.shift[j]), bound[j] + bound[j, arg], len(shape))
    Z, dZ = float(ex["Z"]), bd["Z"]
    mean = (ex["theta1"] / ex["Z"]).astype(np.float64)
    return ex, bd, mean, ratio_bound(mean, bd["theta1"], dZ, Z)


def check_result(res, a, Y, tables, accumulate=False, rest=None, logdet=0.0, m=None):
    """Every field of a result against the restatement from the whitened (a, Y) that the route used."""
    N, D = Y.shape[0], len(tables)
    k, rows = a.shape[1], a.shape[0]
    shape = R.shape_of(tables)
    chi2x, scale = chi2_many_exact(a, Y, tables, accumulate)
    bound = chi2_many_bound(k, rows, D, scale, accumulate)
    rest = np.zeros(N) if rest is None else rest
    m = rows if m is None else m
    worst = {key: 0.0 for key in ("shift", "chi2_min", "Z", "mean", "cov", "ess", "log_evidence")}
    for j in range(N):
        nj = j + 1 if accumulate else 1
        arg = int(np.ravel_multi_index(tuple(res.map_index[j]), shape))
        best = int(np.argmin(chi2x[j]))
        assert float(chi2x[j, arg] - chi2x[j, best]) <= 2.0 * max(bound[j, arg], bound[j, best])
        assert np.array_equal(res.map_coords[j], [g[i] for g, i in zip(res.grids, res.map_index[j])])
        worst["shift"] = max(worst["shift"], abs(float(res.shift[j] - chi2x[j, arg])) / bound[j, arg])
        # chi2_min is the difference form on the host: the mean of n_j vectors (n_j roundings), the scatter about it a running sum
        # (3 roundings a step), the rest as in the expanded form and on the same scale
        tol = bound[j, arg] + 4 * nj * U53 * scale[j, arg] + 4 * U53 * rest[j]
        worst["chi2_min"] = max(worst["chi2_min"], abs(float(res.chi2_min[j] - rest[j] - chi2x[j, arg])) / tol)
        ex, bd, mean, dmean = moments(res, j, chi2x, bound, tables)
        Z, dZ = float(ex["Z"]), bd["Z"]
        worst["Z"] = max(worst["Z"], abs(res.Z[j] - Z) / dZ)
        worst["mean"] = max(worst["mean"], float((np.abs(res.mean[j] - mean) / dmean).max()))
        second = (ex["theta2"] / ex["Z"]).astype(np.float64)
        cov = (ex["theta2"] / ex["Z"] - np.outer(ex["theta1"], ex["theta1"]) / ex["Z"] ** 2).astype(np.float64)
        dcov = ratio_bound(second, bd["theta2"], dZ, Z) + np.outer(np.abs(mean) + dmean, dmean) + np.outer(dmean, np.abs(mean)) + \
            4 * U53 * (np.abs(second) + np.abs(np.outer(mean, mean)))
        worst["cov"] = max(worst["cov"], float((np.abs(res.cov[j] - cov) / dcov).max()))
        ess = float(ex["Z"] ** 2 / ex["sum_e2"])
        worst["ess"] = max(worst["ess"], abs(res.ess[j] - ess) / (ess * (2 * dZ / Z + bd["sum_e2"] / float(ex["sum_e2"]) + 4 * U53)))
        shift = float(res.shift[j])
        logev = float(np.log(ex["Z"]) - np.longdouble(shift) / 2 - np.longdouble(rest[j]) / 2) - 0.5 * m * nj * math.log(2 * math.pi) - nj * logdet
        dlog = dZ / (Z - dZ) + 8 * U53 * (abs(math.log(Z)) + abs(shift) / 2 + rest[j] / 2 + 0.5 * m * nj * math.log(2 * math.pi) + nj * abs(logdet))
        worst["log_evidence"] = max(worst["log_evidence"], abs(res.log_evidence[j] - logev) / dlog)
    print("max error / bound:", worst)
    assert all(v <= 1.0 for v in worst.values())
    return chi2x, bound
