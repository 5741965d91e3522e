"""Restatements behind ``pgd_grid_misfit``, ``pgd_grid_posterior`` and ``PGD.sensor_posterior`` in ``np.longdouble`` (64-bit
significand), from the same tables, with derived rounding bounds.  u = 2^-53 throughout.

The sample s = (i_0 .. i_{D-1}), last index fastest, has c_k(s) = prod_d T_d[k, i_d] and w_s = prod_d weights_d[i_d].

``chi2_bound``.  chi2[s] = sum_p r_p^2, r_p = y_p - sum_k a_pk c_k(s).
  * c_k is a chain of D multiplications, the first one by 1: at most D roundings, |dc_k| <= D u |c_k|.
  * The inner sum has Kp terms (k padded as the matrix-unit kernel pads it: zeros add no error but may add roundings of partial
    sums), products and additions in any order, fused or not: at most Kp roundings per term, so with the error of c
    |d sum| <= (Kp + D) u sum_k |a_pk| |c_k|.
  * r_p is one more rounding of a number of size at most B_p = sum_k |a_pk| |c_k| + |y_p|: |dr_p| <= (Kp + D + 1) u B_p.
  * chi2 sums Mp squares (m padded to whole tiles of 16; the last two additions are the shuffles): every term passes at most
    Mp + 2 roundings, and d(r_p^2) <= 2 |r_p| |dr_p| with |r_p| <= B_p.
  To first order |fl(chi2) - chi2| <= (2 (Kp + D + 1) + Mp + 2 + 4) u sum_p B_p^2; the + 4 holds the second-order terms.  The
  longdouble restatement adds (2 (k + D + 1) + m + 2) 2^-64 of the same scale.  The bound is in terms of B_p^2, not of chi2: a
  misfit of exactly 0 (data generated at a grid node) is met within it.

``posterior_bounds``.  e_s = w_s exp(-(chi2_s - shift) / 2) with the SAME double ``shift`` on both sides.
  * A chi2 within t_s of the exact one moves e_s by the factor exp(+- t_s / 2): relative expm1(t_s / 2).
  * The argument: the subtraction rounds once (u |chi2_s - shift| absolute, half of it relative to e_s), the halving is exact,
    exp is accurate to 2 ulp (the device library's documented bound is 1 ulp), w_s is a chain of D roundings, the last product
    one more:
        rho_s = expm1(t_s / 2) + (|chi2_s - shift| / 2 + D + 4) u.
  * A sum of S terms e_s x_s, summed in any order, fused or not: every term passes at most S roundings, x_s itself carries
    xr roundings (0 for 1, 1 for an abscissa product, 2 D + 2 for c_i c_j with the rounded e c_i):
        |fl(sum) - sum| <= sum_s |x_s| e_s (rho_s + (S + xr + 2) u) (1 + rho_s).
  For sum e_s^2 the factor of a term is (1 + rho_s)^2 - 1 <= 2 rho_s (1 + rho_s): the bound of sum (2 e_s) e_s with one more
  factor 1 + 2 max rho.  The longdouble restatement's own error, (S + 2 D + 8) 2^-64 of the same sums, is added.

``qr_term``.  More data than modes are reduced by a thin Householder QR of the whitened m x k matrix A: chi2 = |R c - Q^T y|^2 +
|y - Q Q^T y|^2.  By Higham, Accuracy and Stability of Numerical Algorithms, Theorem 19.4, the computed factors satisfy
A + dA = Q R with an exactly orthogonal Q and |dA_j|_2 <= g |a_j|_2 per column, g = c m k u; applying Q^T to y has the same form,
|dy|_2 <= g |y|_2 (Lemma 19.3).  With c = 8 for the blocked LAPACK routine the reduced sum is the exact misfit of the perturbed
data, which differs from |A c - y|^2 by at most 2 |r| d + d^2, d = g (sum_k |a_k|_2 |c_k| + |y|_2) =: g Bn and |r| <= Bn; the
explicit Q of the remainder term loses orthogonality by the same g.  qr_term = 3 g Bn^2 = 24 m k u Bn^2.
"""
import numpy as np

U53 = 2.0 ** -53
U64 = 2.0 ** -64
LD = np.longdouble


def kpad(k):
    """k as k_misfit_mfma pads it."""
    return 16 if k <= 16 else 32 if k <= 32 else 48 if k <= 48 else 64 if k <= 64 else 128 if k <= 128 else 256


def mpad(m):
    return 16 * ((m + 15) // 16)


def shape_of(tables):
    return tuple(int(np.asarray(t).shape[1]) for t in tables)


def indices(n):
    """The D index arrays of all S samples, last dimension fastest."""
    S = int(np.prod(n, dtype=np.int64))
    return np.unravel_index(np.arange(S), tuple(n))


def coefficients(tables):
    """(K, S) longdouble: c_k(s) for every sample of the grid of the tables."""
    idx = indices(shape_of(tables))
    C = np.ones((np.asarray(tables[0]).shape[0], idx[0].size), dtype=LD)
    for d, t in enumerate(tables):
        C = C * np.asarray(t).astype(LD)[:, idx[d]]
    return C


def chi2_exact(a, y, tables):
    """(chi2 (S,) longdouble, B2 (S,) float: sum_p B_p^2)."""
    a, y = np.asarray(a, dtype=np.float64), np.asarray(y, dtype=np.float64).reshape(-1)
    C = coefficients(tables)
    r = y.astype(LD)[:, None] - a.astype(LD) @ C
    B = np.abs(a).astype(LD) @ np.abs(C) + np.abs(y).astype(LD)[:, None]
    return (r * r).sum(axis=0), (B * B).sum(axis=0).astype(np.float64)


def chi2_bound(k, m, ndim, B2):
    return ((2 * (kpad(k) + ndim + 1) + mpad(m) + 6) * U53 + (2 * (k + ndim + 1) + m + 2) * U64) * np.asarray(B2, dtype=np.float64)


def qr_term(a, y, tables):
    """The QR's own term per sample for the whitened (m, k) matrix a and data y."""
    a, y = np.asarray(a, dtype=np.float64), np.asarray(y, dtype=np.float64).reshape(-1)
    m, k = a.shape
    Bn = np.linalg.norm(a, axis=0) @ np.abs(coefficients(tables)).astype(np.float64) + np.linalg.norm(y)
    return 24.0 * m * k * U53 * Bn * Bn


def posterior_exact(chi2, shift, tables, weights, abscissae=None):
    """The sums of pgd_grid_posterior in longdouble from the chi2 values given (any float type) and the double ``shift``: a dict with
    "e" (S,), "Z", "sum_e2", "marginals" (list), "theta1", "theta2" (with abscissae), "coef1", "coef2" (with tables)."""
    n = tuple(int(np.asarray(w).size) for w in weights)
    idx = indices(n)
    w = np.ones(idx[0].size, dtype=LD)
    for d, wd in enumerate(weights):
        w = w * np.asarray(wd).astype(LD)[idx[d]]
    e = w * np.exp(-(np.asarray(chi2).astype(LD) - LD(shift)) / 2)
    out = {"e": e, "Z": e.sum(), "sum_e2": (e * e).sum()}
    out["marginals"] = [np.array([e[idx[d] == i].sum() for i in range(n[d])], dtype=LD) for d in range(len(n))]
    if abscissae is not None:
        th = np.stack([np.asarray(x).astype(LD)[idx[d]] for d, x in enumerate(abscissae)])
        out["theta"] = th
        out["theta1"], out["theta2"] = th @ e, (th * e) @ th.T
    if tables is not None:
        C = coefficients(tables)
        out["C"] = C
        out["coef1"], out["coef2"] = C @ e, (C * e) @ C.T
    return out


def posterior_bounds(ex, chi2, shift, tau, ndim):
    """Bounds of the same sums (floats, same keys) from the dict ``ex`` of ``posterior_exact``; ``tau``: the bound of the chi2 values
    the code under test used against the ones ``ex`` was formed from (0: the same numbers)."""
    e = ex["e"]
    S = e.size
    idx = indices(tuple(m.size for m in ex["marginals"]))
    tau = np.broadcast_to(np.asarray(tau, dtype=np.float64), (S,))
    rho = np.expm1(tau / 2) + (np.abs(np.asarray(chi2, dtype=np.float64) - shift) / 2 + ndim + 4) * U53

    def b(absx, xr):
        t = (absx * e) * ((rho + (S + xr + 2) * U53) * (1 + rho)).astype(LD)
        return t, (S + 2 * ndim + 8) * U64 * (absx * e)

    def total(absx, xr):
        t, r = b(absx, xr)
        return np.asarray(t.sum(axis=-1) + r.sum(axis=-1), dtype=np.float64)

    one = np.ones(S, dtype=LD)
    out = {"Z": float(total(one, 0)), "sum_e2": float(total(2 * e + 0 * one, 1) * (1 + 2 * float(rho.max())))}
    t, r = b(one, 0)
    out["marginals"] = [np.array([float((t + r)[idx[d] == i].sum()) for i in range(mg.size)]) for d, mg in enumerate(ex["marginals"])]
    if "theta" in ex:
        th = np.abs(ex["theta"])
        out["theta1"] = total(th, 0)
        out["theta2"] = total(th[:, None, :] * th[None, :, :], 2)
    if "C" in ex:
        C = np.abs(ex["C"])
        out["coef1"] = total(C, ndim + 1)
        out["coef2"] = total(C[:, None, :] * C[None, :, :], 2 * ndim + 2)
    return out
