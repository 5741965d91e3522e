"""Restatements behind the Gram-block kernel (``pgd_vec_gram``) and the mode compression built on it (``PGD.compress``).

``gram_exact``: G[i, j] = sum_r X[r, i] Y[r, j].  Integer data in int64, exact.  Floating-point data: every product is split
into p + e = x y exactly (Veltkamp / Dekker, no fma needed), ``math.fsum`` adds the 2 m terms of an entry without error, so the
value returned is the exact sum rounded once.

``bound``: |fl - exact| <= (m + 2) 2^-53 sum_r |x_i[r]| |y_j[r]| for any order of m products and m - 1 additions, fused or not -
the argument of ``tests/eval_many_reference.bound`` with m rows in place of K modes.

``compress_reference``: the compression algorithm restated on Gram matrices alone (everything after the Grams is arithmetic on
K x K data): for two dimensions the truncated SVD of the core L_1^T L_2, for more a CP-ALS in the orthonormal coordinates.
"""
import math

import numpy as np

U53 = 2.0 ** -53


def _two_product(a, b):
    """p, e with p + e == a * b exactly (p = fl(a b)); arrays of doubles far from over- and underflow."""
    split = 134217729.0                                  # 2^27 + 1
    p = a * b
    ca, cb = split * a, split * b
    ah, bh = ca - (ca - a), cb - (cb - b)
    al, bl = a - ah, b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def gram_exact(X, Y=None):
    X = np.asarray(X)
    Y = X if Y is None else np.asarray(Y)
    if np.issubdtype(X.dtype, np.integer) and np.issubdtype(Y.dtype, np.integer):
        return X.astype(np.int64).T @ Y.astype(np.int64)
    X, Y = X.astype(np.float64), Y.astype(np.float64)
    out = np.empty((X.shape[1], Y.shape[1]))
    for i in range(X.shape[1]):
        p, e = _two_product(X[:, i:i + 1], Y)            # (m, ky) each
        for j in range(Y.shape[1]):
            out[i, j] = math.fsum(np.concatenate([p[:, j], e[:, j]]))
    return out


def scale(X, Y=None):
    X = np.abs(np.asarray(X, dtype=np.float64))
    return X.T @ (X if Y is None else np.abs(np.asarray(Y, dtype=np.float64)))


def bound(m, B):
    return (m + 2) * U53 * B


# ---------------------------------------------------------------- compression on Gram matrices
def _coordinates(G):
    """L (K x r) with L L^T = G up to the dropped eigenvalues (<= 1e-14 of the largest), and the map back Q diag(lam^-1/2)."""
    lam, Q = np.linalg.eigh(0.5 * (G + G.T))
    keep = lam > 1e-14 * lam[-1]
    lam, Q = lam[keep][::-1], Q[:, keep][:, ::-1]
    return Q * np.sqrt(lam), Q / np.sqrt(lam)


def compress_reference(Gs, tol, max_modes=None, max_sweeps=200):
    """dict(R, rel_error, converged, ranks, W): W[d] (K x R) such that the new modes are F_d W[d].  No balancing, ordering or
    sign convention: compare the represented function, not the factors."""
    D, K = len(Gs), Gs[0].shape[0]
    LP = [_coordinates(G) for G in Gs]
    Ls, Ps = [lp[0] for lp in LP], [lp[1] for lp in LP]
    ranks = [L.shape[1] for L in Ls]
    cap = K if max_modes is None else min(K, max_modes)
    if D == 2:
        U, s, Vt = np.linalg.svd(Ls[0].T @ Ls[1], full_matrices=False)
        tails = np.sqrt(np.concatenate([np.cumsum((s ** 2)[::-1])[::-1], [0.0]])) / np.linalg.norm(s)
        R = int(np.argmax(tails <= tol))
        R = max(1, min(R, cap))
        Bs = [U[:, :R] * s[:R], Vt[:R].T]
        return {"R": R, "rel_error": float(tails[R]), "converged": bool(tails[R] <= tol), "ranks": ranks,
                "W": [P @ B for P, B in zip(Ps, Bs)]}
    # the orthonormal-coordinate residual is exact to rounding, so the error is measured on a dense core when it is small
    weight = np.prod([np.linalg.norm(L, axis=1) for L in Ls], axis=0)
    order = np.argsort(-weight, kind="stable")
    Bs, best = None, None
    for R in range(1, cap + 1):
        new = [L[order[R - 1]].reshape(-1, 1) for L in Ls]
        Bs = new if Bs is None else [np.hstack([B, b]) for B, b in zip(Bs, new)]
        err = None
        for _ in range(max_sweeps):
            for d in range(D):
                H, M = np.ones((R, R)), np.ones((K, R))
                for e in range(D):
                    if e != d:
                        H, M = H * (Bs[e].T @ Bs[e]), M * (Ls[e] @ Bs[e])
                Bs[d] = np.linalg.lstsq(H, (Ls[d].T @ M).T, rcond=None)[0].T
            last, err = err, _dense_error(Ls, Bs)
            if err <= tol or (last is not None and last - err <= 1e-6 * err):
                break
        best = {"R": R, "rel_error": float(err), "converged": bool(err <= tol), "ranks": ranks,
                "W": [P @ B for P, B in zip(Ps, Bs)]}
        if err <= tol:
            break
    return best


def _dense_error(Ls, Bs):
    """|T - That| / |T| from the dense cores (r_1 x ... x r_D entries: small in the tests)."""
    def dense(Fs):
        T = None
        for k in range(Fs[0].shape[0]):
            t = Fs[0][k]
            for F in Fs[1:]:
                t = np.multiply.outer(t, F[k])
            T = t if T is None else T + t
        return T
    T, That = dense(Ls), dense([B.T for B in Bs])
    return float(np.linalg.norm((T - That).ravel()) / np.linalg.norm(T.ravel()))


def dense_field(Fs):
    """sum_k (x)_d Fs[d][:, k] as a dense array (n_1 x ... x n_D)."""
    T = None
    for k in range(Fs[0].shape[1]):
        t = Fs[0][:, k]
        for F in Fs[1:]:
            t = np.multiply.outer(t, F[:, k])
        T = t if T is None else T + t
    return T
