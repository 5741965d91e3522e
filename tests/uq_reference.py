"""Restatements behind ``pgd_quad_forms`` and ``PGD.variance_decomposition``, none of which uses the Q matrices of the frontend.

``dim_quadrature`` / ``brute_force``: Gauss-Legendre points in every cell of every parameter mesh (4 points: exact for the
P2 . P2 . P2 of density times two modes), modes and density evaluated at the points in longdouble, then mean, variance,
Var E[u | mu_i], Var E[u | mu_i, mu_j] and E Var[u | mu_~i] of the field at chosen dofs by tensor quadrature over all parameter
dimensions at once.

``quad_exact``: f_i^T Q f_i.  Integer data in int64, exact; floating-point data in longdouble (64-bit significand).

``bound``: a value is sum_l f_l (sum_k Q_lk f_k): every term passes at most Kpad roundings of the inner sum (products and
additions in any order, fused or not, Kpad = k padded as the kernel pads it), at most Kpad of the outer one and the two
additions of the epilogue, so |fl - exact| <= (2 Kpad + 4) 2^-53 |f_i|^T |Q| |f_i| to first order (the + 4 holds the epilogue and
the second-order terms); the longdouble reference adds (2 k + 4) 2^-64 of the same scale.
"""
import itertools

import numpy as np

U53 = 2.0 ** -53
LD = np.longdouble

_GL4_X, _GL4_W = np.polynomial.legendre.leggauss(4)
GL4_X = (LD(1) + _GL4_X.astype(LD)) / 2          # on [0, 1]; the nodes are doubles: the rule is exact to ~1e-16 of the integral,
GL4_W = _GL4_W.astype(LD) / 2                    # shared by every quantity compared (weights are normalised by their own sum)


def kpad(k):
    """k as the matrix-unit kernel pads it (the plain kernel's chains are shorter)."""
    return 16 if k <= 16 else 32 if k <= 32 else 48 if k <= 48 else 64 if k <= 64 else 128 if k <= 128 else 256


def quad_exact(F, Q):
    """(nq, n): F (n, k) rows f_i, Q (nq, k, k)."""
    F, Q = np.asarray(F), np.asarray(Q)
    if np.issubdtype(F.dtype, np.integer) and np.issubdtype(Q.dtype, np.integer):
        F, Q = F.astype(np.int64), Q.astype(np.int64)
        return np.stack([((F @ q.T) * F).sum(axis=1) for q in Q])
    F, Q = F.astype(LD), Q.astype(LD)
    return np.stack([((F @ q.T) * F).sum(axis=1) for q in Q])


def scale(F, Q):
    F, Q = np.abs(np.asarray(F, dtype=np.float64)), np.abs(np.asarray(Q, dtype=np.float64))
    return np.stack([((F @ q.T) * F).sum(axis=1) for q in Q])


def bound(k, B):
    return ((2 * kpad(k) + 4) * U53 + (2 * k + 4) * 2.0 ** -64) * B


# ---------------------------------------------------------------- tensor quadrature over the parameter domain
def dim_quadrature(V, G, rho=None):
    """(w, Gq): weights (sum 1) and the modes' values (K, points) at the 4 Gauss points of every cell of the interval space V
    (P1 or P2); G (dofs, K) and rho (dofs) or None in the order of Vector.host()."""
    lay, mesh = V._lay, V.mesh()
    X, cells = mesh.coordinates()[:, 0].astype(LD), mesh.cells()
    a, b = X[cells[:, 0]], X[cells[:, 1]]
    l1 = GL4_X[None, :] + 0 * a[:, None]
    l0 = 1 - l1
    if lay.degree == 1:
        nodes, N = cells, np.stack([l0, l1], axis=2)
    else:
        nodes, N = lay.cells, np.stack([l0 * (2 * l0 - 1), l1 * (2 * l1 - 1), 4 * l0 * l1], axis=2)
    nodes = np.asarray(nodes)[:, :N.shape[2]]
    G = np.asarray(G).astype(LD)
    Gq = np.einsum("cpa,cak->kcp", N, G[nodes])                       # (K, cells, 4)
    w = np.abs(b - a)[:, None] * GL4_W[None, :]
    if rho is not None:
        w = w * np.einsum("cpa,ca->cp", N, np.asarray(rho).astype(LD)[nodes])
    w = w.reshape(-1)
    return w / w.sum(), Gq.reshape(G.shape[1], -1)


def point_dimension(g):
    """A dimension that is given a value: one point of weight 1 with the modes' values g (K,) there."""
    return np.ones(1, dtype=LD), np.asarray(g).astype(LD).reshape(-1, 1)


def _mean_over(U, ws, axes):
    for ax in sorted(axes, reverse=True):
        U = np.tensordot(U, ws[ax], axes=([ax + 1], [0]))
    return U


def brute_force(F, dims, order=1):
    """F (rows, K) and dims = [(w_d, Gq_d)]: {"mean", "total", (i,), (i, j), ("T", i)} -> (rows,) longdouble, indices i into dims."""
    F = np.asarray(F).astype(LD)
    ws = [w for w, _ in dims]
    P = len(dims)
    T = F
    for _, Gq in dims:                                                # (rows, K, p_1, ..)
        T = T[..., None] * Gq.reshape((1, Gq.shape[0]) + (1,) * (T.ndim - 2) + (Gq.shape[1],))
    U = T.sum(axis=1)                                                 # (rows, p_1, .., p_P)
    everything = list(range(P))
    mean = _mean_over(U, ws, everything)

    def var_of_conditional(keep):                                     # Var E[u | mu_keep]
        E = _mean_over(U, ws, [d for d in everything if d not in keep]) - mean.reshape((-1,) + (1,) * len(keep))
        return _mean_over(E * E, [ws[d] for d in keep], list(range(len(keep))))

    out = {"mean": mean, "total": var_of_conditional(everything)}
    for i in everything:
        if ws[i].size > 1:
            out[(i,)] = var_of_conditional([i])
            D = U - np.expand_dims(_mean_over(U, ws, [i]), i + 1)     # E Var[u | mu_~i], formed directly
            out[("T", i)] = _mean_over(D * D, ws, everything)
    if order >= 2:
        for i, j in itertools.combinations([d for d in everything if ws[d].size > 1], 2):
            out[(i, j)] = var_of_conditional([i, j]) - out[(i,)] - out[(j,)]
    return out


def decomposition_bound(F, dims, ndofs):
    """(bound of a partial variance, bound of the mean) per row of F for moments formed in double from the mass atom.

    A moment of dimension d is a product with the mass atom (rows of at most 5 entries), a dot over n_d dofs, the centring
    and the division by the density's integral: at most n_d + 10 roundings, relative to the sum of the absolute terms -
    int rho |G_k - m_k| |G_l - m_l| =: Ch_d for C_d and mh_d mh_d^T, mh_d = int rho |G_k|, for M_d (an error of m shifts the
    centred modes by a constant and enters C only squared).  The entrywise products over the dimensions add those counts, the
    form adds 2 Kpad + 4 (``bound``), all relative to |f_i|^T (o_d (Ch_d + Mh_d)) |f_i|, which dominates every |Q_B|."""
    F = np.abs(np.asarray(F)).astype(LD)
    K = F.shape[1]
    H, mh_all = np.ones((K, K), dtype=LD), np.ones(K, dtype=LD)
    for w, Gq in dims:
        m, mh = (Gq * w).sum(axis=1), (np.abs(Gq) * w).sum(axis=1)
        A = np.abs(Gq - m[:, None])
        H = H * ((A * w) @ A.T + np.outer(mh, mh))
        mh_all = mh_all * mh
    c = sum(n + 10 for n in ndofs)
    var = (c + 2 * kpad(K) + 4) * U53 * ((F @ H) * F).sum(axis=1)
    return var.astype(np.float64), ((c + K + 2) * U53 * (F @ mh_all)).astype(np.float64)
