"""numpy / ``np.longdouble`` restatement of the two stages behind ``PGD.evaluate_gradient_many``, written independently of
pgdrome_amd/model.py, with the rounding bounds the tests hold the library to.  u = 2^-53 throughout.

Stage 1 (``pgd_cell_gradient``): on a P1 cell with vertices x_0 .. x_G the gradient of a nodal field solves E g = du, row a of
E the edge x_{a+1} - x_0 and du_a = u_{a+1} - u_0 (``np.linalg.solve`` on the cell's edge matrix).  Integer data on integer
or half-integer coordinates: the solution is rounded to integers and VERIFIED by (2 E) g == 2 du in int64, so it is exact.  Floating-point data: the
float64 solution gets two steps of iterative refinement with residuals in long double, which leaves an error of order
(cond u)^2 - nothing next to the bound below.  The planes are out[i] = scale * sum_j L[i][j] g[j], g[c G + d] = d u_c / d x_d.

Bound of stage 1, from operation counts of a kernel that forms the inverse from cofactors and the determinant in doubles.
Write A[a][d] for the sum of the ABSOLUTE values of the products that make cofactor (a, d), divided by |det|: A >= |inv|
entry by entry, with equality where no two products cancel (every axis-aligned lattice), and kappa = sum_d |E[0][d]| A[0][d]
>= 1 for the same majorant of the determinant's expansion.
  * an edge entry is one subtraction (1 u); a 3-D cofactor is two products and a subtraction of such entries: at most 4 u
    relative to its absolute products; the determinant is three products with cofactors and two additions: at most 8 u kappa
    relative to itself; the reciprocal and the product with it: 2 u.  So |inv_computed - inv| <= (8 kappa + 6) u A.
    (1-D and 2-D take fewer operations; the same count bounds them.)
  * du_a is one subtraction (1 u), g[c][d] = sum_a du_a inv[a][d] is G products and G - 1 additions (G u):
    |g_computed - g| <= (8 kappa + 7 + G) u  Gabs,   Gabs[c G + d] = sum_a |du_a| A[a][d].
  * out[i] is qin = ncomp G products, qin - 1 additions and the product with the scale (qin + 1) u.
  |out_computed[i] - out[i]| <= (8 kappa + G + qin + 12) u |scale| sum_j |L[i][j]| Gabs[j]
the last 4 of the 12 units covering the second-order terms and the reference's own rounding.  ``plane_bound`` returns it.
A perturbation of the nodal values by at most W >= 0 moves out[i] by at most |scale| sum_j |L[i][j]| sum_a (W_{a+1} + W_0)
|inv[a][d]| (``plane_shift``): what two evaluation orders of u itself may differ by, seen through the gradient.

Stage 2 (``pgd_eval_batch_norm``): v = sqrt(sum_i u_i^2), u_i = sum_t C[t][j] P_t[i][e].  Integer data: the u_i and the sum
of squares in int64, exact.  Floating-point data: long double.  Each computed u_i is off by at most
e_i = (K + 2) u sum_t |C[t][j]| |P_t[i][e]| (``tests.eval_many_reference.bound``: any order of K products and K - 1
additions).  Through the sum of squares and the root: | ||u + e|| - ||u|| | <= ||e|| in exact arithmetic; the q fused
multiply-adds of the sum of squares make it (1 + theta) times the exact one, |theta| <= (q + 1) u, so its root is off by a
factor (q + 1) u / 2, and the correctly rounded root adds 1 u:
  |v_computed - v| <= ||e||_2 + (q / 2 + 3) u (v + ||e||_2)
with one and a half spare units for second-order terms and the reference's rounding.  ``norm_bound`` takes any component-wise
bound e, so the frontend tests can add what stage 1 and another summation order contribute.  Neither bound is fitted to the
code under test."""
import numpy as np

from tests.eval_many_reference import U53, product

LD = np.longdouble


def _is_int(*arrays):
    return all(np.issubdtype(np.asarray(a).dtype, np.integer) for a in arrays)


def cell_edges(X, cells, dtype=LD):
    """E[e, a, d] = x_{a+1}[d] - x_0[d] for every cell."""
    X = np.asarray(X).reshape(len(X), -1).astype(dtype)
    return X[cells[:, 1:]] - X[cells[:, :1]]


def cell_gradients(X, cells, U):
    """g[e, c * G + d] = d u_c / d x_d on cell e for nodal values U (nodes, ncomp): int64 and exact for integer U on integer
    or half-integer coordinates, long double otherwise."""
    U = np.asarray(U).reshape(len(U), -1)
    nc, G, ncomp = cells.shape[0], cells.shape[1] - 1, U.shape[1]
    X2 = 2.0 * np.asarray(X, dtype=np.float64)               # (a "crossed" mesh has its midpoints on half-integers)
    if _is_int(U) and np.array_equal(np.rint(X2), X2):
        E2 = cell_edges(np.rint(X2).astype(np.int64), cells, np.int64)
        dU = U.astype(np.int64)[cells[:, 1:]] - U.astype(np.int64)[cells[:, :1]]            # (cells, a, c)
        g = np.rint(np.linalg.solve(0.5 * E2.astype(np.float64), dU.astype(np.float64))).astype(np.int64)      # (cells, d, c)
        assert np.array_equal(E2 @ g, 2 * dU), "the gradient of this integer field is not an integer vector"
        return np.transpose(g, (0, 2, 1)).reshape(nc, ncomp * G)
    E = cell_edges(X, cells)
    Ul = U.astype(LD)
    dU = Ul[cells[:, 1:]] - Ul[cells[:, :1]]
    E64 = E.astype(np.float64)
    g = np.linalg.solve(E64, dU.astype(np.float64)).astype(LD)
    for _ in range(2):
        r = dU - np.einsum("ead,edc->eac", E, g)
        g = g + np.linalg.solve(E64, r.astype(np.float64)).astype(LD)
    return np.transpose(g, (0, 2, 1)).reshape(nc, ncomp * G)


def planes(X, cells, U, L, scale=None):
    """(q, cells): out[i, e] = scale[e] * sum_j L[i, j] g[e, j]; int64 where everything is an integer."""
    g = cell_gradients(X, cells, U)
    if _is_int(g, L) and (scale is None or _is_int(scale)):
        out = np.asarray(L, dtype=np.int64) @ g.T
        return out if scale is None else out * np.asarray(scale, dtype=np.int64)[None, :]
    out = np.asarray(L).astype(LD) @ g.astype(LD).T
    return out if scale is None else out * np.asarray(scale).astype(LD)[None, :]


def geometry_majorants(X, cells):
    """A (cells, a, d) and kappa (cells,) of the stage-1 bound."""
    E = cell_edges(X, cells, np.float64)
    Ea = np.abs(E)
    nc, G = E.shape[0], E.shape[1]
    det = np.abs(np.linalg.det(E))
    if G == 1:
        cofabs = np.ones((nc, 1, 1))
    elif G == 2:
        cofabs = np.empty((nc, 2, 2))
        for a in range(2):
            for d in range(2):
                cofabs[:, a, d] = Ea[:, 1 - a, 1 - d]
    else:
        cofabs = np.empty((nc, 3, 3))
        for a in range(3):
            a1, a2 = (a + 1) % 3, (a + 2) % 3
            for d in range(3):
                d1, d2 = (d + 1) % 3, (d + 2) % 3
                cofabs[:, a, d] = Ea[:, a1, d1] * Ea[:, a2, d2] + Ea[:, a1, d2] * Ea[:, a2, d1]
    A = cofabs / det[:, None, None]
    kappa = (Ea[:, 0, :] * A[:, 0, :]).sum(axis=1)
    return A, np.maximum(kappa, 1.0)


def _spread(cells, W, M):
    """sum_a (W_{a+1} combined with W_0 by `+`) M[a][d] -> (cells, ncomp * G); W (nodes, ncomp) >= 0, M (cells, a, d) >= 0."""
    nc, G, ncomp = cells.shape[0], cells.shape[1] - 1, W.shape[1]
    dW = W[cells[:, 1:]] + W[cells[:, :1]]                                     # (cells, a, c)
    return np.einsum("ead,eac->ecd", M, dW).reshape(nc, ncomp * G)


def plane_bound(X, cells, U, L, scale=None):
    """(q, cells): the stage-1 rounding bound of the module docstring."""
    U = np.asarray(U, dtype=np.float64).reshape(len(U), -1)
    G, qin = cells.shape[1] - 1, np.asarray(L).shape[1]
    A, kappa = geometry_majorants(X, cells)
    dU = np.abs(U[cells[:, 1:]] - U[cells[:, :1]])
    Gabs = np.einsum("ead,eac->ecd", A, dU).reshape(cells.shape[0], -1)
    sc = np.ones(cells.shape[0]) if scale is None else np.abs(np.asarray(scale, dtype=np.float64))
    return (8.0 * kappa + G + qin + 12.0)[None, :] * U53 * sc[None, :] * (np.abs(np.asarray(L, dtype=np.float64)) @ Gabs.T)


def plane_shift(X, cells, W, L, scale=None):
    """(q, cells): how far a perturbation of the nodal values by at most W (nodes, ncomp) can move the planes."""
    W = np.asarray(W, dtype=np.float64).reshape(len(W), -1)
    inv = np.abs(np.transpose(np.linalg.inv(cell_edges(X, cells, np.float64)), (0, 2, 1)))      # |inv(E^T)[a][d]|
    sc = np.ones(cells.shape[0]) if scale is None else np.abs(np.asarray(scale, dtype=np.float64))
    return (1.0 + 64 * U53) * sc[None, :] * (np.abs(np.asarray(L, dtype=np.float64)) @ _spread(cells, W, inv).T)


def evaluate_norm_reference(P, C, threshold):
    """P: (K, q, m) planes per mode, C: (K, S).  dict: U (q, m, S) the combined planes, SS their sum of squares (int64 and
    exact for integer data), V = sqrt(SS) (m, S; float64 from int64, long double otherwise), min / max (S), env_min / env_max
    (m), exceed (m, counts of V > threshold, decided on SS in integers), B (q, m, S) = sum_t |C| |P|."""
    P, C = np.asarray(P), np.asarray(C)
    K, q, m = P.shape
    U = np.stack([product(P[:, i, :].T, C) for i in range(q)])
    B = np.stack([np.abs(P[:, i, :].T.astype(np.float64)) @ np.abs(C.astype(np.float64)) for i in range(q)])
    SS = (U * U).sum(axis=0)
    if _is_int(U):
        V = np.sqrt(SS.astype(np.float64))                  # SS < 2^53: exact conversion, correctly rounded root
        exceed = (SS > threshold * threshold).sum(axis=1) if threshold is not None else None
    else:
        V = np.sqrt(SS)
        exceed = (V > threshold).sum(axis=1) if threshold is not None else None
    return {"U": U, "SS": SS, "V": V, "min": V.min(axis=0), "max": V.max(axis=0), "env_min": V.min(axis=1),
            "env_max": V.max(axis=1), "exceed": exceed, "B": B}


def norm_bound(e, V):
    """|v_computed - v| <= ||e||_2 + (q / 2 + 3) u (v + ||e||_2) for component-wise bounds e (q, ...) on the u_i."""
    e = np.asarray(e, dtype=np.float64)
    ne = np.sqrt((e * e).sum(axis=0)) * (1.0 + 8 * U53)
    return ne + (e.shape[0] / 2.0 + 3.0) * U53 * (np.asarray(V, dtype=np.float64) + ne)


def product_bound(K, B):
    """e_i of stage 2: (K + 2) u sum_t |c_t| |p_t|."""
    return (K + 2) * U53 * np.asarray(B, dtype=np.float64)


# ------------------------------------------------------------------------------------------ through the frontend
def loop_reference(sol, fixed_dim, free_dim, coords, attri, L, scale=None):
    """What ``PGD.evaluate_gradient_many`` must agree with: for every sample ``PGD.evaluate`` and then the reference gradient of
    that field.  Returns V (S, cells) in long double and the bound (S, cells) on |value - V| for a code that derives the planes
    per mode and combines them: with W = (K + 2) u sum_k |c_k| |F_k| (what the evaluated field itself may be off by),
    b_k = ``plane_bound`` of mode k and P_k its planes,
      e_i = plane_shift(W)_i + sum_k |c_k| b_k,i + (K + 2) u sum_k |c_k| (|P_k,i| + b_k,i),   bound = norm_bound(e, V)."""
    att = sol.mesh[fixed_dim].attributes[attri]
    K = sol.used_numModes
    V0 = att.interpolationfct[0].function_space()
    mesh, ncomp = V0.mesh(), V0._ncomp
    X, cells = mesh.coordinates(), mesh.cells()
    F = [att.interpolationfct[k].vector().host().reshape(-1, ncomp) for k in range(K)]
    Pk = [np.abs(planes(X, cells, F[k], L, scale).astype(np.float64)) for k in range(K)]
    bk = [plane_bound(X, cells, F[k], L, scale) for k in range(K)]
    Cm = sol.mode_factors_many(free_dim, coords, attri)
    Vs, Bs = [], []
    for j, c in enumerate(np.asarray(coords, dtype=np.float64).reshape(len(coords), -1)):
        u = sol.evaluate(fixed_dim, free_dim, list(c), attri).vector().host().reshape(-1, ncomp)
        p = planes(X, cells, u, L, scale)
        v = np.sqrt((p * p).sum(axis=0))
        ca = np.abs(Cm[:, j])
        W = (K + 2) * U53 * sum(ca[k] * np.abs(F[k]) for k in range(K))
        e = plane_shift(X, cells, W, L, scale) + sum(ca[k] * bk[k] for k in range(K)) \
            + (K + 2) * U53 * sum(ca[k] * (Pk[k] + bk[k]) for k in range(K))
        Vs.append(v)
        Bs.append(norm_bound(e, v))
    return np.array(Vs), np.array(Bs)


def check_result(res, V, Bd, threshold):
    """Every output of an EvalManyResult (stats, envelope, exceedance at ``threshold``, fields) inside the bound Bd (S, cells)
    around V (S, cells)."""
    S = V.shape[0]
    V64 = V.astype(np.float64)
    slack = Bd + 2 * U53 * V64                               # (the float64 image of the long double reference)
    fields = np.array([f.vector().host() for f in res.fields])
    assert fields.shape == V.shape
    assert np.all(np.abs(fields.astype(LD) - V).astype(np.float64) <= Bd)
    assert np.all(np.abs(res.min - V64.min(axis=1)) <= slack.max(axis=1))
    assert np.all(np.abs(res.max - V64.max(axis=1)) <= slack.max(axis=1))
    assert np.array_equal(res.max_abs, res.max)
    assert np.all(np.abs(res.envelope_min.vector().host() - V64.min(axis=0)) <= slack.max(axis=0))
    assert np.all(np.abs(res.envelope_max.vector().host() - V64.max(axis=0)) <= slack.max(axis=0))
    clear = np.abs(V64 - threshold) > slack                  # pairs whose side of the threshold rounding cannot change
    lo = (clear & (V64 > threshold)).sum(axis=0) / S
    hi = lo + (~clear).sum(axis=0) / S
    ex = res.exceedance.vector().host()
    assert np.all(ex >= lo - 1e-15) and np.all(ex <= hi + 1e-15)
    # the statistics and the fields of the one call are the same numbers
    assert np.array_equal(res.min, fields.min(axis=1)) and np.array_equal(res.max, fields.max(axis=1))
    assert np.array_equal(ex, (fields > threshold).sum(axis=0) / S)


def samples_of(sol, dims, S, seed):
    """S coordinate sets of the free dimensions ``dims``: seeded uniform, plus both ends and a middle node of each mesh."""
    rng = np.random.default_rng(seed)
    cols = []
    for d in dims:
        X = np.sort(sol.mesh[d].dataX)
        c = rng.uniform(X[0], X[-1], size=S)
        c[0], c[1], c[2] = X[0], X[-1], X[len(X) // 2]
        cols.append(c)
    return np.stack(cols, axis=1)


def run_and_check(sol, free_dim, coords, quantity, scale, **kw):
    """evaluate_gradient_many with every output, held to ``loop_reference``; the threshold is the median of the reference."""
    from pgdrome_amd import fem
    V = sol.mesh[0].attributes[0].interpolationfct[0].function_space()
    mesh = V.mesh()
    L = fem.gradient_quantity(quantity, mesh.geometry().dim(), V._ncomp)
    sc = None if scale is None else (scale.vector().host() if isinstance(scale, fem.Function) else np.full(mesh.num_cells(), float(scale)))
    ref, Bd = loop_reference(sol, 0, free_dim, coords, 0, L, sc)
    threshold = float(np.median(ref.astype(np.float64)))
    res = sol.evaluate_gradient_many(0, free_dim, coords, 0, quantity=quantity, scale=scale, stats=True, envelope=True,
                                     threshold=threshold, fields=True, **kw)
    check_result(res, ref, Bd, threshold)
    return res, threshold


def two_valued(mesh, lo, hi):
    """A DG0 Function: ``lo`` on the cells left of the middle of the mesh in x, ``hi`` on the others."""
    from pgdrome_amd import fem
    f = fem.Function(fem.FunctionSpace(mesh, "DG", 0))
    mid = mesh.coordinates()[mesh.cells()].mean(axis=1)[:, 0]
    f.vector()[:] = np.where(mid < 0.5 * (mesh.coordinates()[:, 0].min() + mesh.coordinates()[:, 0].max()), lo, hi)
    return f
