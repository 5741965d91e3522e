"""numpy / ``np.longdouble`` restatement of stage 1 of ``PGD.evaluate_gradient_many`` on P2 modes (``pgd_cell_gradient_p2``), written
from the shape functions and independently of pgdrome_amd/model.py and of the kernel's text, with the rounding bound the tests hold
the library to.  Stage 2 is that of tests/eval_gradient_reference.py (``evaluate_norm_reference``, ``norm_bound``,
``product_bound``), on entries instead of cells.  u = 2^-53 throughout.

A P2 simplex has the nodes (its record): the G + 1 vertices, then the midpoints of the local edges ``EDGES[G]``.  With barycentric
coordinates l_0 .. l_G the shape functions are N_i = l_i (2 l_i - 1) for vertex i and N_ab = 4 l_a l_b for the edge (a, b).  In
reference coordinates xi_a = l_{a+1} (l_0 = 1 - sum xi), d l_i / d xi_a = [i == a + 1] - [i == 0], so
    d N_i  / d xi_a = (4 l_i - 1) d l_i / d xi_a,      d N_ab / d xi_c = 4 (l_b d l_a / d xi_c + l_a d l_b / d xi_c),
du_a = sum_j d N_j / d xi_a u_j, and the gradient solves E g = du with row a of E the edge x_{a+1} - x_0 (the cell is straight, so
the map is that of the vertices).  ``shape_derivatives`` returns the matrix D[j][a] = d N_j / d xi_a: in int64 when 4 l is an
integer (then 4 l_i - 1 and 4 l_b are), in long double otherwise - from the float64 lam the library gets, converted exactly.

Integer nodal values, L, scale, integer or half-integer vertex coordinates and integer 4 lam: du is formed in int64, the solution
is rounded to integers and VERIFIED by (2 E) g == 2 du in int64, so the reference is exact.  Otherwise long double, the float64
solution with two steps of iterative refinement (residuals in long double), as ``cell_gradients`` there.
Planes: out[i, a, e] = scale[e] sum_j L[i][j] g[a, e, j], g[c G + d] = d u_c / d x_d at point a of cell e; the library's vector
is this array flattened (plane, point, cell).

Bound of stage 1 (``plane_bound_p2``), in the style of ``plane_bound``: the same geometry majorants A (cells, a, d) and kappa of
the cofactor inverse of the vertices' edge matrix, |inv_computed - inv| <= (8 kappa + 6) u A, and for the nodal part the majorant
    M[c][a] = sum_j |d N_j / d xi_a| |u_j,c|
which holds for a code that forms every coefficient d N_j / d xi_a in one piece - in particular 4 l_0 - 4 l_{a+1} for the edge
(0, a + 1), whose two terms cancel; a code that sums them apart is not covered.  Operation count of du_a for such a code: a
coefficient is at most one rounding (4 l is exact, 4 l_i - 1 and 4 l_0 - 4 l_{a+1} are one subtraction; relative to itself);
vertex a + 1 and its G - 1 other edges are one product and G - 1 additions, vertex 0 and its G - 1 other edges the same, their
difference one subtraction, the shared edge one product and one addition: no partial sum sees more than G + 3 roundings, each
relative to a sum of absolute terms, so |du_computed - du| <= (G + 3) u M (the P1 kernel: 1 u |du|).  Then as there: g[c][d] =
sum_a du_a inv[a][d] is G products and G - 1 additions (G u), out[i] is qin = ncomp G products, qin - 1 additions and the
product with the scale (qin + 1) u:
  |out_computed[i] - out[i]| <= (8 kappa + 2 G + qin + 14) u |scale| sum_j |L[i][j]| Gabs[j],  Gabs[c G + d] = sum_a M[c][a] A[a][d]
the last 4 of the 14 units covering the second-order terms and the reference's own rounding.  A perturbation of the nodal values
by at most W >= 0 moves out[i] by at most |scale| sum_j |L[i][j]| sum_a (sum_j |D[j][a]| W_j) |inv[a][d]| (``plane_shift_p2``).
Neither is fitted to the code under test."""
import numpy as np

from tests.eval_gradient_reference import LD, check_result, geometry_majorants, norm_bound
from tests.eval_many_reference import U53

EDGES = {1: ((0, 1),), 2: ((1, 2), (0, 2), (0, 1)), 3: ((2, 3), (1, 3), (1, 2), (0, 3), (0, 2), (0, 1))}      # UFC local edges


def _is_int(*arrays):
    return all(np.issubdtype(np.asarray(a).dtype, np.integer) for a in arrays)


def shape_values(lam, G):
    """N[j] at the barycentric point lam (float64): the vertices, then the edges."""
    l = np.asarray(lam, dtype=np.float64)
    return np.array([l[i] * (2.0 * l[i] - 1.0) for i in range(G + 1)] + [4.0 * l[a] * l[b] for a, b in EDGES[G]])


def shape_derivatives(lam, G):
    """D[j, a] = d N_j / d xi_a at lam: int64 where 4 lam is an integer, long double (of the float64 lam) otherwise."""
    l64 = np.asarray(lam, dtype=np.float64)
    l4 = 4.0 * l64
    if np.array_equal(np.rint(l4), l4):
        l4, one, dt = np.rint(l4).astype(np.int64), 1, np.int64
    else:
        l4, one, dt = 4 * l64.astype(LD), LD(1), LD
    dl = np.zeros((G + 1, G), dtype=dt)             # d l_i / d xi_a
    dl[0, :] = -1
    for a in range(G):
        dl[a + 1, a] = 1
    rows = [(l4[i] - one) * dl[i] for i in range(G + 1)] + [l4[b] * dl[a] + l4[a] * dl[b] for a, b in EDGES[G]]
    return np.array(rows, dtype=dt)


def point_gradients(coords, rec, U, lam):
    """g[a, e, c * G + d] = d u_c / d x_d at point lam[a] of cell e.  coords: the layout's node coordinates (only the vertices'
    are read), rec: (cells, nodes per cell) records, U: (nodes, ncomp).  int64 and exact for integer data (module docstring),
    long double otherwise."""
    U = np.asarray(U).reshape(len(U), -1)
    coords = np.asarray(coords, dtype=np.float64).reshape(len(coords), -1)
    nc, G, ncomp = rec.shape[0], coords.shape[1], U.shape[1]
    assert rec.shape[1] == (G + 1) * (G + 2) // 2
    vert = rec[:, :G + 1]
    Ds = [shape_derivatives(l, G) for l in np.asarray(lam, dtype=np.float64)]
    X2 = 2.0 * coords
    out = []
    if _is_int(U) and all(_is_int(D) for D in Ds) and np.array_equal(np.rint(X2[vert]), X2[vert]):
        Xi = np.rint(X2).astype(np.int64)
        E2 = Xi[vert[:, 1:]] - Xi[vert[:, :1]]                                   # twice the edges, (cells, a, d)
        Un = U.astype(np.int64)[rec]                                             # (cells, j, c)
        for D in Ds:
            du = np.einsum("ja,ejc->eac", D, Un)
            g = np.rint(np.linalg.solve(0.5 * E2.astype(np.float64), du.astype(np.float64))).astype(np.int64)      # (cells, d, c)
            assert np.array_equal(E2 @ g, 2 * du), "the gradient of this integer field is not an integer vector"
            out.append(np.transpose(g, (0, 2, 1)).reshape(nc, ncomp * G))
        return np.stack(out)
    Xl = coords.astype(LD)
    E = Xl[vert[:, 1:]] - Xl[vert[:, :1]]
    E64 = E.astype(np.float64)
    Un = U.astype(LD)[rec]
    for D in Ds:
        du = np.einsum("ja,ejc->eac", D.astype(LD), Un)
        g = np.linalg.solve(E64, du.astype(np.float64)).astype(LD)
        for _ in range(2):
            r = du - np.einsum("ead,edc->eac", E, g)
            g = g + np.linalg.solve(E64, r.astype(np.float64)).astype(LD)
        out.append(np.transpose(g, (0, 2, 1)).reshape(nc, ncomp * G))
    return np.stack(out)


def planes_p2(coords, rec, U, lam, L, scale=None):
    """(q, npt, cells): out[i, a, e] = scale[e] * sum_j L[i, j] g[a, e, j]; int64 where everything is an integer."""
    g = point_gradients(coords, rec, U, lam)
    if _is_int(g, L) and (scale is None or _is_int(scale)):
        out = np.einsum("ij,aej->iae", np.asarray(L, dtype=np.int64), g)
        return out if scale is None else out * np.asarray(scale, dtype=np.int64)[None, None, :]
    out = np.einsum("ij,aej->iae", np.asarray(L).astype(LD), g.astype(LD))
    return out if scale is None else out * np.asarray(scale).astype(LD)[None, None, :]


def _nodal_majorant(rec, W, lam, G):
    """M[a_point, e, a, c] = sum_j |D[j][a]| W[rec[e, j], c] for W (nodes, ncomp) >= 0."""
    Wn = W[rec]
    return np.stack([np.einsum("ja,ejc->eac", np.abs(shape_derivatives(l, G).astype(np.float64)), Wn)
                     for l in np.asarray(lam, dtype=np.float64)])


def plane_bound_p2(coords, rec, U, lam, L, scale=None):
    """(q, npt, cells): the stage-1 rounding bound of the module docstring."""
    U = np.abs(np.asarray(U, dtype=np.float64).reshape(len(U), -1))
    coords = np.asarray(coords, dtype=np.float64).reshape(len(coords), -1)
    G, qin, nc = coords.shape[1], np.asarray(L).shape[1], rec.shape[0]
    A, kappa = geometry_majorants(coords, rec[:, :G + 1])
    M = _nodal_majorant(rec, U, lam, G)                                          # (npt, cells, a, c)
    Gabs = np.einsum("ead,peac->pecd", A, M).reshape(M.shape[0], nc, -1)
    sc = np.ones(nc) if scale is None else np.abs(np.asarray(scale, dtype=np.float64))
    return (8.0 * kappa + 2 * G + qin + 14.0)[None, None, :] * U53 * sc[None, None, :] * \
        np.einsum("ij,pej->ipe", np.abs(np.asarray(L, dtype=np.float64)), Gabs)


def plane_shift_p2(coords, rec, W, lam, L, scale=None):
    """(q, npt, cells): how far a perturbation of the nodal values by at most W (nodes, ncomp) can move the planes."""
    W = np.abs(np.asarray(W, dtype=np.float64).reshape(len(W), -1))
    coords = np.asarray(coords, dtype=np.float64).reshape(len(coords), -1)
    G, nc = coords.shape[1], rec.shape[0]
    Xv = coords[rec[:, :G + 1]]
    inv = np.abs(np.transpose(np.linalg.inv(Xv[:, 1:] - Xv[:, :1]), (0, 2, 1)))                 # |inv(E^T)[a][d]|
    M = _nodal_majorant(rec, W, lam, G)
    spread = np.einsum("ead,peac->pecd", inv, M).reshape(M.shape[0], nc, -1)
    sc = np.ones(nc) if scale is None else np.abs(np.asarray(scale, dtype=np.float64))
    return (1.0 + 64 * U53) * sc[None, None, :] * np.einsum("ij,pej->ipe", np.abs(np.asarray(L, dtype=np.float64)), spread)


def points_of(at, G):
    """The barycentric points behind the frontend's two names."""
    return np.full((1, G + 1), 1.0 / (G + 1)) if at == "midpoint" else np.eye(G + 1)


def loop_reference_p2(sol, fixed_dim, free_dim, coords, attri, lam, L, scale=None):
    """``tests.eval_gradient_reference.loop_reference`` for P2 modes at the points ``lam``: for every sample ``PGD.evaluate`` and
    the restatement's planes of that field.  Returns V (S, npt * cells) in long double, entries point-major, and the bound on
    |value - V| for a code that derives the planes per mode and combines them, or combines the nodal modes first:
      e_i = plane_shift_p2(W)_i + sum_k |c_k| b_k,i + (K + 2) u sum_k |c_k| (|P_k,i| + b_k,i),  W = (K + 2) u sum_k |c_k| |F_k|,
    b_k = ``plane_bound_p2`` of mode k and P_k its planes; bound = norm_bound(e, V)."""
    att = sol.mesh[fixed_dim].attributes[attri]
    K = sol.used_numModes
    V0 = att.interpolationfct[0].function_space()
    ncomp = V0._ncomp
    lay = V0._lay.base if ncomp > 1 else V0._lay
    X, rec = lay.coords, lay.cells
    flat = lambda p: np.asarray(p).reshape(p.shape[0], -1)
    F = [att.interpolationfct[k].vector().host().reshape(-1, ncomp) for k in range(K)]
    Pk = [np.abs(flat(planes_p2(X, rec, F[k], lam, L, scale)).astype(np.float64)) for k in range(K)]
    bk = [flat(plane_bound_p2(X, rec, F[k], lam, L, scale)) for k in range(K)]
    Cm = sol.mode_factors_many(free_dim, coords, attri)
    Vs, Bs = [], []
    for j, c in enumerate(np.asarray(coords, dtype=np.float64).reshape(len(coords), -1)):
        u = sol.evaluate(fixed_dim, free_dim, list(c), attri).vector().host().reshape(-1, ncomp)
        p = flat(planes_p2(X, rec, u, lam, L, scale))
        v = np.sqrt((p * p).sum(axis=0))
        ca = np.abs(Cm[:, j])
        W = (K + 2) * U53 * sum(ca[k] * np.abs(F[k]) for k in range(K))
        e = flat(plane_shift_p2(X, rec, W, lam, L, scale)) + sum(ca[k] * bk[k] for k in range(K)) \
            + (K + 2) * U53 * sum(ca[k] * (Pk[k] + bk[k]) for k in range(K))
        Vs.append(v)
        Bs.append(norm_bound(e, v))
    return np.array(Vs), np.array(Bs)


def check_vertices_result(res, V, Bd, npt):
    """The outputs of an ``at="vertices"`` call - statistics, the two envelopes reduced over a cell's points - inside the bound Bd
    (S, npt * cells) around V (S, npt * cells, point-major)."""
    V64 = V.astype(np.float64)
    slack = Bd + 2 * U53 * V64
    nc = V.shape[1] // npt
    assert np.all(np.abs(res.min - V64.min(axis=1)) <= slack.max(axis=1))
    assert np.all(np.abs(res.max - V64.max(axis=1)) <= slack.max(axis=1))
    assert np.array_equal(res.max_abs, res.max)
    cell_slack = slack.max(axis=0).reshape(npt, nc).max(axis=0)
    emn, emx = res.envelope_min.vector().host(), res.envelope_max.vector().host()
    assert emn.shape == (nc,) and res.envelope_max.function_space()._dg0
    assert np.all(np.abs(emn - V64.min(axis=0).reshape(npt, nc).min(axis=0)) <= cell_slack)
    assert np.all(np.abs(emx - V64.max(axis=0).reshape(npt, nc).max(axis=0)) <= cell_slack)


def run_and_check_p2(sol, free_dim, coords, quantity, scale, at, **kw):
    """evaluate_gradient_many(at=...) with every output the choice allows, held to ``loop_reference_p2``; returns the result, the
    reference V (S, entries) and its bound."""
    from pgdrome_amd import fem
    V = sol.mesh[0].attributes[0].interpolationfct[0].function_space()
    mesh = V.mesh()
    G = mesh.topology().dim()
    L = fem.gradient_quantity(quantity, mesh.geometry().dim(), V._ncomp)
    sc = None if scale is None else (scale.vector().host() if isinstance(scale, fem.Function) else np.full(mesh.num_cells(), float(scale)))
    ref, Bd = loop_reference_p2(sol, 0, free_dim, coords, 0, points_of(at, G), L, sc)
    if at == "midpoint":
        threshold = float(np.median(ref.astype(np.float64)))
        res = sol.evaluate_gradient_many(0, free_dim, coords, 0, quantity=quantity, scale=scale, stats=True, envelope=True,
                                         threshold=threshold, fields=True, at=at, **kw)
        check_result(res, ref, Bd, threshold)
    else:
        res = sol.evaluate_gradient_many(0, free_dim, coords, 0, quantity=quantity, scale=scale, stats=True, envelope=True, at=at, **kw)
        check_vertices_result(res, ref, Bd, G + 1)
        assert res.fields is None and res.exceedance is None
    return res, ref, Bd
