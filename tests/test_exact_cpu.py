"""The numpy oracle and the form grammar against an exact rational reference (tests/exact_reference.py), on a CPU.

Every atom kind and every derivative pair (a, b) of oracle.fem_numpy.assemble_atom is compared entry by entry with the
exact values, on sheared, jittered, reordered and renumbered meshes, long-row fans and P2 layouts built from them.  The
frontend (pgdrome_amd.fem) runs on the numpy backends: functionals of polynomial Functions must equal q . (A_exact p) -
exact, since p and q lie in the space - and the matrices of the bilinear forms must be the exact atoms, which pins the
test / trial and a / b mapping of the grammar.  The same checks run on the HIP backend in tests/test_exact_gpu.py.

Tolerance: |got_ij - exact_ij| <= 1e-14 max_j S_ij per row, S_ij = sum over cells |K_e,ij| (about 45 eps).
"""
from fractions import Fraction

import numpy as np
import pytest

from oracle import fem_numpy as F
from oracle.backend_numpy import NumpyBackend
from pgdrome_amd import fem
from tests import exact_reference as X
from tests.robin_reference import FacetNumpyBackend

EPS = np.finfo(np.float64).eps
MESHES = X.mesh_matrix()


@pytest.mark.parametrize("D,degree", [(1, 1), (1, 2), (2, 1), (2, 2), (3, 1), (3, 2)])
def test_reference_checks_itself_against_sympy(D, degree):
    """q . (A p) of the helper equals sympy's integrate over a small domain, every kind and (a, b), and the facet masses."""
    if D == 1:
        c, e = np.array([[0.25], [1.0], [1.75], [2.5]]), np.array([[0, 1], [1, 2], [2, 3]], dtype=np.int32)
        facets = np.array([[0], [3]])
    elif D == 2:
        c = X.shear(np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 0.5], [1.0, 0.5]]), X.SHEAR2)
        e = np.array([[0, 1, 3], [2, 3, 0]], dtype=np.int32)              # the second cell with reversed orientation
        facets = np.array([[0, 1], [3, 2]])
    else:
        c = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.25, 1.0, 0.0], [0.5, 0.5, 1.25], [1.0, 1.0, 1.0]])
        e = np.array([[0, 1, 2, 3], [1, 3, 2, 4]], dtype=np.int32)
        facets = np.array([[0, 1, 2], [1, 4, 3]])
    if degree == 2:
        if D == 3:
            e = e[:1]                                                     # one cell: sympy on P2 tetrahedra is slow
        c, e = F.p2_interval_nodes(c, e) if D == 1 else F.p2_simplex_nodes(c, e)
        facets = None
    assert X.self_check(D, degree, c, e, facets=facets)


def test_reference_facet_masses_of_p2_against_sympy():
    """P2 facet masses (edge and triangle facets: vertices, then the facet's edge nodes in the UFC order)."""
    c = X.shear(np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 0.5], [1.0, 0.5]]), X.SHEAR2)
    nodes, tab = F.p2_simplex_nodes(c, np.array([[0, 1, 3], [0, 2, 3]], dtype=np.int32))
    # edge (0, 1) of cell 0 is its local edge 2 (node tab[0, 5]); edge (2, 3) of cell 1 its local edge 0 (tab[1, 3])
    assert X.self_check(2, 2, nodes, tab, facets=np.array([[0, 1, tab[0, 5]], [3, 2, tab[1, 3]]]))
    c3 = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.25, 1.0, 0.0], [0.5, 0.5, 1.25]])
    nodes, tab = F.p2_simplex_nodes(c3, np.array([[0, 1, 2, 3]], dtype=np.int32))
    # facet (0, 1, 2): its edges (1, 2), (0, 2), (0, 1) are the cell's local edges 2, 4, 5
    assert X.self_check(3, 2, nodes, tab, facets=np.array([[0, 1, 2, tab[0, 6], tab[0, 8], tab[0, 9]]]))


def oracle_bound(lay, kind, S, w):
    """1e-14 max_j S_ij, plus 4 eps times the inverse-rounding scale of the row (exact_reference.inverse_rounding_floor).
    The oracle takes gradients from np.linalg.inv (LU): a component that vanishes exactly in every cell of a row (the apex
    of the planar cone fan: grad lambda is vertical) comes out as ~1e-17, not 0, so max_j S_ij = 0 cannot bound it.
    The added term is that rounding of the inverse itself, 4 eps relative to the gradient norms - it is not a tolerance
    on the closed forms."""
    return 1e-14 * lay.row_max(S) + 4 * EPS * X.inverse_rounding_floor(lay, kind, w)


@pytest.mark.parametrize("name", sorted(MESHES))
def test_oracle_atoms_are_exact(name):
    coords, cells = MESHES[name]()
    lay = X.ExactLayout(coords, cells)
    w = X.weight_of(lay.coords)
    for kind, a, b in X.kinds_and_pairs(lay.D):
        wk = w if kind in (X.WMASS, X.WSTIFF) else None
        vals, S = lay.atom(kind, a, b, wk)
        ref = F.assemble_atom(lay.coords, lay.cells.astype(np.int32), kind, a, b, wk)
        assert np.array_equal(ref.indptr, lay.rp) and np.array_equal(ref.indices, lay.cols)
        err = X.exact_errors(ref.data, vals)
        bound = oracle_bound(lay, kind, S, wk)
        assert np.all(err <= bound), (name, X.KIND_NAMES[kind], a, b, float((err / np.maximum(bound, 1e-300)).max()))


# ------------------------------------------------------------------------------------------------- frontend
def polys(D, degree):
    """(f, g, w) as C expressions with small dyadic coefficients: exact in float64 at the dyadic nodes."""
    f = "0.5 + 2*x[0]" + (" - 3*x[1]" if D > 1 else "") + (" + x[2]" if D > 2 else "")
    g = "-1 + x[0]" + (" + 2*x[1]" if D > 1 else "") + (" - 0.5*x[2]" if D > 2 else "")
    w = "3 + 0.5*x[0]" + (" + 0.25*x[1]" if D > 1 else "") + (" - 0.25*x[2]" if D > 2 else "")
    if degree == 2:
        f += " + x[0]*x[0]" + (" - 2*x[0]*x[1] + 0.5*x[1]*x[1]" if D > 1 else "") + (" + x[1]*x[2] - x[2]*x[2]" if D > 2 else "")
        g += " - 0.5*x[0]*x[0]" + (" + x[0]*x[1]" if D > 1 else "") + (" + 2*x[0]*x[2]" if D > 2 else "")
        w += " + 0.25*x[0]*x[0]" + (" + 0.125*x[1]*x[1]" if D > 1 else "")
    return f, g, w


def exact_nodal(expr, coords):
    """Exact values of a polynomial C expression at the nodes (Python evaluates the same text on Fractions)."""
    out = np.empty(coords.shape[0], dtype=object)
    for k, row in enumerate(coords):
        out[k] = eval(expr, {"__builtins__": {}}, {"x": [Fraction(float(v)) for v in row]})
    return out


FRONTEND = {                     # (mesh, degree); the P2 tetrahedra on a smaller sheared box
    "interval_p1": ("p1_interval_nonuniform", 1),
    "interval_p2": ("p1_interval_nonuniform", 2),
    "tri_shear_p1": ("p1_tri_shear", 1),
    "tri_reversed_p1": ("p1_tri_reversed", 1),
    "tri_shear_p2": ("p1_tri_shear", 2),
    "tri_reversed_p2": ("p1_tri_reversed", 2),
    "tet_reordered_p1": ("p1_tet_reordered", 1),
    "tet_shear_p2": ("small_tet_shear", 2),
}


def frontend_mesh(name):
    if name == "small_tet_shear":
        c, e = F.box_mesh((0.0, 0.0, 0.0), (0.5, 0.5, 0.5), 2, 2, 1)
        return fem.Mesh(X.shear(c, X.SHEAR3), X.reorder_cells(e, 11))
    c, e = MESHES[name]()
    return fem.Mesh(c, e)


def exterior_facets(lay, D):
    """Node tuples (vertices, then for P2 the facet's edge nodes in the UFC order) of the exterior facets - from the
    layout's cell table, independently of the frontend's facet search - and the subset on the side x_0 = max."""
    vc = lay.cells[:, :D + 1].astype(np.int64)
    if D == 1:
        cnt = np.bincount(vc.ravel(), minlength=lay.n)
        tup = np.where(cnt == 1)[0].reshape(-1, 1)
    else:
        seen = {}
        for c in vc:
            for j in range(D + 1):
                f = tuple(sorted(np.delete(c, j)))
                seen[f] = seen.get(f, 0) + 1
        fac = [f for f, k in seen.items() if k == 1]
        if lay.degree == 2:
            edge = {}
            for c in np.asarray(lay.cells):
                for e, (p, q) in enumerate(X.UFC_EDGES[D]):
                    edge[tuple(sorted((c[p], c[q])))] = c[D + 1 + e]
            loc = ((0, 1),) if D == 2 else X.UFC_EDGES[2]
            fac = [f + tuple(edge[tuple(sorted((f[p], f[q])))] for p, q in loc) for f in fac]
        tup = np.array(sorted(fac), dtype=np.int64)
    G = 1 if D == 1 else D
    right = tup[np.all(lay.coords[tup[:, :G], 0] >= right_half(lay.coords), axis=1)]
    return tup, right


def right_half(coords):
    """Threshold of the tagged facets: those with every vertex at x_0 >= the middle of the x_0 range (non-empty on
    sheared meshes too, where no facet lies on a line x_0 = max)."""
    return 0.5 * (coords[:, 0].min() + coords[:, 0].max())


def tagged_measure(mesh, tag=7):
    fv, ext = mesh.facets()
    X0 = mesh.coordinates()[:, 0]
    mf = fem.MeshFunction("size_t", mesh, mesh.topology().dim() - 1, 0)
    mf.array()[np.where(ext & np.all(X0[fv] >= right_half(mesh.coordinates()), axis=1))[0]] = tag
    return fem.Measure("ds", domain=mesh, subdomain_data=mf)(tag)


def check_scalar(got, lay, vals, S, q, p, what):
    """got == q . (A_exact p) to 1e-14 sum_ij |q_i| S_ij |p_j|."""
    exact = X.exact_dot(q, lay.matvec(vals, p))
    qa = np.abs(np.array([float(v) for v in q]))
    scale = float(qa @ (X.product_bound(lay, S, np.array([float(v) for v in p]), tol=1.0)))
    err = abs(float(Fraction(float(got)) - exact))
    assert err <= 1e-14 * scale, (what, float(got), float(exact), err / (1e-14 * scale))
    return err / (1e-14 * scale) if scale > 0 else 0.0


def check_frontend_functionals(mesh, degree):
    """Every functional of the issue's list on the current backend against q . (A_exact p); returns the largest error as a
    fraction of the bound."""
    V = fem.FunctionSpace(mesh, "P", degree)
    lay = V._lay
    D = mesh.topology().dim()
    fs, gs, ws = polys(D, degree)
    f = fem.interpolate(fem.Expression(fs, degree=degree), V)
    g = fem.interpolate(fem.Expression(gs, degree=degree), V)
    w = fem.interpolate(fem.Expression(ws, degree=degree), V)
    ex = X.ExactLayout(lay.coords, lay.cells)
    p, q, wn = (exact_nodal(s, lay.coords) for s in (fs, gs, ws))
    one = np.array([Fraction(1)] * lay.n, dtype=object)
    # the premise: the nodal values the frontend holds are the exact ones
    for fn, ev in ((f, p), (g, q), (w, wn)):
        assert all(Fraction(float(a)) == b for a, b in zip(fn.vector().host(), ev))       # (host(): layout order)
    wf = np.array([float(v) for v in wn])
    worst = 0.0

    def chk(form, kind, a, b, left, right, wk=None, what=""):
        nonlocal worst
        vals, S = ex.atom(kind, a, b, wk)
        worst = max(worst, check_scalar(fem.assemble(form), ex, vals, S, left, right, what))

    dx = fem.dx
    chk(f * g * dx, X.MASS, 0, 0, q, p, what="f g")
    chk(fem.inner(fem.grad(f), fem.grad(g)) * dx, X.STIFF, 0, 0, q, p, what="grad f . grad g")
    chk(w * fem.inner(fem.grad(f), fem.grad(g)) * dx, X.WSTIFF, 0, 0, q, p, wf, what="w grad f . grad g")
    chk(f * g * w * dx, X.WMASS, 0, 0, q, p, wf, what="f g w")
    chk(f * dx, X.MASS, 0, 0, one, p, what="f")
    for a in range(D):
        chk(f.dx(a) * g * dx, X.CONV, a, 0, q, p, what="f_{,%d} g" % a)
        chk(f * g.dx(a) * dx, X.CONVT, 0, a, q, p, what="f g_{,%d}" % a)
        chk(f.dx(a) * dx, X.CONV, a, 0, one, p, what="f_{,%d}" % a)
        for b in range(D):
            chk(f.dx(a) * g.dx(b) * dx, X.DUDV, a, b, q, p, what="f_{,%d} g_{,%d}" % (a, b))
    # exterior facets: f ds, f g ds(tag)
    allf, right = exterior_facets(lay, D)
    vals, S = X.facet_mass(ex, allf)
    worst = max(worst, check_scalar(fem.assemble(f * fem.ds(mesh)), ex, vals, S, one, p, "f ds"))
    assert right.shape[0] > 0
    vals, S = X.facet_mass(ex, right)
    worst = max(worst, check_scalar(fem.assemble(f * g * tagged_measure(mesh)), ex, vals, S, q, p, "f g ds(tag)"))
    return worst


def check_frontend_matrices(mesh, degree):
    """The matrices of u_{,a} v_{,b}, u_{,a} v, u v_{,b} entry by entry against the exact atoms (dof order)."""
    V = fem.FunctionSpace(mesh, "P", degree)
    lay = V._lay
    D = mesh.topology().dim()
    ex = X.ExactLayout(lay.coords, lay.cells)
    u, v = fem.TrialFunction(V), fem.TestFunction(V)
    perm = fem.vertex_to_dof_map(V)
    worst = 0.0
    forms = [(u * v, X.MASS, 0, 0), (fem.inner(fem.grad(u), fem.grad(v)), X.STIFF, 0, 0)]
    for a in range(D):
        forms += [(u.dx(a) * v, X.CONV, a, 0), (u * v.dx(a), X.CONVT, 0, a)]
        forms += [(u.dx(a) * v.dx(b), X.DUDV, a, b) for b in range(D)]
    for integrand, kind, a, b in forms:
        got = fem.assemble(integrand * fem.dx).array()
        vals, S = ex.atom(kind, a, b)
        E = ex.dense(vals)[np.ix_(perm, perm)]
        Sd = np.zeros((ex.n, ex.n))
        rows = np.repeat(np.arange(ex.n), np.diff(ex.rp))
        Sd[rows, ex.cols] = S
        bound = 1e-14 * Sd.max(axis=1)[perm]
        err = np.array([[abs(float(Fraction(float(gij)) - eij)) for gij, eij in zip(gr, er)] for gr, er in zip(got, E)])
        q = err.max(axis=1) / np.maximum(bound, 1e-300)
        assert np.all(err <= bound[:, None]), (X.KIND_NAMES[kind], a, b, float(q.max()))
        worst = max(worst, float(q.max()))
    return worst


def strain_3d(w):
    """Voigt strain (e_xx, e_yy, e_zz, gamma_yz, gamma_xz, gamma_xy) of a 3-D vector field."""
    return fem.as_vector([w[0].dx(0), w[1].dx(1), w[2].dx(2), w[1].dx(2) + w[2].dx(1), w[0].dx(2) + w[2].dx(0),
                          w[0].dx(1) + w[1].dx(0)])


VOIGT = {2: [[(0, 0)], [(1, 1)], [(0, 1), (1, 0)]],                   # strain component -> [(field component, derivative)]
         3: [[(0, 0)], [(1, 1)], [(2, 2)], [(1, 2), (2, 1)], [(0, 2), (2, 0)], [(0, 1), (1, 0)]]}
C2 = np.array([[2.0, 0.5, 0.0], [0.5, 1.5, 0.25], [0.0, 0.25, 0.75]])
C3 = np.array([[2.0, 0.5, 0.5, 0.0, 0.0, 0.25], [0.5, 2.0, 0.5, 0.0, 0.0, 0.0], [0.5, 0.5, 2.0, 0.0, 0.125, 0.0],
               [0.0, 0.0, 0.0, 0.75, 0.0, 0.0], [0.0, 0.0, 0.125, 0.0, 0.75, 0.0], [0.25, 0.0, 0.0, 0.0, 0.0, 0.5]])


def check_elasticity(mesh, degree):
    """inner(C strain(u), strain(v)) dx as q . (A p) for polynomial vector fields p, q against the exact dudv blocks."""
    from tests import elastic2d_problem as E2
    D = mesh.topology().dim()
    V = fem.VectorFunctionSpace(mesh, "P", degree)
    C = C2 if D == 2 else C3
    strain = (lambda w: E2.strain(fem, w)) if D == 2 else strain_3d
    u, v = fem.TrialFunction(V), fem.TestFunction(V)
    A = fem.assemble(fem.inner(fem.as_matrix(C.tolist()) * strain(u), strain(v)) * fem.dx).array()
    base = V._lay.base
    ex = X.ExactLayout(base.coords, base.cells)
    fs = [polys(D, degree)[k % 3] for k in range(D)]
    gs = [polys(D, degree)[(k + 1) % 3] for k in range(D)]
    P = [exact_nodal(s, base.coords) for s in fs]                       # P[c] = nodal values of component c
    Q = [exact_nodal(s, base.coords) for s in gs]
    exact, scale = Fraction(0), 0.0
    for r in range(C.shape[0]):
        for s in range(C.shape[1]):
            if C[r, s] == 0.0:
                continue
            for c, a in VOIGT[D][s]:
                for d, b in VOIGT[D][r]:
                    vals, S = ex.atom(X.DUDV, a, b)
                    exact += Fraction(C[r, s]) * X.exact_dot(Q[d], ex.matvec(vals, P[c]))
                    qa = np.abs(np.array([float(t) for t in Q[d]]))
                    scale += abs(C[r, s]) * float(qa @ X.product_bound(ex, S, np.array([float(t) for t in P[c]]), tol=1.0))
    pv = np.array([[float(P[c][i]) for c in range(D)] for i in range(ex.n)]).ravel()     # dof = ncomp node + component
    qv = np.array([[float(Q[c][i]) for c in range(D)] for i in range(ex.n)]).ravel()
    got = float(qv @ (A @ pv))
    # the dense float product adds its own rounding: n eps sum |q| |A| |p| (far below the scale for these sizes)
    err = abs(float(Fraction(got) - exact))
    slack = ex.n * D * EPS * float(np.abs(qv) @ (np.abs(A) @ np.abs(pv)))
    assert err <= 1e-14 * scale + slack, (D, degree, got, float(exact), err / (1e-14 * scale))
    f = fem.interpolate(fem.Expression(tuple(fs), degree=degree), V)
    g = fem.interpolate(fem.Expression(tuple(gs), degree=degree), V)
    assert np.array_equal(f.vector().host(), pv) and np.array_equal(g.vector().host(), qv)
    fun = fem.assemble(fem.inner(fem.as_matrix(C.tolist()) * strain(f), strain(g)) * fem.dx)
    err = abs(float(Fraction(float(fun)) - exact))
    assert err <= 1e-14 * scale, (D, degree, float(fun), float(exact), err / (1e-14 * scale))
    return err / (1e-14 * scale)


@pytest.fixture
def numpy_backend():
    old = fem._backend
    fem.set_backend(FacetNumpyBackend())
    fem.clear_caches()
    yield fem.get_backend()
    fem.set_backend(old)
    fem.clear_caches()


@pytest.mark.parametrize("case", sorted(FRONTEND))
def test_frontend_functionals_are_exact_on_the_oracle(numpy_backend, case):
    name, degree = FRONTEND[case]
    assert isinstance(numpy_backend, NumpyBackend)
    check_frontend_functionals(frontend_mesh(name), degree)


@pytest.mark.parametrize("case", sorted(FRONTEND))
def test_frontend_bilinear_forms_are_the_exact_atoms(numpy_backend, case):
    name, degree = FRONTEND[case]
    check_frontend_matrices(frontend_mesh(name), degree)


@pytest.mark.parametrize("name,degree", [("p1_tri_shear", 1), ("p1_tri_reversed", 2), ("p1_tet_reordered", 1),
                                         ("small_tet_shear", 2)])
def test_frontend_elasticity_is_exact(numpy_backend, name, degree):
    check_elasticity(frontend_mesh(name), degree)
