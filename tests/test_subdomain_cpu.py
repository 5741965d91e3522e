"""Cell-subdomain integrals dx(id) on a CPU: the Measure spellings and refusals, the grammar on CellNumpyBackend (the numpy
oracle plus masked atoms, tests/subdomain_reference.py), the atom caches against every way a MeshFunction changes, the
functional paths (plain and inside a functional_scope), vector-valued spaces and inclusion_heat against a direct solve."""
import numpy as np
import pytest
import scipy.sparse as sps
import scipy.sparse.linalg as spla

from oracle import fem_numpy as FN
from oracle.backend_numpy import NumpyBackend
from pgdrome_amd import fem, problems
from tests import subdomain_reference as SR
from tests import weighted_reference as W

P = fem.Point


@pytest.fixture(autouse=True)
def cell_backend():
    old = fem._backend
    be = fem.set_backend(SR.CellNumpyBackend())
    fem.clear_caches()
    yield be
    fem.set_backend(old)
    fem.clear_caches()


def _two_materials(mesh):
    """Cell markers 1 / 2: cells whose midpoint has x[0] below / above the middle of the mesh."""
    X, C = mesh.coordinates(), mesh.cells()
    mid = X[C].mean(axis=1)[:, 0]
    cf = fem.MeshFunction("size_t", mesh, mesh.topology().dim(), 1)
    cf.array()[mid > 0.5 * (X[:, 0].min() + X[:, 0].max())] = 2
    return cf


def _square():
    return fem.RectangleMesh(P(0, 0), P(1, 1), 6, 5, "crossed")


# ------------------------------------------------------------------------------------------------------- Measure
def test_measure_spellings():
    m = _square()
    cf = _two_materials(m)
    for meas in (fem.Measure("dx", domain=m, subdomain_data=cf)(1), fem.dx(m, subdomain_data=cf)(1),
                 fem.dx(1, domain=m, subdomain_data=cf), fem.dx(subdomain_data=cf)(1), fem.dx(subdomain_id=1, subdomain_data=cf)):
        assert meas.kind == "dx" and meas.mesh is m and meas.subdomain_data is cf and meas.subdomain_id == 1
    dxs = fem.Measure("dx", domain=m, subdomain_data=cf)
    assert dxs.subdomain_id is None and dxs(2).subdomain_id == 2 and dxs(np.int64(2)).subdomain_id == 2


def test_measure_refusals():
    m, other = _square(), _square()
    cf = _two_materials(m)
    with pytest.raises(ValueError):
        fem.dx(1)                                                           # an id without data
    with pytest.raises(ValueError):
        fem.Measure("dx", domain=m, subdomain_id=1)
    with pytest.raises(ValueError):
        fem.Measure("dx", domain=m, subdomain_data=fem.MeshFunction("size_t", m, 1, 0))(1)    # facet markers
    with pytest.raises(ValueError):
        fem.Measure("dx", domain=other, subdomain_data=cf)(1)              # data of another mesh
    with pytest.raises(ValueError):
        fem.Measure("dx", domain=m, subdomain_data=fem.MeshFunction("double", m, 2, 0.0))(1)
    with pytest.raises(ValueError):
        fem.Measure("dx", domain=m, subdomain_data=fem.MeshFunction("bool", m, 2, False))
    with pytest.raises(ValueError):
        fem.dx(1.5, domain=m, subdomain_data=cf)
    with pytest.raises(NotImplementedError):
        fem.Measure("dx", domain=m, subdomain_data=cf)((1, 2))
    with pytest.raises(NotImplementedError):
        fem.Measure("dx", domain=m, subdomain_data=cf, subdomain_id=(1, 2))
    # the integrand on another mesh than the markers
    V = fem.FunctionSpace(other, "CG", 1)
    u, v = fem.TrialFunction(V), fem.TestFunction(V)
    with pytest.raises(ValueError):
        fem.assemble(u * v * fem.dx(1, domain=m, subdomain_data=cf)).array()


def test_data_without_id_is_the_whole_domain(cell_backend):
    m = _square()
    cf = _two_materials(m)
    V = fem.FunctionSpace(m, "CG", 1)
    F = fem.interpolate(fem.Expression("1.0 + x[0]*x[1]", degree=1), V)
    u, v = fem.TrialFunction(V), fem.TestFunction(V)
    dxs = fem.Measure("dx", domain=m, subdomain_data=cf)
    assert fem.assemble(F * F * dxs) == fem.assemble(F * F * fem.dx(m))
    assert np.array_equal(fem.assemble(fem.inner(fem.grad(u), fem.grad(v)) * dxs).array(),
                          fem.assemble(fem.inner(fem.grad(u), fem.grad(v)) * fem.dx).array())
    assert cell_backend.cell_atoms == []


# ---------------------------------------------------------------------------------------------------- grammar
def _sum_checks(m, degree=1):
    cf = _two_materials(m)
    dxs = fem.Measure("dx", domain=m, subdomain_data=cf)
    V = fem.FunctionSpace(m, "CG", degree)
    F = fem.interpolate(fem.Expression("1.0 + x[0]*x[0]", degree=2), V)
    G = fem.interpolate(fem.Expression("2.0 - x[0]", degree=1), V)
    u, v = fem.TrialFunction(V), fem.TestFunction(V)
    gd = fem.inner(fem.grad(u), fem.grad(v))
    ax = m.geometry().dim() - 1
    # functionals
    for form in (lambda d: F * G * d, lambda d: fem.inner(fem.grad(F), fem.grad(G)) * d, lambda d: F.dx(0) * G * d,
                 lambda d: G * F * F * d, lambda d: fem.Constant(2.0) * d):
        whole, parts = fem.assemble(form(fem.dx(m))), fem.assemble(form(dxs(1))) + fem.assemble(form(dxs(2)))
        assert abs(whole - parts) <= 1e-13 * max(1.0, abs(whole))
        assert fem.assemble(form(dxs(1)) + form(dxs(2))) == pytest.approx(whole, rel=1e-13, abs=1e-13)
    # vectors
    for form in (lambda d: G * v * d, lambda d: fem.inner(fem.grad(F), fem.grad(v)) * d, lambda d: F.dx(0) * v * d):
        whole = fem.assemble(form(fem.dx(m))).get_local()
        parts = fem.assemble(form(dxs(1)) + form(dxs(2))).get_local()
        assert np.abs(whole - parts).max() <= 1e-13 * np.abs(whole).max()
    # matrices
    for form in (lambda d: gd * d, lambda d: u * v * d, lambda d: u.dx(0) * v.dx(ax) * d, lambda d: u.dx(ax) * v * d,
                 lambda d: G * u * v * d):
        whole = fem.assemble(form(fem.dx(m))).array()
        parts = fem.assemble(form(dxs(1)) + form(dxs(2))).array()
        assert np.abs(whole - parts).max() <= 1e-13 * np.abs(whole).max()
        one = fem.assemble(form(dxs(1))).array()
        assert np.abs(one).max() > 0 and np.abs(one - whole).max() > 0


@pytest.mark.parametrize("mk,degree", [(lambda: fem.IntervalMesh(9, 0.0, 1.0), 1), (lambda: fem.IntervalMesh(9, 0.0, 1.0), 2),
                                       (_square, 1), (_square, 2),
                                       (lambda: fem.BoxMesh(P(0, 0, 0), P(1, 1, 1), 3, 2, 3), 1)])
def test_subdomains_sum_to_the_whole_domain(mk, degree):
    _sum_checks(mk(), degree)


def test_cell_atoms_against_the_exact_subset_reference(cell_backend):
    m = fem.RectangleMesh(P(0, 0), P(1, 1), 3, 2, "crossed")
    lay = W.WeightedExactLayout(m.coordinates(), m.cells())
    ctx = cell_backend
    mh = ctx.mesh(m.coordinates(), m.cells())
    rp, cols = ctx.mesh_pattern(mh)
    for name, mask in SR.masks(m.num_cells(), seed=3).items():
        for kind, a, b in [(FN.MASS, 0, 0), (FN.STIFF, 0, 0), (FN.DUDV, 1, 0), (FN.CONV, 1, 0), (FN.CONVT, 0, 1)]:
            vals, S = SR.subset_atom(lay, kind, a, b, None, mask)
            got = SR.on_pattern(ctx._obj[ctx.atom_cells(mh, kind, a, b, 0, mask)][1], rp, cols)
            ex = np.array([float(x) for x in vals])
            assert np.all(np.abs(got - ex) <= 1e-14 * lay.row_max(S) + 1e-300), (name, kind)
            if name == "none":
                assert not any(vals)
            if name == "all":
                full, _ = lay.atom(kind, a, b)
                assert all(x == y for x, y in zip(vals, full))


# ------------------------------------------------------------------------------------------------- never stale
def _routes():
    def set_all(cf, m):
        cf.set_all(2)

    def item(cf, m):
        cf[0] = 2 if cf[0] == 1 else 1

    def mark(cf, m):
        class Left(fem.SubDomain):
            def inside(self, x, on_boundary):
                return x[0] <= 0.34
        Left().mark(cf, 2)

    def write(cf, m):
        cf.array()[:3] = 2

    return {"set_all": set_all, "item": item, "mark": mark, "array_write": write}


@pytest.mark.parametrize("route", sorted(_routes()))
def test_changed_markers_give_new_atoms(cell_backend, route):
    m = _square()
    cf = _two_materials(m)
    dxs = fem.Measure("dx", domain=m, subdomain_data=cf)
    V = fem.FunctionSpace(m, "CG", 1)
    F = fem.interpolate(fem.Expression("1.0 + x[0]", degree=1), V)
    u, v = fem.TrialFunction(V), fem.TestFunction(V)

    def direct():
        sel = cf.array() == 1
        K = FN.assemble_atom(m.coordinates(), m.cells()[sel], FN.STIFF) if sel.any() else sps.csr_matrix((V.dim(), V.dim()))
        M = FN.assemble_atom(m.coordinates(), m.cells()[sel], FN.MASS) if sel.any() else sps.csr_matrix((V.dim(), V.dim()))
        f = F.vector().get_local()
        return f @ (M @ f), M @ f, K

    def ours():
        return (fem.assemble(F * F * dxs(1)), fem.assemble(F * v * dxs(1)).get_local(),
                fem.assemble(fem.inner(fem.grad(u), fem.grad(v)) * dxs(1)))

    s0, b0, A0 = ours()
    n0 = len(cell_backend.cell_atoms)
    s1, b1, A1 = ours()                                    # unchanged markers: nothing is assembled again
    A1.array()
    n1 = len(cell_backend.cell_atoms)
    A0.array()
    assert len(cell_backend.cell_atoms) == n1 and s1 == s0 and np.array_equal(b1, b0)
    assert n1 == n0 + 1                                     # (the matrix's atom: assembled once, when first used)
    _routes()[route](cf, m)
    s2, b2, A2 = ours()
    ref_s, ref_b, ref_K = direct()
    assert len(cell_backend.cell_atoms) > n1
    assert s2 == pytest.approx(ref_s, rel=1e-12, abs=1e-14) and s2 != s0
    assert np.allclose(b2, ref_b, rtol=1e-12, atol=1e-14)
    p = fem.vertex_to_dof_map(V)
    assert np.allclose(A2.array(), ref_K.toarray()[np.ix_(p, p)], rtol=1e-12, atol=1e-12)


def test_functionals_in_and_out_of_a_scope(cell_backend):
    """assemble(F*G*dx(1)) never takes the whole domain, on repeated calls and inside a functional_scope whose plan was
    recorded before the markers changed."""
    m = _square()
    cf = _two_materials(m)
    dxs = fem.Measure("dx", domain=m, subdomain_data=cf)
    V = fem.FunctionSpace(m, "CG", 1)
    F = fem.interpolate(fem.Expression("1.0 + x[0]", degree=1), V)
    G = fem.interpolate(fem.Expression("2.0 + x[1]", degree=1), V)

    def ref(sid):
        sel = cf.array() == sid
        M = FN.assemble_atom(m.coordinates(), m.cells()[sel], FN.MASS)
        return F.vector().get_local() @ (M @ G.vector().get_local())

    whole = fem.assemble(F * G * fem.dx(m))
    for _ in range(3):
        for sid in (1, 2):
            assert fem.assemble(F * G * dxs(sid)) == pytest.approx(ref(sid), rel=1e-13)
            assert abs(fem.assemble(F * G * dxs(sid)) - whole) > 1e-3 * abs(whole)
    for rep in range(4):
        if rep == 2:
            cf.array()[: m.num_cells() // 3] = 2
        with fem.functional_scope(("subdomain-test", 0), [F.vector()]):
            v1, v2 = fem.assemble(F * G * dxs(1)), fem.assemble(G * F * dxs(2))
        assert v1 == pytest.approx(ref(1), rel=1e-13) and v2 == pytest.approx(ref(2), rel=1e-13)
        assert v1 + v2 == pytest.approx(whole, rel=1e-13)


def test_vector_valued_spaces_embed_the_masked_atom(cell_backend):
    m = _square()
    cf = _two_materials(m)
    dxs = fem.Measure("dx", domain=m, subdomain_data=cf)
    V = fem.VectorFunctionSpace(m, "CG", 1)
    u, v = fem.TrialFunction(V), fem.TestFunction(V)

    forms = [lambda d: fem.inner(u, v) * d, lambda d: u[0] * v[1] * d, lambda d: u[1].dx(0) * v[0].dx(1) * d]
    for form in forms:
        whole = fem.assemble(form(fem.dx(m))).array()
        one, two = fem.assemble(form(dxs(1))).array(), fem.assemble(form(dxs(2))).array()
        assert np.abs(one + two - whole).max() <= 1e-13 * np.abs(whole).max()
        assert np.abs(one).max() > 0 and np.abs(two).max() > 0
    # the blocks of the masked scalar atom
    Vs = fem.FunctionSpace(m, "CG", 1)
    us, vs = fem.TrialFunction(Vs), fem.TestFunction(Vs)
    Ms = fem.assemble(us * vs * dxs(1)).array()
    Mv = fem.assemble(fem.inner(u, v) * dxs(1)).array()
    assert np.count_nonzero(Mv) == 2 * np.count_nonzero(Ms) and Mv.sum() == pytest.approx(2 * Ms.sum(), rel=1e-14)
    assert np.allclose(np.sort(Mv.ravel())[-2 * np.count_nonzero(Ms):], np.sort(np.repeat(Ms[Ms != 0], 2)), rtol=0, atol=1e-16)
    # a marker change frees the masked source and the embeddings built from it
    lay = V._lay
    cf.array()[:4] = 2
    Mv2 = fem.assemble(fem.inner(u, v) * dxs(1)).array()
    assert np.abs(Mv2 - Mv).max() > 0
    assert len(lay.base._cell_atoms) == 1
    assert {k[1] for k in lay._catoms} == {a for a, _, _ in lay.base._cell_atoms.values()}


def test_elasticity_two_materials_sums(cell_backend):
    m = fem.BoxMesh(P(0, 0, 0), P(1, 1, 1), 2, 3, 2)
    cf = _two_materials(m)
    dxs = fem.Measure("dx", domain=m, subdomain_data=cf)
    V = fem.VectorFunctionSpace(m, "CG", 1)
    u, v = fem.TrialFunction(V), fem.TestFunction(V)
    C = problems._voigt_C(0.3)
    e = fem.inner(C * problems._strain(u), problems._strain(v))
    whole = fem.assemble(3.0 * e * fem.dx(m)).array()
    A = fem.assemble(3.0 * e * dxs(1) + 3.0 * e * dxs(2))
    assert A.is_symmetric()
    assert np.abs(A.array() - whole).max() <= 1e-13 * np.abs(whole).max()
    B = fem.assemble(1.0 * e * dxs(1) + 5.0 * e * dxs(2)).array()
    assert np.abs(B - whole).max() > 1e-3 * np.abs(whole).max()


# ---------------------------------------------------------------------------------------------------- refusals
def test_backend_without_atom_cells_refuses():
    fem.set_backend(NumpyBackend())
    m = _square()
    cf = _two_materials(m)
    V = fem.FunctionSpace(m, "CG", 1)
    F = fem.interpolate(fem.Expression("1.0", degree=1), V)
    with pytest.raises(NotImplementedError, match="atom_cells"):
        fem.assemble(F * F * fem.dx(1, domain=m, subdomain_data=cf))
    u, v = fem.TrialFunction(V), fem.TestFunction(V)
    with pytest.raises(NotImplementedError, match="atom_cells"):
        fem.assemble(u * v * fem.dx(1, domain=m, subdomain_data=cf)).array()


def test_sharded_layout_refuses():
    c, e = FN.box_mesh((0, 0, 0), (1, 1, 1), 2, 2, 3)
    n = c.shape[0]
    mesh = fem.Mesh(c, e, part=fem.Partition(None, 0, n, n, 0, 0, 0))
    cf = fem.MeshFunction("size_t", mesh, 3, 1)
    lay = mesh.layout(1)
    with pytest.raises(NotImplementedError, match="sharded"):
        lay.atom(FN.MASS, cells=fem._CellSet(cf, 1))
    with pytest.raises(NotImplementedError, match="sharded"):
        fem._block_layout(mesh, 1, 3).atom(FN.MASS, cells=fem._CellSet(cf, 1), cv=0, cu=0)


# ---------------------------------------------------------------------------------------------- inclusion_heat
def direct_inclusion(spec):
    """The separated two-material problem as ONE linear system over space x kappa, solved directly: U[:, j] is the discrete
    solution at the kappa node j that the PGD expansion converges to."""
    mesh, kmesh = spec["Vs"][0].mesh(), spec["Vs"][1].mesh()
    X, C = mesh.coordinates(), mesh.cells()
    kx, kc = kmesh.coordinates(), kmesh.cells()
    mk = spec["param"]["markers"].array()
    Ko = FN.assemble_atom(X, C[mk == problems.OUTSIDE], FN.STIFF)
    Ki = FN.assemble_atom(X, C[mk == problems.INCLUSION], FN.STIFF)
    M = FN.assemble_atom(X, C, FN.MASS)
    Mk, Wk = FN.assemble_atom(kx, kc, FN.MASS), FN.assemble_atom(kx, kc, FN.WMASS, 0, 0, kx[:, 0].copy())
    nx, nk = X.shape[0], kx.shape[0]
    A = (sps.kron(Ko, Mk) + sps.kron(Ki, Wk)).tocsr()
    b = spec["param"]["f"] * np.kron(M @ np.ones(nx), Mk @ np.ones(nk))
    free = np.where(~np.repeat(mesh.vertex_on_boundary(), nk))[0]
    U = np.zeros(nx * nk)
    U[free] = spla.spsolve(A[free][:, free].tocsc(), b[free])
    return U.reshape(nx, nk)


INCLUSION_TOL = 1e-5


def check_inclusion_heat(spec, p, js):
    sol = p.return_PGD()
    U = direct_inclusion(spec)
    knodes = spec["Vs"][1].mesh().coordinates()[:, 0]
    errs = []
    for j in js:
        u = sol.evaluate(0, [1], [knodes[j]], 0).compute_vertex_values()
        errs.append(float(np.linalg.norm(u - U[:, j]) / np.linalg.norm(U[:, j])))
    print("inclusion_heat: modes %d, relative L2 errors at kappa = %s: %s" % (p.PGD_modes, list(knodes[list(js)]), errs))
    assert max(errs) <= INCLUSION_TOL
    return errs


def test_inclusion_heat_against_a_direct_solve(cell_backend):
    from pgdrome_amd.solver import PGDProblem
    spec = problems.inclusion_heat(fem.RectangleMesh(P(0, 0), P(1, 1), 12, 12, "crossed"), n_k=9, k_range=(0.1, 10.0),
                                   PGD_nmax=15, PGD_tol=1e-9)
    mk = spec["param"]["markers"].array()
    assert (mk == problems.INCLUSION).sum() > 0 and (mk == problems.OUTSIDE).sum() > 0
    p = PGDProblem(**spec)
    p.solve_PGD(_problem="linear")
    check_inclusion_heat(spec, p, [0, 2, 4, 6, 8])
