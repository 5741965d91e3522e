"""Robin boundary terms on the MI355X: the facet atom (pgd_atom_assemble_facets) against a scipy assembly of the
closed-form facet masses, the frontend's bilinear ds grammar, the structured-grid products of an operator that
contains it, and the parametric Robin heat problem end to end against direct FEM solves."""
import numpy as np
import pytest
import scipy.sparse as sps
import scipy.sparse.linalg as spla

from oracle import fem_numpy as FN
from pgdrome_amd import fem, problems
from pgdrome_amd._lib import PgdError
from tests.robin_reference import facet_mass_matrix, facet_measures, on_pattern

pytestmark = pytest.mark.gpu
P = fem.Point


@pytest.fixture(scope="module", autouse=True)
def hip_backend():
    from pgdrome_amd.hip_backend import HipBackend
    old = fem._backend
    be = fem.set_backend(HipBackend(0))
    fem.clear_caches()
    yield be
    fem.set_backend(old)
    fem.clear_caches()


LAYOUTS = {
    "p1_interval": (lambda: fem.IntervalMesh(12, -1.0, 2.0), 1),
    "p1_rect_right": (lambda: fem.RectangleMesh(P(0, 0), P(2, 1), 7, 5), 1),
    "p1_rect_crossed": (lambda: fem.RectangleMesh(P(0, 0), P(1, 1), 6, 4, "crossed"), 1),
    "p1_box": (lambda: fem.BoxMesh(P(0, 0, 0), P(1, 2, 1.5), 5, 4, 6), 1),
    "p2_interval": (lambda: fem.IntervalMesh(9, 0.0, 1.0), 2),
    "p2_triangle": (lambda: fem.RectangleMesh(P(0, 0), P(1, 1), 5, 4, "crossed"), 2),
    "p2_tetrahedron": (lambda: fem.BoxMesh(P(0, 0, 0), P(1, 1, 2), 3, 4, 3), 2),
}


def _facet_sets(mesh):
    fv, ext = mesh.facets()
    mf = fem.MeshFunction("size_t", mesh, mesh.topology().dim() - 1, 0)
    X = mesh.coordinates()
    right = np.where(ext & (X[fv, 0].min(axis=1) > X[:, 0].max() - 1e-12))[0]
    mf.array()[right] = 7
    return {"exterior": fem._ds_facet_ids(mesh, fem.ds(mesh)),
            "tagged": fem._ds_facet_ids(mesh, fem.Measure("ds", domain=mesh, subdomain_data=mf)(7))}


@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_facet_atom_values(ctx, name):
    mk, degree = LAYOUTS[name]
    mesh = mk()
    lay = mesh.layout(degree)
    mh = ctx.mesh_upload(lay.coords, lay.cells)
    rp, cols = ctx.mesh_pattern(mh)
    try:
        for key, ids in _facet_sets(mesh).items():
            assert ids.size > 0
            tup = fem._facet_node_tuples(lay, ids)
            a = ctx.atom_assemble_facets(mh, tup)
            got = ctx.atom_download(a, cols.size)
            ref = on_pattern(facet_mass_matrix(lay.coords, tup, lay.n), rp, cols)
            # every entry to 1e-14 relative; entries outside the facet couplings exactly 0
            assert np.all(np.abs(got - ref) <= 1e-14 * np.abs(ref)), (key, np.max(np.abs(got - ref)))
            R = sps.csr_matrix((got, cols, rp), shape=(lay.n, lay.n))
            one = np.ones(lay.n)
            assert abs(one @ (R @ one) - facet_measures(lay.coords, tup[:, :mesh.topology().dim()]).sum()) <= \
                1e-13 * facet_measures(lay.coords, tup[:, :mesh.topology().dim()]).sum()
            b = ctx.atom_assemble_facets(mh, tup)
            assert np.array_equal(ctx.atom_download(b, cols.size), got)          # bit-identical from run to run
            ctx.atom_free(a)
            ctx.atom_free(b)
    finally:
        ctx.mesh_free(mh)


def test_facet_atom_rejects_bad_facets(ctx):
    mesh = fem.RectangleMesh(P(0, 0), P(1, 1), 6, 6)
    lay = mesh.layout(1)
    mh = ctx.mesh_upload(lay.coords, lay.cells)
    try:
        for bad in (np.array([[0, 48]]),                     # two corners of the square: not coupled, not a facet of the mesh
                    np.array([[0, 49]]),                     # node out of range
                    np.array([[0, 1, 2]])):                  # three nodes per facet on a P1 triangle layout
            with pytest.raises(PgdError) as e:
                ctx.atom_assemble_facets(mh, bad)
            assert e.value.code == -1
        good = ctx.atom_assemble_facets(mh, np.array([[0, 1]]))       # the context is fine afterwards
        ctx.atom_free(good)
    finally:
        ctx.mesh_free(mh)


def _host_matrix(A):
    be = fem.get_backend()
    op = A.op()
    rp, cols = be.mesh_pattern(A.lay.handle())
    vals = be.atom_values(op, cols.size)
    be.atom_free(op)
    return sps.csr_matrix((vals, cols, rp), shape=(A.lay.n, A.lay.n))


class _RightFace(fem.SubDomain):
    def inside(self, x, on_boundary):
        return (x[0] > 1.0 - 1e-12) & on_boundary


@pytest.mark.parametrize("vector", [False, True])
@pytest.mark.parametrize("name", ["p1_rect_crossed", "p2_triangle", "p1_box", "p2_tetrahedron"])
def test_frontend_robin_forms(name, vector):
    mesh = LAYOUTS[name][0]()
    degree = LAYOUTS[name][1]
    gdim = mesh.geometry().dim()
    mf_sub = fem.MeshFunction("size_t", mesh, gdim - 1, 0)
    _RightFace().mark(mf_sub, 4)                                     # markers by SubDomain ...
    mf_arr = fem.MeshFunction("size_t", mesh, gdim - 1, 0)
    fv, ext = mesh.facets()
    mf_arr.array()[np.where(ext & (mesh.coordinates()[fv, 1].max(axis=1) < 1e-12))[0]] = 5      # ... and by hand
    measures = [fem.ds(mesh), fem.Measure("ds", domain=mesh, subdomain_data=mf_sub)(4),
                fem.Measure("ds", domain=mesh, subdomain_data=mf_arr)(5)]
    if vector:
        V = fem.VectorFunctionSpace(mesh, "CG", degree)
        e = tuple("1.0 + x[0]*x[%d]" % k for k in range(gdim))
        F = fem.interpolate(fem.Expression(e, degree=2), V)
        G = fem.interpolate(fem.Expression(tuple("2.0 - x[%d]" % ((k + 1) % gdim) for k in range(gdim)), degree=1), V)
        scalar = V._lay.base
    else:
        V = fem.FunctionSpace(mesh, "CG", degree)
        F = fem.interpolate(fem.Expression("1.0 + x[0]*x[0]", degree=2), V)
        G = fem.interpolate(fem.Expression("2.0 - 0.5*x[1]", degree=1), V)
        scalar = V._lay
    u, v = fem.TrialFunction(V), fem.TestFunction(V)
    f, g = F._vec.host(), G._vec.host()
    for m in measures:
        Rs = facet_mass_matrix(scalar.coords, fem._facet_node_tuples(scalar, fem._ds_facet_ids(mesh, m)), scalar.n)
        assert Rs.nnz > 0
        R = sps.kron(Rs, sps.eye(gdim)).tocsr() if vector else Rs
        A = _host_matrix(fem.assemble(fem.Constant(1.5) * (fem.dot(u, v) if vector else u * v) * m))
        assert np.max(np.abs((A - 1.5 * R).toarray())) <= 1e-14 * np.max(np.abs(R.toarray()))
        fg = fem.assemble((fem.dot(F, G) if vector else F * G) * m)
        assert abs(fg - f @ (R @ g)) <= 1e-13 * (np.abs(f) @ (np.abs(R) @ np.abs(g)))
        b = fem.assemble((fem.dot(F, v) if vector else F * v) * m).host()
        assert np.max(np.abs(b - R @ f)) <= 1e-13 * np.max(np.abs(R) @ np.abs(f))
        if vector:
            A10 = _host_matrix(fem.assemble(u[0] * v[1] * m))
            E = sps.csr_matrix(([1.0], ([1], [0])), shape=(gdim, gdim))
            assert np.max(np.abs((A10 - sps.kron(Rs, E)).toarray())) <= 1e-14 * np.max(np.abs(Rs.toarray()))


def test_structured_robin_operator(hip_backend):
    """48^3 box, K + h R with R on all six faces: the default product (diagonal form + its row classes, as a solve or a host-driven
    loop sets them up) equals the CSR product bit for bit, runs in k_spmv_diac_march2, and the PCG solve agrees with a sparse direct
    solve."""
    ctx = hip_backend.ctx
    mesh = fem.BoxMesh(P(0, 0, 0), P(1, 1, 1), 47, 47, 47)
    lay = mesh.layout(1)
    n = lay.n
    mh = lay.handle()
    K = lay.atom(fem.STIFF)
    tup = fem._facet_node_tuples(lay, fem._ds_facet_ids(mesh, fem.ds(mesh)))
    R = ctx.atom_assemble_facets(mh, tup)
    h = 3.7
    x = np.random.default_rng(1).uniform(-1, 1, n)
    xv, yv = ctx.vec_from(x), ctx.vec_alloc(n)
    try:
        ctx.tune(7, 3)                                               # the z-march on this grid size, as at the bench sizes
        op = ctx.op_combine(mh, [K, R], [1.0, h])
        classes = ctx.op_classify(op)
        c0 = ctx.kernel_counts()
        ctx.spmv(op, xv, yv)
        kc = ctx.kernel_counts()
        y_fast = ctx.vec_download(yv)
        ctx.tune(7, 0)
        ctx.tune(27, 0)
        ctx.tune(14, 0)
        op_csr = ctx.op_combine(mh, [K, R], [1.0, h])
        ctx.spmv(op_csr, xv, yv)
        y_csr = ctx.vec_download(yv)
    finally:
        ctx.tune(7, 0)
        ctx.tune(27, 1)
        ctx.tune(14, 1)
    print("robin structured product: %d row classes, kernels %s" % (classes, {k: kc[k] - c0[k] for k in kc}))
    assert classes > 0 and kc["diac_march"] == c0["diac_march"] + 1
    assert np.array_equal(y_fast, y_csr)
    rp, cols = ctx.mesh_pattern(mh)
    A = sps.csr_matrix((ctx.atom_download(op_csr, cols.size), cols, rp), shape=(n, n))
    Kh = sps.csr_matrix((ctx.atom_download(K, cols.size), cols, rp), shape=(n, n))
    Rh = facet_mass_matrix(lay.coords, tup, n)
    assert abs(spla.norm(A - Kh - h * Rh)) <= 1e-13 * spla.norm(A)
    b = A @ np.ones(n) + 0.1 * x
    bv, sv = ctx.vec_from(b), ctx.vec_alloc(n)
    ctx.vec_fill(sv, 0.0)
    c0 = ctx.kernel_counts()
    it, rel = ctx.pcg_solve(op, bv, sv, 1e-12, 0.0, 20000)
    kc = ctx.kernel_counts()
    print("robin structured PCG: %d iterations, kernels %s" % (it, {k: kc[k] - c0[k] for k in kc}))
    ref = spla.spsolve(A.tocsc(), b)
    assert np.linalg.norm(ctx.vec_download(sv) - ref) <= 1e-8 * np.linalg.norm(ref), (it, rel)
    for hdl in (op, op_csr, R):
        ctx.atom_free(hdl)
    for v in (xv, yv, bv, sv):
        ctx.vec_free(v)


def _direct_robin(spec):
    """The separated Robin heat problem as ONE linear system over space x h, assembled here (oracle P1 atoms, the closed-form
    facet masses, Kronecker products) and solved directly: U[:, j] is the discrete solution at the h node j that the PGD
    expansion converges to."""
    mesh, hmesh = spec["Vs"][0].mesh(), spec["Vs"][1].mesh()
    X, C = mesh.coordinates(), mesh.cells()
    hx, hc = hmesh.coordinates(), hmesh.cells()
    par = spec["param"]
    K, M = FN.assemble_atom(X, C, FN.STIFF), FN.assemble_atom(X, C, FN.MASS)
    tup = fem._facet_node_tuples(mesh.layout(1), fem._ds_facet_ids(mesh, par["ds_robin"]))
    R = facet_mass_matrix(X, tup, X.shape[0])
    Mh, Wh = FN.assemble_atom(hx, hc, FN.MASS), FN.assemble_atom(hx, hc, FN.WMASS, 0, 0, hx[:, 0].copy())
    nx, nh = X.shape[0], hx.shape[0]
    A = (sps.kron(par["k"] * K, Mh) + sps.kron(R, Wh)).tocsr()
    b = np.kron(M @ np.ones(nx), Mh @ np.ones(nh)) + par["u_inf"] * np.kron(R @ np.ones(nx), Wh @ np.ones(nh))
    fixed = mesh.vertex_on_boundary() & (X[:, 0] < X[:, 0].min() + 1e-10)
    free = np.where(~np.repeat(fixed, nh))[0]
    U = np.zeros(nx * nh)
    U[free] = spla.spsolve(A[free][:, free].tocsc(), b[free])
    return U.reshape(nx, nh)


# relative L2 at the sampled h nodes, PGD (20 modes, fixed-point tol 1e-8) vs the direct solve of the separated system: measured
# 1.0e-6 (h = 0.1) and below 7e-7 elsewhere with the numpy oracle plus reference facet atoms; bar ten times that
ROBIN_TOL = 1e-5


def _check_against_direct(spec, p, js):
    sol = p.return_PGD()
    U = _direct_robin(spec)
    hnodes = spec["Vs"][1].mesh().coordinates()[:, 0]
    errs = []
    for j in js:
        u = sol.evaluate(0, [1], [hnodes[j]], 0).compute_vertex_values()
        errs.append(float(np.linalg.norm(u - U[:, j]) / np.linalg.norm(U[:, j])))
    print("robin_heat: modes %d, relative L2 errors at h = %s: %s" % (p.PGD_modes, list(hnodes[list(js)]), errs))
    assert max(errs) <= ROBIN_TOL
    return errs


def test_robin_heat_2d_against_direct_solves():
    from pgdrome_amd.solver import PGDProblem
    spec = problems.robin_heat(fem.RectangleMesh(P(0, 0), P(1, 1), 24, 24, "crossed"), n_h=17, h_range=(0.1, 100.0),
                               PGD_nmax=20, PGD_tol=1e-8)
    p = PGDProblem(**spec)
    p.solve_PGD(_problem="linear")
    _check_against_direct(spec, p, [0, 3, 8, 12, 16])


def test_robin_heat_box_multigrid_request(hip_backend):
    from pgdrome_amd.solver import PGDProblem

    def run(prec):
        fem.clear_caches()
        spec = problems.robin_heat(fem.BoxMesh(P(0, 0, 0), P(1, 1, 1), 32, 32, 32), n_h=9, h_range=(0.1, 100.0),
                                   PGD_nmax=6, PGD_tol=1e-8)
        p = PGDProblem(**spec)
        settings = {"linear_solver": "cg", "relative_tolerance": 1e-10}
        if prec is not None:
            settings["preconditioner"] = prec
        st0 = dict(fem.STATS)
        p.solve_PGD(_problem="linear", settings=settings)
        used = {k: fem.STATS.get(k, 0) - st0.get(k, 0) for k in ("linear_solves", "mg_solves")}
        return spec, p, used
    _, pj, uj = run(None)
    _, pm, um = run("amg")
    print("robin_heat box: jacobi %s, amg request %s" % (uj, um))
    assert pj.PGD_modes == pm.PGD_modes and pj.num_fp_it == pm.num_fp_it
    for d in range(2):
        for k in range(pj.PGD_modes):
            a, b = pj.PGD_func[d][k].compute_vertex_values(), pm.PGD_func[d][k].compute_vertex_values()
            assert np.linalg.norm(a - b) <= 1e-6 * np.linalg.norm(a)
    assert all(np.isfinite(f.compute_vertex_values()).all() for f in pj.PGD_func[0])
