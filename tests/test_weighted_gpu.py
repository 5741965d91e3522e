"""Weighted derivative atoms (kinds 7-9) on the MI355X: every kind and (da, db) against the exact rational reference
(tests/weighted_reference.py) in k_assemble_p1<D>, k_assemble_p2_interval and k_assemble_p2_simplex<D>, the identities
between the kinds, the C-ABI's refusals, the frontend on the HIP backend, a weighted operator through pgd_op_combine on a
structured grid, a variable-velocity convection-diffusion solve and the graded-material PGD problem end to end.

Bound: |got_ij - exact_ij| <= 1e-14 max_j S_ij per row (S_ij = sum over cells |K_e,ij|).  Run with -s to see the largest
error per kernel family as a fraction of the bound.
"""
from fractions import Fraction

import numpy as np
import pytest
import scipy.sparse as sps
import scipy.sparse.linalg as spla

from oracle import fem_numpy as FN
from pgdrome_amd import fem, problems
from pgdrome_amd._lib import PgdError
from tests import exact_reference as X
from tests import test_exact_cpu as T
from tests import test_weighted_cpu as TW
from tests import weighted_reference as W

pytestmark = pytest.mark.gpu

MESHES = X.mesh_matrix()
TOL = 1e-14
WORST = {}
P = fem.Point


def note(family, q):
    WORST[family] = max(WORST.get(family, 0.0), float(q))


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    print("\nlargest error / bound per kernel family and new kind:")
    for k in sorted(WORST):
        print("  %-44s %.4f" % (k, WORST[k]))


@pytest.fixture(scope="module")
def hip_backend():
    from pgdrome_amd.hip_backend import HipBackend
    old = fem._backend
    be = fem.set_backend(HipBackend(0))
    fem.clear_caches()
    yield be
    fem.set_backend(old)
    fem.clear_caches()


def asm_family(lay, lattice=None):
    if lay.degree == 2:
        return "assemble_p2_interval" if lay.D == 1 else "assemble_p2_simplex<%d>" % lay.D
    return "assemble_p1<%d>" % lay.D + ("" if lattice is None else " lattice knob %d" % lattice)


def device_atom(ctx, h, kind, a, b, w, nnz):
    wv = ctx.vec_from(w) if w is not None else 0
    try:
        at = ctx.atom_assemble(h, kind, a, b, wv)
        got = ctx.atom_download(at, nnz)
        ctx.atom_free(at)
    finally:
        if wv:
            ctx.vec_free(wv)
    return got


def check_new_atoms(ctx, h, lay, w, family):
    out = {}
    for kind, a, b in W.kinds_and_pairs(lay.D):
        got = device_atom(ctx, h, kind, a, b, w, lay.nnz)
        vals, S = lay.atom(kind, a, b, w)
        q = X.entry_excess(lay, got, vals, S, TOL)
        note("%s %s" % (family, W.KIND_NAMES[kind]), q)
        assert q <= 1.0, (family, W.KIND_NAMES[kind], a, b, q)
        out[(kind, a, b)] = got
    return out


@pytest.mark.parametrize("name", sorted(MESHES))
def test_new_atoms_are_exact(ctx, name):
    lay = W.WeightedExactLayout(*MESHES[name]())
    h = ctx.mesh_upload(lay.coords, lay.cells.astype(np.int32))
    try:
        check_new_atoms(ctx, h, lay, X.weight_of(lay.coords), asm_family(lay))
    finally:
        ctx.mesh_free(h)


@pytest.mark.parametrize("name", sorted(X.LATTICE_SHAPES))
def test_new_atoms_on_lattice_boxes_under_every_lattice_form(ctx, name):
    """Weighted kinds take k_assemble_p1<3> with lattice steps (never the unweighted regular kernel): exact under
    PGD_TUNE_ASM_LATTICE 1, 3 and 2, and the three forms bit for bit the same."""
    lay = W.WeightedExactLayout(*X.lattice_box(X.LATTICE_SHAPES[name]))
    h = ctx.mesh_upload(lay.coords, lay.cells.astype(np.int32))
    w = X.weight_of(lay.coords)
    got = {}
    try:
        assert ctx.mesh_lattice(h)[0]
        for knob in (1, 3, 2):
            ctx.tune(20, knob)
            got[knob] = check_new_atoms(ctx, h, lay, w, asm_family(lay, knob))
    finally:
        ctx.tune(20, 1)
        ctx.mesh_free(h)
    for key in got[1]:
        assert np.array_equal(got[1][key], got[3][key]) and np.array_equal(got[1][key], got[2][key]), key


@pytest.mark.parametrize("name", ["p1_tri_crossed", "p1_tet_renumbered", "p2_tri_jitter", "p2_tet_reordered",
                                  "p2_interval_nonuniform"])
def test_identities_between_kinds(ctx, name):
    """sum_a WDUDV(a, a) = WSTIFF and WCONVT(b) = WCONV(b)^T within the bound; with w = 2, WDUDV = 2 DUDV."""
    lay = W.WeightedExactLayout(*MESHES[name]())
    h = ctx.mesh_upload(lay.coords, lay.cells.astype(np.int32))
    w = X.weight_of(lay.coords)
    rows = np.repeat(np.arange(lay.n), np.diff(lay.rp))
    try:
        tot = sum(device_atom(ctx, h, W.WDUDV, a, a, w, lay.nnz) for a in range(lay.D))
        ws = device_atom(ctx, h, X.WSTIFF, 0, 0, w, lay.nnz)
        S = sum(lay.atom(W.WDUDV, a, a, w)[1] for a in range(lay.D))
        assert np.all(np.abs(tot - ws) <= TOL * lay.row_max(S) * lay.D)
        for b in range(lay.D):
            c = device_atom(ctx, h, W.WCONV, b, 0, w, lay.nnz)
            ct = device_atom(ctx, h, W.WCONVT, 0, b, w, lay.nnz)
            A = sps.csr_matrix((c, lay.cols, lay.rp), shape=(lay.n, lay.n))
            At = sps.csr_matrix((ct, lay.cols, lay.rp), shape=(lay.n, lay.n))
            S = lay.atom(W.WCONV, b, 0, w)[1]
            Sm = sps.csr_matrix((S, lay.cols, lay.rp), shape=(lay.n, lay.n))
            bound = TOL * np.maximum(lay.row_max(S), np.asarray(Sm.T.max(axis=1).todense()).ravel()[rows])
            assert np.all(np.abs(np.asarray((A.T - At)[rows, lay.cols]).ravel()) <= 2 * bound)
            for a in range(lay.D):
                two = device_atom(ctx, h, W.WDUDV, a, b, np.full(lay.n, 2.0), lay.nnz)
                one = device_atom(ctx, h, X.DUDV, a, b, None, lay.nnz)
                S = lay.atom(X.DUDV, a, b)[1]
                assert np.all(np.abs(two - 2.0 * one) <= 2 * TOL * lay.row_max(S))
    finally:
        ctx.mesh_free(h)


def test_abi_refusals(ctx):
    c, e = FN.box_mesh((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), 2, 2, 2)
    h = ctx.mesh_upload(c, e)
    short = ctx.vec_from(np.ones(c.shape[0] - 1))
    ok = ctx.vec_from(np.ones(c.shape[0]))
    try:
        for kind in W.NEW_KINDS:
            for wv in (0, short):
                with pytest.raises(PgdError) as ei:
                    ctx.atom_assemble(h, kind, 0, 1, wv)
                assert ei.value.code == -1
            with pytest.raises(PgdError) as ei:
                ctx.atom_assemble(h, kind, 3, 0, ok)                   # derivative axis out of range
            assert ei.value.code == -1
            ctx.atom_free(ctx.atom_assemble(h, kind, 2, 1, ok))
        for kind in (10, -1):
            with pytest.raises(PgdError) as ei:
                ctx.atom_assemble(h, kind, 0, 0, ok)
            assert ei.value.code == -1
    finally:
        ctx.vec_free(short)
        ctx.vec_free(ok)
        ctx.mesh_free(h)


# ------------------------------------------------------------------------------------------ frontend on the device
@pytest.mark.parametrize("name,degree", TW.SCALAR)
def test_frontend_weighted_forms_on_the_device(hip_backend, name, degree):
    mesh = T.frontend_mesh(name)
    q, refs = TW.check_weighted_matrices(mesh, degree)
    note("frontend matrices", q)
    note("frontend functionals", TW.check_weighted_functionals(mesh, degree))
    note("frontend linear forms", TW.check_weighted_linear_forms(mesh, degree))


@pytest.mark.parametrize("name,degree", TW.ELASTIC)
def test_frontend_weighted_elasticity_on_the_device(hip_backend, name, degree):
    note("frontend weighted elasticity / density", TW.check_weighted_elasticity(T.frontend_mesh(name), degree))


def test_component_gradients_on_the_device(hip_backend):
    TW.check_component_gradients()


def test_weighted_structured_operator(hip_backend):
    """48^3 box, K + WDUDV(0, 1; w) + WCONV(2; w): the rows do not repeat, the row classes fall back without loss - the default
    product equals the CSR product bit for bit - and the operator is the sum of its atoms."""
    ctx = hip_backend.ctx
    mesh = fem.BoxMesh(P(0, 0, 0), P(1, 1, 1), 47, 47, 47)
    lay = mesh.layout(1)
    n, mh = lay.n, lay.handle()
    w = fem.Vector(lay.space(), 1.0 + lay.coords[:, 0] + 0.5 * lay.coords[:, 2] ** 2)
    atoms = [lay.atom(fem.STIFF), lay.atom(fem.WDUDV, 0, 1, w), lay.atom(fem.WCONV, 2, 0, w)]
    coefs = [1.0, 0.75, -2.5]
    x = np.random.default_rng(1).uniform(-1, 1, n)
    xv, yv = ctx.vec_from(x), ctx.vec_alloc(n)
    try:
        ctx.tune(7, 3)
        op = ctx.op_combine(mh, atoms, coefs)
        classes = ctx.op_classify(op)
        c0 = ctx.kernel_counts()
        ctx.spmv(op, xv, yv)
        kc = ctx.kernel_counts()
        y_fast = ctx.vec_download(yv)
        ctx.tune(7, 0)
        ctx.tune(27, 0)
        ctx.tune(14, 0)
        op_csr = ctx.op_combine(mh, atoms, coefs)
        ctx.spmv(op_csr, xv, yv)
        y_csr = ctx.vec_download(yv)
    finally:
        ctx.tune(7, 0)
        ctx.tune(27, 1)
        ctx.tune(14, 1)
    print("weighted structured product: %d row classes, kernels %s" % (classes, {k: kc[k] - c0[k] for k in kc}))
    assert np.array_equal(y_fast, y_csr)
    rp, cols = ctx.mesh_pattern(mh)
    A = sps.csr_matrix((ctx.atom_download(op_csr, cols.size), cols, rp), shape=(n, n))
    parts = [sps.csr_matrix((ctx.atom_download(a, cols.size), cols, rp), shape=(n, n)) for a in atoms]
    assert spla.norm(A - sum(c * p for c, p in zip(coefs, parts))) <= 1e-14 * spla.norm(A)
    for hdl in (op, op_csr):
        ctx.atom_free(hdl)
    for v in (xv, yv):
        ctx.vec_free(v)


def _exact_csr(ex, kind, a=0, b=0, w=None):
    vals, _ = ex.atom(kind, a, b, w)
    return sps.csr_matrix((np.array([float(v) for v in vals]), ex.cols, ex.rp), shape=(ex.n, ex.n))


def test_rotating_flow_convection_diffusion(hip_backend):
    """kappa grad u . grad v + b . grad u v = v, u = 0 on the boundary, b = (-(y - 1/2), x - 1/2): BiCGStab, against spsolve of
    the exact-reference matrix."""
    mesh = fem.UnitSquareMesh(16, 16)
    V = fem.FunctionSpace(mesh, "P", 1)
    kappa = 0.0625
    bx, by = fem.Expression("-(x[1] - 0.5)", degree=1), fem.Expression("x[0] - 0.5", degree=1)
    u, v = fem.TrialFunction(V), fem.TestFunction(V)
    a = fem.Constant(kappa) * fem.inner(fem.grad(u), fem.grad(v)) * fem.dx + (bx * u.dx(0) * v + by * u.dx(1) * v) * fem.dx
    L = fem.Constant(1.0) * v * fem.dx
    sol = fem.Function(V)
    info = fem.solve(a == L, sol, fem.DirichletBC(V, 0.0, lambda x, on_boundary: on_boundary),
                     solver_parameters={"relative_tolerance": 1e-13, "maximum_iterations": 20000})
    print("rotating flow: %s" % (info,))
    assert info["method"] == "jacobi_bicgstab"
    lay = V._lay
    ex = W.WeightedExactLayout(lay.coords, lay.cells)
    A = (kappa * _exact_csr(ex, X.STIFF) + _exact_csr(ex, W.WCONV, 0, 0, -(lay.coords[:, 1] - 0.5))
         + _exact_csr(ex, W.WCONV, 1, 0, lay.coords[:, 0] - 0.5))
    b = _exact_csr(ex, X.MASS) @ np.ones(ex.n)
    free = np.where(~lay.on_boundary())[0]
    ref = np.zeros(ex.n)
    ref[free] = spla.spsolve(A[free][:, free].tocsc(), b[free])
    got = sol.vector().host()
    err = np.linalg.norm(got - ref) / np.linalg.norm(ref)
    print("rotating flow: relative error against the direct solve %.3e" % err)
    assert err <= 1e-8


def test_weighted_operator_multigrid_request_takes_jacobi_pcg(hip_backend):
    """sum_a w u_{,a} v_{,a} on a box (SPD, not one stencil): an "amg" request is answered by the Jacobi-PCG."""
    mesh = fem.BoxMesh(P(0, 0, 0), P(1, 1, 1), 16, 16, 16)
    V = fem.FunctionSpace(mesh, "P", 1)
    w = fem.interpolate(fem.Expression("1 + x[0] + x[1]*x[2]", degree=1), V)
    u, v = fem.TrialFunction(V), fem.TestFunction(V)
    a = sum(w * u.dx(k) * v.dx(k) * fem.dx for k in range(3))
    sol = fem.Function(V)
    st0 = fem.STATS.get("mg_solves", 0)
    info = fem.solve(a == fem.Constant(1.0) * v * fem.dx, sol, fem.DirichletBC(V, 0.0, lambda x, on_boundary: on_boundary),
                     solver_parameters={"preconditioner": "amg", "relative_tolerance": 1e-10})
    print("weighted operator, amg request: %s" % (info,))
    assert info["method"] == "jacobi_pcg" and fem.STATS.get("mg_solves", 0) == st0


def _exact_block(ex, kind, a, b, w=None):
    vals, _ = ex.atom(kind, a, b, w)
    return sps.csr_matrix((np.array([float(t) for t in vals]), ex.cols, ex.rp), shape=(ex.n, ex.n)).toarray()


def _direct_graded(spec, nu=0.3, k_found=2.0):
    """The separated graded-block problem as ONE system over space x theta (Kronecker products), solved directly.  The space
    blocks come from the exact reference (dudv / wdudv per strain pair, mass per component; dof = 3 node + component), not
    from the library, so the comparison checks the weighted atoms as well as the PGD separation."""
    Vx, Vt = spec["Vs"]
    base = Vx._lay.base
    ex = W.WeightedExactLayout(base.coords, base.cells)
    g = spec["param"]["grading"]
    wn = g.eval_at(base.coords) if isinstance(g, fem.Expression) else g.vector().host()
    lam, mu = nu / ((1.0 + nu) * (1.0 - 2.0 * nu)), 1.0 / (2.0 * (1.0 + nu))
    C = np.diag([lam + 2 * mu] * 3 + [mu] * 3)
    C[:3, :3] += lam * (1 - np.eye(3))
    n3 = 3 * ex.n
    K1, Kg, M = np.zeros((n3, n3)), np.zeros((n3, n3)), np.zeros((n3, n3))
    for r in range(6):
        for s in range(6):
            if C[r, s] == 0.0:
                continue
            for c, a in T.VOIGT[3][s]:                       # trial u[c]_{,a}
                for d, b in T.VOIGT[3][r]:                   # test v[d]_{,b}
                    K1[d::3, c::3] += C[r, s] * _exact_block(ex, X.DUDV, a, b)
                    Kg[d::3, c::3] += C[r, s] * _exact_block(ex, W.WDUDV, a, b, wn)
    Ms = _exact_block(ex, X.MASS, 0, 0)
    for c in range(3):
        M[c::3, c::3] = Ms
    load = np.zeros(n3)
    load[2::3] = -Ms @ np.ones(ex.n)
    tx, tc = Vt.mesh().coordinates(), Vt.mesh().cells()
    Mt = FN.assemble_atom(tx, tc, FN.MASS).toarray()
    Wt = FN.assemble_atom(tx, tc, FN.WMASS, 0, 0, tx[:, 0].copy()).toarray()
    A = np.kron(K1, Mt) + np.kron(Kg, Wt) + k_found * np.kron(M, Mt)
    b = np.kron(load, Mt @ np.ones(tx.shape[0]))
    fixed = np.repeat(base.on_boundary() & (base.coords[:, 0] < 1e-12), 3)
    free = np.where(~np.repeat(fixed, tx.shape[0]))[0]
    U = np.zeros(A.shape[0])
    U[free] = np.linalg.solve(A[np.ix_(free, free)], b[free])
    return U.reshape(n3, tx.shape[0])


@pytest.mark.parametrize("degree", [1, 2])
def test_graded_block_against_direct_solve(hip_backend, degree):
    from pgdrome_amd.solver import PGDProblem
    mesh = fem.BoxMesh(P(0, 0, 0), P(1.0, 0.5, 0.5), 4, 2, 2) if degree == 1 else fem.BoxMesh(P(0, 0, 0), P(1.0, 0.5, 0.5), 2, 1, 1)
    grading = fem.Expression("x[0]*x[0] + 0.5*x[1]", degree=2)
    spec = problems.graded_block(mesh, grading, n_t=9, t_range=(0.0, 2.0), degree=degree, PGD_nmax=12, PGD_tol=1e-9)
    p = PGDProblem(**spec)
    p.solve_PGD(_problem="linear", settings={"linear_solver": "cg", "relative_tolerance": 1e-12})
    U = _direct_graded(spec)
    sol = p.return_PGD()
    tn = spec["Vs"][1].mesh().coordinates()[:, 0]
    errs = []
    for j in range(tn.size):
        u = sol.evaluate(0, [1], [tn[j]], 0)
        uv = np.asarray(u).ravel() if isinstance(u, np.ndarray) else u.vector().host()
        errs.append(float(np.linalg.norm(uv - U[:, j]) / np.linalg.norm(U[:, j])))
    print("graded_block P%d: %d modes, largest relative L2 error against the direct solve %.3e" % (degree, p.PGD_modes, max(errs)))
    assert max(errs) <= 1e-5
