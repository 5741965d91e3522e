"""Cell-weighted atoms (pgd_atom_assemble_cellwise) and DG0 coefficients in dx forms on the MI355X, against the exact rational
reference sum_c kappa_c K_c (tests/cellwise_reference.py).

Atoms: |got_ij - exact_ij| <= 1e-14 max_j S_ij per row, S_ij = sum_c |kappa_c| |K_c,ij| over the marked cells - the bound of
tests/test_exact_gpu.py and tests/test_subdomain_gpu.py, unchanged: the one extra multiply per local entry adds at most
2^-53 S_ij, about 1 % of it.  kappa = 1, kappa = a 0/1 indicator and kappa = 0.5 reproduce pgd_atom_assemble,
pgd_atom_assemble_cells and half the unweighted atom bit for bit (the factors 0, 1 and 2^k are exact, fused or not).
Run with -s for the largest error per kernel family."""
import ctypes as ct
from fractions import Fraction

import numpy as np
import pytest
import scipy.sparse as sps
import scipy.sparse.linalg as spla

from oracle import fem_numpy as FN
from pgdrome_amd import fem, problems
from pgdrome_amd._lib import PgdError
from tests import cellwise_reference as CR
from tests import exact_reference as X
from tests import subdomain_reference as SR
from tests import test_cellwise_cpu as CC
from tests import test_subdomain_gpu as SG
from tests import vmg_reference as V
from tests import weighted_reference as W

pytestmark = pytest.mark.gpu
P = fem.Point
TOL = 1e-14
WORST = {}

# the ten layouts of the masked atoms, and a lattice of 8 x 6 x 5 cells: 378 rows - more than one 256-row workgroup - with three
# different extents, the smallest shape at which the cube index and its strides can go wrong across a workgroup boundary
BIG = "lattice_8x6x5"
BIG_SHAPE = (8, 6, 5)
LAYOUTS = dict(SG.LAYOUTS)
LAYOUTS.update({"p1_lattice8x6x5_knob%d" % k: (BIG, k) for k in (1, 2, 3)})
_EXACT, _REF = {}, {}


def exact_layout(name):
    if name == BIG:
        if name not in _EXACT:
            _EXACT[name] = W.WeightedExactLayout(*X.lattice_box(BIG_SHAPE))
        return _EXACT[name]
    return SG.exact_layout(name)


def reference(name, lay, kind, a, b, w, kappa, mname, mask):
    """(values, S) of the exact sum, computed once per layout and shared by its knobs."""
    key = (name, kind, a, b, "all" if mname is None else mname)
    if key not in _REF:
        _REF[key] = CR.cellwise_atom(lay, kind, a, b, w, kappa, None if mname in (None, "all") else mask)
    return _REF[key]


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    print("\nlargest error / bound per family (cell-weighted atoms):")
    for k in sorted(WORST):
        print("  %-36s %.4f" % (k, WORST[k]))


def _family(name, lay, knob):
    return SG._family(lay, knob) + (" 8x6x5" if name == BIG else "")


@pytest.mark.parametrize("case", sorted(LAYOUTS))
def test_cell_weighted_atoms_are_exact(ctx, case):
    name, knob = LAYOUTS[case]
    lay = exact_layout(name)
    h = ctx.mesh_upload(lay.coords, lay.cells.astype(np.int32))
    w = X.weight_of(lay.coords)
    nc = lay.cells.shape[0]
    kappa = CR.dyadic_field(nc)
    wv, cv = ctx.vec_from(w), ctx.vec_from(kappa)
    fam = _family(name, lay, knob)
    masks = SR.masks(nc, seed=7)                   # (one set per layout: the reference is shared between the knobs)
    try:
        if knob is not None:
            assert ctx.mesh_lattice(h)[0]
            ctx.tune(20, knob)
        for kind, a, b in X.kinds_and_pairs(lay.D) + W.kinds_and_pairs(lay.D):
            weighted = kind >= X.WMASS
            S_full = reference(name, lay, kind, a, b, w if weighted else None, kappa, None, None)[1]
            for mname, mask in [(None, None)] + sorted(masks.items()):
                at = ctx.atom_assemble_cellwise(h, kind, a, b, wv if weighted else 0, cv, mask, nc)
                got = ctx.atom_download(at, lay.nnz)
                ctx.atom_free(at)
                vals, S = reference(name, lay, kind, a, b, w if weighted else None, kappa, mname, mask)
                q = SG.excess(lay, got, vals, S, S_full)
                WORST[fam] = max(WORST.get(fam, 0.0), q)
                assert q <= 1.0, (fam, mname, kind, a, b, q)
                if mname == "none":
                    assert not got.any(), (fam, kind, a, b)
                if mask is not None:
                    assert not got[~SR.touched(lay, mask)].any(), (fam, mname, kind, a, b)      # exact zeros off the subset
    finally:
        ctx.tune(20, 1)
        ctx.vec_free(wv)
        ctx.vec_free(cv)
        ctx.mesh_free(h)


@pytest.mark.parametrize("case", sorted(LAYOUTS))
def test_identities_bit_for_bit(ctx, case):
    name, knob = LAYOUTS[case]
    lay = exact_layout(name)
    h = ctx.mesh_upload(lay.coords, lay.cells.astype(np.int32))
    nc = lay.cells.shape[0]
    half = SR.masks(nc, seed=7)["half"]
    wv = ctx.vec_from(X.weight_of(lay.coords))
    one, ind, hv = ctx.vec_from(np.ones(nc)), ctx.vec_from(half.astype(np.float64)), ctx.vec_from(np.full(nc, 0.5))
    bits = lambda x: x.view(np.int64)

    def get(at):
        out = ctx.atom_download(at, lay.nnz)
        ctx.atom_free(at)
        return out
    try:
        if knob is not None:
            ctx.tune(20, knob)
        for kind, a, b in X.kinds_and_pairs(lay.D) + W.kinds_and_pairs(lay.D):
            ww = wv if kind >= X.WMASS else 0
            plain = get(ctx.atom_assemble(h, kind, a, b, ww))
            masked = get(ctx.atom_assemble_cells(h, kind, a, b, ww, half))
            assert np.array_equal(bits(get(ctx.atom_assemble_cellwise(h, kind, a, b, ww, one, None, nc))), bits(plain)), (case, kind, a, b)
            assert np.array_equal(bits(get(ctx.atom_assemble_cellwise(h, kind, a, b, ww, ind, None, nc))), bits(masked)), (case, kind, a, b)
            assert np.array_equal(bits(get(ctx.atom_assemble_cellwise(h, kind, a, b, ww, hv, None, nc))), bits(0.5 * plain)), (case, kind, a, b)
            # ... and composed with a mask: kappa = 1 over the marked cells is the masked atom
            assert np.array_equal(bits(get(ctx.atom_assemble_cellwise(h, kind, a, b, ww, one, half, nc))), bits(masked)), (case, kind, a, b)
    finally:
        ctx.tune(20, 1)
        for v in (wv, one, ind, hv):
            ctx.vec_free(v)
        ctx.mesh_free(h)


def test_invalid_arguments_leave_no_atom(ctx):
    lay = exact_layout("p1_tri_crossed")
    h = ctx.mesh_upload(lay.coords, lay.cells.astype(np.int32))
    nc = lay.cells.shape[0]
    blk = ctx.mesh_blocked(h, 2)
    cv, short, nodal = ctx.vec_from(np.ones(nc)), ctx.vec_from(np.ones(nc - 1)), ctx.vec_from(np.ones(lay.n))
    assert lay.n != nc
    try:
        a0 = ctx.atom_assemble(h, X.MASS)
        ctx.atom_free(a0)
        for call in (lambda: ctx.atom_assemble_cellwise(h, X.MASS, 0, 0, 0, cv, None, nc - 1),             # a wrong nc
                     lambda: ctx.atom_assemble_cellwise(h, X.MASS, 0, 0, 0, cv, np.ones(nc + 1, np.uint8)),
                     lambda: ctx.atom_assemble_cellwise(h, X.MASS, 0, 0, 0, short, None, nc),              # cvec of the wrong length
                     lambda: ctx.atom_assemble_cellwise(h, X.MASS, 0, 0, 0, nodal, None, nc),
                     lambda: ctx.atom_assemble_cellwise(h, X.MASS, 0, 0, 0, h, None, nc),                  # ... not a vector
                     lambda: ctx.atom_assemble_cellwise(h, X.MASS, 0, 0, 0, 0, None, nc),
                     lambda: ctx.atom_assemble_cellwise(blk, X.MASS, 0, 0, 0, cv, None, nc),               # a blocked layout
                     lambda: ctx.atom_assemble_cellwise(h, 42, 0, 0, 0, cv, None, nc),                     # an unknown kind
                     lambda: ctx.atom_assemble_cellwise(h, X.WMASS, 0, 0, 0, cv, None, nc),                # weighted, no wvec
                     lambda: ctx.atom_assemble_cellwise(h, X.DUDV, 2, 0, 0, cv, None, nc),                 # an axis out of range
                     lambda: ctx.atom_assemble_cellwise(h, X.DUDV, 0, -1, 0, cv, None, nc)):
            with pytest.raises(PgdError):
                call()
        out = ct.c_int64(0)
        assert ctx.lib.pgd_atom_assemble_cellwise(ctx.h, h, X.MASS, 0, 0, 0, short, None, nc, ct.byref(out)) == -1 and out.value == 0
        # no atom behind: the next atom takes the handle the first one had
        a1 = ctx.atom_assemble(h, X.MASS)
        assert a1 == a0
        ctx.atom_free(a1)
    finally:
        for v in (cv, short, nodal):
            ctx.vec_free(v)
        ctx.mesh_free(blk)
        ctx.mesh_free(h)


# ------------------------------------------------------------------------------------------ frontend on the device
@pytest.fixture(scope="module")
def hip_backend():
    from pgdrome_amd.hip_backend import HipBackend
    old = fem._backend
    be = fem.set_backend(HipBackend(0))
    fem.clear_caches()
    yield be
    fem.set_backend(old)
    fem.clear_caches()


MESHES = [lambda: fem.RectangleMesh(P(0, 0), P(1, 1), 5, 4, "crossed"), lambda: fem.BoxMesh(P(0, 0, 0), P(1, 1, 1), 3, 2, 3)]


@pytest.mark.parametrize("mk", MESHES)
def test_frontend_is_exact_on_the_device(hip_backend, mk):
    m = mk()
    kappa = CC._field(m)
    kv = kappa.vector().get_local()
    Vh = fem.FunctionSpace(m, "CG", 1)
    F = fem.interpolate(fem.Expression("1.0 + x[0]*x[0]/4", degree=2), Vh)
    G = fem.interpolate(fem.Expression("2.0 - x[0]/8", degree=1), Vh)
    u, v = fem.TrialFunction(Vh), fem.TestFunction(Vh)
    lay = W.WeightedExactLayout(m.coordinates(), m.cells())
    p = fem.vertex_to_dof_map(Vh)
    f, g = F.compute_vertex_values(), G.compute_vertex_values()
    csr = lambda S: sps.csr_matrix((S, lay.cols, lay.rp), shape=(lay.n, lay.n))
    for form, kind in [(kappa * F * G * fem.dx(m), X.MASS), (kappa * fem.inner(fem.grad(F), fem.grad(G)) * fem.dx(m), X.STIFF),
                       (F.dx(0) * kappa * G * fem.dx(m), X.CONVT)]:
        vals, S = CR.cellwise_atom(lay, kind, 0, 0, None, kv)
        ex = SG._exact_dot(f, vals, lay, g)
        got = fem.assemble(form)
        assert abs(Fraction(got) - ex) <= 1e-13 * float(np.abs(f) @ (csr(S) @ np.abs(g))), kind
    # load vector and matrix
    vals, S = CR.cellwise_atom(lay, X.MASS, 0, 0, None, kv)
    b_ex = np.array([float(t) for t in lay.matvec(vals, g)])
    b = fem.assemble(kappa * G * v * fem.dx).get_local()[p]
    assert np.all(np.abs(b - b_ex) <= 1e-13 * (csr(S) @ np.abs(g)) + 1e-300)
    vals, S = CR.cellwise_atom(lay, X.STIFF, 0, 0, None, kv)
    A = fem.assemble(3.0 * kappa * fem.inner(fem.grad(u), fem.grad(v)) * fem.dx).array()
    Ad = np.array([[float(t) for t in r] for r in lay.dense(vals)]) * 3.0
    Sd = lay.dense(S.astype(object))
    bound = 3e-14 * np.array([[float(t) for t in r] for r in Sd]).max(axis=1, keepdims=True)
    assert np.all(np.abs(A - Ad) <= bound + 1e-300)


@pytest.mark.parametrize("mk", MESHES)
def test_cell_weighted_elasticity(hip_backend, mk):
    """kappa inner(C eps(u), eps(v)) dx on a VectorFunctionSpace on the device against the oracle's cell-weighted atoms."""
    m = mk()
    D = m.geometry().dim()
    kappa = CC._field(m, CR.level_field(m.num_cells(), 5))
    Vh = fem.VectorFunctionSpace(m, "CG", 1)
    u, v = fem.TrialFunction(Vh), fem.TestFunction(Vh)
    if D == 3:
        energy = fem.inner(problems._voigt_C(0.3) * problems._strain(u), problems._strain(v))
    else:
        lam, mu = 0.6, 0.4
        energy = (2 * mu * (u[0].dx(0) * v[0].dx(0) + u[1].dx(1) * v[1].dx(1))
                  + mu * (u[0].dx(1) + u[1].dx(0)) * (v[0].dx(1) + v[1].dx(0))
                  + lam * (u[0].dx(0) + u[1].dx(1)) * (v[0].dx(0) + v[1].dx(1)))
    A = fem.assemble(kappa * energy * fem.dx)
    assert A.is_symmetric()
    got = A.array()
    old = fem._backend
    fem.set_backend(CR.CellwiseNumpyBackend())
    try:
        ref = fem.assemble(kappa * energy * fem.dx).array()
    finally:
        fem.set_backend(old)
    assert np.abs(got - ref).max() <= 1e-13 * np.abs(ref).max()


def test_cell_weighted_box_operator(ctx):
    """K[kappa] + 0.5 M with the hull eliminated on a 10^3-cell box, kappa the seeded 8-level field: the device product against
    the CSR product of the oracle's operator, and a PCG solve against spsolve."""
    c, e = FN.box_mesh((0, 0, 0), (1, 1, 1), 10, 10, 10)
    kappa = CR.level_field(e.shape[0], 11)
    h = ctx.mesh_upload(c, e)
    cv = ctx.vec_from(kappa)
    K, M = ctx.atom_assemble_cellwise(h, FN.STIFF, 0, 0, 0, cv, None, e.shape[0]), ctx.atom_assemble(h, FN.MASS)
    bc = np.where(np.any((c <= 1e-12) | (c >= 1 - 1e-12), axis=1))[0].astype(np.int32)
    op = ctx.op_combine(h, [K, M], [1.0, 0.5], bc)
    A = (CR.stiffness(c, e, kappa) + 0.5 * FN.assemble_atom(c, e, FN.MASS)).tocsr()
    A, _ = FN.apply_dirichlet(A, np.zeros(c.shape[0]), bc)
    x = np.random.default_rng(5).uniform(-1, 1, c.shape[0])
    xv, yv = ctx.vec_from(x), ctx.vec_alloc(c.shape[0])
    ctx.spmv(op, xv, yv)
    y = ctx.vec_download(yv)
    assert np.all(np.abs(y - A @ x) <= 1e-13 * (abs(A) @ np.abs(x)) + 1e-300)
    print("cell-weighted box operator: product form %d" % ctx.atom_product_form(op))
    b = A @ np.ones(c.shape[0])
    bv, sv = ctx.vec_from(b), ctx.vec_alloc(c.shape[0])
    it, rel = ctx.pcg_solve(op, bv, sv, 1e-12, 0.0, 20000)
    ref = spla.spsolve(A.tocsc(), b)
    assert np.linalg.norm(ctx.vec_download(sv) - ref) <= 1e-8 * np.linalg.norm(ref), (it, rel)
    for a in (op, K, M):
        ctx.atom_free(a)
    for vv in (xv, yv, bv, sv, cv):
        ctx.vec_free(vv)
    ctx.mesh_free(h)


# ------------------------------------------------------------------------------------------------------ V-cycle
BOXES = {"17x17x17": (17, 17, 17), "33x25x20": (33, 25, 20)}


@pytest.mark.parametrize("box", sorted(BOXES))
def test_vcycle_on_a_random_eight_level_field(ctx, box):
    """K[kappa], kappa a random 8-level cell-wise field in {0.5 ... 64}, Dirichlet set "face", right-hand side seed 11, rtol
    1e-12: under PGD_TUNE_PCG_PRECOND = 2 a solve of the V-cycle (no fallback) with the iteration count of the numpy restatement
    on the oracle's operator, fewer iterations than the Jacobi-PCG, the direct solution to 1e-8."""
    shape = BOXES[box]
    coords, cells = V.box(shape)
    n = coords.shape[0]
    kappa = CR.level_field(cells.shape[0], 11)
    h = ctx.mesh_upload(coords, cells.astype(np.int32))
    cv = ctx.vec_from(kappa)
    rtol = 1e-12
    atoms = []
    try:
        assert ctx.mesh_lattice(h)[0]
        atoms = [ctx.atom_assemble_cellwise(h, FN.STIFF, 0, 0, 0, cv, None, cells.shape[0])]
        bc = np.asarray(V.dirichlet_sets(coords)["face"], dtype=np.int32)
        A = V.apply_dirichlet_exact(sps.csr_matrix(CR.stiffness(coords, cells, kappa)), bc)
        b = np.random.default_rng(11).uniform(-1, 1, n)
        bv = ctx.vec_from(b)
        got = {}
        for prec in (2, 0):
            mg0, v0 = ctx.mg_stats(), ctx.vmg_stats()
            ctx.tune(40, prec)
            op = ctx.op_combine(h, atoms, [1.0], bc)
            xv = ctx.vec_alloc(n)
            it, rel = ctx.pcg_solve(op, bv, xv, rtol, 0.0, 5000)
            got[prec] = (it, rel, ctx.vec_download(xv))
            ctx.vec_free(xv)
            ctx.atom_free(op)
            mg1, v1 = ctx.mg_stats(), ctx.vmg_stats()
            assert mg1 == mg0
            assert v1["solves"] == v0["solves"] + (1 if prec == 2 else 0) and v1["fallbacks"] == v0["fallbacks"]
        ctx.vec_free(bv)
        xr, itr, relr = V.pcg(A, b, shape, rtol=rtol)
        _, itj, _ = V.pcg(A, b, shape, rtol=rtol, precond="jacobi")
        print("%s cell-wise field: device %d iterations (restatement %d), Jacobi-PCG device %d (restatement %d)"
              % (box, got[2][0], itr, got[0][0], itj))
        it, rel, x = got[2]
        assert rel <= rtol
        assert it == itr
        assert it < got[0][0]
        ref = spla.spsolve(A.tocsc(), b)
        assert np.linalg.norm(x - ref) <= 1e-8 * np.linalg.norm(ref)
        assert np.linalg.norm(got[0][2] - ref) <= 1e-8 * np.linalg.norm(ref)
    finally:
        ctx.tune(40, 0)
        for a in atoms:
            ctx.atom_free(a)
        ctx.vec_free(cv)
        ctx.mesh_free(h)


# ------------------------------------------------------------------------------------------------- cellwise_heat
@pytest.mark.parametrize("mk", [lambda: fem.RectangleMesh(P(0, 0), P(1, 1), 16, 16, "crossed"),
                                lambda: fem.BoxMesh(P(0, 0, 0), P(1, 1, 1), 7, 7, 7)])
def test_cellwise_heat_against_direct_solves(hip_backend, mk):
    from pgdrome_amd.solver import PGDProblem
    spec = CC.heat_spec(mk())
    p = PGDProblem(**spec)
    p.solve_PGD(_problem="linear")
    CC.check_cellwise_heat(spec, p, [0, 2, 4, 6, 8])


def test_cellwise_heat_reproduces_inclusion_heat(hip_backend):
    CC.check_reproduces_inclusion_heat(fem.RectangleMesh(P(0, 0), P(1, 1), 12, 12, "crossed"))


def test_cellwise_heat_under_vmg(hip_backend):
    """BoxMesh 16^3 (4913 nodes, above the cycle's 4096-node floor): every spatial solve of the run goes through the V-cycle
    ("vmg_pcg"), and the modes are those of the Jacobi-PCG run to 1e-6."""
    from pgdrome_amd.solver import PGDProblem

    def run(prec):
        fem.clear_caches()
        spec = CC.heat_spec(fem.BoxMesh(P(0, 0, 0), P(1, 1, 1), 16, 16, 16), PGD_nmax=6, PGD_tol=1e-8)
        p = PGDProblem(**spec)
        settings = {"linear_solver": "cg", "relative_tolerance": 1e-10}
        if prec is not None:
            settings["preconditioner"] = prec
        st0 = dict(fem.STATS)
        p.solve_PGD(_problem="linear", settings=settings)
        return p, {k: fem.STATS.get(k, 0) - st0.get(k, 0) for k in ("linear_solves", "mg_solves", "vmg_solves", "pcg_iterations")}
    pj, uj = run(None)
    pv, uv = run("vmg")
    print("cellwise_heat 16^3: jacobi %s, vmg %s" % (uj, uv))
    assert pj.PGD_modes == pv.PGD_modes and pj.num_fp_it == pv.num_fp_it
    for d in range(2):
        for k in range(pj.PGD_modes):
            a, b = pj.PGD_func[d][k].compute_vertex_values(), pv.PGD_func[d][k].compute_vertex_values()
            assert np.linalg.norm(a - b) <= 1e-6 * np.linalg.norm(a)
    assert uj["vmg_solves"] == 0 and uv["mg_solves"] == 0
    assert uv["vmg_solves"] == sum(pv.num_fp_it)                 # method "vmg_pcg" for every spatial solve
    assert uv["pcg_iterations"] < uj["pcg_iterations"]


def test_solver_routing(hip_backend):
    """An operator with a cell-weighted atom: Jacobi-PCG on an "amg" request, the V-cycle on "vmg"."""
    def solve(prec):
        mesh = fem.BoxMesh(P(0, 0, 0), P(1, 1, 1), 16, 16, 16)
        Vh = fem.FunctionSpace(mesh, "P", 1)
        kappa = CC._field(mesh, CR.level_field(mesh.num_cells(), 11))
        u, v = fem.TrialFunction(Vh), fem.TestFunction(Vh)
        sol = fem.Function(Vh)
        info = fem.solve(kappa * fem.inner(fem.grad(u), fem.grad(v)) * fem.dx == fem.Constant(1.0) * v * fem.dx, sol,
                         fem.DirichletBC(Vh, 0.0, lambda x, on_boundary: on_boundary),
                         solver_parameters={"preconditioner": prec, "relative_tolerance": 1e-10})
        return info, sol.compute_vertex_values()
    info_v, xv = solve("vmg")
    info_a, xa = solve("amg")
    print("cell-weighted operator: vmg request %s, amg request %s" % (info_v, info_a))
    assert info_v["method"] == "vmg_pcg" and info_a["method"] == "jacobi_pcg"
    assert info_v["iterations"] < info_a["iterations"]
    assert np.linalg.norm(xv - xa) <= 1e-8 * np.linalg.norm(xa)
