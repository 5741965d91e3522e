"""The row-class product of P2 operators on 3-D box lattices on the device (pgdrome_amd/csrc/pgd_p2lat.hip: k_p2lat_extract /
k_spmv_p2lat, PGD_TUNE_SPMV_P2_LATTICE = 59, settings["p2_product"] = "lattice") against the CSR product of the same operator: the
same fma chain per row on the same rows per workgroup, so everything is compared for EQUALITY - products, partial sums, whole
solves under the Jacobi-PCG and under the p-multigrid cycle - and against the matrix read back from the backend by the standard
bound of the chain.  The operators are built through the frontend on the HIP backend (tests/pmg_reference.py)."""
import numpy as np
import pytest

from pgdrome_amd import fem, problems
from tests import pmg_reference as PM

pytestmark = pytest.mark.gpu
P = fem.Point
KNOB, KNOB_ROWS, KNOB_PRECOND = 59, 1, 40
SLOT = 60

# (vertices per axis) a partial last workgroup at every workgroup size, most nodes on the hull, the vertex / edge row boundary inside a wave
SHAPES = {"3x3x3": (3, 3, 3), "5x4x3": (5, 4, 3), "9x7x6": (9, 7, 6)}
BOXES = {"17x17x17": (17, 17, 17), "21x19x17": (21, 19, 17)}       # the smallest the p-multigrid cycle takes
NAMES = ["clamped", "roller", "scalar_hull"]
_SPACES, _OPS = {}, {}


@pytest.fixture(scope="module")
def hip_backend():
    from pgdrome_amd.hip_backend import HipBackend
    old = fem._backend
    be = fem.set_backend(HipBackend(0))
    fem.clear_caches()
    yield be
    _SPACES.clear()
    _OPS.clear()
    fem.set_backend(old)
    fem.clear_caches()


def _operator(be, shape, name):
    """(fem.Matrix, its scipy copy read back from the backend, the Dirichlet dofs) of a case on a box, its layout bound; built once."""
    if (shape, name) not in _OPS:
        nc = PM.CASES[name][0]
        if (shape, nc) not in _SPACES:
            _SPACES[(shape, nc)] = PM.space(shape, nc)
        Vh = _SPACES[(shape, nc)]
        assert Vh._lay.bind_p2_lattice(be)
        _OPS[(shape, name)] = PM.operator(Vh, name)
    return _OPS[(shape, name)]


def _products(ctx, op, x, w):
    """y = A x, and the slot values of spmv_dot_slot with w = x and with w != x, under the knob as it is set."""
    n = x.size
    xv, wv, yv = ctx.vec_from(x), ctx.vec_from(w), ctx.vec_alloc(n)
    try:
        ctx.flags_reset()
        ctx.spmv(op, xv, yv)
        y = ctx.vec_download(yv)
        ctx.spmv_dot_slot(op, xv, yv, xv, 0, -1, SLOT)
        sxx = ctx.slots_download(SLOT, 1)[0]
        y2 = ctx.vec_download(yv)
        ctx.spmv_dot_slot(op, xv, yv, wv, 0, -1, SLOT)
        swx = ctx.slots_download(SLOT, 1)[0]
        return y, y2, sxx, swx
    finally:
        for v in (xv, wv, yv):
            ctx.vec_free(v)


def _both(ctx, op, x, w):
    """_products under knob 0 and knob 1 (+ the products counted under each)."""
    out = {}
    try:
        for knob in (0, 1):
            p0 = ctx.p2_product(knob)
            out[knob] = _products(ctx, op, x, w) + (ctx.p2lat_stats()["products"] - p0,)
    finally:
        ctx.p2_product(False)
    return out


def _assert_same_bits(out):
    y0, y02, sxx0, swx0, moved0 = out[0]
    y1, y12, sxx1, swx1, moved1 = out[1]
    assert np.array_equal(y0, y1) and np.array_equal(y02, y12) and np.array_equal(y0, y02)
    assert sxx0 == sxx1 and swx0 == swx1
    assert moved0 == 0 and moved1 == 3


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_product_bits_and_bound(hip_backend, shape, name):
    """ctx.spmv and spmv_dot_slot (w = x, w != x) under knob 0 and knob 1, with 64, 128 and 256 rows per workgroup: y passes
    np.array_equal and the slot values are equal.  (np.array_equal compares values: +0.0 and -0.0 are equal.  The form adds
    fma(0.0, x, acc) for a slot the row does not store, which can turn an accumulator of -0.0 into +0.0 and nothing else.)
    Against the matrix M read back from the backend, row by row: |y - M x| <= 2 gamma_L (|M| |x|), gamma_L = L u / (1 - L u),
    L = 65 ncomp, u = 2^-53 - the standard bound for the difference of two chains of at most L terms, nothing in it measured."""
    ctx, shp = hip_backend.ctx, SHAPES[shape]
    A, M, _ = _operator(hip_backend, shp, name)
    nc = PM.CASES[name][0]
    rng = np.random.default_rng(23)
    x, w = rng.uniform(-1, 1, M.shape[0]), rng.uniform(-1, 1, M.shape[0])
    u = 2.0 ** -53
    L = 65 * nc
    gamma = L * u / (1 - L * u)
    op = A.op()
    try:
        st0, b0, p0 = ctx.p2lat_stats(), ctx.bdia_stats(), ctx.pmg_stats()
        for rows in (64, 128, 256):
            ctx.tune(KNOB_ROWS, rows)
            out = _both(ctx, op, x, w)
            _assert_same_bits(out)
            err = np.abs(out[1][0] - M @ x)
            bound = 2 * gamma * (abs(M) @ np.abs(x))
            print("%s %s R=%d: max |y - Mx| / bound = %.3g" % (shape, name, rows, np.max(err / np.maximum(bound, 1e-300))))
            assert np.all(err <= bound)
        st1 = ctx.p2lat_stats()
        assert st1["forms_built"] == st0["forms_built"] + 1 and st1["fallbacks"] == st0["fallbacks"]      # one operator, one form
        assert st1["extract_ms"] > st0["extract_ms"]
        assert ctx.bdia_stats() == b0 and ctx.pmg_stats() == p0
    finally:
        ctx.tune(KNOB_ROWS, 64)
        ctx.atom_free(op)


def test_both_product_knobs_on_and_the_knob_off(hip_backend):
    """With knobs 58 and 59 both on a P2 operator that takes the row-class form is not offered to the row-diagonal one; with 59 off
    and 58 on it is that form's fallback as before, and no counter of this form moves."""
    ctx, shp = hip_backend.ctx, SHAPES["5x4x3"]
    A, M, _ = _operator(hip_backend, shp, "clamped")
    x = np.random.default_rng(3).uniform(-1, 1, M.shape[0])
    xv, yv = ctx.vec_from(x), ctx.vec_alloc(x.size)
    op = A.op()
    try:
        ctx.tune(KNOB, 0)
        ctx.spmv(op, xv, yv)
        y0 = ctx.vec_download(yv)
        s0, b0 = ctx.p2lat_stats(), ctx.bdia_stats()
        ctx.tune(58, 1)
        ctx.tune(KNOB, 1)
        ctx.spmv(op, xv, yv)
        s1, b1 = ctx.p2lat_stats(), ctx.bdia_stats()
        assert np.array_equal(ctx.vec_download(yv), y0)
        assert s1["forms_built"] == s0["forms_built"] + 1 and s1["products"] == s0["products"] + 1 and s1["fallbacks"] == s0["fallbacks"]
        assert b1 == b0
        ctx.tune(KNOB, 0)
        ctx.spmv(op, xv, yv)
        s2, b2 = ctx.p2lat_stats(), ctx.bdia_stats()
        assert np.array_equal(ctx.vec_download(yv), y0)
        assert (s2["forms_built"], s2["products"], s2["fallbacks"]) == (s1["forms_built"], s1["products"], s1["fallbacks"])
        assert b2["fallbacks"] == b1["fallbacks"] + 1 and b2["forms_built"] == b1["forms_built"] and b2["products"] == b1["products"]
    finally:
        ctx.tune(58, 0)
        ctx.tune(KNOB, 0)
        ctx.atom_free(op)
        ctx.vec_free(xv)
        ctx.vec_free(yv)


@pytest.mark.parametrize("name", ["clamped", "scalar_hull"])
def test_stale_values_and_atoms(hip_backend, name):
    """A second set of coefficients combined into the SAME operator handle: the next product equals the CSR product of the new
    values - not the old form's - and a form was built again.  An atom has no such form: its product stays on CSR and counts
    nowhere."""
    ctx, shp = hip_backend.ctx, SHAPES["9x7x6"]
    A, M, bc = _operator(hip_backend, shp, name)
    n = M.shape[0]
    rng = np.random.default_rng(31)
    x, w = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    handles, coefs = A.merged()
    lay = A.lay.handle()
    op = hip_backend.combine(lay, handles, coefs, A.bc_vertices, 0)
    try:
        st0 = ctx.p2lat_stats()
        first = _both(ctx, op, x, w)
        _assert_same_bits(first)
        st1 = ctx.p2lat_stats()
        assert st1["forms_built"] == st0["forms_built"] + 1 and st1["fallbacks"] == st0["fallbacks"]
        assert np.linalg.norm(first[1][0] - M @ x) <= 1e-13 * np.linalg.norm(M @ x)
        other = [c * (3.0 if k % 2 == 0 else 0.25) for k, c in enumerate(coefs)]
        assert hip_backend.combine(lay, handles, other, A.bc_vertices, op) == op
        second = _both(ctx, op, x, w)
        _assert_same_bits(second)
        st2 = ctx.p2lat_stats()
        assert st2["forms_built"] == st1["forms_built"] + 1 and st2["fallbacks"] == st1["fallbacks"]
        rp, cols = ctx.mesh_pattern(lay)
        import scipy.sparse as sps
        M2 = sps.csr_matrix((ctx.atom_download(op, cols.size), cols, rp), shape=M.shape)
        assert not np.array_equal(first[1][0], second[1][0])
        assert np.linalg.norm(second[1][0] - M2 @ x) <= 1e-13 * np.linalg.norm(M2 @ x)
        assert np.linalg.norm(second[1][0] - M @ x) > 1e-3 * np.linalg.norm(M @ x)
        p0 = ctx.p2_product(True)
        yv, xv = ctx.vec_alloc(n), ctx.vec_from(x)
        ctx.spmv(handles[0], xv, yv)
        after = ctx.p2lat_stats()
        assert ctx.p2_product(False) == p0 and after["fallbacks"] == st2["fallbacks"] and after["forms_built"] == st2["forms_built"]
        ctx.vec_free(xv)
        ctx.vec_free(yv)
    finally:
        ctx.p2_product(False)
        ctx.atom_free(op)


def test_two_components_through_mesh_blocked(hip_backend):
    """ncomp = 2 over the bound scalar P2 layout of a 5 x 4 x 3 box through mesh_blocked / atom_embed (the frontend has no spelling
    for it): the same bits as the CSR product at every workgroup size, one form, and y is the read-back matrix's product."""
    import scipy.sparse as sps
    from oracle import fem_numpy as F
    ctx, shape, ncomp = hip_backend.ctx, SHAPES["5x4x3"], 2
    if (shape, 1) not in _SPACES:
        _SPACES[(shape, 1)] = PM.space(shape, 1)
    Vh = _SPACES[(shape, 1)]
    assert Vh._lay.bind_p2_lattice(hip_backend)
    h = Vh._lay.handle()
    bh = ctx.mesh_blocked(h, ncomp)
    K = Mm = 0
    for a in range(ncomp):
        for b in range(ncomp):
            for da, db, cv, cu, coef in ((a, a, b, b, 1.0 + (a == b)), (b, a, a, b, 0.5)) if a != b else ((a, a, a, a, 2.0),):
                at = ctx.atom_assemble(h, F.DUDV, da, db, 0)
                K = ctx.atom_embed(bh, at, cv, cu, coef, K)
                ctx.atom_free(at)
        at = ctx.atom_assemble(h, F.MASS, 0, 0, 0)
        Mm = ctx.atom_embed(bh, at, a, a, 1.0, Mm)
        ctx.atom_free(at)
    n = ncomp * Vh._lay.n
    bc = np.arange(0, 2 * ncomp, dtype=np.int32)
    op = ctx.op_combine(bh, [K, Mm], [1.0, 2.0], bc, 0)
    rng = np.random.default_rng(41)
    x, w = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    try:
        st0 = ctx.p2lat_stats()
        for rows in (64, 128, 256):
            ctx.tune(KNOB_ROWS, rows)
            out = _both(ctx, op, x, w)
            _assert_same_bits(out)
        st1 = ctx.p2lat_stats()
        assert st1["forms_built"] == st0["forms_built"] + 1 and st1["fallbacks"] == st0["fallbacks"]
        rp, cols = ctx.mesh_pattern(bh)
        M = sps.csr_matrix((ctx.atom_download(op, cols.size), cols, rp), shape=(n, n))
        assert np.linalg.norm(out[1][0] - M @ x) <= 1e-13 * np.linalg.norm(M @ x)
    finally:
        ctx.tune(KNOB_ROWS, 64)
        ctx.p2_product(False)
        for a in (K, Mm, op):
            ctx.atom_free(a)
        ctx.mesh_free(bh)


def _solve(ctx, A, b, prec, knob, rtol=1e-12, maxit=5000):
    """pgd_pcg_solve under PGD_TUNE_PCG_PRECOND = prec and PGD_TUNE_SPMV_P2_LATTICE = knob from a zero start, on a freshly combined
    operator: (iterations, relres, x)."""
    op = A.op()
    bv, xv = ctx.vec_from(b), ctx.vec_alloc(b.size)
    try:
        ctx.tune(KNOB_PRECOND, prec)
        ctx.tune(KNOB, knob)
        it, rel = ctx.pcg_solve(op, bv, xv, rtol, 0.0, maxit)
        return it, rel, ctx.vec_download(xv)
    finally:
        ctx.tune(KNOB_PRECOND, 0)
        ctx.tune(KNOB, 0)
        ctx.vec_free(bv)
        ctx.vec_free(xv)
        ctx.atom_free(op)


@pytest.mark.parametrize("prec", [0, 4])
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("box", sorted(BOXES))
def test_solves_are_bit_identical(hip_backend, box, name, prec):
    """pgd_pcg_solve from a zero start to rtol 1e-12 under the Jacobi-PCG and the p-multigrid cycle: between knob 0 and knob 1 the
    iteration count and relres are equal and x passes np.array_equal; the cycle's solves are counted as before, every solve under
    1 builds one form, launches products from it and none falls back, and the same solve twice is identical."""
    ctx, shape, rtol = hip_backend.ctx, BOXES[box], 1e-12
    A, M, _ = _operator(hip_backend, shape, name)
    b = np.random.default_rng(11).uniform(-1, 1, M.shape[0])
    c0, s0 = ctx.pmg_stats(), ctx.p2lat_stats()
    it0, rel0, x0 = _solve(ctx, A, b, prec, 0)
    c1, s1 = ctx.pmg_stats(), ctx.p2lat_stats()
    it1, rel1, x1 = _solve(ctx, A, b, prec, 1)
    c2, s2 = ctx.pmg_stats(), ctx.p2lat_stats()
    it2, rel2, x2 = _solve(ctx, A, b, prec, 1)
    s3 = ctx.p2lat_stats()
    print("%s %s precond %d: %d iterations, relres %.3g; counters %s -> %s -> %s" % (box, name, prec, it1, rel1, s1, s2, s3))
    assert rel0 <= rtol and rel1 <= rtol
    assert it0 == it1 == it2 and rel0 == rel1 == rel2
    assert np.array_equal(x0, x1) and np.array_equal(x1, x2)
    used = 1 if prec == 4 else 0
    for a, z in ((c0, c1), (c1, c2)):
        assert z["solves"] == a["solves"] + used and z["fallbacks"] == a["fallbacks"]
    assert (s1["forms_built"], s1["products"], s1["fallbacks"]) == (s0["forms_built"], s0["products"], s0["fallbacks"])
    for a, z in ((s1, s2), (s2, s3)):
        assert z["forms_built"] == a["forms_built"] + 1 and z["fallbacks"] == a["fallbacks"] and z["products"] > a["products"]


def _fallback_cases():
    from tests.test_pmg_gpu import _crossed_box
    hull = lambda x, on_boundary: on_boundary

    def poisson(mesh, degree):
        Vh = fem.FunctionSpace(mesh, "P", degree)
        u, v = fem.TrialFunction(Vh), fem.TestFunction(Vh)
        return Vh, fem.inner(fem.grad(u), fem.grad(v)) * fem.dx, fem.Constant(1.0) * v * fem.dx, fem.DirichletBC(Vh, 0.0, hull)

    def vector_p1():
        Vh = fem.VectorFunctionSpace(fem.BoxMesh(P(0, 0, 0), P(1, 1, 1), 8, 8, 8), "P", 1)
        u, v = fem.TrialFunction(Vh), fem.TestFunction(Vh)
        a = sum(u[i].dx(k) * v[i].dx(k) * fem.dx for i in range(3) for k in range(3)) + fem.dot(u, v) * fem.dx
        return Vh, a, fem.Constant(-1.0) * v[2] * fem.dx, fem.DirichletBC(Vh, fem.Constant((0.0, 0.0, 0.0)), hull)
    return {"crossed_box": lambda: poisson(_crossed_box(8), 2),
            "p2_in_2d": lambda: poisson(fem.RectangleMesh(P(0, 0), P(1, 1), 40, 40), 2),
            "two_vertices_along_x": lambda: poisson(fem.BoxMesh(P(0, 0, 0), P(1, 1, 1), 1, 8, 8), 2),
            "vector_p1": vector_p1}


@pytest.mark.parametrize("case", ["crossed_box", "p2_in_2d", "two_vertices_along_x", "vector_p1"])
def test_what_does_not_qualify_keeps_csr_and_is_counted(hip_backend, case):
    """A crossed box (the binding refuses it), P2 on a rectangle (never bound) and a box with 2 vertices along an axis: the CSR
    product, one fallback per operator, the solution to rtol.  A vector-valued P1 space moves no counter and keeps the method and
    the iterations it has without the key."""
    Vh, a, L, bc = _fallback_cases()[case]()
    rtol = 1e-10
    s0, st0 = hip_backend.p2lat_stats(), dict(fem.STATS)
    sol = fem.Function(Vh)
    info = fem.solve(a == L, sol, bc, solver_parameters={"p2_product": "lattice", "relative_tolerance": rtol})
    s1 = hip_backend.p2lat_stats()
    print("%s under p2_product=lattice: %s, counters %s -> %s" % (case, info, s0, s1))
    assert info["product"] == "csr" and info["relres"] <= rtol
    assert s1["forms_built"] == s0["forms_built"] and s1["products"] == s0["products"]
    assert fem.STATS.get("p2_lattice_solves", 0) == st0.get("p2_lattice_solves", 0)
    if case == "vector_p1":
        assert s1["fallbacks"] == s0["fallbacks"]
        plain = fem.solve(a == L, fem.Function(Vh), bc, solver_parameters={"relative_tolerance": rtol})
        assert plain["method"] == info["method"] and plain["iterations"] == info["iterations"]
    else:
        assert s1["fallbacks"] == s0["fallbacks"] + 1


def _elastic_solve(prec, product, cells=16):
    mesh = fem.BoxMesh(P(0, 0, 0), P(1, 1, 1), cells, cells, cells)
    Vh = fem.VectorFunctionSpace(mesh, "P", 2)
    u, v = fem.TrialFunction(Vh), fem.TestFunction(Vh)
    a = (fem.inner(problems._voigt_C(0.3) * problems._strain(u), problems._strain(v)) + fem.Constant(2.0) * fem.inner(u, v)) * fem.dx
    sol = fem.Function(Vh)
    prm = {"relative_tolerance": 1e-10}
    if prec is not None:
        prm["preconditioner"] = prec
    if product is not None:
        prm["p2_product"] = product
    info = fem.solve(a == fem.dot(fem.Constant((0.0, 0.0, -1.0)), v) * fem.dx, sol,
                     fem.DirichletBC(Vh, fem.Constant((0.0, 0.0, 0.0)), problems._clamped), solver_parameters=prm)
    return info, sol.vector().get_local()


def _poisson_solve(prec, product, cells=16):
    mesh = fem.BoxMesh(P(0, 0, 0), P(1, 1, 1), cells, cells, cells)
    Vh = fem.FunctionSpace(mesh, "P", 2)
    u, v = fem.TrialFunction(Vh), fem.TestFunction(Vh)
    sol = fem.Function(Vh)
    prm = {"relative_tolerance": 1e-10}
    if prec is not None:
        prm["preconditioner"] = prec
    if product is not None:
        prm["p2_product"] = product
    info = fem.solve(fem.inner(fem.grad(u), fem.grad(v)) * fem.dx == fem.Constant(1.0) * v * fem.dx, sol,
                     fem.DirichletBC(Vh, 0.0, lambda x, on_boundary: on_boundary), solver_parameters=prm)
    return info, sol.vector().get_local()


@pytest.mark.parametrize("prec", [None, "pmg"])
@pytest.mark.parametrize("problem", ["elasticity", "poisson"])
def test_frontend_key_switches_the_product(hip_backend, problem, prec):
    """Degree 2 on a 16^3-cell box with and without settings["p2_product"] = "lattice": info["product"] and
    STATS["p2_lattice_solves"] say which product ran; iteration counts and solutions are equal; the knob is off behind the solve."""
    solve = _elastic_solve if problem == "elasticity" else _poisson_solve
    st0 = dict(fem.STATS)
    info_c, xc = solve(prec, None)
    info_e, xe = solve(prec, "csr")
    st1 = dict(fem.STATS)
    info_l, xl = solve(prec, "lattice")
    st2 = dict(fem.STATS)
    print("%s 16^3 cells P2, preconditioner %s: %s | %s" % (problem, prec, info_c, info_l))
    assert info_c["product"] == "csr" and info_e["product"] == "csr" and info_l["product"] == "p2_lattice"
    assert info_c["method"] == info_l["method"] == ("pmg_pcg" if prec else "jacobi_pcg")
    assert st1.get("p2_lattice_solves", 0) == st0.get("p2_lattice_solves", 0)
    assert st2["p2_lattice_solves"] == st1.get("p2_lattice_solves", 0) + 1
    assert info_c["iterations"] == info_l["iterations"] == info_e["iterations"] and info_c["relres"] == info_l["relres"]
    assert np.array_equal(xc, xl) and np.array_equal(xc, xe)
    # the knob is off again behind the solve: a product on a bound P2 operator moves no counter
    ctx = hip_backend.ctx
    A, M, _ = _operator(hip_backend, SHAPES["5x4x3"], "scalar_hull")
    s0 = ctx.p2lat_stats()
    op = A.op()
    xv, yv = ctx.vec_from(np.ones(M.shape[0])), ctx.vec_alloc(M.shape[0])
    try:
        ctx.spmv(op, xv, yv)
    finally:
        ctx.atom_free(op)
        ctx.vec_free(xv)
        ctx.vec_free(yv)
    assert ctx.p2lat_stats() == s0


def test_pgd_run_is_identical_under_the_key(hip_backend):
    """problems.elastic_block with degree 2 on a 16^3-cell box, two modes, under "pmg" with and without the key: the same modes, the
    same fixed-point passes, every mode np.array_equal, every spatial solve from the form."""
    from pgdrome_amd.solver import PGDProblem

    def run(product):
        fem.clear_caches()
        mesh = fem.BoxMesh(P(0, 0, 0), P(1, 1, 1), 16, 16, 16)
        p = PGDProblem(**problems.elastic_block(mesh, degree=2, PGD_nmax=2))
        settings = {"linear_solver": "cg", "relative_tolerance": 1e-10, "preconditioner": "pmg"}
        if product is not None:
            settings["p2_product"] = product
        st0 = dict(fem.STATS)
        p.solve_PGD(_problem="linear", settings=settings)
        return p, {k: fem.STATS.get(k, 0) - st0.get(k, 0) for k in ("linear_solves", "pmg_solves", "p2_lattice_solves", "pcg_iterations")}
    pc, uc = run(None)
    pl, ul = run("lattice")
    print("elastic_block degree 2, 16^3 cells under pmg: csr %s, lattice %s" % (uc, ul))
    assert pc.PGD_modes == pl.PGD_modes and pc.num_fp_it == pl.num_fp_it
    for d in range(2):
        for k in range(pc.PGD_modes):
            assert np.array_equal(pc.PGD_func[d][k].vector().get_local(), pl.PGD_func[d][k].vector().get_local())
    assert uc["p2_lattice_solves"] == 0 and ul["p2_lattice_solves"] == ul["pmg_solves"] == uc["pmg_solves"] == sum(pl.num_fp_it)
    assert uc["pcg_iterations"] == ul["pcg_iterations"]
