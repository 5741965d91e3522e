"""The row-diagonal product of vector-valued P1 operators on box lattices on the device (pgdrome_amd/csrc/pgd_bdia.hip: k_bdia_extract /
k_spmv_bdia, PGD_TUNE_SPMV_BLOCK_DIA = 58, settings["block_product"] = "diagonal") against the CSR product of the same operator:
the same fma chain per row on the same rows per workgroup, so everything is compared for EQUALITY - products, partial sums, whole
solves - and against the matrix read back from the backend by the standard bound of the chain.  The operators are built through
the frontend on the HIP backend (tests/cmg_reference.py)."""
import numpy as np
import pytest

from oracle import fem_numpy as F
from pgdrome_amd import fem, problems
from tests import cmg_reference as CM

pytestmark = pytest.mark.gpu
P = fem.Point
NC = 3
KNOB, KNOB_ROWS, KNOB_PRECOND = 58, 1, 40
SLOT = 60

SHAPES = {"5x4x3": (5, 4, 3), "9x7x6": (9, 7, 6), "33x25x20": (33, 25, 20)}     # 180 rows: a partial last workgroup, every node on the hull
BOXES = {"17x17x17": (17, 17, 17), "33x25x20": (33, 25, 20)}
OPERATORS = {"clamped": ("elastic", "clamped", 2.0), "roller": ("elastic", "roller", 2.0), "graded": ("graded", "clamped", 2.0)}
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


def _operator(shape, name):
    """(fem.Matrix, its scipy copy read back from the backend), built once per module."""
    if (shape, name) not in _OPS:
        if shape not in _SPACES:
            _SPACES[shape] = CM.vector_space(shape)
        family, case, k_found = OPERATORS[name]
        _OPS[(shape, name)] = CM.frontend_operator(_SPACES[shape], family, CM.dirichlet_dofs(shape, NC, case), k_found=k_found)
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
            p0 = ctx.block_product(knob)
            out[knob] = _products(ctx, op, x, w) + (ctx.bdia_stats()["products"] - p0,)
    finally:
        ctx.block_product(False)
    return out


def _assert_same_bits(out):
    y0, y02, sxx0, swx0, moved0 = out[0]
    y1, y12, sxx1, swx1, moved1 = out[1]
    assert np.array_equal(y0, y1) and np.array_equal(y02, y12) and np.array_equal(y0, y02)
    assert sxx0 == sxx1 and swx0 == swx1
    assert moved0 == 0 and moved1 == 3


@pytest.mark.parametrize("name", sorted(OPERATORS))
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_product_bits_and_bound(hip_backend, shape, name):
    """ctx.spmv and spmv_dot_slot (w = x, w != x) under knob 0 and knob 1, with 64, 128 and 256 rows per workgroup: y passes
    np.array_equal and the slot values are equal.  (np.array_equal compares values: +0.0 and -0.0 are equal.  The form adds
    fma(0.0, x, acc) for an entry the row does not store, which can turn an accumulator of -0.0 into +0.0 and nothing else.)
    Against the matrix M read back from the backend, row by row: |y - M x| <= 2 gamma_45 (|M| |x|), gamma_45 = 45 u / (1 - 45 u),
    u = 2^-53 - the standard bound for the difference of two 45-term chains, nothing in it measured."""
    ctx, shp = hip_backend.ctx, SHAPES[shape]
    A, M = _operator(shp, name)
    rng = np.random.default_rng(23)
    x, w = rng.uniform(-1, 1, M.shape[0]), rng.uniform(-1, 1, M.shape[0])
    u = 2.0 ** -53
    gamma = 45 * u / (1 - 45 * u)
    op = A.op()
    try:
        st0 = ctx.bdia_stats()
        for rows in (64, 128, 256):
            ctx.tune(KNOB_ROWS, rows)
            out = _both(ctx, op, x, w)
            _assert_same_bits(out)
            err = np.abs(out[1][0] - M @ x)
            bound = 2 * gamma * (abs(M) @ np.abs(x))
            print("%s %s R=%d: max |y - Mx| / bound = %.3g" % (shape, name, rows, np.max(err / np.maximum(bound, 1e-300))))
            assert np.all(err <= bound)
        st1 = ctx.bdia_stats()
        assert st1["forms_built"] == st0["forms_built"] + 1 and st1["fallbacks"] == st0["fallbacks"]      # one operator, one form
        assert st1["extract_ms"] > st0["extract_ms"]
    finally:
        ctx.tune(KNOB_ROWS, 64)
        ctx.atom_free(op)


def _lattice_operator(ctx, shape, ncomp, coefs, bc, op=0):
    """An elasticity-like operator on a blocked layout of ncomp components over the 3-D box lattice, through pgd_mesh_blocked /
    pgd_atom_embed / pgd_op_combine: coefs[0] * (sum of embedded dudv atoms) + coefs[1] * (mass on the diagonal blocks)."""
    cells = tuple(n - 1 for n in shape)
    coords, tets = F.box_mesh((0, 0, 0), tuple(c / 8 for c in cells), *cells)
    h = ctx.mesh_upload(coords, tets)
    assert ctx.mesh_sym_info(h)["nx"] == shape[0] and ctx.mesh_sym_info(h)["ny"] == shape[1]
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
    return h, bh, (K, Mm), ctx.op_combine(bh, [K, Mm], coefs, bc, op)


def _read(ctx, bh, op):
    import scipy.sparse as sps
    rp, cols = ctx.mesh_pattern(bh)
    return sps.csr_matrix((ctx.atom_download(op, cols.size), cols, rp), shape=(rp.size - 1, rp.size - 1))


def test_two_components_on_a_3d_lattice_and_stale_values(hip_backend):
    """ncomp = 2 over a 9 x 7 x 6 lattice through mesh_blocked / atom_embed (the frontend has no spelling for it): the same bits as
    the CSR product.  Then a second set of coefficients is combined into the SAME operator handle: the next product equals the CSR
    product of the new values - not the old form's - and a form was built again."""
    ctx, shape, ncomp = hip_backend.ctx, (9, 7, 6), 2
    n = shape[0] * shape[1] * shape[2] * ncomp
    bc = CM.dofs_of(CM.node_sets(shape)["x0"], ncomp)
    rng = np.random.default_rng(31)
    x, w = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    h, bh, atoms, op = _lattice_operator(ctx, shape, ncomp, [1.0, 2.0], bc)
    try:
        st0 = ctx.bdia_stats()
        first = _both(ctx, op, x, w)
        _assert_same_bits(first)
        st1 = ctx.bdia_stats()
        assert st1["forms_built"] == st0["forms_built"] + 1 and st1["fallbacks"] == st0["fallbacks"]
        M1 = _read(ctx, bh, op)
        assert ctx.op_combine(bh, list(atoms), [3.0, 0.25], bc, op) == op
        second = _both(ctx, op, x, w)
        _assert_same_bits(second)
        st2 = ctx.bdia_stats()
        assert st2["forms_built"] == st1["forms_built"] + 1 and st2["fallbacks"] == st1["fallbacks"]
        M2 = _read(ctx, bh, op)
        assert not np.array_equal(first[1][0], second[1][0])
        assert np.linalg.norm(second[1][0] - M2 @ x) <= 1e-13 * np.linalg.norm(M2 @ x)
        assert np.linalg.norm(second[1][0] - M1 @ x) > 1e-3 * np.linalg.norm(M1 @ x)
        # an atom has no such form: its product stays on CSR and counts nowhere
        p0 = ctx.block_product(True)
        yv, xv = ctx.vec_alloc(n), ctx.vec_from(x)
        ctx.spmv(atoms[0], xv, yv)
        assert ctx.block_product(False) == p0 and ctx.bdia_stats()["fallbacks"] == st2["fallbacks"]
        ctx.vec_free(xv)
        ctx.vec_free(yv)
    finally:
        ctx.block_product(False)
        for a in atoms + (op,):
            ctx.atom_free(a)
        ctx.mesh_free(bh)
        ctx.mesh_free(h)


def _solve(ctx, A, b, prec, knob, rtol=1e-12, maxit=5000):
    """pgd_pcg_solve under PGD_TUNE_PCG_PRECOND = prec and PGD_TUNE_SPMV_BLOCK_DIA = knob from a zero start, on a freshly combined
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


@pytest.mark.parametrize("prec", [0, 3])
@pytest.mark.parametrize("name", sorted(OPERATORS))
@pytest.mark.parametrize("box", sorted(BOXES))
def test_solves_are_bit_identical(hip_backend, box, name, prec):
    """pgd_pcg_solve from a zero start to rtol 1e-12 under the Jacobi-PCG and the component-wise V-cycle: between knob 0 and knob 1
    the iteration count is equal and x passes np.array_equal; the cycle's solves are counted as before, every solve under 1 builds
    one form and none falls back, and the same solve twice is identical."""
    ctx, shape, rtol = hip_backend.ctx, BOXES[box], 1e-12
    A, M = _operator(shape, name)
    b = np.random.default_rng(11).uniform(-1, 1, M.shape[0])
    c0, s0 = ctx.cmg_stats(), ctx.bdia_stats()
    it0, rel0, x0 = _solve(ctx, A, b, prec, 0)
    c1, s1 = ctx.cmg_stats(), ctx.bdia_stats()
    it1, rel1, x1 = _solve(ctx, A, b, prec, 1)
    c2, s2 = ctx.cmg_stats(), ctx.bdia_stats()
    it2, rel2, x2 = _solve(ctx, A, b, prec, 1)
    s3 = ctx.bdia_stats()
    print("%s %s precond %d: %d iterations, relres %.3g; counters %s -> %s -> %s" % (box, name, prec, it1, rel1, s1, s2, s3))
    assert rel0 <= rtol and rel1 <= rtol
    assert it0 == it1 == it2 and rel0 == rel1 == rel2
    assert np.array_equal(x0, x1) and np.array_equal(x1, x2)
    used = 1 if prec == 3 else 0
    for a, z in ((c0, c1), (c1, c2)):
        assert z["solves"] == a["solves"] + used and z["fallbacks"] == a["fallbacks"]
    assert (s1["forms_built"], s1["products"], s1["fallbacks"]) == (s0["forms_built"], s0["products"], s0["fallbacks"])
    for a, z in ((s1, s2), (s2, s3)):
        assert z["forms_built"] == a["forms_built"] + 1 and z["fallbacks"] == a["fallbacks"] and z["products"] > a["products"]


def _fallback_cases():
    hull = lambda x, on_boundary: on_boundary

    def vector(mesh, degree):
        Vh = fem.VectorFunctionSpace(mesh, "P", degree)
        nc = mesh.geometry().dim()
        u, v = fem.TrialFunction(Vh), fem.TestFunction(Vh)
        a = sum(u[i].dx(k) * v[i].dx(k) * fem.dx for i in range(nc) for k in range(nc)) + fem.dot(u, v) * fem.dx
        return Vh, a, fem.Constant(-1.0) * v[nc - 1] * fem.dx, fem.DirichletBC(Vh, fem.Constant((0.0,) * nc), hull)

    def scalar():
        Vh = fem.FunctionSpace(fem.BoxMesh(P(0, 0, 0), P(1, 1, 1), 16, 16, 16), "P", 1)
        u, v = fem.TrialFunction(Vh), fem.TestFunction(Vh)
        return Vh, fem.inner(fem.grad(u), fem.grad(v)) * fem.dx, fem.Constant(1.0) * v * fem.dx, fem.DirichletBC(Vh, 0.0, hull)
    return {"scalar_p1": scalar,
            "vector_p2": lambda: vector(fem.BoxMesh(P(0, 0, 0), P(1, 1, 1), 9, 9, 9), 2),
            "crossed_rectangle": lambda: vector(fem.RectangleMesh(P(0, 0), P(1, 1), 80, 80, "crossed"), 1),
            "right_rectangle": lambda: vector(fem.RectangleMesh(P(0, 0), P(1, 1), 80, 80, "right"), 1)}


@pytest.mark.parametrize("case", ["scalar_p1", "vector_p2", "crossed_rectangle", "right_rectangle"])
def test_what_does_not_qualify_keeps_csr_and_is_counted(hip_backend, case):
    """Vector-valued P2, crossed and 2-D bases: the CSR product, one fallback per operator, the solution to rtol.  A scalar space
    moves no counter and keeps the method it has without the key."""
    Vh, a, L, bc = _fallback_cases()[case]()
    rtol = 1e-10
    s0, st0 = hip_backend.bdia_stats(), dict(fem.STATS)
    sol = fem.Function(Vh)
    info = fem.solve(a == L, sol, bc, solver_parameters={"block_product": "diagonal", "relative_tolerance": rtol})
    s1 = hip_backend.bdia_stats()
    print("%s under block_product=diagonal: %s, counters %s -> %s" % (case, info, s0, s1))
    assert info["product"] == "csr" and info["relres"] <= rtol
    assert s1["forms_built"] == s0["forms_built"] and s1["products"] == s0["products"]
    assert fem.STATS.get("block_dia_solves", 0) == st0.get("block_dia_solves", 0)
    if case == "scalar_p1":
        assert s1["fallbacks"] == s0["fallbacks"]
        plain = fem.solve(a == L, fem.Function(Vh), bc, solver_parameters={"relative_tolerance": rtol})
        assert plain["method"] == info["method"] and plain["iterations"] == info["iterations"]
    else:
        assert s1["fallbacks"] == s0["fallbacks"] + 1


def _elastic_solve(prec, product, cells=16):
    mesh = fem.BoxMesh(P(0, 0, 0), P(1, 1, 1), cells, cells, cells)
    Vh = fem.VectorFunctionSpace(mesh, "P", 1)
    u, v = fem.TrialFunction(Vh), fem.TestFunction(Vh)
    a = (fem.inner(problems._voigt_C(0.3) * problems._strain(u), problems._strain(v)) + fem.Constant(2.0) * fem.inner(u, v)) * fem.dx
    sol = fem.Function(Vh)
    prm = {"relative_tolerance": 1e-10}
    if prec is not None:
        prm["preconditioner"] = prec
    if product is not None:
        prm["block_product"] = product
    info = fem.solve(a == fem.dot(fem.Constant((0.0, 0.0, -1.0)), v) * fem.dx, sol,
                     fem.DirichletBC(Vh, fem.Constant((0.0, 0.0, 0.0)), problems._clamped), solver_parameters=prm)
    return info, sol.vector().get_local()


@pytest.mark.parametrize("prec", [None, "cmg"])
def test_frontend_key_switches_the_product(hip_backend, prec):
    """Elasticity on a 16^3-cell vector space with and without settings["block_product"] = "diagonal": info["product"] and
    STATS["block_dia_solves"] say which product ran; iteration counts and solutions are equal."""
    st0 = dict(fem.STATS)
    info_c, xc = _elastic_solve(prec, None)
    info_e, xe = _elastic_solve(prec, "csr")
    st1 = dict(fem.STATS)
    info_d, xd = _elastic_solve(prec, "diagonal")
    st2 = dict(fem.STATS)
    print("elasticity 16^3, preconditioner %s: %s | %s" % (prec, info_c, info_d))
    assert info_c["product"] == "csr" and info_e["product"] == "csr" and info_d["product"] == "block_dia"
    assert info_c["method"] == info_d["method"] == ("cmg_pcg" if prec else "jacobi_pcg")
    assert st1.get("block_dia_solves", 0) == st0.get("block_dia_solves", 0)
    assert st2["block_dia_solves"] == st1.get("block_dia_solves", 0) + 1
    assert info_c["iterations"] == info_d["iterations"] == info_e["iterations"] and info_c["relres"] == info_d["relres"]
    assert np.array_equal(xc, xd) and np.array_equal(xc, xe)
    assert hip_backend.bdia_stats()["products"] == hip_backend.block_product(False)      # the knob is off again behind the solve


def test_pgd_run_is_identical_under_the_key(hip_backend):
    """problems.elastic_block on a 16^3-cell box under "cmg" with and without the key: the same modes, the same fixed-point passes,
    every mode np.array_equal, every spatial solve from the form."""
    from pgdrome_amd.solver import PGDProblem

    def run(product):
        fem.clear_caches()
        mesh = fem.BoxMesh(P(0, 0, 0), P(1, 1, 1), 16, 16, 16)
        p = PGDProblem(**problems.elastic_block(mesh))
        settings = {"linear_solver": "cg", "relative_tolerance": 1e-10, "preconditioner": "cmg"}
        if product is not None:
            settings["block_product"] = product
        st0 = dict(fem.STATS)
        p.solve_PGD(_problem="linear", settings=settings)
        return p, {k: fem.STATS.get(k, 0) - st0.get(k, 0) for k in ("linear_solves", "cmg_solves", "block_dia_solves", "pcg_iterations")}
    pc, uc = run(None)
    pd, ud = run("diagonal")
    print("elastic_block 16^3 under cmg: csr %s, diagonal %s" % (uc, ud))
    assert pc.PGD_modes == pd.PGD_modes and pc.num_fp_it == pd.num_fp_it
    for d in range(2):
        for k in range(pc.PGD_modes):
            assert np.array_equal(pc.PGD_func[d][k].vector().get_local(), pd.PGD_func[d][k].vector().get_local())
    assert uc["block_dia_solves"] == 0 and ud["block_dia_solves"] == ud["cmg_solves"] == uc["cmg_solves"] == sum(pd.num_fp_it)
    assert uc["pcg_iterations"] == ud["pcg_iterations"]
