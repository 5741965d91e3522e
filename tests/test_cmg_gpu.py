"""The component-wise multigrid preconditioner for vector-valued P1 operators on box lattices on the device
(pgdrome_amd/csrc/pgd_vmg.hip: k_cmg_extract / k_cmg_split / k_cmg_merge, PGD_TUNE_PCG_PRECOND = 3,
settings["preconditioner"] = "cmg") against its numpy restatement tests/cmg_reference.py, a direct solve, and the Jacobi-PCG.
The operators are built through the frontend on the HIP backend and read back from it for the restatement."""
import numpy as np
import pytest

from pgdrome_amd import fem, problems
from tests import cmg_reference as CM

pytestmark = pytest.mark.gpu
P = fem.Point
NC = 3

BOXES = {"17x17x17": (17, 17, 17), "33x25x20": (33, 25, 20)}      # the second: even node counts, a far face without coarse nodes
# (family, Dirichlet set, k_found): elasticity clamped at x = 0; the same with the hull eliminated; roller supports (+ foundation:
# SPD); the weighted operator of problems.graded_block at theta = 1
OPERATORS = {"clamped": ("elastic", "clamped", 2.0), "hull": ("elastic", "hull", 0.0), "roller": ("elastic", "roller", 2.0),
             "graded": ("graded", "clamped", 2.0)}
_SPACES = {}


@pytest.fixture(scope="module")
def hip_backend():
    from pgdrome_amd.hip_backend import HipBackend
    old = fem._backend
    be = fem.set_backend(HipBackend(0))
    fem.clear_caches()
    yield be
    _SPACES.clear()
    fem.set_backend(old)
    fem.clear_caches()


def _space(shape, step=1.0 / 16):
    if (shape, step) not in _SPACES:
        _SPACES[(shape, step)] = CM.vector_space(shape, step=step)
    return _SPACES[(shape, step)]


def _solve(ctx, A, b, prec, rtol, maxit=5000):
    """pgd_pcg_solve under PGD_TUNE_PCG_PRECOND = prec from a zero start: (iterations, relres, x)."""
    op = A.op()
    bv, xv = ctx.vec_from(b), ctx.vec_alloc(b.size)
    try:
        ctx.tune(40, prec)
        it, rel = ctx.pcg_solve(op, bv, xv, rtol, 0.0, maxit)
        return it, rel, ctx.vec_download(xv)
    finally:
        ctx.tune(40, 0)
        ctx.vec_free(bv)
        ctx.vec_free(xv)
        ctx.atom_free(op)


@pytest.mark.parametrize("name", sorted(OPERATORS))
@pytest.mark.parametrize("box", sorted(BOXES))
def test_solve_equals_the_restatement(hip_backend, box, name):
    """pgd_pcg_solve under PGD_TUNE_PCG_PRECOND = 3: the restatement's iteration count to +-1 (reordered sums), its solution to 1e-9,
    the direct solution to 1e-8, the eliminated dofs exactly b; counted as a solve of the component cycle and by no other counter;
    fewer iterations than the same solve under 0."""
    ctx, shape, rtol = hip_backend.ctx, BOXES[box], 1e-12
    family, case, k_found = OPERATORS[name]
    bc = CM.dirichlet_dofs(shape, NC, case)
    A, M = CM.frontend_operator(_space(shape), family, bc, k_found=k_found)
    b = np.random.default_rng(11).uniform(-1, 1, M.shape[0])
    mg0, v0, c0 = ctx.mg_stats(), ctx.vmg_stats(), ctx.cmg_stats()
    it, rel, x = _solve(ctx, A, b, 3, rtol)
    mg1, v1, c1 = ctx.mg_stats(), ctx.vmg_stats(), ctx.cmg_stats()
    itj, relj, xj = _solve(ctx, A, b, 0, rtol)
    xr, itr, relr = CM.pcg(M, b, shape, NC, rtol=rtol)
    print("%s %s: device %d iterations (restatement %d), Jacobi-PCG device %d; counters %s -> %s" % (box, name, it, itr, itj, c0, c1))
    assert rel <= rtol
    assert abs(it - itr) <= 1
    assert np.linalg.norm(x - xr) <= 1e-9 * np.linalg.norm(xr)
    ref = CM.direct_solve(M, b, shape, NC)
    assert np.linalg.norm(x - ref) <= 1e-8 * np.linalg.norm(ref)
    assert np.array_equal(x[bc], b[bc])
    assert it < itj
    assert c1["solves"] == c0["solves"] + 1 and c1["fallbacks"] == c0["fallbacks"]
    assert c1["levels"] == 2 and c1["setup_ms"] > c0["setup_ms"]
    assert mg1 == mg0 and v1 == v0
    assert ctx.cmg_stats()["solves"] == c1["solves"] and ctx.cmg_stats()["fallbacks"] == c1["fallbacks"]      # (the solve under 0 counts nowhere)


def test_march_and_plain_kernels_agree(hip_backend):
    """A 72 x 70 x 24-node base lattice: level 0 of every component runs its two passes in k_vmg_march (counted), with
    PGD_TUNE_MG_MARCH_MIN = 0 in the plain kernels: the same cycle up to the order of the sums."""
    ctx, shape = hip_backend.ctx, (72, 70, 24)
    bc = CM.dirichlet_dofs(shape, NC, "clamped")
    A, M = CM.frontend_operator(_space(shape, 1.0 / 64), "elastic", bc, k_found=2.0)
    b = np.random.default_rng(3).uniform(-1, 1, M.shape[0])
    out = {}
    try:
        for march_min in (64, 0):
            ctx.tune(42, march_min)
            m0 = ctx.cmg_stats()["march_passes"]
            it, rel, x = _solve(ctx, A, b, 3, 1e-10, 2000)
            out[march_min] = (it, x, ctx.cmg_stats()["march_passes"] - m0)
            assert rel <= 1e-10
    finally:
        ctx.tune(42, 64)
        _SPACES.pop((shape, 1.0 / 64), None)
    print("72x70x24: %d iterations with the march (%d passes), %d with the plain kernels" % (out[64][0], out[64][2], out[0][0]))
    assert out[64][2] > 0 and out[0][2] == 0
    assert abs(out[64][0] - out[0][0]) <= 1
    assert np.linalg.norm(out[64][1] - out[0][1]) <= 1e-8 * np.linalg.norm(out[0][1])
    assert np.linalg.norm(b - M @ out[64][1]) <= 1.05e-10 * np.linalg.norm(b)


def test_the_same_solve_twice_is_bit_identical(hip_backend):
    ctx, shape = hip_backend.ctx, BOXES["33x25x20"]
    A, M = CM.frontend_operator(_space(shape), "elastic", CM.dirichlet_dofs(shape, NC, "roller"), k_found=2.0)
    b = np.random.default_rng(19).uniform(-1, 1, M.shape[0])
    it1, _, x1 = _solve(ctx, A, b, 3, 1e-10)
    it2, _, x2 = _solve(ctx, A, b, 3, 1e-10)
    assert it1 == it2 and np.array_equal(x1, x2)


def _elastic_solve(prec, cells=16, degree=1):
    mesh = fem.BoxMesh(P(0, 0, 0), P(1, 1, 1), cells, cells, cells)
    Vh = fem.VectorFunctionSpace(mesh, "P", degree)
    u, v = fem.TrialFunction(Vh), fem.TestFunction(Vh)
    a = (fem.inner(problems._voigt_C(0.3) * problems._strain(u), problems._strain(v)) + fem.Constant(2.0) * fem.inner(u, v)) * fem.dx
    sol = fem.Function(Vh)
    prm = {"relative_tolerance": 1e-10}
    if prec is not None:
        prm["preconditioner"] = prec
    info = fem.solve(a == fem.dot(fem.Constant((0.0, 0.0, -1.0)), v) * fem.dx, sol,
                     fem.DirichletBC(Vh, fem.Constant((0.0, 0.0, 0.0)), problems._clamped), solver_parameters=prm)
    return info, sol.vector().get_local()


def test_frontend_cmg_request_runs_the_cycle(hip_backend):
    """Elasticity on a 16^3-cell vector space: "cmg" and "component_multigrid" are answered by the component cycle, "vmg" and no
    preconditioner by the Jacobi-PCG."""
    st0 = dict(fem.STATS)
    info_c, xc = _elastic_solve("cmg")
    st1 = dict(fem.STATS)
    info_j, xj = _elastic_solve(None)
    info_v, _ = _elastic_solve("vmg")
    st2 = dict(fem.STATS)
    print("elasticity 16^3: cmg request %s, no preconditioner %s, vmg request %s" % (info_c, info_j, info_v))
    assert info_c["method"] == "cmg_pcg" and st1.get("cmg_solves", 0) == st0.get("cmg_solves", 0) + 1
    assert st1["pcg_iterations"] == st0["pcg_iterations"] + info_c["iterations"]
    assert info_j["method"] == "jacobi_pcg" and info_v["method"] == "jacobi_pcg"
    assert st2.get("cmg_solves", 0) == st1.get("cmg_solves", 0)
    assert info_c["iterations"] < info_j["iterations"]
    assert np.linalg.norm(xc - xj) <= 1e-8 * np.linalg.norm(xj)
    info_w, xw = _elastic_solve("component_multigrid")
    assert info_w["method"] == "cmg_pcg" and info_w["iterations"] == info_c["iterations"]
    assert fem.STATS.get("cmg_solves", 0) == st2.get("cmg_solves", 0) + 1


def test_pgd_run_agrees_under_cmg(hip_backend):
    """problems.elastic_block on a 16^3-cell box under the Jacobi-PCG and under "cmg": the same modes and fixed-point passes, every
    spatial solve through the component cycle, fewer PCG iterations in sum."""
    from pgdrome_amd.solver import PGDProblem

    def run(prec):
        fem.clear_caches()
        mesh = fem.BoxMesh(P(0, 0, 0), P(1, 1, 1), 16, 16, 16)
        p = PGDProblem(**problems.elastic_block(mesh))
        settings = {"linear_solver": "cg", "relative_tolerance": 1e-10}
        if prec is not None:
            settings["preconditioner"] = prec
        st0 = dict(fem.STATS)
        p.solve_PGD(_problem="linear", settings=settings)
        return p, {k: fem.STATS.get(k, 0) - st0.get(k, 0) for k in ("linear_solves", "mg_solves", "vmg_solves", "cmg_solves", "pcg_iterations")}
    pj, uj = run(None)
    pc, uc = run("cmg")
    print("elastic_block 16^3: jacobi %s, cmg %s" % (uj, uc))
    assert pj.PGD_modes == pc.PGD_modes and pj.num_fp_it == pc.num_fp_it
    for d in range(2):
        for k in range(pj.PGD_modes):
            a, b = pj.PGD_func[d][k].vector().get_local(), pc.PGD_func[d][k].vector().get_local()
            assert np.linalg.norm(a - b) <= 1e-6 * np.linalg.norm(a)
    assert uj["cmg_solves"] == 0 and uc["mg_solves"] == 0 and uc["vmg_solves"] == 0
    assert uc["cmg_solves"] == sum(pc.num_fp_it)
    assert uc["pcg_iterations"] < uj["pcg_iterations"]


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
            "small_lattice": lambda: vector(fem.BoxMesh(P(0, 0, 0), P(1, 1, 1), 12, 12, 12), 1),       # 2197 nodes: no hierarchy
            "crossed_rectangle": lambda: vector(fem.RectangleMesh(P(0, 0), P(1, 1), 80, 80, "crossed"), 1)}


@pytest.mark.parametrize("case", ["scalar_p1", "vector_p2", "small_lattice", "crossed_rectangle"])
def test_what_does_not_qualify_takes_jacobi_and_is_counted(hip_backend, case):
    Vh, a, L, bc = _fallback_cases()[case]()
    sol = fem.Function(Vh)
    c0, v0, st0 = hip_backend.cmg_stats(), hip_backend.vmg_stats(), dict(fem.STATS)
    info = fem.solve(a == L, sol, bc, solver_parameters={"preconditioner": "cmg", "relative_tolerance": 1e-10})
    c1 = hip_backend.cmg_stats()
    print("%s under cmg: %s, counters %s -> %s" % (case, info, c0, c1))
    assert info["method"] == "jacobi_pcg" and info["relres"] <= 1e-10
    assert c1["fallbacks"] == c0["fallbacks"] + 1 and c1["solves"] == c0["solves"]
    assert hip_backend.vmg_stats() == v0
    assert fem.STATS.get("cmg_solves", 0) == st0.get("cmg_solves", 0)
