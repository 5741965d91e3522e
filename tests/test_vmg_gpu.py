"""The variable-coefficient multigrid preconditioner on the device (pgdrome_amd/csrc/pgd_vmg.hip, PGD_TUNE_PCG_PRECOND = 2,
settings["preconditioner"] = "vmg") against its numpy restatement tests/vmg_reference.py, a direct solve, and the Jacobi-PCG."""
import numpy as np
import pytest
import scipy.sparse as sps
import scipy.sparse.linalg as spla

from oracle import fem_numpy as FN
from pgdrome_amd import fem, problems
from tests import vmg_reference as V
from tests.mg_cycle_cases import family as _family      # (shared with tests/test_mg_cycles_gpu.py)

pytestmark = pytest.mark.gpu
P = fem.Point

BOXES = {"17x17x17": (17, 17, 17), "33x25x20": (33, 25, 20)}      # the second: even node counts, a far face without coarse nodes
FAMILIES = ("weighted", "two_material", "robin", "mixed", "constant")


@pytest.fixture(scope="module")
def hip_backend():
    from pgdrome_amd.hip_backend import HipBackend
    old = fem._backend
    be = fem.set_backend(HipBackend(0))
    fem.clear_caches()
    yield be
    fem.set_backend(old)
    fem.clear_caches()


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("box", sorted(BOXES))
def test_solve_equals_the_restatement(ctx, box, family):
    """pgd_pcg_solve under PGD_TUNE_PCG_PRECOND = 2 on operators built through the C-ABI: the iteration count of the numpy restatement,
    its solution to 1e-9, the direct solution to 1e-8; counted as a solve of the new cycle, not as a fallback, and not by
    pgd_mg_counts.  The same operator under 0 gives the Jacobi-PCG's (larger) count and the same solution.  (rtol 1e-12, so that
    the comparison with the direct solve is one of the solves and not of the operators' condition numbers.)"""
    shape = BOXES[box]
    coords, cells = V.box(shape)
    n = coords.shape[0]
    h = ctx.mesh_upload(coords, cells.astype(np.int32))
    extra = []
    rtol = 1e-12
    try:
        assert ctx.mesh_lattice(h)[0]
        atoms, coefs, bc, A, extra = _family(ctx, h, coords, cells, family)
        bc = np.asarray(bc, dtype=np.int32)
        A = V.apply_dirichlet_exact(sps.csr_matrix(A), bc)
        rng = np.random.default_rng(11)
        b = rng.uniform(-1, 1, n)
        bv = ctx.vec_from(b)
        extra.append(bv)
        got = {}
        for prec in (2, 0):
            mg0, v0 = ctx.mg_stats(), ctx.vmg_stats()
            ctx.tune(40, prec)
            op = ctx.op_combine(h, atoms, coefs, bc)
            xv = ctx.vec_alloc(n)
            it, rel = ctx.pcg_solve(op, bv, xv, rtol, 0.0, 5000)
            got[prec] = (it, rel, ctx.vec_download(xv))
            ctx.vec_free(xv)
            ctx.atom_free(op)
            mg1, v1 = ctx.mg_stats(), ctx.vmg_stats()
            assert mg1 == mg0
            assert v1["solves"] == v0["solves"] + (1 if prec == 2 else 0) and v1["fallbacks"] == v0["fallbacks"]
            if prec == 2:
                assert v1["levels"] == 2 and v1["setup_ms"] > v0["setup_ms"]
        xr, itr, relr = V.pcg(A, b, shape, rtol=rtol)
        _, itj, _ = V.pcg(A, b, shape, rtol=rtol, precond="jacobi")
        print("%s %s: device %d iterations (restatement %d), Jacobi-PCG device %d (restatement %d)"
              % (box, family, got[2][0], itr, got[0][0], itj))
        it, rel, x = got[2]
        assert rel <= rtol
        assert it == itr
        assert np.linalg.norm(x - xr) <= 1e-9 * np.linalg.norm(xr)
        ref = spla.spsolve(A.tocsc(), b)
        assert np.linalg.norm(x - ref) <= 1e-8 * np.linalg.norm(ref)
        assert np.array_equal(x[bc], b[bc])
        assert it < got[0][0]
        assert np.linalg.norm(x - got[0][2]) <= 1e-8 * np.linalg.norm(ref)
    finally:
        ctx.tune(40, 0)
        for a in locals().get("atoms", []):
            ctx.atom_free(a)
        for v in extra:
            ctx.vec_free(v)
        ctx.mesh_free(h)


@pytest.mark.parametrize("shape", [(72, 70, 24), (65, 71, 9)], ids=lambda s: "%dx%dx%d" % s)
def test_march_and_plain_kernels_agree(ctx, shape):
    """Level 0 runs its two passes in k_vmg_march (counted), with PGD_TUNE_MG_MARCH_MIN = 0 in the plain kernels: the same cycle up
    to the order of the partial sums of r . z.  65 x 71 x 9 (41 535 nodes, three levels) is the smallest lattice that adds what
    72 x 70 x 24 does not reach: an odd ny (the last thread pair of a patch has a live lower and a dead upper row, in both epilogues
    and in the dot), a second x tile one node wide, and marches of three planes (every march pays the prologue and, from the second
    on, the hand-over of the plane below)."""
    coords, cells = V.box(shape, steps=(1.0 / 64,) * 3)
    n = coords.shape[0]
    h = ctx.mesh_upload(coords, cells.astype(np.int32))
    w = 1.0 + coords[:, 0] * coords[:, 1] + coords[:, 2]
    wv = ctx.vec_from(w)
    a = ctx.atom_assemble(h, FN.WSTIFF, 0, 0, wv)
    bc = V.dirichlet_sets(coords)["face"].astype(np.int32)
    b = np.random.default_rng(3).uniform(-1, 1, n)
    bv = ctx.vec_from(b)
    out = {}
    try:
        for march_min in (64, 0):
            ctx.tune(40, 2)
            ctx.tune(42, march_min)
            m0 = ctx.vmg_stats()["march_passes"]
            op = ctx.op_combine(h, [a], [1.0], bc)
            xv = ctx.vec_alloc(n)
            it, rel = ctx.pcg_solve(op, bv, xv, 1e-10, 0.0, 2000)
            out[march_min] = (it, ctx.vec_download(xv), ctx.vmg_stats()["march_passes"] - m0)
            assert rel <= 1e-10
            ctx.vec_free(xv)
            ctx.atom_free(op)
        print("%dx%dx%d: %d iterations with the march (%d passes), %d with the plain kernels" % (*shape, out[64][0], out[64][2], out[0][0]))
        assert out[64][2] > 0 and out[0][2] == 0                   # (launches issued: a replayed chunk of iterations counts once)
        assert abs(out[64][0] - out[0][0]) <= 1
        assert np.linalg.norm(out[64][1] - out[0][1]) <= 1e-8 * np.linalg.norm(out[0][1])
        A = V.apply_dirichlet_exact(sps.csr_matrix(FN.assemble_atom(coords, cells, FN.WSTIFF, 0, 0, w)), bc)
        assert np.linalg.norm(b - A @ out[64][1]) <= 1.05e-10 * np.linalg.norm(b)
    finally:
        ctx.tune(40, 0)
        ctx.tune(42, 64)
        ctx.atom_free(a)
        ctx.vec_free(wv)
        ctx.vec_free(bv)
        ctx.mesh_free(h)


def _weighted_solve(prec):
    mesh = fem.BoxMesh(P(0, 0, 0), P(1, 1, 1), 16, 16, 16)
    Vh = fem.FunctionSpace(mesh, "P", 1)
    w = fem.interpolate(fem.Expression("1 + x[0] + x[1]*x[2]", degree=1), Vh)
    u, v = fem.TrialFunction(Vh), fem.TestFunction(Vh)
    a = sum(w * u.dx(k) * v.dx(k) * fem.dx for k in range(3))
    sol = fem.Function(Vh)
    info = fem.solve(a == fem.Constant(1.0) * v * fem.dx, sol, fem.DirichletBC(Vh, 0.0, lambda x, on_boundary: on_boundary),
                     solver_parameters={"preconditioner": prec, "relative_tolerance": 1e-10})
    return info, sol.compute_vertex_values()


def test_frontend_vmg_request_runs_the_cycle(hip_backend):
    """sum_a w u_{,a} v_{,a} on a box (SPD, not one stencil): "vmg" is answered by the new cycle, "amg" still by the Jacobi-PCG."""
    st0 = dict(fem.STATS)
    info_v, xv = _weighted_solve("vmg")
    st1 = dict(fem.STATS)
    info_a, xa = _weighted_solve("amg")
    st2 = dict(fem.STATS)
    print("weighted operator: vmg request %s, amg request %s" % (info_v, info_a))
    assert info_v["method"] == "vmg_pcg" and st1.get("vmg_solves", 0) == st0.get("vmg_solves", 0) + 1
    assert st1.get("mg_solves", 0) == st0.get("mg_solves", 0)
    assert info_a["method"] == "jacobi_pcg"
    assert st2.get("vmg_solves", 0) == st1.get("vmg_solves", 0) and st2.get("mg_solves", 0) == st1.get("mg_solves", 0)
    assert info_v["iterations"] < info_a["iterations"]
    assert np.linalg.norm(xv - xa) <= 1e-8 * np.linalg.norm(xa)
    info_w, _ = _weighted_solve("variable_multigrid")
    assert info_w["method"] == "vmg_pcg"


@pytest.mark.parametrize("name", ["inclusion_heat", "robin_heat"])
def test_pgd_runs_agree_under_vmg(hip_backend, name):
    """A 32^3 box under the Jacobi-PCG and under "vmg": the same modes and fixed-point passes, every spatial solve through the new
    cycle, fewer PCG iterations in sum."""
    from pgdrome_amd.solver import PGDProblem

    def run(prec):
        fem.clear_caches()
        mesh = fem.BoxMesh(P(0, 0, 0), P(1, 1, 1), 32, 32, 32)
        if name == "inclusion_heat":
            spec = problems.inclusion_heat(mesh, n_k=9, PGD_nmax=6, PGD_tol=1e-8)
        else:
            spec = problems.robin_heat(mesh, n_h=9, h_range=(0.1, 100.0), PGD_nmax=6, PGD_tol=1e-8)
        p = PGDProblem(**spec)
        settings = {"linear_solver": "cg", "relative_tolerance": 1e-10}
        if prec is not None:
            settings["preconditioner"] = prec
        st0 = dict(fem.STATS)
        p.solve_PGD(_problem="linear", settings=settings)
        used = {k: fem.STATS.get(k, 0) - st0.get(k, 0) for k in ("linear_solves", "mg_solves", "vmg_solves", "pcg_iterations")}
        return p, used
    pj, uj = run(None)
    pv, uv = run("vmg")
    print("%s 32^3: jacobi %s, vmg %s" % (name, uj, uv))
    print("%s 32^3: PCG iterations in sum: jacobi %d, vmg %d" % (name, uj["pcg_iterations"], uv["pcg_iterations"]))
    assert pj.PGD_modes == pv.PGD_modes and pj.num_fp_it == pv.num_fp_it
    for d in range(2):
        for k in range(pj.PGD_modes):
            a, b = pj.PGD_func[d][k].compute_vertex_values(), pv.PGD_func[d][k].compute_vertex_values()
            assert np.linalg.norm(a - b) <= 1e-6 * np.linalg.norm(a)
    assert uj["vmg_solves"] == 0 and uv["mg_solves"] == 0
    assert uv["vmg_solves"] == sum(pv.num_fp_it)
    assert uv["pcg_iterations"] < uj["pcg_iterations"]


def _fallback_cases():
    def vector():
        mesh = fem.BoxMesh(P(0, 0, 0), P(1, 1, 1), 12, 12, 12)
        Vh = fem.VectorFunctionSpace(mesh, "P", 1)
        u, v = fem.TrialFunction(Vh), fem.TestFunction(Vh)
        a = sum(u[i].dx(k) * v[i].dx(k) * fem.dx for i in range(3) for k in range(3)) + fem.dot(u, v) * fem.dx
        L = fem.Constant(-1.0) * v[2] * fem.dx
        return Vh, a, L, fem.DirichletBC(Vh, fem.Constant((0.0, 0.0, 0.0)), lambda x, on_boundary: on_boundary)

    def p2():
        mesh = fem.BoxMesh(P(0, 0, 0), P(1, 1, 1), 9, 9, 9)
        Vh = fem.FunctionSpace(mesh, "P", 2)
        u, v = fem.TrialFunction(Vh), fem.TestFunction(Vh)
        return (Vh, fem.inner(fem.grad(u), fem.grad(v)) * fem.dx, fem.Constant(1.0) * v * fem.dx,
                fem.DirichletBC(Vh, 0.0, lambda x, on_boundary: on_boundary))

    def crossed():
        mesh = fem.RectangleMesh(P(0, 0), P(1, 1), 80, 80, "crossed")
        Vh = fem.FunctionSpace(mesh, "P", 1)
        u, v = fem.TrialFunction(Vh), fem.TestFunction(Vh)
        return (Vh, fem.inner(fem.grad(u), fem.grad(v)) * fem.dx, fem.Constant(1.0) * v * fem.dx,
                fem.DirichletBC(Vh, 0.0, lambda x, on_boundary: on_boundary))
    return {"vector_valued": vector, "p2": p2, "crossed_rectangle": crossed}


@pytest.mark.parametrize("case", ["vector_valued", "p2", "crossed_rectangle"])
def test_what_does_not_qualify_takes_jacobi_and_is_counted(hip_backend, case):
    Vh, a, L, bc = _fallback_cases()[case]()
    sol = fem.Function(Vh)
    v0, st0 = hip_backend.vmg_stats(), dict(fem.STATS)
    info = fem.solve(a == L, sol, bc, solver_parameters={"preconditioner": "vmg", "relative_tolerance": 1e-10})
    v1 = hip_backend.vmg_stats()
    print("%s under vmg: %s, counters %s -> %s" % (case, info, v0, v1))
    assert info["method"] == "jacobi_pcg" and info["relres"] <= 1e-10
    assert v1["fallbacks"] == v0["fallbacks"] + 1 and v1["solves"] == v0["solves"]
    assert fem.STATS.get("vmg_solves", 0) == st0.get("vmg_solves", 0)
