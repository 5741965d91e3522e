"""The p-multigrid preconditioner for P2 operators on box lattices on the device (pgdrome_amd/csrc/pgd_pmg.hip: pgd_mesh_p2_bind,
k_pmg_scan / k_pmg_galerkin / k_pmg_restrict / k_pmg_prolong, PGD_TUNE_PCG_PRECOND = 4, settings["preconditioner"] = "pmg") against
its numpy restatement tests/pmg_reference.py, a direct solve, and the Jacobi-PCG.  The operators are built through the frontend on
the HIP backend and read back from it for the restatement.  Boxes: the smallest vertex lattices that still have a hierarchy - a
cube, unequal axes, an even count along x."""
import numpy as np
import pytest

from pgdrome_amd import fem, problems
from tests import pmg_reference as PM

pytestmark = pytest.mark.gpu
P = fem.Point

BOXES = {"17x17x17": (17, 17, 17), "21x19x17": (21, 19, 17), "18x17x17": (18, 17, 17)}
_SPACES, _OPS, _REFS, _DIRECT = {}, {}, {}, {}


@pytest.fixture(scope="module")
def hip_backend():
    from pgdrome_amd.hip_backend import HipBackend
    old = fem._backend
    be = fem.set_backend(HipBackend(0))
    fem.clear_caches()
    yield be
    for d in (_SPACES, _OPS, _REFS, _DIRECT):
        d.clear()
    fem.set_backend(old)
    fem.clear_caches()


def _space(shape, nc):
    if (shape, nc) not in _SPACES:
        _SPACES[(shape, nc)] = PM.space(shape, nc)
    return _SPACES[(shape, nc)]


def _operator(be, box, name):
    """(fem.Matrix, scipy CSR, Dirichlet dofs, edge end vertices, seeded right-hand side) of a case on a box, its layout bound."""
    if (box, name) not in _OPS:
        Vh = _space(BOXES[box], PM.CASES[name][0])
        assert Vh._lay.bind_p2_lattice(be)
        A, M, bc = PM.operator(Vh, name)
        b = np.random.default_rng(11).uniform(-1, 1, M.shape[0])
        _OPS[(box, name)] = (A, M, bc, PM.base_layout(Vh).edge_vertices, b)
    return _OPS[(box, name)]


def _reference(be, box, name):
    """The restatement's hierarchy of a case, built once."""
    if (box, name) not in _REFS:
        _, M, _, ev, _ = _operator(be, box, name)
        _REFS[(box, name)] = PM.build(M, BOXES[box], ev, PM.CASES[name][0])
    return _REFS[(box, name)]


def _direct(be, box, name):
    """The direct solution of a case, computed once."""
    if (box, name) not in _DIRECT:
        _, M, _, _, b = _operator(be, box, name)
        nc = PM.CASES[name][0]
        _DIRECT[(box, name)] = PM.direct_solve(M, b, _space(BOXES[box], nc), nc)
    return _DIRECT[(box, name)]


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


def test_binding_takes_the_boxes_and_refuses_what_is_not_one(hip_backend):
    """pgd_mesh_p2_bind accepts the P2 layouts of the three boxes; it refuses - without an error - an edge list in which two end
    vertices are swapped so that an edge leaves the pattern, and the P1 layout of another box."""
    ctx = hip_backend.ctx
    for box, shape in BOXES.items():
        base = PM.base_layout(_space(shape, 1))
        p2 = ctx.mesh_upload(base.coords, base.cells)             # (a handle of the test's own: the layout's binding stays as it is)
        p1 = base.mesh.layout(1).handle()
        try:
            ev = np.asarray(base.edge_vertices)
            assert ctx.mesh_p2_bind(p2, p1, ev), box
            bad = ev.copy()
            bad[0, 1], bad[-1, 1] = ev[-1, 1], ev[0, 1]
            assert not ctx.mesh_p2_bind(p2, p1, bad), box
            assert ctx.mesh_p2_bind(p2, p1, ev), box              # (a later call decides anew)
            other = PM.base_layout(_space(BOXES["21x19x17" if box != "21x19x17" else "17x17x17"], 1)).mesh.layout(1).handle()
            assert not ctx.mesh_p2_bind(p2, other, ev), box
            assert not ctx.mesh_p2_bind(p2, p2, ev), box          # (a P2 layout is no lattice)
        finally:
            ctx.mesh_free(p2)


@pytest.mark.parametrize("name", ["clamped", "roller", "scalar_hull"])
@pytest.mark.parametrize("box", sorted(BOXES))
def test_galerkin_blocks_equal_the_restatement(hip_backend, box, name):
    """pgd_pmg_coarse after a solve under PGD_TUNE_PCG_PRECOND = 4, every component: the eliminated bytes of the restatement,
    identity rows exact, exact zeros where the restatement stores nothing, every other entry within
    2 gamma_n (|P|^T |A| |P|)_IJ, gamma_n = n eps / (1 - n eps), n the largest number of terms summed into one entry (the
    weights 1, 1/2 and 1/4 are exact, only the additions round - in the device's sum and in the restatement's)."""
    ctx, shape = hip_backend.ctx, BOXES[box]
    A, M, bc, ev, b = _operator(hip_backend, box, name)
    nc, nvert = PM.CASES[name][0], int(np.prod(shape))
    H = _reference(hip_backend, box, name)
    c0 = ctx.pmg_stats()
    _solve(ctx, A, b, 4, 1e-2, 2)
    c1 = ctx.pmg_stats()
    assert c1["solves"] == c0["solves"] + 1 and c1["fallbacks"] == c0["fallbacks"]
    el = PM.eliminated_dofs(M)
    for c in range(nc):
        slots, elb = ctx.pmg_coarse(c, nvert)
        assert np.array_equal(elb.astype(bool), H.levels[c][0].el)
        assert np.array_equal(elb.astype(bool), el[c::nc][:nvert])
        ref, stored = PM.slots_of(H.B[c], shape)
        fixed = elb.astype(bool)
        assert np.all(slots[0, fixed] == 1.0) and np.all(slots[1:, fixed] == 0.0)
        assert np.all(slots[~stored] == 0.0)
        mag, cnt = PM.galerkin_bound(M, nvert, ev, nc, c, el)
        n = int(cnt.max())
        eps = 2.0 ** -53
        gamma = n * eps / (1.0 - n * eps)
        bound, _ = PM.slots_of(mag, shape)
        err = np.abs(slots - ref)
        worst = float((err[stored] / np.maximum(bound[stored], 1e-300)).max()) if stored.any() else 0.0
        print("%s %s component %d: %d stored entries, n = %d, largest error / (|P|^T |A| |P|) = %.3g (bound %.3g)"
              % (box, name, c, int(stored.sum()), n, worst, 2 * gamma))
        assert np.all(err <= 2.0 * gamma * bound)


# Every case is held to the direct solution.  For the elasticity cases (108 000 unknowns and more) that is the expensive part of
# this file - about half a minute each behind the nested dissection of pmg_reference.direct_solve - so it is computed once per case
# (_direct) and the set is the smallest that puts every box under the three-component kernels: roller supports (three different
# eliminated sets) on the three boxes, the clamped block on the cube.
SOLVES = [(box, name) for box in sorted(BOXES) for name in ("roller", "scalar_hull")] + [("17x17x17", "clamped")]


@pytest.mark.parametrize("box,name", SOLVES)
def test_solve_equals_the_restatement(hip_backend, box, name):
    """pgd_pcg_solve under PGD_TUNE_PCG_PRECOND = 4: the restatement's iteration count to +-1 (reordered sums), its solution to 1e-9,
    the direct solution to 1e-8, the eliminated dofs exactly b; counted as a
    solve of the p-multigrid cycle and by no other counter; fewer iterations than the same solve under 0."""
    ctx, shape, rtol = hip_backend.ctx, BOXES[box], 1e-12
    A, M, bc, ev, b = _operator(hip_backend, box, name)
    nc = PM.CASES[name][0]
    mg0, v0, cm0, p0 = ctx.mg_stats(), ctx.vmg_stats(), ctx.cmg_stats(), ctx.pmg_stats()
    it, rel, x = _solve(ctx, A, b, 4, rtol)
    form = ctx.pcg_last_form()
    mg1, v1, cm1, p1 = ctx.mg_stats(), ctx.vmg_stats(), ctx.cmg_stats(), ctx.pmg_stats()
    itj, relj, xj = _solve(ctx, A, b, 0, rtol)
    xr, itr, relr = PM.pcg(M, b, shape, ev, nc, rtol=rtol)
    print("%s %s: device %d iterations (restatement %d), Jacobi-PCG device %d; counters %s -> %s" % (box, name, it, itr, itj, p0, p1))
    assert rel <= rtol
    assert abs(it - itr) <= 1
    assert np.linalg.norm(x - xr) <= 1e-9 * np.linalg.norm(xr)
    ref = _direct(hip_backend, box, name)
    assert np.linalg.norm(x - ref) <= 1e-8 * np.linalg.norm(ref)
    assert np.array_equal(x[bc], b[bc])
    assert it < itj
    assert p1["solves"] == p0["solves"] + 1 and p1["fallbacks"] == p0["fallbacks"]
    assert p1["levels"] == 2 and p1["setup_ms"] > p0["setup_ms"]
    assert mg1 == mg0 and v1 == v0 and cm1 == cm0
    assert form == ("PRECOND", "PMG")
    assert ctx.pmg_stats()["solves"] == p1["solves"] and ctx.pmg_stats()["fallbacks"] == p1["fallbacks"]      # (the solve under 0 counts nowhere)


def test_the_same_solve_twice_is_bit_identical(hip_backend):
    ctx = hip_backend.ctx
    A, M, bc, ev, b = _operator(hip_backend, "18x17x17", "roller")
    it1, _, x1 = _solve(ctx, A, b, 4, 1e-10)
    it2, _, x2 = _solve(ctx, A, b, 4, 1e-10)
    assert it1 == it2 and np.array_equal(x1, x2)


def _elastic_solve(prec, cells=16):
    mesh = fem.BoxMesh(P(0, 0, 0), P(1, 1, 1), cells, cells, cells)
    Vh = fem.VectorFunctionSpace(mesh, "P", 2)
    u, v = fem.TrialFunction(Vh), fem.TestFunction(Vh)
    a = (fem.inner(problems._voigt_C(0.3) * problems._strain(u), problems._strain(v)) + fem.Constant(2.0) * fem.inner(u, v)) * fem.dx
    sol = fem.Function(Vh)
    prm = {"relative_tolerance": 1e-10}
    if prec is not None:
        prm["preconditioner"] = prec
    info = fem.solve(a == fem.dot(fem.Constant((0.0, 0.0, -1.0)), v) * fem.dx, sol,
                     fem.DirichletBC(Vh, fem.Constant((0.0, 0.0, 0.0)), problems._clamped), solver_parameters=prm)
    return info, sol.vector().get_local()


def _poisson_solve(prec, cells=16):
    mesh = fem.BoxMesh(P(0, 0, 0), P(1, 1, 1), cells, cells, cells)
    Vh = fem.FunctionSpace(mesh, "P", 2)
    u, v = fem.TrialFunction(Vh), fem.TestFunction(Vh)
    sol = fem.Function(Vh)
    prm = {"relative_tolerance": 1e-10}
    if prec is not None:
        prm["preconditioner"] = prec
    info = fem.solve(fem.inner(fem.grad(u), fem.grad(v)) * fem.dx == fem.Constant(1.0) * v * fem.dx, sol,
                     fem.DirichletBC(Vh, 0.0, lambda x, on_boundary: on_boundary), solver_parameters=prm)
    return info, sol.vector().get_local()


@pytest.mark.parametrize("problem", ["elasticity", "poisson"])
def test_frontend_pmg_request_runs_the_cycle(hip_backend, problem):
    """A P2 space on a 16^3-cell box: "pmg" and "p_multigrid" are answered by the p-multigrid cycle; "amg", "vmg", "cmg" and no
    preconditioner by the Jacobi-PCG."""
    solve = _elastic_solve if problem == "elasticity" else _poisson_solve
    st0 = dict(fem.STATS)
    info_p, xp = solve("pmg")
    st1 = dict(fem.STATS)
    info_j, xj = solve(None)
    others = {name: solve(name)[0] for name in ("amg", "vmg", "cmg")}
    st2 = dict(fem.STATS)
    print("%s 16^3 cells P2: pmg request %s, no preconditioner %s, others %s" % (problem, info_p, info_j, others))
    assert info_p["method"] == "pmg_pcg" and st1.get("pmg_solves", 0) == st0.get("pmg_solves", 0) + 1
    assert st1["pcg_iterations"] == st0["pcg_iterations"] + info_p["iterations"]
    assert info_j["method"] == "jacobi_pcg"
    assert all(i["method"] == "jacobi_pcg" for i in others.values())
    assert st2.get("pmg_solves", 0) == st1.get("pmg_solves", 0)
    assert info_p["iterations"] < info_j["iterations"]
    assert np.linalg.norm(xp - xj) <= 1e-8 * np.linalg.norm(xj)
    info_w, _ = solve("p_multigrid")
    assert info_w["method"] == "pmg_pcg" and info_w["iterations"] == info_p["iterations"]
    assert fem.STATS.get("pmg_solves", 0) == st2.get("pmg_solves", 0) + 1


def _crossed_box(n):
    """An n^3-cube box with a vertex in the middle of every cube, 12 tetrahedra per cube (two per face, with the face diagonals of
    the 6-tets-per-cube cut, which match between neighbouring cubes): a 3-D mesh whose vertices are no lattice."""
    coords, _ = fem.box_mesh_arrays((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), n, n, n)
    sx, sy = n + 1, (n + 1) * (n + 1)
    iz, iy, ix = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    v0 = (iz * sy + iy * sx + ix).ravel()
    v1, v2, v3 = v0 + 1, v0 + sx, v0 + sx + 1
    v4, v5, v6, v7 = v0 + sy, v1 + sy, v2 + sy, v3 + sy
    ctr = coords.shape[0] + np.arange(v0.size)
    centres = 0.125 * sum(coords[v] for v in (v0, v1, v2, v3, v4, v5, v6, v7))
    faces = ((v0, v1, v3), (v0, v3, v2), (v4, v5, v7), (v4, v7, v6), (v0, v1, v5), (v0, v5, v4),
             (v2, v3, v7), (v2, v7, v6), (v0, v2, v6), (v0, v6, v4), (v1, v3, v7), (v1, v7, v5))
    cells = np.concatenate([np.stack([a, b, c, ctr], axis=1) for a, b, c in faces], axis=0).astype(np.int32)
    return fem.Mesh(np.concatenate([coords, centres], axis=0), cells)


def _fallback_cases():
    hull = lambda x, on_boundary: on_boundary

    def poisson(mesh, degree):
        Vh = fem.FunctionSpace(mesh, "P", degree)
        u, v = fem.TrialFunction(Vh), fem.TestFunction(Vh)
        return Vh, fem.inner(fem.grad(u), fem.grad(v)) * fem.dx, fem.Constant(1.0) * v * fem.dx, fem.DirichletBC(Vh, 0.0, hull)
    return {"p1_space": lambda: poisson(fem.BoxMesh(P(0, 0, 0), P(1, 1, 1), 16, 16, 16), 1),
            "p2_in_2d": lambda: poisson(fem.RectangleMesh(P(0, 0), P(1, 1), 40, 40), 2),
            "crossed_box": lambda: poisson(_crossed_box(8), 2),
            "small_lattice": lambda: poisson(fem.BoxMesh(P(0, 0, 0), P(1, 1, 1), 8, 8, 8), 2)}       # 9^3 vertices: no hierarchy


@pytest.mark.parametrize("case", ["p1_space", "p2_in_2d", "crossed_box", "small_lattice"])
def test_what_does_not_qualify_takes_jacobi_and_is_counted(hip_backend, case):
    Vh, a, L, bc = _fallback_cases()[case]()
    sol = fem.Function(Vh)
    p0, c0, v0, st0 = hip_backend.pmg_stats(), hip_backend.cmg_stats(), hip_backend.vmg_stats(), dict(fem.STATS)
    info = fem.solve(a == L, sol, bc, solver_parameters={"preconditioner": "pmg", "relative_tolerance": 1e-10})
    p1 = hip_backend.pmg_stats()
    print("%s under pmg: %s, counters %s -> %s" % (case, info, p0, p1))
    assert info["method"] == "jacobi_pcg" and info["relres"] <= 1e-10
    assert p1["fallbacks"] == p0["fallbacks"] + 1 and p1["solves"] == p0["solves"]
    assert hip_backend.cmg_stats() == c0 and hip_backend.vmg_stats() == v0
    assert fem.STATS.get("pmg_solves", 0) == st0.get("pmg_solves", 0)


def test_pgd_run_agrees_under_pmg(hip_backend):
    """problems.elastic_block with degree 2 on a 16^3-cell box, two modes, under the Jacobi-PCG and under "pmg": the same modes and
    fixed-point passes, every spatial solve through the p-multigrid cycle."""
    from pgdrome_amd.solver import PGDProblem

    def run(prec):
        fem.clear_caches()
        mesh = fem.BoxMesh(P(0, 0, 0), P(1, 1, 1), 16, 16, 16)
        p = PGDProblem(**problems.elastic_block(mesh, degree=2, PGD_nmax=2))
        settings = {"linear_solver": "cg", "relative_tolerance": 1e-10}
        if prec is not None:
            settings["preconditioner"] = prec
        st0 = dict(fem.STATS)
        p.solve_PGD(_problem="linear", settings=settings)
        return p, {k: fem.STATS.get(k, 0) - st0.get(k, 0) for k in ("linear_solves", "mg_solves", "vmg_solves", "cmg_solves", "pmg_solves", "pcg_iterations")}
    pj, uj = run(None)
    pp, up = run("pmg")
    print("elastic_block degree 2, 16^3 cells: jacobi %s, pmg %s" % (uj, up))
    assert pj.PGD_modes == pp.PGD_modes and pj.num_fp_it == pp.num_fp_it
    for d in range(2):
        for k in range(pj.PGD_modes):
            a, b = pj.PGD_func[d][k].vector().get_local(), pp.PGD_func[d][k].vector().get_local()
            assert np.linalg.norm(a - b) <= 1e-6 * np.linalg.norm(a)
    assert uj["pmg_solves"] == 0 and up["mg_solves"] == 0 and up["vmg_solves"] == 0 and up["cmg_solves"] == 0
    assert up["pmg_solves"] == sum(pp.num_fp_it)
    assert up["pcg_iterations"] < uj["pcg_iterations"]
