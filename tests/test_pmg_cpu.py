"""The p-multigrid preconditioner for P2 operators on box lattices (pgdrome_amd/csrc/pgd_pmg.hip, PGD_TUNE_PCG_PRECOND = 4,
settings["preconditioner"] = "pmg") checked without a GPU, on its numpy restatement tests/pmg_reference.py; tests/test_pmg_gpu.py
compares the HIP path with it.  The operators are assembled by the numpy oracle backend through the frontend on the
6-tets-per-cube box with 17^3 vertices (33^3 P2 nodes): the spatial operator of problems.elastic_block (nu = 0.3) and the scalar
stiffness form.  Operators, Jacobi counts and direct solutions are computed once per case and shared.
"""
import functools

import numpy as np
import pytest

from tests import pmg_reference as PM
from tests import vmg_reference as V

S17 = (17, 17, 17)
NVERT = 17 ** 3


@pytest.fixture(scope="module")
def oracle_backend():
    from oracle.backend_numpy import NumpyBackend
    from pgdrome_amd import fem
    old = fem._backend
    be = fem.set_backend(NumpyBackend())
    fem.clear_caches()
    yield be
    _case.cache_clear()
    _hierarchy.cache_clear()
    _direct.cache_clear()
    if old is not None:
        fem.set_backend(old)
    else:
        fem._backend = None
    fem.clear_caches()


@functools.lru_cache(maxsize=None)
def _case(name):
    """(space, operator with the case's Dirichlet dofs as identity rows, those dofs, edge end vertices, seeded right-hand side)."""
    nc = PM.CASES[name][0]
    Vh = PM.space(S17, nc)
    _, A, bc = PM.operator(Vh, name)
    assert abs(A - A.T).max() <= 1e-14 * abs(A).max()
    return Vh, A, bc, PM.base_layout(Vh).edge_vertices, np.random.default_rng(7).uniform(-1, 1, A.shape[0])


@functools.lru_cache(maxsize=None)
def _hierarchy(name):
    _, A, _, ev, _ = _case(name)
    return PM.build(A, S17, ev, PM.CASES[name][0])


@functools.lru_cache(maxsize=None)
def _direct(name):
    Vh, A, _, _, b = _case(name)
    return PM.direct_solve(A, b, Vh, PM.CASES[name][0])


@pytest.mark.parametrize("name", ["clamped", "hull", "scalar_hull"])
def test_galerkin_blocks_lie_on_the_pattern_and_keep_the_eliminated_sets(oracle_backend, name):
    """Every B_c = P_c^T A_cc P_c stores nothing off the 15-point pattern of the vertex lattice, its rows without couplings are the
    vertex part of the P2 eliminated set, it is symmetric, and two levels are built."""
    _, A, bc, ev, _ = _case(name)
    nc = PM.CASES[name][0]
    el = PM.eliminated_dofs(A)
    assert np.array_equal(np.where(el)[0], bc)
    H = _hierarchy(name)
    for c in range(nc):
        B = H.B[c]
        off, big = V.off_pattern_max(B, S17)
        assert off == 0 and big > 0
        assert np.array_equal(V.eliminated_rows(B), el[c::nc][:NVERT])
        assert abs(B - B.T).max() <= 1e-14 * big
    assert [len(l) for l in H.levels] == [2] * nc


@pytest.mark.parametrize("name", ["clamped", "roller", "scalar_hull"])
def test_preconditioner_is_symmetric_positive_and_zero_on_eliminated_dofs(oracle_backend, name):
    """u^T M v = v^T M u to 1e-12 relative and v^T M v > 0 for 5 seeded pairs; M v vanishes on the eliminated dofs."""
    _, A, _, _, _ = _case(name)
    H = _hierarchy(name)
    rng = np.random.default_rng(5)
    for _ in range(5):
        u, v = rng.uniform(-1, 1, A.shape[0]), rng.uniform(-1, 1, A.shape[0])
        Mu, Mv = PM.apply(H, u), PM.apply(H, v)
        assert abs(u @ Mv - v @ Mu) <= 1e-12 * abs(u @ Mv)
        assert v @ Mv > 0.0 and u @ Mu > 0.0
        assert np.all(Mv[H.el] == 0.0) and np.all(Mu[H.el] == 0.0)


@pytest.mark.parametrize("name", ["clamped", "hull", "scalar_hull"])
def test_pcg_agrees_with_the_direct_solve_and_halves_the_jacobi_count(oracle_backend, name):
    """pmg_reference.pcg at rtol 1e-10 reproduces the direct solution to 1e-8 with fewer than half of the Jacobi-PCG's iterations
    (the restatement's counts: 69 / 703 clamped, 53 / 273 hull, 34 / 149 scalar)."""
    _, A, _, ev, b = _case(name)
    nc = PM.CASES[name][0]
    x, it, rel = PM.pcg(A, b, S17, ev, nc, rtol=1e-10)
    xj, itj, relj = PM.pcg(A, b, rtol=1e-10, precond="jacobi")
    print("17^3 vertices %s: p-multigrid %d iterations, Jacobi %d (%.2f)" % (name, it, itj, it / itj))
    assert rel <= 1e-10 and relj <= 1e-10
    ref = _direct(name)
    assert np.linalg.norm(x - ref) <= 1e-8 * np.linalg.norm(ref)
    assert np.linalg.norm(xj - ref) <= 1e-8 * np.linalg.norm(ref)
    assert 2 * it < itj


def test_roller_supports_give_three_different_eliminated_sets(oracle_backend):
    """Only u_x fixed on x = 0 and only u_z on z = 0, plus the foundation term (SPD): every component has its own coarse eliminated
    set, and PCG converges to the direct solution with x = b on the fixed dofs."""
    Vh, A, bc, ev, b = _case("roller")
    H = _hierarchy("roller")
    el = [l[0].el for l in H.levels]
    sets = PM.node_sets(Vh)
    vx0, vz0 = sets["x0"][sets["x0"] < NVERT], sets["z0"][sets["z0"] < NVERT]
    assert np.array_equal(np.where(el[0])[0], vx0) and not el[1].any() and np.array_equal(np.where(el[2])[0], vz0)
    assert not np.array_equal(el[0], el[2])
    x, it, rel = PM.pcg(A, b, S17, ev, 3, rtol=1e-10)
    print("17^3 vertices roller: p-multigrid %d iterations" % it)
    assert rel <= 1e-10
    assert np.array_equal(x[bc], b[bc])
    ref = _direct("roller")
    assert np.linalg.norm(x - ref) <= 1e-8 * np.linalg.norm(ref)


@pytest.mark.parametrize("prec", ["pmg", "p_multigrid"])
def test_frontend_names_and_a_backend_without_the_cycle(oracle_backend, prec):
    """The names are disjoint from the other three families; the numpy oracle backend has no precondition_p and answers a P2 space
    with the Jacobi-PCG, moving no counter."""
    from pgdrome_amd import fem
    names = set(fem.P_MULTIGRID_NAMES)
    assert prec in names
    assert not names & (set(fem.MULTIGRID_NAMES) | set(fem.VARIABLE_MULTIGRID_NAMES) | set(fem.COMPONENT_MULTIGRID_NAMES))
    assert not hasattr(oracle_backend, "precondition_p")
    mesh = fem.BoxMesh(fem.Point(0, 0, 0), fem.Point(1, 1, 1), 4, 4, 4)
    Vh = fem.VectorFunctionSpace(mesh, "P", 2)
    u, v = fem.TrialFunction(Vh), fem.TestFunction(Vh)
    a = sum(u[i].dx(k) * v[i].dx(k) * fem.dx for i in range(3) for k in range(3)) + fem.dot(u, v) * fem.dx
    sol = fem.Function(Vh)
    st0 = dict(fem.STATS)
    info = fem.solve(a == fem.Constant(-1.0) * v[2] * fem.dx, sol,
                     fem.DirichletBC(Vh, fem.Constant((0.0, 0.0, 0.0)), lambda x, on_boundary: on_boundary),
                     solver_parameters={"preconditioner": prec, "relative_tolerance": 1e-10})
    assert info["method"] == "jacobi_pcg" and info["relres"] <= 1e-10
    assert fem.STATS.get("pmg_solves", 0) == st0.get("pmg_solves", 0)
    assert len(Vh._lay.base._p2_bound) == 0          # (no binding was asked for)
