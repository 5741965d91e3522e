"""The component-wise multigrid preconditioner for vector-valued P1 operators on box lattices (pgdrome_amd/csrc/pgd_vmg.hip,
PGD_TUNE_PCG_PRECOND = 3, settings["preconditioner"] = "cmg") checked without a GPU, on its numpy restatement
tests/cmg_reference.py; tests/test_cmg_gpu.py compares the HIP path with it.  The operators are assembled by the numpy oracle
backend through the frontend: the spatial operator of problems.elastic_block (nu = 0.3) on the 6-tets-per-cube box.
"""
import functools

import numpy as np
import pytest

from tests import cmg_reference as CM
from tests import vmg_reference as V

NC = 3
S17 = (17, 17, 17)


@pytest.fixture(scope="module")
def oracle_backend():
    from oracle.backend_numpy import NumpyBackend
    from pgdrome_amd import fem
    old = fem._backend
    be = fem.set_backend(NumpyBackend())
    fem.clear_caches()
    yield be
    if old is not None:
        fem.set_backend(old)
    else:
        fem._backend = None
    fem.clear_caches()


@functools.lru_cache(maxsize=None)
def _operator(shape, case, k_found):
    """(operator with the case's Dirichlet dofs as identity rows, seeded right-hand side)."""
    Vh = CM.vector_space(shape)
    _, A = CM.frontend_operator(Vh, "elastic", CM.dirichlet_dofs(shape, NC, case), k_found=k_found)
    assert abs(A - A.T).max() <= 1e-14 * abs(A).max()
    return A, np.random.default_rng(7).uniform(-1, 1, A.shape[0])


@pytest.mark.parametrize("case", ["clamped", "hull"])
def test_diagonal_blocks_lie_on_the_15_point_pattern(oracle_backend, case):
    """Every diagonal block of the 17^3 operator stores nothing off the 15-point pattern of the base lattice and builds 2 levels."""
    A, _ = _operator(S17, case, 0.0)
    for c in range(NC):
        B = CM.component_operator(A, NC, c)
        off, big = V.off_pattern_max(B, S17)
        assert off == 0 and big > 0
        assert np.all(B.diagonal() == 1.0)
    levels = CM.build(A, S17, NC)
    assert [len(l) for l in levels] == [2, 2, 2]
    nbc = CM.dirichlet_dofs(S17, NC, case).size
    assert sum(int(l[0].el.sum()) for l in levels) == nbc


def test_33_cubed_builds_three_levels(oracle_backend):
    shape = (33, 33, 33)
    A, _ = _operator(shape, "clamped", 0.0)
    for c in range(NC):
        assert V.off_pattern_max(CM.component_operator(A, NC, c), shape)[0] == 0
    levels = CM.build(A, shape, NC)
    assert [len(l) for l in levels] == [3, 3, 3]
    assert [l[-1].A.shape[0] for l in levels] == [9 ** 3] * 3


@pytest.mark.parametrize("case", ["clamped", "roller"])
def test_preconditioner_is_symmetric_and_positive(oracle_backend, case):
    """u^T M v = v^T M u to 1e-12 relative and v^T M v > 0 for 5 seeded pairs (M of the unscaled system)."""
    A, _ = _operator(S17, case, 2.0)
    levels, s = CM.build(A, S17, NC), CM.scaling(A)
    rng = np.random.default_rng(5)
    for _ in range(5):
        u, v = rng.uniform(-1, 1, A.shape[0]), rng.uniform(-1, 1, A.shape[0])
        Mu, Mv = CM.apply(levels, s, u), CM.apply(levels, s, v)
        assert abs(u @ Mv - v @ Mu) <= 1e-12 * abs(u @ Mv)
        assert v @ Mv > 0.0 and u @ Mu > 0.0
        assert np.all(Mv[CM.eliminated_dofs(levels)] == 0.0)


CASES = [("clamped", 0.0), ("clamped", 2.0), ("hull", 0.0)]


@pytest.mark.parametrize("case,k_found", CASES)
def test_pcg_agrees_with_the_direct_solve_and_halves_the_jacobi_count(oracle_backend, case, k_found):
    """cmg_reference.pcg at rtol 1e-10 reproduces spsolve to 1e-8 with fewer than half of the Jacobi-PCG's iterations (measured with
    the scaled-residual stop test: 0.18, 0.17 and 0.30 of them)."""
    A, b = _operator(S17, case, k_found)
    x, it, rel = CM.pcg(A, b, S17, NC, rtol=1e-10)
    xj, itj, relj = CM.pcg(A, b, S17, NC, rtol=1e-10, precond="jacobi")
    print("17^3 %s k_found %g: component cycle %d iterations, Jacobi %d (%.2f)" % (case, k_found, it, itj, it / itj))
    assert rel <= 1e-10 and relj <= 1e-10
    ref = CM.direct_solve(A, b, S17, NC)
    assert np.linalg.norm(x - ref) <= 1e-8 * np.linalg.norm(ref)
    assert np.linalg.norm(xj - ref) <= 1e-8 * np.linalg.norm(ref)
    assert 2 * it < itj


def test_roller_supports_give_three_different_eliminated_sets(oracle_backend):
    """Only u_x fixed on x = 0 and only u_z on z = 0, plus the foundation term (SPD): every component has its own eliminated set, and
    PCG converges to the direct solution."""
    A, b = _operator(S17, "roller", 2.0)
    levels = CM.build(A, S17, NC)
    el = [l[0].el for l in levels]
    sets = CM.node_sets(S17)
    assert np.array_equal(np.where(el[0])[0], sets["x0"]) and not el[1].any() and np.array_equal(np.where(el[2])[0], sets["z0"])
    assert not np.array_equal(el[0], el[2])
    x, it, rel = CM.pcg(A, b, S17, NC, rtol=1e-10)
    _, itj, _ = CM.pcg(A, b, S17, NC, rtol=1e-10, precond="jacobi")
    print("17^3 roller: component cycle %d iterations, Jacobi %d" % (it, itj))
    assert rel <= 1e-10 and it < itj
    bc = CM.dirichlet_dofs(S17, NC, "roller")
    assert np.array_equal(x[bc], b[bc])
    ref = CM.direct_solve(A, b, S17, NC)
    assert np.linalg.norm(x - ref) <= 1e-8 * np.linalg.norm(ref)


@pytest.mark.parametrize("prec", ["cmg", "component_multigrid"])
def test_frontend_names_and_a_backend_without_the_cycle(oracle_backend, prec):
    """The names are disjoint from the other two families; the numpy oracle backend has no precondition_component and answers with
    the Jacobi-PCG."""
    from pgdrome_amd import fem
    names = set(fem.COMPONENT_MULTIGRID_NAMES)
    assert prec in names and not names & set(fem.MULTIGRID_NAMES) and not names & set(fem.VARIABLE_MULTIGRID_NAMES)
    assert not hasattr(oracle_backend, "precondition_component")
    mesh = fem.BoxMesh(fem.Point(0, 0, 0), fem.Point(1, 1, 1), 5, 5, 5)
    Vh = fem.VectorFunctionSpace(mesh, "P", 1)
    u, v = fem.TrialFunction(Vh), fem.TestFunction(Vh)
    a = sum(u[i].dx(k) * v[i].dx(k) * fem.dx for i in range(3) for k in range(3)) + fem.dot(u, v) * fem.dx
    sol = fem.Function(Vh)
    st0 = dict(fem.STATS)
    info = fem.solve(a == fem.Constant(-1.0) * v[2] * fem.dx, sol,
                     fem.DirichletBC(Vh, fem.Constant((0.0, 0.0, 0.0)), lambda x, on_boundary: on_boundary),
                     solver_parameters={"preconditioner": prec, "relative_tolerance": 1e-10})
    assert info["method"] == "jacobi_pcg" and info["relres"] <= 1e-10
    assert fem.STATS.get("cmg_solves", 0) == st0.get("cmg_solves", 0)
