"""fem.gradient_quantity and PGD.evaluate_gradient_many on the host path (oracle backend, no GPU): analytic strain states,
a loop over PGD.evaluate with the reference gradient of tests/eval_gradient_reference.py inside its derived bounds, the
refusals and the cache of the derived modes."""
import math

import numpy as np
import pytest

from oracle.backend_numpy import NumpyBackend
from pgdrome_amd import fem, problems
from pgdrome_amd.model import PGD
from pgdrome_amd.solver import FD_matrices, PGDProblem
from tests import heat1d_problem
from tests.eval_gradient_reference import (cell_gradients, evaluate_norm_reference, norm_bound, planes, run_and_check, samples_of,
                                           two_valued)

E_MOD, NU, EPS = 210.0, 0.3, 1e-3
MU = E_MOD / (2.0 * (1.0 + NU))


@pytest.fixture(scope="module")
def oracle():
    old = fem._backend
    fem.set_backend(NumpyBackend())
    fem.clear_caches()
    yield
    fem.set_backend(old)
    fem.clear_caches()


def one_mode_solution(mesh, V, values):
    """A separated solution of one mode: the given nodal values (vertex order) on ``mesh`` times the constant 1 on an interval."""
    f = fem.Function(V)
    f.vector()._host = np.array(values, dtype=np.float64).reshape(-1)
    f.vector().touched_host()
    pm = fem.IntervalMesh(2, 0.0, 1.0)
    one = fem.Function(fem.FunctionSpace(pm, "CG", 1))
    one.vector().set_local(np.ones(3))
    return PGD(name="synthetic", n_modes=1, fmeshes=[mesh, pm], pgd_modes=[[f], [one]], name_coord=["x", "p"])


def test_reference_restatement_on_integers():
    mesh = fem.RectangleMesh(fem.Point(0, 0), fem.Point(3, 2), 3, 2)
    X, cells = mesh.coordinates(), mesh.cells()
    U = np.stack([2 * X[:, 0] - 3 * X[:, 1] + 1, X[:, 0] + 5 * X[:, 1]], axis=1).astype(np.int64)
    g = cell_gradients(X, cells, U)
    assert g.dtype == np.int64 and np.all(g == np.array([2, -3, 1, 5]))
    L = np.array([[1, 0, 0, 1], [0, 2, -1, 0]])
    p = planes(X, cells, U, L, np.arange(1, len(cells) + 1))
    assert np.array_equal(p, np.outer([7, -7], np.arange(1, len(cells) + 1)))
    r = evaluate_norm_reference(np.array([[[3], [0]], [[0], [1]]]), np.array([[1, 2], [4, 0]]), math.sqrt(30.5))
    assert r["SS"].tolist() == [[25, 36]] and r["V"].tolist() == [[5.0, 6.0]] and r["exceed"].tolist() == [1]
    assert r["min"].tolist() == [5.0, 6.0] and r["env_max"].tolist() == [6.0]
    assert norm_bound(np.zeros((2, 3)), np.ones(3)).max() < 1e-15


STATES_3D = {
    "uniaxial": (lambda X: np.stack([EPS * X[:, 0], -NU * EPS * X[:, 1], -NU * EPS * X[:, 2]], axis=1), E_MOD * EPS),
    "shear": (lambda X: np.stack([EPS * X[:, 1], 0 * X[:, 0], 0 * X[:, 0]], axis=1), math.sqrt(3.0) * MU * EPS),
    "hydrostatic": (lambda X: EPS * X, 0.0),
}
# plane strain (eps_zz = 0): a uniaxial STRESS sigma_xx = s has the lateral strain eps_yy = -nu / (1 - nu) eps_xx, s = E eps_xx /
# (1 - nu^2), sigma_zz = nu s and so the von Mises stress s sqrt(1 - nu + nu^2); an equal in-plane stretch eps is not free of
# deviatoric stress there (sigma_xx - sigma_zz = 2 mu eps): von Mises stress 2 mu eps
STATES_2D = {
    "uniaxial": (lambda X: np.stack([EPS * X[:, 0], -NU / (1.0 - NU) * EPS * X[:, 1]], axis=1),
                 E_MOD * EPS / (1.0 - NU * NU) * math.sqrt(1.0 - NU + NU * NU)),
    "shear": (lambda X: np.stack([EPS * X[:, 1], 0 * X[:, 0]], axis=1), math.sqrt(3.0) * MU * EPS),
    "hydrostatic": (lambda X: EPS * X, 2.0 * MU * EPS),
}


@pytest.mark.parametrize("state", list(STATES_3D))
@pytest.mark.parametrize("dim", [3, 2])
def test_von_mises_of_analytic_strain_states(oracle, dim, state):
    """scale = 2 mu = E / (1 + nu) turns the quantity into the von Mises stress: uniaxial stress E eps, pure shear sqrt(3) mu
    gamma, hydrostatic strain 0 (to 1e-13 of the unit scale E eps), in every cell; 2-D is plane strain."""
    if dim == 3:
        mesh = fem.BoxMesh(fem.Point(0, 0, 0), fem.Point(1, 1, 1), 2, 2, 2)
        field, expected = STATES_3D[state]
    else:
        mesh = fem.RectangleMesh(fem.Point(0, 0), fem.Point(1, 1), 3, 2)
        field, expected = STATES_2D[state]
    V = fem.VectorFunctionSpace(mesh, "CG", 1)
    X = mesh.coordinates()
    L = fem.gradient_quantity("von_mises", dim, dim)
    assert L.shape == (6 if dim == 3 else 4, dim * dim)
    p = planes(X, mesh.cells(), field(X), L * (2.0 * MU))
    direct = np.sqrt((p * p).sum(axis=0)).astype(np.float64)
    sol = one_mode_solution(mesh, V, field(X))
    res = sol.evaluate_gradient_many(0, [1], [[0.5]], 0, quantity="von_mises", scale=2.0 * MU, envelope=True, fields=True)
    through = res.fields[0].vector().host()
    assert res.fields[0].function_space()._dg0 and through.shape == (mesh.num_cells(),)
    for got in (direct, through, res.envelope_max.vector().host()):
        assert np.all(np.abs(got - expected) <= 1e-13 * E_MOD * EPS), (state, np.abs(got - expected).max())
    assert abs(res.max[0] - expected) <= 1e-13 * E_MOD * EPS and res.max_abs[0] == res.max[0]


def test_gradient_quantity_matrices():
    assert np.array_equal(fem.gradient_quantity("gradient_norm", 3, 1), np.eye(3))
    assert np.array_equal(fem.gradient_quantity("gradient_norm", 2, 3), np.eye(6))
    for bad in (("von_mises", 3, 1), ("von_mises", 2, 3), ("von_mises", 1, 1), ("tresca", 3, 3), ("gradient_norm", 4, 1)):
        with pytest.raises(ValueError):
            fem.gradient_quantity(*bad)


def test_host_path_on_the_heat_problem(oracle):
    sol = heat1d_problem.run(fem, PGDProblem, FD_matrices, fd_time=False).return_PGD()
    coords = samples_of(sol, (1, 2), 21, 11)
    res, threshold = run_and_check(sol, [1, 2], coords, "gradient_norm", 0.5, sample_chunk=8)
    # the chunking of the host path changes nothing, and outputs that were not asked for are absent
    one = sol.evaluate_gradient_many(0, [1, 2], coords, 0, scale=0.5, envelope=True, sample_chunk=1000)
    assert np.array_equal(one.min, res.min) and np.array_equal(one.envelope_max.vector().host(), res.envelope_max.vector().host())
    assert one.fields is None and one.exceedance is None
    mesh = sol.mesh[0].attributes[0].interpolationfct[0].function_space().mesh()
    assert res.envelope_min.function_space()._dg0 and res.envelope_min.function_space().mesh() is mesh


def test_host_path_on_reaction_diffusion_with_a_cellwise_scale(oracle):
    mesh = fem.RectangleMesh(fem.Point(0, 0), fem.Point(1.5, 1), 5, 4)
    p = PGDProblem(**problems.reaction_diffusion(mesh, 9, PGD_nmax=3))
    p.solve_PGD(_problem="linear")
    sol = p.return_PGD()
    run_and_check(sol, [1], samples_of(sol, (1,), 17, 3), "gradient_norm", two_valued(mesh, 0.7, 2.5))


@pytest.fixture(scope="module")
def elastic(oracle):
    mesh = fem.BoxMesh(fem.Point(0, 0, 0), fem.Point(2, 1, 1), 3, 3, 3)
    p = PGDProblem(**problems.elastic_block(mesh, 7, PGD_nmax=3))
    p.solve_PGD(_problem="linear", settings={"relative_tolerance": 1e-11})
    return mesh, p.return_PGD()


def test_host_path_on_the_elastic_block(elastic):
    mesh, sol = elastic
    run_and_check(sol, [1], samples_of(sol, (1,), 17, 5), "von_mises", two_valued(mesh, 1.0 / (1.0 + NU), 3.0 / (1.0 + NU)))
    run_and_check(sol, [1], samples_of(sol, (1,), 5, 6), "gradient_norm", None)


def test_cache_of_the_derived_modes(elastic):
    mesh, sol = elastic
    coords = samples_of(sol, (1,), 5, 7)
    scale = two_valued(mesh, 1.0, 2.0)
    builds = lambda: fem.STATS.get("gradient_mode_builds", 0)
    sol.evaluate_gradient_many(0, [1], coords, 0, quantity="von_mises", scale=scale)
    n0 = builds()
    a = sol.evaluate_gradient_many(0, [1], coords, 0, quantity="von_mises", scale=scale)
    assert builds() == n0                                       # reused
    scale.vector()[:] = 2.0 * scale.vector()[:]
    b = sol.evaluate_gradient_many(0, [1], coords, 0, quantity="von_mises", scale=scale)
    assert builds() == n0 + 1                                   # the scale's vector changed: rebuilt
    assert np.allclose(b.max, 2.0 * a.max, rtol=1e-14, atol=0.0)
    sol.evaluate_gradient_many(0, [1], coords, 0, quantity="gradient_norm", scale=scale)
    assert builds() == n0 + 2                                   # another quantity: the key changed, the old planes are dropped
    assert sol.mesh[0].attributes[0]._gradient_modes.key[0] == "gradient_norm"


def test_refusals(elastic, oracle, monkeypatch):
    mesh, sol = elastic
    coords = samples_of(sol, (1,), 4, 8)
    other = fem.BoxMesh(fem.Point(0, 0, 0), fem.Point(2, 1, 1), 3, 3, 3)
    with pytest.raises(ValueError):
        sol.evaluate_gradient_many(0, [1], coords, 0, scale=two_valued(other, 1.0, 2.0))          # a scale of another mesh
    with pytest.raises(ValueError):
        sol.evaluate_gradient_many(0, [1], coords, 0, scale=fem.Function(fem.FunctionSpace(mesh, "CG", 1)))      # not DG0
    with pytest.raises(ValueError):
        sol.evaluate_gradient_many(0, [1], coords, 0, quantity="tresca")
    nbytes = sol.used_numModes * 6 * mesh.num_cells() * 8
    with pytest.raises(ValueError, match=str(nbytes)):
        sol.evaluate_gradient_many(0, [1], coords, 0, quantity="von_mises", modes_max_bytes=nbytes - 1)
    sol.evaluate_gradient_many(0, [1], coords, 0, quantity="von_mises", modes_max_bytes=nbytes)
    with pytest.raises(ValueError, match=str(mesh.num_cells() * 4 * 8)):
        sol.evaluate_gradient_many(0, [1], coords, 0, fields=True, fields_max_bytes=mesh.num_cells() * 4 * 8 - 1)
    # von Mises of a scalar field
    heat = heat1d_problem.run(fem, PGDProblem, FD_matrices, fd_time=False).return_PGD()
    hc = samples_of(heat, (1, 2), 3, 9)
    with pytest.raises(ValueError):
        heat.evaluate_gradient_many(0, [1, 2], hc, 0, quantity="von_mises")
    # P2 modes
    m2 = fem.IntervalMesh(4, 0.0, 1.0)
    V2 = fem.FunctionSpace(m2, "CG", 2)
    with pytest.raises(NotImplementedError):
        one_mode_solution(m2, V2, np.arange(V2.dim())).evaluate_gradient_many(0, [1], [[0.5]], 0)
    # a row-sharded fixed dimension
    with monkeypatch.context() as mp:
        mp.setattr(mesh, "part", fem.Partition(None, 0, 8, 16, 0, 1, 0), raising=False)
        with pytest.raises(NotImplementedError):
            sol.evaluate_gradient_many(0, [1], coords, 0)
    # the interp1d (array) mode
    for d in (1, 2):
        heat.mesh[d].attributes[0].interpolationInfo = {"name": 0, "kind": "linear"}
        heat.mesh[d].attributes[0].interpolationfct = []
    with pytest.raises(ValueError):
        heat.evaluate_gradient_many(0, [1, 2], hc, 0)
