"""PGD.evaluate_gradient_many(planes="fused" / "auto") on the host path (oracle backend, no GPU): the fused path keeps no
planes - per sample chunk it combines the nodal modes and takes the cell gradients of the chunk's fields - and is held to the
same loop over PGD.evaluate, inside the same derived bounds of tests/eval_gradient_reference.py, as the stored path.  That bound
is written for a code that derives the planes per mode and combines them; a code that combines first is covered by its
``plane_shift`` term (the evaluated field's own rounding seen through the gradient)."""
import numpy as np
import pytest

from oracle.backend_numpy import NumpyBackend
from pgdrome_amd import fem, problems
from pgdrome_amd.model import PGD
from pgdrome_amd.solver import PGDProblem
from tests.eval_gradient_reference import check_result, loop_reference, run_and_check, samples_of, two_valued

NU = 0.3


@pytest.fixture(scope="module")
def oracle():
    old = fem._backend
    fem.set_backend(NumpyBackend())
    fem.clear_caches()
    yield
    fem.set_backend(old)
    fem.clear_caches()


@pytest.fixture(scope="module")
def elastic(oracle):
    mesh = fem.BoxMesh(fem.Point(0, 0, 0), fem.Point(2, 1, 1), 3, 3, 3)
    p = PGDProblem(**problems.elastic_block(mesh, 7, PGD_nmax=3))
    p.solve_PGD(_problem="linear", settings={"relative_tolerance": 1e-11})
    return mesh, p.return_PGD()


@pytest.fixture(scope="module")
def diffusion(oracle):
    mesh = fem.RectangleMesh(fem.Point(0, 0), fem.Point(1.5, 1), 6, 5)
    p = PGDProblem(**problems.reaction_diffusion(mesh, 9, PGD_nmax=3))
    p.solve_PGD(_problem="linear")
    return mesh, p.return_PGD()


def interval_solution():
    """One mode on an interval (steps of 0.3: no binary fractions) times the constant 1 on a parameter interval."""
    mesh = fem.IntervalMesh(7, 0.0, 2.1)
    f = fem.Function(fem.FunctionSpace(mesh, "CG", 1))
    f.vector()._host = np.random.default_rng(3).standard_normal(8)
    f.vector().touched_host()
    pm = fem.IntervalMesh(2, 0.0, 1.0)
    one = fem.Function(fem.FunctionSpace(pm, "CG", 1))
    one.vector().set_local(np.ones(3))
    return PGD(name="synthetic", n_modes=1, fmeshes=[mesh, pm], pgd_modes=[[f], [one]], name_coord=["x", "p"])


def builds():
    return fem.STATS.get("gradient_mode_builds", 0)


def fused_calls():
    return fem.STATS.get("eval_gradient_fused_calls", 0)


def test_fused_von_mises_of_the_elastic_block(elastic):
    mesh, sol = elastic
    n0 = fused_calls()
    run_and_check(sol, [1], samples_of(sol, (1,), 17, 5), "von_mises", two_valued(mesh, 1.0 / (1.0 + NU), 3.0 / (1.0 + NU)),
                  planes="fused", sample_chunk=5)
    assert fused_calls() == n0 + 1


def test_fused_flux_of_reaction_diffusion(diffusion):
    mesh, sol = diffusion
    run_and_check(sol, [1], samples_of(sol, (1,), 17, 3), "gradient_norm", None, planes="fused")
    run_and_check(sol, [1], samples_of(sol, (1,), 9, 4), "gradient_norm", 0.7, planes="fused", sample_chunk=4)


def test_fused_on_a_one_mode_interval(oracle):
    sol = interval_solution()
    run_and_check(sol, [1], np.array([[0.0], [1.0], [0.5], [0.3]]), "gradient_norm", None, planes="fused")


def test_fused_builds_and_caches_nothing(elastic):
    mesh, sol = elastic
    att = sol.mesh[0].attributes[0]
    coords = samples_of(sol, (1,), 5, 7)
    scale = two_valued(mesh, 1.0, 2.0)
    for start in ("empty", "filled"):
        if start == "empty":
            att._gradient_modes = None
        else:
            sol.evaluate_gradient_many(0, [1], coords, 0, quantity="von_mises", scale=scale)
            assert att._gradient_modes is not None
        before, n0 = att._gradient_modes, builds()
        sol.evaluate_gradient_many(0, [1], coords, 0, quantity="gradient_norm", scale=scale, planes="fused")
        assert att._gradient_modes is before and builds() == n0, start
    # the stored planes survived the fused call of another quantity: the next stored call reuses them
    sol.evaluate_gradient_many(0, [1], coords, 0, quantity="von_mises", scale=scale)
    assert builds() == n0


def test_modes_max_bytes_one_byte_short(elastic):
    mesh, sol = elastic
    coords = samples_of(sol, (1,), 6, 8)
    scale = two_valued(mesh, 1.0 / (1.0 + NU), 3.0 / (1.0 + NU))
    nbytes = sol.used_numModes * 6 * mesh.num_cells() * 8
    with pytest.raises(ValueError, match=str(nbytes)):
        sol.evaluate_gradient_many(0, [1], coords, 0, quantity="von_mises", scale=scale, modes_max_bytes=nbytes - 1, planes="stored")
    n0, f0 = builds(), fused_calls()
    run_and_check(sol, [1], coords, "von_mises", scale, planes="auto", modes_max_bytes=nbytes - 1)
    assert builds() == n0 and fused_calls() == f0 + 1               # "auto" went the fused way
    sol.mesh[0].attributes[0]._gradient_modes = None
    run_and_check(sol, [1], coords, "von_mises", scale, planes="auto", modes_max_bytes=nbytes)
    assert builds() == n0 + 1 and fused_calls() == f0 + 1           # ... and the stored way where the planes fit
    run_and_check(sol, [1], coords, "von_mises", scale, planes="fused", modes_max_bytes=0)
    assert fused_calls() == f0 + 2


def test_an_unknown_planes_value_is_refused(elastic):
    mesh, sol = elastic
    with pytest.raises(ValueError, match="nonsense"):
        sol.evaluate_gradient_many(0, [1], samples_of(sol, (1,), 4, 8), 0, planes="nonsense")


@pytest.mark.parametrize("case", ["elastic", "diffusion"])
def test_fused_and_stored_agree_within_their_bounds(case, request):
    mesh, sol = request.getfixturevalue(case)
    quantity, scale = ("von_mises", two_valued(mesh, 0.5, 2.0)) if case == "elastic" else ("gradient_norm", None)
    coords = samples_of(sol, (1,), 11, 12)
    V = sol.mesh[0].attributes[0].interpolationfct[0].function_space()
    L = fem.gradient_quantity(quantity, mesh.geometry().dim(), V._ncomp)
    ref, Bd = loop_reference(sol, 0, [1], coords, 0, L, None if scale is None else scale.vector().host())
    threshold = float(np.median(ref.astype(np.float64)))
    out = {}
    for planes in ("stored", "fused"):
        out[planes] = sol.evaluate_gradient_many(0, [1], coords, 0, quantity=quantity, scale=scale, envelope=True, threshold=threshold,
                                                 fields=True, planes=planes)
        check_result(out[planes], ref, Bd, threshold)
    a, b = out["stored"], out["fused"]
    fa, fb = (np.array([f.vector().host() for f in r.fields]) for r in (a, b))
    assert np.all(np.abs(fa - fb) <= 2.0 * Bd)                      # each within Bd of the one reference
    for x, y, bd in ((a.min, b.min, Bd.max(axis=1)), (a.max, b.max, Bd.max(axis=1)),
                     (a.envelope_min.vector().host(), b.envelope_min.vector().host(), Bd.max(axis=0)),
                     (a.envelope_max.vector().host(), b.envelope_max.vector().host(), Bd.max(axis=0))):
        assert np.all(np.abs(x - y) <= 2.0 * bd)
    assert np.array_equal(a.coefficients, b.coefficients)
