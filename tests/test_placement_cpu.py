"""PGD.sensor_placement without a GPU: the numpy route (design_update_numpy, design_gains_numpy) and the frontend against the
longdouble restatement of tests/placement_reference.py inside its derived bounds; the determinant-lemma identity, submodularity, the
closed form for modes linear in one parameter, installed / exclude / ties, the grouping, the default prior precision, every refusal."""
import numpy as np
import pytest

from oracle.backend_numpy import NumpyBackend
from pgdrome_amd import fem, model
from pgdrome_amd.model import PGD
from tests import placement_reference as PR

CANDS = [[0.15, 0.2], [0.5, 0.5], [0.93, 0.11], [0.3, 0.8], [0.71, 0.64], [0.05, 0.95], [0.62, 0.33], [0.4, 0.1], [0.85, 0.85],
         [0.22, 0.47], [0.58, 0.91], [0.77, 0.29]]
# the shapes of tests/test_placement_gpu.py that a longdouble greedy run takes a moment for
SHAPES = [((5,), 1, 3, 1), ((17,), 5, 17, 1), ((5, 7, 3), 17, 37, 1), ((5, 7, 3), 17, 37, 3), ((1, 9, 1), 48, 16, 2),
          ((2, 2, 2, 2, 2, 3), 64, 130, 2)]
IDS = ["n%s-k%d-M%d-R%d" % ("x".join(map(str, s[0])), s[1], s[2], s[3]) for s in SHAPES]


@pytest.fixture(scope="module")
def oracle():
    old = fem._backend
    fem.set_backend(NumpyBackend())
    fem.clear_caches()
    yield
    fem.set_backend(old)
    fem.clear_caches()


def function(V, a):
    f = fem.Function(V)
    f.vector()._host = np.array(a, dtype=np.float64)
    f.vector().touched_host()
    return f


def make(spaces, mats):
    modes = [[function(V, F[:, k]) for k in range(F.shape[1])] for V, F in zip(spaces, mats)]
    return PGD(name="synthetic", n_modes=mats[0].shape[1], fmeshes=[V.mesh() for V in spaces], pgd_modes=modes,
               name_coord=["x%d" % d for d in range(len(spaces))], modes_info=["U", "Node", "Scalar"])


@pytest.fixture(scope="module")
def two_parameters(oracle):
    """Five seeded modes on a rectangle (fixed), a P1 and a P2 interval; twelve candidate points; grids of 9 and 6 abscissae."""
    rng = np.random.default_rng(11)
    V = fem.FunctionSpace(fem.RectangleMesh(fem.Point(0, 0), fem.Point(1, 1), 5, 4), "CG", 1)
    Vp = fem.FunctionSpace(fem.IntervalMesh(6, 0.0, 2.0), "CG", 1)
    Vq = fem.FunctionSpace(fem.IntervalMesh(4, -1.0, 1.0), "CG", 2)
    K = 5
    mats = [rng.standard_normal((V.dim(), K)), 1.0 + 0.4 * rng.standard_normal((Vp.dim(), K)), 1.0 + 0.4 * rng.standard_normal((Vq.dim(), K))]
    sol = make([V, Vp, Vq], mats)
    grids = [np.sort(rng.uniform(0.0, 2.0, 9)), np.linspace(-0.9, 0.95, 6)]
    return sol, grids


def restate(sol, grids, sigma, gradient, **kw):
    """The grid and the whitened rows the frontend works with, from the solution's own tables."""
    K = sol.used_numModes
    tables = [np.ascontiguousarray(sol._free_modes_at(d, x, 0)) for d, x in zip((1, 2), grids)]
    dtables = [np.ascontiguousarray(sol._free_mode_derivatives_at(d, x, 0)) for d, x in zip((1, 2), grids)]
    weights = []
    for x in grids:
        w = model.trapezoid_weights(x)
        weights.append(w / w.sum())
    A = np.ascontiguousarray(sol.sensor_modes(CANDS, 0, 0, gradient=gradient).host()[:K].T / sigma)
    return PR.grid_of(tables, dtables, weights), A, weights


# ------------------------------------------------------------------------------------------ the arithmetic alone
@pytest.mark.parametrize("grid,k,M,R", SHAPES, ids=IDS)
def test_numpy_arithmetic_against_the_restatement(grid, k, M, R):
    cs = PR.recipe(grid, k, M, R)
    g = PR.grid_of(cs["tables"], cs["dtables"], cs["weights"])
    state = model.design_state_numpy(grid)
    args = (state, cs["tables"], cs["dtables"], cs["weights"])
    ld0, cov0 = model.design_update_numpy(*args, h0=cs["H0"])
    rows = cs["a"][:2 * R]
    ld, cov = model.design_update_numpy(*args, rows=rows)
    # H, W, the sums
    H, dH = PR.h_exact(g, cs["H0"], rows)
    assert np.all(np.abs(state["H"] - H.astype(np.float64)) <= dH + np.abs(H.astype(np.float64)) * PR.U)
    E, bE = PR.w_backward_bound(state["H"], state["W"])
    print("W H W^T - I: max error / bound", float(np.max(np.abs(E) / bE)))
    assert np.all(np.abs(E) <= bE) and np.all(np.triu(state["W"], 1) == 0.0)
    ldx, b_ld, covx, b_cov = PR.sums_exact(g, H, dH)
    print("log det: error / bound", float(abs(ld - ldx) / b_ld), " covariance:", float(np.max(np.abs(cov - covx) / b_cov)))
    assert abs(ld - ldx) <= b_ld and np.all(np.abs(cov - covx) <= b_cov) and np.array_equal(cov, cov.T)
    # the gains at that state
    gains = model.design_gains_numpy(cs["a"], R, *args)
    gx, bound = PR.gains_exact(g, cs["a"], R, state["W"])
    ratio = np.abs(gains - gx).astype(np.float64) / bound
    print("gains: max error / bound", float(ratio.max()))
    assert np.all(ratio <= 1.0) and np.all(gains > 0.0)
    # chunks of samples change the sums by rounding only
    small = model.design_gains_numpy(cs["a"], R, *args, work=M * R * len(grid) * 7)
    assert np.all(np.abs(small - gx).astype(np.float64) <= bound)


@pytest.mark.parametrize("grid,k,M,R", SHAPES, ids=IDS)
def test_the_recipe_keeps_best_and_runner_up_apart(grid, k, M, R):
    cs = PR.recipe(grid, k, M, R)
    g = PR.grid_of(cs["tables"], cs["dtables"], cs["weights"])
    ref = PR.greedy(g, cs["a"], R, cs["H0"], min(6, M - 1))
    print("relative gaps", ref["gap"])
    assert min(ref["gap"]) >= 1e-5
    for step, j in enumerate(ref["selected"]):
        assert ref["gap"][step] * float(ref["gains"][step][j]) > 10.0 * ref["bounds"][step].max()


# ------------------------------------------------------------------------------------------ the frontend
@pytest.mark.parametrize("gradient,prior_precision", [(False, None), (True, None), (True, "full")], ids=["R1", "R2", "R2-full-prior"])
def test_frontend_against_the_restatement(two_parameters, gradient, prior_precision):
    sol, grids = two_parameters
    sigma, n_select = 0.3, 5
    if prior_precision == "full":
        prior_precision = np.array([[2.0, 0.7], [0.7, 1.5]])
    res = sol.sensor_placement(0, [1, 2], 0, CANDS, n_select, grids=grids, sigma=sigma, gradient=gradient, prior_precision=prior_precision,
                               keep_gains=True)
    assert res.path == "numpy"
    g, A, weights = restate(sol, grids, sigma, gradient)
    R = 2 if gradient else 1
    ref = PR.greedy(g, A, R, res.prior_precision, n_select)
    # the condition of the selection, on the reference: every gap is more than ten times the bound
    for step, j in enumerate(ref["selected"]):
        assert ref["gap"][step] * float(ref["gains"][step][j]) > 10.0 * ref["bounds"][step].max(), step
    assert list(res.selected) == ref["selected"]
    assert np.array_equal(res.selected_points, np.asarray(CANDS)[res.selected])
    for step in range(n_select):
        ratio = np.abs(res.gain_history[step] - ref["gains"][step]).astype(np.float64) / ref["bounds"][step]
        print("step", step, "gains: max error / bound", float(ratio.max()))
        assert np.all(ratio <= 1.0)
        assert res.gains[step] == res.gain_history[step][res.selected[step]]
    assert np.array_equal(res.first_gains, res.gain_history[0])
    # the determinant lemma: a chosen gain is the difference of the utilities the updates report
    assert res.utility[0] == 0.0 and res.utility.shape == (n_select + 1,)
    for step in range(n_select):
        tol = ref["bounds"][step][res.selected[step]] + 0.5 * (ref["logdet_bound"][step] + ref["logdet_bound"][step + 1])
        assert abs(res.gains[step] - (res.utility[step + 1] - res.utility[step])) <= tol
        assert abs(res.utility[step + 1] - float(0.5 * (ref["logdet"][step + 1] - ref["logdet"][0]))) <= 0.5 * (
            ref["logdet_bound"][step + 1] + ref["logdet_bound"][0])
    # submodularity: the chosen gains do not increase, up to the bound
    for step in range(1, n_select):
        assert res.gains[step] <= res.gains[step - 1] + ref["bounds"][step].max() + ref["bounds"][step - 1].max()
        assert np.all(res.gain_history[step] <= res.gain_history[step - 1] + ref["bounds"][step] + ref["bounds"][step - 1])
    # the expected posterior covariance
    assert res.expected_cov.shape == (n_select + 1, 2, 2)
    for step in range(n_select + 1):
        assert np.all(np.abs(res.expected_cov[step] - ref["cov"][step]).astype(np.float64) <= ref["cov_bound"][step])
    assert np.all(np.diff(np.trace(res.expected_cov, axis1=1, axis2=2)) < 0.0)


def test_modes_linear_in_one_parameter_have_the_closed_form(oracle):
    rng = np.random.default_rng(5)
    V = fem.FunctionSpace(fem.RectangleMesh(fem.Point(0, 0), fem.Point(1, 1), 5, 4), "CG", 1)
    Vp = fem.FunctionSpace(fem.IntervalMesh(8, 0.0, 2.0), "CG", 1)
    K = 4
    x = np.asarray(Vp.tabulate_dof_coordinates(), dtype=np.float64).reshape(Vp.dim(), -1)[:, 0]
    alpha, beta = np.array([1.0, -0.5, 0.25, 2.0]), np.array([0.5, -1.25, 2.0, 0.75])      # (dyadic: the nodal values are exact)
    Fp = alpha[None, :] + beta[None, :] * x[:, None]
    sol = make([V, Vp], [rng.standard_normal((V.dim(), K)), Fp])
    grid = np.array([0.25, 0.5, 0.75, 1.0, 1.5])                # (nodes of the mesh: 0.25 apart - every derivative is exact)
    h0, sigma = 3.0, 0.5
    res = sol.sensor_placement(0, [1], 0, CANDS, 1, grids=[grid], sigma=sigma, prior_precision=[[h0]])
    phi = sol.sensor_modes(CANDS, 0, 0).host()[:K].T / sigma
    gj = phi @ beta
    expected = 0.5 * np.log1p(gj * gj / h0)
    assert np.all(np.abs(res.first_gains - expected) <= 1e-13 * expected)
    assert res.selected[0] == int(np.argmax(expected))


def test_installed_exclude_and_ties(two_parameters):
    sol, grids = two_parameters
    cands = CANDS + [CANDS[4]]                                    # candidate 12 is candidate 4 again
    call = lambda n, **kw: sol.sensor_placement(0, [1, 2], 0, cands, n, grids=grids, sigma=0.3, **kw)
    free = call(3, keep_gains=True)
    assert free.first_gains[12] == free.first_gains[4]
    best = int(free.selected[0])
    # a tie goes to the lower index, and the twin of a chosen candidate is still on offer
    rest = [j for j in range(13) if j not in (4, 12)]
    tie = call(2, exclude=rest)
    assert list(tie.selected) == [4, 12] and tie.gains[1] < tie.gains[0]
    # exclude: the best one is never chosen, the run is otherwise the same
    ex = call(2, exclude=[best])
    assert best not in ex.selected and ex.selected[0] == int(np.argsort(-free.first_gains, kind="stable")[1])
    assert np.array_equal(ex.first_gains, free.first_gains)
    # installed: applied first, in order; the run then continues as the free one does after choosing them
    inst = call(1, installed=list(free.selected[:2]), keep_gains=True)
    assert inst.selected[0] == free.selected[2] and len(inst.installed_gains) == 2 and inst.utility.shape == (4,)
    g, A, _ = restate(sol, grids, 0.3, False)
    A = np.concatenate([A, A[4:5]])
    ref = PR.greedy(g, A, 1, free.prior_precision, 1, installed=list(free.selected[:2]))
    for i in range(2):
        assert abs(inst.installed_gains[i] - float(ref["installed_gains"][i])) <= ref["installed_bounds"][i]
        assert abs(inst.installed_gains[i] - free.gains[i]) <= 2.0 * ref["installed_bounds"][i]
    assert np.all(np.abs(inst.gain_history[0] - ref["gains"][0]).astype(np.float64) <= ref["bounds"][0])
    assert np.allclose(inst.utility[1:3], free.utility[1:3], rtol=0, atol=1e-12) and inst.expected_cov.shape == (2, 2, 2)
    # nothing to choose: the state after the installed ones alone
    none = call(0, installed=[3])
    assert none.selected.size == 0 and none.utility.shape == (2,) and none.expected_cov.shape == (1, 2, 2)


def test_group_entry_against_point(two_parameters):
    sol, grids = two_parameters
    kw = dict(grids=grids, sigma=0.3, keep_gains=True)
    point = sol.sensor_placement(0, [1, 2], 0, CANDS, 3, group="point", **kw)
    entry = sol.sensor_placement(0, [1, 2], 0, CANDS, 3, group="entry", **kw)
    for key in ("selected", "gains", "utility", "gain_history", "expected_cov", "selected_points"):
        assert np.array_equal(getattr(point, key), getattr(entry, key)), key
    # with the gradients every point has two entries: twice the candidates, each with one row
    sig = np.linspace(0.2, 0.5, 24).reshape(12, 2)
    ge = sol.sensor_placement(0, [1, 2], 0, CANDS, 3, group="entry", gradient=True, **{**kw, "sigma": sig})
    assert ge.first_gains.shape == (24,) and np.array_equal(ge.selected_points, np.asarray(CANDS)[ge.selected // 2])
    g, A, _ = restate(sol, grids, 1.0, True)
    ref = PR.greedy(g, A / sig.reshape(-1, 1), 1, ge.prior_precision, 3)
    assert list(ge.selected) == ref["selected"]
    assert np.all(np.abs(ge.gain_history[2] - ref["gains"][2]).astype(np.float64) <= ref["bounds"][2])


def test_default_prior_precision(two_parameters):
    sol, grids = two_parameters
    res = sol.sensor_placement(0, [1, 2], 0, CANDS, 1, grids=grids, prior={2: lambda x: 1.0 + x * x})
    want = []
    for d, x in zip((1, 2), grids):
        w = model.trapezoid_weights(x) * (1.0 + x * x if d == 2 else 1.0)
        w = w / w.sum()
        mean = float(w @ x)
        want.append(1.0 / float(w @ (x - mean) ** 2))
    assert np.allclose(np.diag(res.prior_precision), want, rtol=1e-12, atol=0) and res.prior_precision[0, 1] == 0.0
    with pytest.raises(ValueError, match="zero variance"):
        sol.sensor_placement(0, [1, 2], 0, CANDS, 1, grids=[grids[0], np.array([0.5])])
    one = sol.sensor_placement(0, [1, 2], 0, CANDS, 1, grids=[grids[0], np.array([0.5])], prior_precision=np.eye(2))
    assert one.selected.shape == (1,)


def test_refusals(two_parameters, monkeypatch):
    sol, grids = two_parameters
    call = lambda n=2, **kw: sol.sensor_placement(0, [1, 2], 0, CANDS, n, **{"grids": grids, **kw})
    with pytest.raises(ValueError, match="12 candidates are on offer"):
        call(13)
    with pytest.raises(ValueError, match="9 candidates are on offer"):
        call(10, installed=[1], exclude=[2, 3])
    with pytest.raises(ValueError, match="candidates are on offer"):
        call(-1)
    for key in ("installed", "exclude"):
        for bad in ([12], [-1], [0, 40]):
            with pytest.raises(ValueError, match="%s names candidate" % key):
                call(**{key: bad})
    with pytest.raises(ValueError, match="coords"):
        call(coords=np.zeros((4, 2)))
    with pytest.raises(ValueError, match="coords"):
        call(grids=None, coords=np.zeros((4, 2)))
    with pytest.raises(ValueError, match="exactly one of grids and coords"):
        call(grids=None)
    with pytest.raises(ValueError, match="group must be"):
        call(group="cell")
    with pytest.raises(ValueError, match="sigma must be finite"):
        call(sigma=0.0)
    with pytest.raises(ValueError, match="sigma has"):
        call(sigma=np.ones(5))
    for bad in (np.eye(3), np.array([[1.0, 2.0], [2.0, 1.0]]), np.array([[1.0, 0.1], [0.2, 1.0]]), np.array([[1.0, np.nan], [np.nan, 1.0]])):
        with pytest.raises(ValueError, match="symmetric positive definite"):
            call(prior_precision=bad)
    with pytest.raises(NotImplementedError, match="no design_gains"):
        call(device=True)
    # more than 64 modes or more than 3 rows on the device: the limits are module constants, lowered here
    monkeypatch.setattr(model, "PLACEMENT_MAX_MODES", 4)
    with pytest.raises(ValueError, match=r"PGD\.compress.*group=\"entry\""):
        call(device=True)
    assert call().path == "numpy"
    monkeypatch.setattr(model, "PLACEMENT_MAX_MODES", 64)
    monkeypatch.setattr(model, "PLACEMENT_MAX_ROWS", 1)
    with pytest.raises(ValueError, match=r"5 modes and 2 rows per candidate"):
        call(device=True, gradient=True)
    assert call(gradient=True).path == "numpy"
