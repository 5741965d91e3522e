"""PGD.sensor_posterior_many and grid_posterior_many_numpy on the numpy route (oracle backend, no GPU) against the longdouble
restatement and the derived bounds of tests/posterior_many_reference.py, against sensor_posterior one data set at a time, every
refusal, the chunking of the data sets, and sensor_posterior itself against the untouched numpy arithmetic it had before its setup
was shared.  Every input is seeded."""
import math

import numpy as np
import pytest

from oracle.backend_numpy import NumpyBackend
from pgdrome_amd import fem, model
from pgdrome_amd.model import PGD
from tests import posterior_many_reference as RM
from tests import posterior_reference as R

U53 = 2.0 ** -53
PTS = [[0.15, 0.2], [0.5, 0.5], [0.93, 0.11], [0.3, 0.8], [0.71, 0.64], [0.05, 0.95], [0.62, 0.33]]


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
    """Five seeded modes on a rectangle (fixed), a P1 and a P2 interval; seven sensors; grids of 9 and 6 abscissae."""
    rng = np.random.default_rng(7)
    V = fem.FunctionSpace(fem.RectangleMesh(fem.Point(0, 0), fem.Point(1, 1), 5, 4), "CG", 1)
    Vp = fem.FunctionSpace(fem.IntervalMesh(6, 0.0, 2.0), "CG", 1)
    Vq = fem.FunctionSpace(fem.IntervalMesh(4, -1.0, 1.0), "CG", 2)
    K = 5
    mats = [rng.standard_normal((V.dim(), K)), 1.0 + 0.4 * rng.standard_normal((Vp.dim(), K)), 1.0 + 0.4 * rng.standard_normal((Vq.dim(), K))]
    sol = make([V, Vp, Vq], mats)
    grids = [np.sort(rng.uniform(0.0, 2.0, 9)), np.linspace(-1.0, 1.0, 6)]
    tables = [np.ascontiguousarray(sol._free_modes_at(d, g, 0)) for d, g in zip((1, 2), grids)]
    phi = sol.sensor_modes(PTS, 0, 0).host()[:K].T
    node = (4, 2)
    truth = phi @ (tables[0][:, node[0]] * tables[1][:, node[1]])
    return sol, grids, tables, phi, node, truth


def stream(truth, N, noise, seed):
    return truth[None, :] + noise * np.random.default_rng(seed).standard_normal((N, truth.size))


# ------------------------------------------------------------------------------------------ the arithmetic alone
@pytest.mark.parametrize("grid,k,m,nd", [((5, 7, 3), 5, 17, 9), ((17,), 17, 1, 3), ((2, 2, 2, 2, 2, 3), 4, 16, 5)], ids=["3d", "1d", "6d"])
@pytest.mark.parametrize("accumulate", [False, True], ids=["each", "accumulate"])
def test_numpy_arithmetic_against_the_restatement(grid, k, m, nd, accumulate):
    rng = np.random.default_rng(100 * k + m + nd)
    tables = [1.0 + 0.5 * rng.standard_normal((k, n)) for n in grid]
    a = rng.standard_normal((m, k)) / np.sqrt(k)
    c = np.ones(k)
    for t, i in zip(tables, np.unravel_index(rng.integers(0, int(np.prod(grid))), grid)):
        c = c * t[:, i]
    Y = (a @ c)[None, :] + 0.4 * rng.standard_normal((nd, m))
    weights = [rng.uniform(0.2, 1.0, n) for n in grid]
    absc = [np.sort(rng.uniform(-1.0, 2.0, n)) for n in grid]
    u, alpha, beta = RM.data_sets(Y, accumulate)
    out = model.grid_posterior_many_numpy(a, u, alpha, beta, tables, weights, abscissae=absc, want=model.POST_THETA, sample_chunk=37)
    chi2x, scale = RM.chi2_many_exact(a, Y, tables, accumulate)
    worst = RM.check(out, chi2x, RM.chi2_many_bound(k, m, len(grid), scale, accumulate), weights, absc)
    print("max error / bound:", worst)
    assert all(v <= 1.0 for v in worst.values())
    # the sample chunks do not move the minima; without the bit there are no moments
    again = model.grid_posterior_many_numpy(a, u, alpha, beta, tables, weights, sample_chunk=1 << 12)
    assert np.array_equal(again["argmin"], out["argmin"]) and "theta1" not in again


# ------------------------------------------------------------------------------------------ the frontend
def test_frontend_against_the_restatement(two_parameters):
    sol, grids, tables, phi, node, truth = two_parameters
    sigma = np.random.default_rng(3).uniform(0.05, 0.2, len(PTS))
    data = stream(truth, 6, sigma, 11)
    prior = {1: lambda x: math.exp(-0.5 * (x - 1.0) ** 2), 2: np.linspace(1.0, 2.0, 6)}
    res = sol.sensor_posterior_many(0, [1, 2], 0, PTS, data, grids=grids, sigma=sigma, prior=prior, reduce=False)
    assert res.path == "numpy" and res.mean.shape == (6, 2) and res.cov.shape == (6, 2, 2) and res.map_index.shape == (6, 2)
    RM.check_result(res, phi / sigma[:, None], data / sigma, tables, logdet=float(np.sum(np.log(sigma))))
    # data shaped like the samples of evaluate_sensor_response_many, and outputs=(): no moments
    bare = sol.sensor_posterior_many(0, [1, 2], 0, PTS, data.reshape((6,) + tuple(sol.sensor_modes(PTS, 0, 0).shape)), grids=grids,
                                     sigma=sigma, prior=prior, reduce=False, outputs=())
    assert bare.mean is None and bare.cov is None and np.array_equal(bare.Z, res.Z) and np.array_equal(bare.log_evidence, res.log_evidence)


def test_accumulate_against_the_cumulative_restatement(two_parameters):
    sol, grids, tables, phi, node, truth = two_parameters
    sigma = 0.3
    data = stream(truth, 7, sigma, 12)
    res = sol.sensor_posterior_many(0, [1, 2], 0, PTS, data, grids=grids, sigma=sigma, accumulate=True, reduce=False)
    RM.check_result(res, phi / sigma, data / sigma, tables, accumulate=True, logdet=len(PTS) * math.log(sigma))
    # more data, less spread
    assert res.cov[-1].trace() < res.cov[0].trace()


def test_the_thin_qr_reduces_all_data_sets_at_once(two_parameters):
    """Seven sensors, five modes: the default route runs on R (5 x 5) and Q^T Y; the remainder of every data set enters chi2_min and
    the evidence.  The restatement is that of the reduced problem with the remainder added (the QR's own term: posterior_reference)."""
    sol, grids, tables, phi, node, truth = two_parameters
    sigma = 0.25
    data = stream(truth, 5, sigma, 13)
    A, Y = phi / sigma, data / sigma
    Q, Rm = np.linalg.qr(A)
    Zr = Y @ Q
    r = Y - Zr @ Q.T
    for accumulate in (False, True):
        res = sol.sensor_posterior_many(0, [1, 2], 0, PTS, data, grids=grids, sigma=sigma, accumulate=accumulate)
        rest = np.einsum("np,np->n", r, r)
        RM.check_result(res, Rm, Zr, tables, accumulate=accumulate, rest=np.cumsum(rest) if accumulate else rest,
                     logdet=len(PTS) * math.log(sigma), m=len(PTS))


def test_one_data_set_equals_sensor_posterior(two_parameters):
    sol, grids, tables, phi, node, truth = two_parameters
    sigma = 0.2
    data = stream(truth, 1, sigma, 14)
    many = sol.sensor_posterior_many(0, [1, 2], 0, PTS, data, grids=grids, sigma=sigma, reduce=False)
    one = sol.sensor_posterior(0, [1, 2], 0, PTS, data[0], grids=grids, sigma=sigma, reduce=False, outputs=("theta",), keep_chi2=True)
    assert one.path == "numpy" and many.path == "numpy"
    a, Y = phi / sigma, data / sigma
    chi2x, scale = RM.chi2_many_exact(a, Y, tables)
    bound = RM.chi2_many_bound(5, len(PTS), 2, scale)
    ex, bd, mean, dmean = RM.moments(many, 0, chi2x, bound, tables)
    # sensor_posterior's own side: the difference form within chi2_bound of the same exact misfits
    _, B2 = R.chi2_exact(a, Y[0], tables)
    tau = R.chi2_bound(5, len(PTS), 2, B2)
    ex1 = R.posterior_exact(chi2x[0], one.shift, None, one.weights, one.grids)
    bd1 = R.posterior_bounds(ex1, chi2x[0].astype(np.float64), one.shift, tau, 2)
    dmean1 = RM.ratio_bound(mean, bd1["theta1"], bd1["Z"], float(ex1["Z"]))
    assert np.all(np.abs(many.mean[0] - one.mean) <= dmean + dmean1)
    assert tuple(many.map_index[0]) == one.map_index                     # (the gap of this case is far above the bounds:)
    assert RM.gap(chi2x)[0] > 4 * bound[0].max()
    arg = int(np.argmin(chi2x[0]))
    assert abs(many.chi2_min[0] - one.chi2_min) <= 2 * tau[arg]
    dlog = bd["Z"] / float(ex["Z"]) + bd1["Z"] / float(ex1["Z"]) + bound[0, arg] + tau[arg] + 16 * U53 * abs(one.log_evidence)
    assert abs(many.log_evidence[0] - one.log_evidence) <= dlog


def test_accumulated_step_equals_sensor_posterior_of_the_mean(two_parameters):
    """All data up to step n under sigma is the mean of the n + 1 vectors under sigma / sqrt(n + 1), up to a factor free of the
    parameters: the same mean and MAP.  Data at a node plus small noise: the exact runner-up gap is stated and checked."""
    sol, grids, tables, phi, node, truth = two_parameters
    sigma = 0.05
    data = stream(truth, 6, 0.2 * sigma, 15)
    many = sol.sensor_posterior_many(0, [1, 2], 0, PTS, data, grids=grids, sigma=sigma, accumulate=True, reduce=False)
    a, Y = phi / sigma, data / sigma
    chi2x, scale = RM.chi2_many_exact(a, Y, tables, accumulate=True)
    bound = RM.chi2_many_bound(5, len(PTS), 2, scale, accumulate=True)
    assert np.all(RM.gap(chi2x) > 4 * bound.max(axis=1))
    for n in (0, 2, 5):
        sn = sigma / math.sqrt(n + 1)
        ybar = data[:n + 1].mean(axis=0)
        one = sol.sensor_posterior(0, [1, 2], 0, PTS, ybar, grids=grids, sigma=sn, reduce=False, outputs=("theta",))
        assert tuple(many.map_index[n]) == one.map_index == node
        ex, bd, mean, dmean = RM.moments(many, n, chi2x, bound, tables)
        # sensor_posterior's side from ITS whitened inputs (the mean is rounded: n + 2 roundings of data of the size of its scale)
        chi1, B2 = R.chi2_exact(phi / sn, ybar / sn, tables)
        tau = R.chi2_bound(5, len(PTS), 2, B2) + 2 * (n + 4) * U53 * B2
        ex1 = R.posterior_exact(chi1, one.shift, None, one.weights, one.grids)
        bd1 = R.posterior_bounds(ex1, chi1.astype(np.float64), one.shift, tau, 2)
        mean1 = (ex1["theta1"] / ex1["Z"]).astype(np.float64)
        assert np.all(np.abs(one.mean - mean1) <= RM.ratio_bound(mean1, bd1["theta1"], bd1["Z"], float(ex1["Z"])))
        assert np.all(np.abs(many.mean[n] - one.mean) <= dmean + 2 * RM.ratio_bound(mean1, bd1["theta1"], bd1["Z"], float(ex1["Z"])))


def test_the_chunks_of_data_sets_change_no_bit(two_parameters):
    sol, grids, tables, phi, node, truth = two_parameters
    data = stream(truth, 10, 0.3, 16)
    runs = [sol.sensor_posterior_many(0, [1, 2], 0, PTS, data, grids=grids, sigma=0.3, accumulate=acc, data_chunk=ch)
            for acc in (False, True) for ch in (1, 7, 10)]
    for base in (0, 3):
        for res in runs[base + 1:base + 3]:
            for key in ("chi2_min", "map_index", "map_coords", "log_evidence", "ess", "mean", "cov", "Z", "shift"):
                assert np.array_equal(getattr(res, key), getattr(runs[base], key)), key
    assert not np.array_equal(runs[0].mean, runs[3].mean)


def test_refusals(two_parameters, monkeypatch):
    sol, grids, tables, phi, node, truth = two_parameters
    data = stream(truth, 3, 0.3, 17)
    call = lambda d=data, **kw: sol.sensor_posterior_many(0, [1, 2], 0, PTS, d, **{"grids": grids, **kw})
    with pytest.raises(NotImplementedError, match="sensor_posterior takes them"):
        call(grids=None, coords=np.zeros((4, 2)))
    with pytest.raises(NotImplementedError, match="sensor_posterior takes them"):
        call(coords=np.zeros((4, 2)))
    for bad in (data[0], data[:, :6], data.reshape(3, 7, 1), np.zeros((0, 7))):
        with pytest.raises(ValueError, match="data has shape"):
            call(bad)
    for v in (np.nan, np.inf):
        d = data.copy()
        d[1, 3] = v
        with pytest.raises(ValueError, match="not finite"):
            call(d)
    for outputs in (("marginals",), ("theta", "coef")):
        with pytest.raises(ValueError, match="unknown outputs"):
            call(outputs=outputs)
    with pytest.raises(ValueError, match="data_chunk"):
        call(data_chunk=0)
    with pytest.raises(ValueError, match="sigma must be finite"):
        call(sigma=0.0)
    with pytest.raises(ValueError, match="exactly one of grids and coords"):
        call(grids=None)
    with pytest.raises(NotImplementedError, match="no grid_posterior_many"):
        call(device=True)
    # more than 64 modes or rows: the limits are module constants, lowered here instead of building a 65-mode solution
    monkeypatch.setattr(model, "POSTERIOR_MANY_MAX_MODES", 4)
    with pytest.raises(ValueError, match="compress the solution first"):
        call()
    monkeypatch.setattr(model, "POSTERIOR_MANY_MAX_MODES", 64)
    monkeypatch.setattr(model, "POSTERIOR_MANY_MAX_ROWS", 6)
    with pytest.raises(ValueError, match="7 rows and 5 modes"):
        call(reduce=False)
    assert call().path == "numpy"                                          # (the QR brings the 7 rows down to 5)


def test_64_modes_and_rows_are_taken_and_65_refused(oracle):
    rng = np.random.default_rng(65)
    V, Vp = fem.FunctionSpace(fem.IntervalMesh(80, 0.0, 1.0), "CG", 1), fem.FunctionSpace(fem.IntervalMesh(3, 0.0, 1.0), "CG", 1)
    pts = np.linspace(0.01, 0.99, 66)[:, None]
    grid = [np.array([0.0, 0.5, 1.0])]
    for K, rows, reduce, ok in ((64, 64, False, True), (65, 65, True, False), (64, 65, False, False), (64, 66, True, True)):
        sol = make([V, Vp], [rng.standard_normal((V.dim(), K)), 1.0 + 0.3 * rng.standard_normal((Vp.dim(), K))])
        data = rng.standard_normal((2, rows))
        if ok:
            assert sol.sensor_posterior_many(0, [1], 0, pts[:rows], data, grids=grid, reduce=reduce).Z.shape == (2,)
        else:
            with pytest.raises(ValueError, match="at most 64 and 64 are possible: compress"):
                sol.sensor_posterior_many(0, [1], 0, pts[:rows], data, grids=grid, reduce=reduce)


# ------------------------------------------------------------------------------------------ sensor_posterior keeps its bits
@pytest.mark.parametrize("noise", ["sigma", "sigma-array", "cov"])
@pytest.mark.parametrize("reduce", [False, True], ids=["rows", "qr"])
def test_sensor_posterior_is_what_it_was(two_parameters, noise, reduce):
    """Its setup is now shared with sensor_posterior_many: the results are, bit for bit, what the untouched grid_misfit_numpy and
    grid_posterior_numpy give for inputs whitened and reduced by the statements the method had before."""
    from scipy.linalg import solve_triangular
    sol, grids, tables, phi, node, truth = two_parameters
    rng = np.random.default_rng(21)
    m = len(PTS)
    data = truth + 0.2 * rng.standard_normal(m)
    prior = {2: np.linspace(1.0, 2.0, 6)}
    if noise == "cov":
        G = rng.standard_normal((m, m))
        cov = 0.04 * (np.eye(m) + 0.1 * G @ G.T)
        L = np.linalg.cholesky(cov)
        A, y, logdet, kw = solve_triangular(L, phi, lower=True), solve_triangular(L, data, lower=True), float(np.sum(np.log(np.diag(L)))), dict(cov=cov)
    else:
        sg = np.asarray(0.2 if noise == "sigma" else rng.uniform(0.1, 0.3, m))
        sgb = np.broadcast_to(sg.reshape(-1) if sg.ndim else sg, (m,))
        A, y, logdet, kw = phi / sgb[:, None], data / sgb, float(np.sum(np.log(sgb))), dict(sigma=sg)
    rest = 0.0
    if reduce:
        Q, Rm = np.linalg.qr(A)
        z = Q.T @ y
        r = y - Q @ z
        A, y, rest = Rm, z, float(r @ r)
    A, y = np.ascontiguousarray(A), np.ascontiguousarray(y)
    res = sol.sensor_posterior(0, [1, 2], 0, PTS, data, grids=grids, prior=prior, reduce=reduce, keep_chi2=True, **kw)
    chi2, cmin, arg = model.grid_misfit_numpy(A, y, tables)
    want = model.POST_MARGINALS | model.POST_THETA | model.POST_COEF
    sums = model.grid_posterior_numpy(chi2, cmin, [9, 6], res.weights, tables=tables, abscissae=grids, want=want)
    Z = sums["Z"]
    assert res.Z == Z and res.shift == cmin and res.chi2_min == cmin + rest
    assert np.array_equal(np.asarray(res.chi2).reshape(-1), chi2 + rest)
    assert res.map_index == tuple(int(i) for i in np.unravel_index(arg, (9, 6)))
    assert res.log_evidence == math.log(Z) - 0.5 * (cmin + rest) - 0.5 * m * math.log(2.0 * math.pi) - logdet
    assert res.ess == Z * Z / sums["sum_e2"]
    mean = sums["theta1"] / Z
    assert np.array_equal(res.mean, mean) and np.array_equal(res.cov, sums["theta2"] / Z - np.outer(mean, mean))
    assert np.array_equal(res.coef_mean, sums["coef1"] / Z) and np.array_equal(res.coef_second, sums["coef2"] / Z)
    for d in range(2):
        assert np.array_equal(res.marginals[d], sums["marginals"][d] / Z)
