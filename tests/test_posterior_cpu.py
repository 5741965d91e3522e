"""PGD.sensor_posterior / posterior_predictive on the numpy route (oracle backend, no GPU) against the longdouble restatement and
the derived bounds of tests/posterior_reference.py, an analytic Gaussian case and the fields of evaluate_many.  Every input is seeded.

A quotient q = N / Z of two sums within dN and dZ of their exact values is within (dN + |q| dZ) / (Z - dZ) + 2 u |q| of the exact
quotient (``ratio_bound``)."""
import math

import numpy as np
import pytest

from oracle.backend_numpy import NumpyBackend
from pgdrome_amd import fem, model
from pgdrome_amd.model import PGD
from tests import posterior_reference as R

U53 = 2.0 ** -53


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


def interval_space(cells, a, b, degree=1):
    return fem.FunctionSpace(fem.IntervalMesh(cells, a, b), "CG", degree)


def ratio_bound(q, dN, dZ, Z):
    return (np.asarray(dN) + np.abs(q) * dZ) / (Z - dZ) + 2 * U53 * np.abs(q)


PTS = [[0.15, 0.2], [0.5, 0.5], [0.93, 0.11], [0.3, 0.8], [0.71, 0.64], [0.05, 0.95], [0.62, 0.33]]


@pytest.fixture(scope="module")
def two_parameters(oracle):
    """Five seeded modes on a rectangle (fixed), a P1 and a P2 interval; seven sensors; grids of 9 and 6 abscissae."""
    rng = np.random.default_rng(7)
    V = fem.FunctionSpace(fem.RectangleMesh(fem.Point(0, 0), fem.Point(1, 1), 5, 4), "CG", 1)
    Vp, Vq = interval_space(6, 0.0, 2.0, 1), interval_space(4, -1.0, 1.0, 2)
    K = 5
    mats = [rng.standard_normal((V.dim(), K)), 1.0 + 0.4 * rng.standard_normal((Vp.dim(), K)), 1.0 + 0.4 * rng.standard_normal((Vq.dim(), K))]
    sol = make([V, Vp, Vq], mats)
    grids = [np.sort(rng.uniform(0.0, 2.0, 9)), np.linspace(-1.0, 1.0, 6)]
    tables = [np.ascontiguousarray(sol._free_modes_at(d, g, 0)) for d, g in zip((1, 2), grids)]
    phi = sol.sensor_modes(PTS, 0, 0).host()[:K].T
    node = (4, 2)
    truth = phi @ (tables[0][:, node[0]] * tables[1][:, node[1]])
    return sol, grids, tables, phi, node, truth, rng


def check_against_restatement(res, a, y, tables, rest_bound=0.0, logdet=0.0, m=None):
    """Every field of a grids-mode result against the restatement from the whitened (a, y) that the route used."""
    k, nd = a.shape[1], len(tables)
    shape = R.shape_of(tables)
    chi2x, B2 = R.chi2_exact(a, y, tables)
    tau = R.chi2_bound(k, a.shape[0], nd, B2) + rest_bound
    got = np.asarray(res.chi2).reshape(-1)
    worst = {"chi2": float((np.abs(got - chi2x) / tau).max())}
    arg = int(np.ravel_multi_index(res.map_index, shape))
    assert got[arg] == got.min() and arg == int(np.argmin(got)) and res.chi2_min == got[arg]
    shift = float(got.min())
    ex = R.posterior_exact(chi2x, shift, tables, res.weights, res.grids)
    bd = R.posterior_bounds(ex, chi2x.astype(np.float64), shift, tau, nd)
    Z, dZ = float(ex["Z"]), bd["Z"]
    for d in range(nd):
        q = (ex["marginals"][d] / ex["Z"]).astype(np.float64)
        worst["marginal %d" % d] = float((np.abs(res.marginals[d] - q) / ratio_bound(q, bd["marginals"][d], dZ, Z)).max())
        assert abs(res.marginals[d].sum() - 1.0) <= 4 * dZ / Z + shape[d] * U53
    mean = (ex["theta1"] / ex["Z"]).astype(np.float64)
    dmean = ratio_bound(mean, bd["theta1"], dZ, Z)
    worst["mean"] = float((np.abs(res.mean - mean) / dmean).max())
    second = (ex["theta2"] / ex["Z"]).astype(np.float64)
    cov = (ex["theta2"] / ex["Z"] - np.outer(ex["theta1"], ex["theta1"]) / ex["Z"] ** 2).astype(np.float64)
    dcov = ratio_bound(second, bd["theta2"], dZ, Z) + np.outer(np.abs(mean) + dmean, dmean) + np.outer(dmean, np.abs(mean)) + \
        4 * U53 * (np.abs(second) + np.abs(np.outer(mean, mean)))
    worst["cov"] = float((np.abs(res.cov - cov) / dcov).max())
    c1, c2 = (ex["coef1"] / ex["Z"]).astype(np.float64), (ex["coef2"] / ex["Z"]).astype(np.float64)
    worst["coef_mean"] = float((np.abs(res.coef_mean - c1) / ratio_bound(c1, bd["coef1"], dZ, Z)).max())
    worst["coef_second"] = float((np.abs(res.coef_second - c2) / ratio_bound(c2, bd["coef2"], dZ, Z)).max())
    assert np.array_equal(res.coef_second, res.coef_second.T)
    ess = float(ex["Z"] ** 2 / ex["sum_e2"])
    worst["ess"] = abs(res.ess - ess) / (ess * (2 * dZ / Z + bd["sum_e2"] / float(ex["sum_e2"]) + 4 * U53))
    m = a.shape[0] if m is None else m
    logev = float(np.log(ex["Z"]) - np.longdouble(shift) / 2) - 0.5 * m * math.log(2 * math.pi) - logdet
    dlog = dZ / (Z - dZ) + 8 * U53 * (abs(math.log(Z)) + shift / 2 + 0.5 * m * math.log(2 * math.pi) + abs(logdet))
    worst["log_evidence"] = abs(res.log_evidence - logev) / dlog
    print("max error / bound:", worst)
    assert all(v <= 1.0 for v in worst.values())
    return chi2x, tau


def test_numpy_route_equals_the_restatement(two_parameters):
    sol, grids, tables, phi, node, truth, rng = two_parameters
    sigma = rng.uniform(0.05, 0.2, len(PTS))
    data = truth + sigma * rng.standard_normal(len(PTS))
    prior = {1: lambda x: math.exp(-0.5 * (x - 1.0) ** 2), 2: np.linspace(1.0, 2.0, 6)}
    res = sol.sensor_posterior(0, [1, 2], 0, PTS, data, grids=grids, sigma=sigma, prior=prior, keep_chi2=True, reduce=False)
    assert res.path == "numpy" and res.chi2.shape == (9, 6)
    for w in res.weights:
        assert abs(w.sum() - 1.0) <= 4 * U53 * w.size
    check_against_restatement(res, phi / sigma[:, None], data / sigma, tables, logdet=float(np.sum(np.log(sigma))))
    # the densities are the masses over the quadrature weights: their trapezoid integral is 1
    for d, g in enumerate(grids):
        q = model.trapezoid_weights(g)
        assert abs((res.densities[d] * q).sum() - 1.0) <= 1e-12


def test_full_covariance_whitens_by_cholesky(two_parameters):
    sol, grids, tables, phi, node, truth, rng = two_parameters
    m = len(PTS)
    G = rng.standard_normal((m, m))
    cov = 0.01 * (G @ G.T + m * np.eye(m))
    data = truth + 0.05 * rng.standard_normal(m)
    res = sol.sensor_posterior(0, [1, 2], 0, PTS, data, grids=grids, cov=cov, keep_chi2=True, reduce=False)
    L = np.linalg.cholesky(cov)
    a, y = np.linalg.solve(L, phi), np.linalg.solve(L, data)
    # the route whitens with a triangular solve, this test with a general one: both are backward stable, the whitened data agree to
    # cond(L) u, which enters chi2 like the QR's perturbation of (a, y)
    extra = np.linalg.cond(L) * R.qr_term(a, y, tables) / (24.0 * m * a.shape[1]) * 8
    check_against_restatement(res, a, y, tables, rest_bound=extra, logdet=float(np.sum(np.log(np.diag(L)))))


def test_qr_reduction_agrees_with_the_full_rows(two_parameters):
    sol, grids, tables, phi, node, truth, rng = two_parameters
    data = truth + 0.1 * rng.standard_normal(len(PTS))
    kw = dict(grids=grids, sigma=0.1, keep_chi2=True)
    full = sol.sensor_posterior(0, [1, 2], 0, PTS, data, reduce=False, **kw)
    red = sol.sensor_posterior(0, [1, 2], 0, PTS, data, **kw)
    a, y = phi / 0.1, data / 0.1
    chi2x, B2 = R.chi2_exact(a, y, tables)
    m, k = a.shape
    assert m > k
    tau_full = R.chi2_bound(k, m, 2, B2)
    # the reduced rows: k of them, |R c| + |z| <= the column norms of a times |c| + |y|, the scale of qr_term; the remainder adds m roundings
    qr = R.qr_term(a, y, tables)
    tau_red = R.chi2_bound(k, k, 2, qr / (24.0 * m * k * U53)) + qr + (m + 2) * U53 * float(y @ y)
    e_full = np.abs(full.chi2.reshape(-1) - chi2x) / tau_full
    e_red = np.abs(red.chi2.reshape(-1) - chi2x) / tau_red
    print("full rows: max error / bound", float(e_full.max()), " reduced:", float(e_red.max()))
    assert e_full.max() <= 1.0 and e_red.max() <= 1.0
    assert np.all(np.abs(full.chi2 - red.chi2).reshape(-1) <= tau_full + tau_red)
    assert red.map_index == full.map_index
    assert abs(red.log_evidence - full.log_evidence) <= 1e-9 * abs(full.log_evidence)


def test_grid_and_the_same_points_as_coords(two_parameters):
    sol, grids, tables, phi, node, truth, rng = two_parameters
    data = truth + 0.1 * rng.standard_normal(len(PTS))
    g = sol.sensor_posterior(0, [1, 2], 0, PTS, data, grids=grids, sigma=0.1, quadrature="none", keep_chi2=True, reduce=False)
    P, Q = np.meshgrid(grids[0], grids[1], indexing="ij")
    coords = np.stack([P.reshape(-1), Q.reshape(-1)], axis=1)
    c = sol.sensor_posterior(0, [1, 2], 0, PTS, data, coords=coords, sigma=0.1, keep_chi2=True, reduce=False)
    a, y = phi / 0.1, data / 0.1
    chi2x, B2 = R.chi2_exact(a, y, tables)
    tau = R.chi2_bound(a.shape[1], a.shape[0], 2, B2)
    assert np.all(np.abs(g.chi2.reshape(-1) - chi2x) <= tau) and np.all(np.abs(c.chi2 - chi2x) <= tau)
    assert np.all(np.abs(g.chi2.reshape(-1) - c.chi2) <= 2 * tau)
    assert c.map_index == int(np.ravel_multi_index(g.map_index, (9, 6))) and np.array_equal(c.map_coords, g.map_coords)
    assert c.marginals is None and c.densities is None
    # unit weights over S on both sides: the same posterior
    assert abs(c.log_evidence - g.log_evidence) <= 1e-10 * abs(g.log_evidence)
    assert np.allclose(c.mean, g.mean, rtol=1e-10, atol=0) and np.allclose(c.cov, g.cov, rtol=1e-8, atol=1e-14)
    assert np.allclose(c.coef_second, g.coef_second, rtol=1e-10, atol=1e-14)


def test_log_evidence_does_not_depend_on_the_shift(two_parameters):
    sol, grids, tables, phi, node, truth, rng = two_parameters
    a, y = phi / 0.1, (truth + 0.1 * rng.standard_normal(len(PTS))) / 0.1
    chi2, cmin, arg = model.grid_misfit_numpy(a, y, tables)
    w = [np.full(9, 1 / 9.0), np.full(6, 1 / 6.0)]
    logs = []
    for shift in (cmin, cmin + 3.0, cmin - 7.5, 0.0):
        sums = model.grid_posterior_numpy(chi2, shift, [9, 6], w)
        ex = R.posterior_exact(chi2, shift, tables, w)
        bd = R.posterior_bounds(ex, chi2, shift, 0.0, 2)
        assert abs(sums["Z"] - float(ex["Z"])) <= bd["Z"]
        logs.append((math.log(sums["Z"]) - 0.5 * shift, bd["Z"] / float(ex["Z"]) + 4 * U53 * (abs(math.log(sums["Z"])) + abs(shift))))
    for v, t in logs[1:]:
        assert abs(v - logs[0][0]) <= t + logs[0][1]


def test_noise_free_data_of_a_node_are_found_there(two_parameters):
    sol, grids, tables, phi, node, truth, rng = two_parameters
    res = sol.sensor_posterior(0, [1, 2], 0, PTS, truth, grids=grids, sigma=0.01, keep_chi2=True, reduce=False)
    a, y = phi / 0.01, truth / 0.01
    chi2x, B2 = R.chi2_exact(a, y, tables)
    tau = R.chi2_bound(a.shape[1], a.shape[0], 2, B2)
    arg = int(np.ravel_multi_index(node, (9, 6)))
    print("chi2_min", res.chi2_min, "bound at the node", tau[arg], "second smallest", np.sort(res.chi2.reshape(-1))[1])
    assert res.map_index == node and np.array_equal(res.map_coords, [grids[0][node[0]], grids[1][node[1]]])
    assert 0.0 <= res.chi2_min <= tau[arg] + float(chi2x[arg])
    # ... and through the QR reduction as well
    red = sol.sensor_posterior(0, [1, 2], 0, PTS, truth, grids=grids, sigma=0.01)
    assert red.map_index == node and 0.0 <= red.chi2_min <= tau[arg] + R.qr_term(a, y, tables)[arg] + (len(PTS) + 2) * U53 * float(y @ y)


def test_linear_gaussian_model_has_the_analytic_posterior(oracle):
    """u = phi theta (K = 1, the P1 mode F(theta) = theta), Gaussian noise and a Gaussian prior: precision 1 / s0^2 + |phi|^2 / sigma^2,
    mean (mu0 / s0^2 + phi . y / sigma^2) / precision.  Tolerance: twice the distance of the longdouble restatement on the same grid
    from the analytic value (the discretisation error, from the reference); the error falls when the step is halved."""
    rng = np.random.default_rng(11)
    V = interval_space(8, 0.0, 1.0)
    Vt = interval_space(10, -4.0, 6.0)
    fx = rng.uniform(0.5, 1.5, V.dim())
    sol = make([V, Vt], [fx.reshape(-1, 1), Vt._lay.coords[:, 0].reshape(-1, 1).copy()])
    pts = [[0.1], [0.37], [0.52], [0.9]]
    phi = sol.sensor_modes(pts, 0, 0).host()[:1].T
    sigma, mu0, s0 = 0.8, 0.5, 1.5
    y = phi[:, 0] * 1.3 + sigma * rng.standard_normal(4)
    prec = 1 / s0 ** 2 + float(phi[:, 0] @ phi[:, 0]) / sigma ** 2
    mean, var = (mu0 / s0 ** 2 + float(phi[:, 0] @ y) / sigma ** 2) / prec, 1 / prec
    sp = math.sqrt(var)
    prior = lambda t: math.exp(-0.5 * ((t - mu0) / s0) ** 2)
    errs = []
    for step in (2.0 * sp, sp):
        grid = np.arange(-4.0 + 0.3 * sp, 6.0, step)
        res = sol.sensor_posterior(0, [1], 0, pts, y, grids=[grid], sigma=sigma, prior={1: prior})
        table = [np.ascontiguousarray(sol._free_modes_at(1, grid, 0))]
        a, yw = phi / sigma, y / sigma
        chi2x, _ = R.chi2_exact(a, yw, table)
        ex = R.posterior_exact(chi2x, float(chi2x.min()), table, res.weights, [grid])
        mref = float(ex["theta1"][0] / ex["Z"])
        vref = float(ex["theta2"][0, 0] / ex["Z"] - (ex["theta1"][0] / ex["Z"]) ** 2)
        dm, dv = abs(mref - mean), abs(vref - var)
        em, ev = abs(res.mean[0] - mean), abs(res.cov[0, 0] - var)
        print("step %.3f: mean error %.3e (restatement %.3e), variance error %.3e (restatement %.3e)" % (step, em, dm, ev, dv))
        assert em <= 2 * dm and ev <= 2 * dv
        errs.append((em, ev))
    assert errs[1][0] < errs[0][0] and errs[1][1] < errs[0][1]


def test_posterior_predictive_against_the_fields_of_evaluate_many(two_parameters):
    sol, _, _, phi, _, _, rng = two_parameters
    grids = [np.linspace(0.2, 1.8, 5), np.linspace(-0.8, 0.9, 4)]
    tables = [np.ascontiguousarray(sol._free_modes_at(d, g, 0)) for d, g in zip((1, 2), grids)]
    data = phi @ (tables[0][:, 2] * tables[1][:, 1]) + 0.3 * rng.standard_normal(len(PTS))
    res = sol.sensor_posterior(0, [1, 2], 0, PTS, data, grids=grids, sigma=0.3, keep_chi2=True)
    mean, variance = sol.posterior_predictive(res, 0, 0)
    P, Q = np.meshgrid(grids[0], grids[1], indexing="ij")
    coords = np.stack([P.reshape(-1), Q.reshape(-1)], axis=1)
    many = sol.evaluate_many(0, [1, 2], coords, 0, stats=False, fields=True)
    U = np.stack([f.vector().host() for f in many.fields], axis=1)                   # (n, 20)
    w = np.outer(res.weights[0], res.weights[1]).reshape(-1)
    p = w * np.exp(-0.5 * (res.chi2.reshape(-1) - res.chi2_min))
    p = p / p.sum()
    mref = U @ p
    vref = ((U - mref[:, None]) ** 2) @ p
    # scale: sum_s p_s (sum_k |f_k| |c_k(s)|)^2; every term of the K^2 products passes at most 2 K + S + 20 roundings on either side,
    # and the variance is the difference of two such sums
    F = np.abs(np.stack([m.vector().host() for m in sol.mesh[0].attributes[0].interpolationfct], axis=1))
    A = F @ np.abs(many.coefficients)
    K, S = F.shape[1], 20
    tol_m = (K + S + 5) * U53 * (A @ p)
    tol_v = 2 * (2 * K + S + 20) * U53 * ((A * A) @ p)
    em = float((np.abs(mean.vector().host() - mref) / tol_m).max())
    ev = float((np.abs(variance.vector().host() - vref) / tol_v).max())
    print("predictive mean: max error / bound", em, " variance:", ev)
    assert em <= 1.0 and ev <= 1.0 and variance.vector().host().min() >= 0.0
    with pytest.raises(ValueError, match="coef"):
        sol.posterior_predictive(sol.sensor_posterior(0, [1, 2], 0, PTS, data, grids=grids, outputs=("theta",)), 0, 0)


def test_refusals(two_parameters):
    sol, grids, tables, phi, node, truth, rng = two_parameters
    call = lambda **kw: sol.sensor_posterior(0, [1, 2], 0, PTS, kw.pop("data", truth), **kw)
    with pytest.raises(ValueError, match="exactly one"):
        call()
    with pytest.raises(ValueError, match="exactly one"):
        call(grids=grids, coords=np.ones((3, 2)))
    with pytest.raises(ValueError, match="unknown outputs"):
        call(grids=grids, outputs=("marginals", "median"))
    with pytest.raises(ValueError, match="quadrature"):
        call(grids=grids, quadrature="simpson")
    with pytest.raises(ValueError, match="grids for"):
        call(grids=grids[:1])
    with pytest.raises(ValueError, match="non-decreasing"):
        call(grids=[grids[0][::-1], grids[1]])
    with pytest.raises(ValueError, match="data has shape"):
        call(grids=grids, data=truth[:-1])
    with pytest.raises(ValueError, match="not finite"):
        call(grids=grids, data=np.where(np.arange(len(PTS)) == 2, np.nan, truth))
    with pytest.raises(ValueError, match="sigma"):
        call(grids=grids, sigma=0.0)
    with pytest.raises(ValueError, match="sigma"):
        call(grids=grids, sigma=np.ones(3))
    with pytest.raises(ValueError, match="cov has shape"):
        call(grids=grids, cov=np.eye(3))
    with pytest.raises(ValueError, match="positive definite"):
        call(grids=grids, cov=-np.eye(len(PTS)))
    with pytest.raises(ValueError, match="prior names"):
        call(grids=grids, prior={0: lambda x: 1.0})
    with pytest.raises(ValueError, match="prior of dimension"):
        call(grids=grids, prior={1: -np.ones(9)})
    with pytest.raises(ValueError, match="no prior"):
        call(coords=np.ones((3, 2)), prior={1: lambda x: 1.0})
    with pytest.raises(ValueError, match="free_dim"):
        sol.sensor_posterior(0, [0, 1], 0, PTS, truth, grids=grids)
    with pytest.raises(NotImplementedError, match="grid_misfit"):
        call(grids=grids, device=True)                                            # the numpy backend has no device route
    with pytest.raises(ValueError, match="outside the mesh"):
        call(grids=[np.linspace(0.0, 2.5, 4), grids[1]])

    # interp1d modes have no mesh to locate points on
    att = sol.mesh[1].attributes[0]
    info = att.interpolationInfo
    att.interpolationInfo = dict(info, name=0)
    try:
        with pytest.raises(ValueError, match="interp1d"):
            call(grids=grids)
    finally:
        att.interpolationInfo = info

    # a row-sharded fixed dimension, as sensor_modes refuses it
    mesh = sol.mesh[0].attributes[0].interpolationfct[0].function_space().mesh()
    mesh.part = object()
    try:
        with pytest.raises(NotImplementedError, match="row-sharded"):
            call(grids=grids)
    finally:
        mesh.part = None


def test_refusals_of_shapes(oracle):
    rng = np.random.default_rng(5)
    V = interval_space(300, 0.0, 1.0)
    pts = np.linspace(0.001, 0.999, 257).reshape(-1, 1)
    # a free dimension that is no interval, and a vector-valued one, in grids mode
    Vr = fem.FunctionSpace(fem.RectangleMesh(fem.Point(0, 0), fem.Point(1, 1), 2, 2), "CG", 1)
    sol = make([V, Vr], [rng.standard_normal((V.dim(), 2)), rng.standard_normal((Vr.dim(), 2))])
    with pytest.raises(NotImplementedError, match="1-D free dimensions"):
        sol.sensor_posterior(0, [1], 0, pts[:3], np.zeros(3), grids=[np.linspace(0, 1, 3)])
    Vv = fem.VectorFunctionSpace(fem.IntervalMesh(4, 0.0, 1.0), "CG", 1, dim=2)
    solv = make([V, Vv], [rng.standard_normal((V.dim(), 2)), rng.standard_normal((Vv.dim(), 2))])
    with pytest.raises(NotImplementedError, match="scalar modes"):
        solv.sensor_posterior(0, [1], 0, pts[:3], np.zeros(3), grids=[np.linspace(0, 1, 3)])
    # more than 256 rows without the reduction, and more than 256 modes: both name compress
    Vt = interval_space(4, 0.0, 1.0)
    sol = make([V, Vt], [rng.standard_normal((V.dim(), 3)), rng.standard_normal((Vt.dim(), 3))])
    grid = [np.linspace(0.0, 1.0, 5)]
    with pytest.raises(ValueError, match="compress"):
        sol.sensor_posterior(0, [1], 0, pts, np.zeros(257), grids=grid, reduce=False)
    assert sol.sensor_posterior(0, [1], 0, pts, np.zeros(257), grids=grid).path == "numpy"          # reduced to 3 rows
    big = make([V, Vt], [rng.standard_normal((V.dim(), 257)), rng.standard_normal((Vt.dim(), 257))])
    with pytest.raises(ValueError, match="compress"):
        big.sensor_posterior(0, [1], 0, pts, np.zeros(257), grids=grid)
