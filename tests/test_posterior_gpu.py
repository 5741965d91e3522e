"""pgd_grid_misfit and pgd_grid_posterior on the MI355X through the C-ABI, and PGD.sensor_posterior end to end: the f64-MFMA
kernels and the plain fma kernels against the longdouble restatement of tests/posterior_reference.py inside its derived bounds,
bit-identical across grid caps and runs, ties, zero weights, underflow, the limit of the coefficient moments and every refusal."""
import ctypes as C

import numpy as np
import pytest

from pgdrome_amd import _lib, fem, model
from pgdrome_amd.model import PGD
from tests import posterior_reference as R

pytestmark = pytest.mark.gpu

PD = C.POINTER(C.c_double)
POISON = -12345.678
ALL = _lib.POST_MARGINALS | _lib.POST_THETA | _lib.POST_COEF
U53 = 2.0 ** -53


class Knobs:
    """variant (1 MFMA, 0 plain) and grid cap of both calls."""

    def __init__(self, ctx, variant=1, grid_max=0):
        self.ctx, self.values = ctx, (variant, grid_max)

    def set(self, variant, grid_max):
        for knob, v in ((_lib.TUNE_MISFIT_VARIANT, variant), (_lib.TUNE_POST_VARIANT, variant),
                        (_lib.TUNE_MISFIT_GRID_MAX, grid_max), (_lib.TUNE_POST_GRID_MAX, grid_max)):
            self.ctx.tune(knob, v)

    def __enter__(self):
        self.set(*self.values)

    def __exit__(self, *exc):
        self.set(1, 0)


# k in {1, 5, 16, 17, 64} x m in {1, 15, 16, 17, 33} rotated over the grids: zero padding of both fragment directions, 16-sample tiles
# that straddle changes of the slow indices, a dimension of length 1, S a multiple of 16 and not, ndim 1, 2, 3 and 6, scattered
# samples (one dimension: the table is the coefficient matrix) of S = 1 and 1000; then the two large instances of the misfit kernel
# (k = 129, 256: no coefficient moments) and a grid of two segments (5863 samples) for the reductions; last the instance between them
# (65 .. 128 modes, two sample tiles per wave) at its smallest k, on two segments whose last sample tile is ragged (4160 samples)
GRIDS = [(3, 5, 7), (1, 33), (16, 16), (2, 2, 2, 3, 2, 2), (1,), (1000,)]
KS, MS = [1, 5, 16, 17, 64], [1, 15, 16, 17, 33]
CASES = [(g, k, MS[(i + j) % 5]) for i, g in enumerate(GRIDS) for j, k in enumerate(KS)]
CASES += [((3, 5, 7), 129, 17), ((16, 16), 256, 33), ((41, 11, 13), 17, 16), ((41, 11, 13), 48, 33), ((65, 64), 65, 17)]
IDS = ["n%s-k%d-m%d" % ("x".join(map(str, g)), k, m) for g, k, m in CASES]

_cache = {}


def case(grid, k, m):
    """Seeded inputs of a case with their restatement, computed once."""
    key = (grid, k, m)
    if key not in _cache:
        rng = np.random.default_rng(1000 * len(grid) + 10 * k + m + sum(grid))
        tables = [1.0 + 0.5 * rng.standard_normal((k, n)) for n in grid]
        a = rng.standard_normal((m, k)) / np.sqrt(k)
        node = rng.integers(0, int(np.prod(grid)))
        c = np.ones(k)
        for t, i in zip(tables, np.unravel_index(node, grid)):
            c = c * t[:, i]
        y = a @ c + 0.3 * rng.standard_normal(m)
        weights = [rng.uniform(0.2, 1.0, n) for n in grid]
        absc = [np.sort(rng.uniform(-1.0, 2.0, n)) for n in grid]
        chi2x, B2 = R.chi2_exact(a, y, tables)
        _cache[key] = dict(tables=tables, a=a, y=y, weights=weights, absc=absc, chi2x=chi2x, tau=R.chi2_bound(k, m, len(grid), B2),
                           S=int(np.prod(grid)))
    return _cache[key]


def run_misfit(ctx, cs):
    h = ctx.vec_alloc(cs["S"])
    try:
        ctx.vec_upload(h, np.full(cs["S"], POISON))
        mn, arg = ctx.grid_misfit(cs["a"], cs["y"], cs["tables"], h)
        return ctx.vec_download(h), mn, arg
    finally:
        ctx.vec_free(h)


def run_posterior(ctx, chi2, shift, cs, want, weights=None):
    h = ctx.vec_from(chi2)
    try:
        return ctx.grid_posterior(h, shift, [t.shape[1] for t in cs["tables"]], cs["weights"] if weights is None else weights,
                                  tables=cs["tables"], abscissae=cs["absc"], want=want)
    finally:
        ctx.vec_free(h)


def flat(out):
    """Every number of a grid_posterior result as one array (bit comparisons)."""
    parts = [np.array([out["Z"], out["sum_e2"]])]
    for key in ("marginals", "theta1", "theta2", "coef1", "coef2"):
        if key in out:
            parts += [np.asarray(p).reshape(-1) for p in (out[key] if key == "marginals" else [out[key]])]
    return np.concatenate(parts)


def check_sums(out, ex, bd, want):
    worst = {"Z": abs(out["Z"] - float(ex["Z"])) / bd["Z"], "sum_e2": abs(out["sum_e2"] - float(ex["sum_e2"])) / bd["sum_e2"]}
    keys = (["marginals"] if want & _lib.POST_MARGINALS else []) + (["theta1", "theta2"] if want & _lib.POST_THETA else []) + \
        (["coef1", "coef2"] if want & _lib.POST_COEF else [])
    for key in keys:
        got = np.concatenate(out[key]) if key == "marginals" else out[key]
        exact = np.concatenate(ex[key]) if key == "marginals" else ex[key]
        bound = np.concatenate(bd[key]) if key == "marginals" else bd[key]
        err = np.abs(got - exact).astype(np.float64)
        assert np.all((bound > 0.0) | (err == 0.0))
        worst[key] = float((err / np.where(bound > 0.0, bound, 1.0)).max())
    if want & _lib.POST_COEF:
        assert np.array_equal(out["coef2"], out["coef2"].T)
    if want & _lib.POST_THETA:
        assert np.array_equal(out["theta2"], out["theta2"].T)
    return worst


@pytest.mark.parametrize("grid,k,m", CASES, ids=IDS)
def test_misfit_and_posterior_against_the_restatement(ctx, grid, k, m):
    cs = case(grid, k, m)
    got = {}
    for name, variant in (("mfma", 1), ("plain", 0)):
        with Knobs(ctx, variant):
            chi2, mn, arg = run_misfit(ctx, cs)
        err = float((np.abs(chi2 - cs["chi2x"]) / cs["tau"]).max())
        print(name, "chi2: max error / bound", err)
        assert err <= 1.0
        assert mn == chi2.min() and arg == int(np.argmin(chi2))                   # (argmin: the first of equal values)
        got[name] = chi2
    assert np.all(np.abs(got["mfma"] - got["plain"]) <= 2 * cs["tau"])

    # the reductions from the device's own chi2 (tau = 0: the same numbers on both sides), shift = its minimum
    chi2 = got["mfma"]
    shift = float(chi2.min())
    want = ALL if k <= _lib.POST_COEF_KMAX else _lib.POST_MARGINALS | _lib.POST_THETA
    ex = R.posterior_exact(chi2, shift, cs["tables"] if want & _lib.POST_COEF else None, cs["weights"], cs["absc"])
    bd = R.posterior_bounds(ex, chi2, shift, 0.0, len(grid))
    outs = {}
    for name, variant in (("mfma", 1), ("plain", 0)):
        with Knobs(ctx, variant):
            outs[name] = run_posterior(ctx, chi2, shift, cs, want)
        worst = check_sums(outs[name], ex, bd, want)
        print(name, "sums: max error / bound", worst)
        assert all(v <= 1.0 for v in worst.values())
    # only the coefficient moments have two variants
    for key in ("Z", "sum_e2", "theta1", "theta2"):
        assert np.array_equal(outs["mfma"][key], outs["plain"][key])


@pytest.mark.parametrize("grid,k,m", [CASES[0], CASES[18], CASES[29], CASES[31], CASES[32], CASES[33], CASES[34]],
                         ids=[IDS[0], IDS[18], IDS[29], IDS[31], IDS[32], IDS[33], IDS[34]])
@pytest.mark.parametrize("variant", [1, 0], ids=["mfma", "plain"])
def test_bit_identical_for_any_grid_and_from_run_to_run(ctx, grid, k, m, variant):
    cs = case(grid, k, m)
    want = ALL if k <= _lib.POST_COEF_KMAX else _lib.POST_MARGINALS | _lib.POST_THETA
    runs = []
    for grid_max in (0, 1, 3, 0):
        with Knobs(ctx, variant, grid_max):
            chi2, mn, arg = run_misfit(ctx, cs)
            sums = run_posterior(ctx, chi2, mn, cs, want)
        runs.append((chi2, mn, arg, flat(sums)))
    for chi2, mn, arg, sums in runs[1:]:
        assert np.array_equal(chi2, runs[0][0]) and mn == runs[0][1] and arg == runs[0][2]
        assert np.array_equal(sums, runs[0][3])


def test_a_duplicated_abscissa_ties_and_the_lower_index_wins(ctx):
    rng = np.random.default_rng(77)
    k, m, grid = 17, 15, (5, 7)
    tables = [1.0 + 0.5 * rng.standard_normal((k, n)) for n in grid]
    tables[0][:, 3] = tables[0][:, 1]                     # abscissa 3 of the slow dimension repeats abscissa 1
    a = rng.standard_normal((m, k))
    y = a @ (tables[0][:, 1] * tables[1][:, 4])           # the data of node (1, 4) = node (3, 4)
    cs = dict(tables=tables, a=a, y=y, S=35)
    for variant in (1, 0):
        with Knobs(ctx, variant):
            chi2, mn, arg = run_misfit(ctx, cs)
        chi2 = chi2.reshape(grid)
        assert np.array_equal(chi2[1], chi2[3])
        assert arg == 1 * 7 + 4 and mn == chi2[1, 4] == chi2[3, 4] == chi2.min()


def test_weights_with_zeros(ctx):
    cs = case((3, 5, 7), 5, 15)
    weights = [w.copy() for w in cs["weights"]]
    weights[0][1] = 0.0
    weights[2][[0, 6]] = 0.0
    with Knobs(ctx):
        chi2, mn, _ = run_misfit(ctx, cs)
        out = run_posterior(ctx, chi2, mn, cs, ALL, weights=weights)
    ex = R.posterior_exact(chi2, mn, cs["tables"], weights, cs["absc"])
    worst = check_sums(out, ex, R.posterior_bounds(ex, chi2, mn, 0.0, 3), ALL)
    print("max error / bound", worst)
    assert all(v <= 1.0 for v in worst.values())
    assert out["marginals"][0][1] == 0.0 and out["marginals"][2][0] == 0.0 and out["marginals"][2][6] == 0.0 and out["Z"] > 0.0


def test_far_off_samples_underflow_and_z_stays_finite(ctx):
    cs = dict(case((16, 16), 16, 16))
    cs["y"] = 1e6 * cs["y"]                                # misfits of the order 1e12, their differences far beyond -2 log(tiny)
    with Knobs(ctx):
        chi2, mn, arg = run_misfit(ctx, cs)
        out = run_posterior(ctx, chi2, mn, cs, ALL)
    assert np.sort(chi2)[1] - mn > 1500.0
    i = np.unravel_index(arg, (16, 16))
    w = 1.0 * cs["weights"][0][i[0]] * cs["weights"][1][i[1]]
    assert np.isfinite(out["Z"]) and out["Z"] == w and out["sum_e2"] == w * w          # exp(0) = 1 at the minimum, 0 everywhere else
    assert out["marginals"][0][i[0]] == w and out["marginals"][0].sum() == w
    assert out["theta1"][0] == w * cs["absc"][0][i[0]]


def raw_posterior(ctx, h, shift, cs, want, k=None, n=None, ndim=None, tables=True, weights=True, absc=True, sums=True, outputs=True):
    """One call of the C entry point with poisoned outputs: (return code, the outputs)."""
    n = np.array([t.shape[1] for t in cs["tables"]] if n is None else n, dtype=np.int32)
    k = cs["tables"][0].shape[0] if k is None else k
    nd = len(n) if ndim is None else ndim
    cat = lambda xs: np.ascontiguousarray(np.concatenate([np.asarray(x, dtype=np.float64).reshape(-1) for x in xs]))
    t, w, x = cat(cs["tables"]), cat(cs["weights"]), cat(cs["absc"])
    kk = cs["tables"][0].shape[0]
    bufs = [np.full(2, POISON), np.full(w.size, POISON), np.full(8, POISON), np.full(64, POISON), np.full(max(k, kk), POISON),
            np.full(max(k, kk) ** 2, POISON)]
    p = lambda arr, on=True: arr.ctypes.data_as(PD) if on else None
    rc = ctx.lib.pgd_grid_posterior(ctx.h, h, shift, p(t, tables), n.ctypes.data_as(_lib.PI32), nd, k, p(w, weights), p(x, absc), want,
                                    p(bufs[0], sums), *[p(b, outputs) for b in bufs[1:]])
    return rc, bufs


def test_coefficient_moments_up_to_64_modes_and_refused_above(ctx):
    cs = case((3, 5, 7), 64, 33)
    with Knobs(ctx):
        chi2, mn, _ = run_misfit(ctx, cs)
        out = run_posterior(ctx, chi2, mn, cs, _lib.POST_COEF)
    assert out["coef2"].shape == (64, 64) and np.all(np.isfinite(out["coef2"]))
    rng = np.random.default_rng(65)
    big = dict(tables=[rng.standard_normal((65, 4))], weights=[np.ones(4)], absc=[np.arange(4.0)])
    h = ctx.vec_from(np.ones(4))
    try:
        rc, bufs = raw_posterior(ctx, h, 1.0, big, _lib.POST_COEF)
        assert rc == -1 and b"PGD_POST_COEF takes 1 .. 64" in ctx.lib.pgd_last_error(ctx.h)
        assert all(np.all(b == POISON) for b in bufs)
        rc, bufs = raw_posterior(ctx, h, 1.0, big, _lib.POST_MARGINALS | _lib.POST_THETA)          # without the bit k does not matter
        assert rc == 0 and bufs[0][0] == 4.0
    finally:
        ctx.vec_free(h)


def test_invalid_arguments_leave_the_outputs_untouched(ctx):
    cs = case((3, 5, 7), 5, 15)
    S = 105
    p = lambda arr: arr.ctypes.data_as(PD)
    n = np.array([3, 5, 7], dtype=np.int32)
    t = np.ascontiguousarray(np.concatenate([x.reshape(-1) for x in cs["tables"]]))
    a, y = np.ascontiguousarray(cs["a"]), np.ascontiguousarray(cs["y"])
    good, short = ctx.vec_from(np.full(S, POISON)), ctx.vec_from(np.full(S - 1, POISON))
    try:
        def misfit(a_=a, y_=y, m=15, k=5, t_=t, n_=n, ndim=3, h=good):
            mn, arg = C.c_double(POISON), C.c_int64(-77)
            rc = ctx.lib.pgd_grid_misfit(ctx.h, None if a_ is None else p(a_), None if y_ is None else p(y_), m, k,
                                         None if t_ is None else p(t_), None if n_ is None else n_.ctypes.data_as(_lib.PI32), ndim, h,
                                         C.byref(mn), C.byref(arg))
            assert mn.value == POISON and arg.value == -77 and np.all(ctx.vec_download(good) == POISON)
            return rc
        huge = np.array([1 << 11, 1 << 10, 1 << 10], dtype=np.int32)                    # S = 2^31
        for kw in (dict(a_=None), dict(y_=None), dict(t_=None), dict(n_=None), dict(m=0), dict(m=257), dict(k=0), dict(k=257), dict(ndim=0),
                   dict(ndim=7), dict(n_=np.array([3, 0, 7], dtype=np.int32)), dict(n_=huge), dict(h=short), dict(h=0), dict(h=123456)):
            assert misfit(**kw) == -1, kw
        ctx.vec_upload(good, np.ones(S))
        post = lambda **kw: raw_posterior(ctx, kw.pop("h", good), kw.pop("shift", 1.0), cs, kw.pop("want", ALL), **kw)
        for kw in (dict(want=8), dict(want=-1), dict(shift=float("nan")), dict(shift=float("inf")), dict(ndim=0), dict(ndim=7),
                   dict(n=[3, 0, 7]), dict(n=[1 << 11, 1 << 10, 1 << 10]), dict(h=short), dict(h=0), dict(weights=False), dict(sums=False),
                   dict(tables=False), dict(absc=False), dict(outputs=False), dict(k=0), dict(k=65), dict(n=[3, 5, 6])):
            rc, bufs = post(**kw)
            assert rc == -1, kw
            assert all(np.all(b == POISON) for b in bufs), kw
        rc, bufs = post(want=0, tables=False, absc=False, outputs=False)                # Z alone needs neither
        assert rc == 0 and bufs[0][0] > 0.0
    finally:
        ctx.vec_free(good)
        ctx.vec_free(short)


# ---------------------------------------------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def hip():
    from pgdrome_amd.hip_backend import HipBackend
    old = fem._backend
    fem.set_backend(HipBackend(0))
    fem.clear_caches()
    yield
    fem.set_backend(old)
    fem.clear_caches()


def test_sensor_posterior_on_the_device_and_in_numpy(hip, monkeypatch):
    """A 41^3 P1 box (>= DEVICE_EVAL_MIN_DOFS) with 12 synthetic modes, parameter dimensions of 33 and 17 nodes, 20 sensor points
    with gradient=True (60 rows, reduced to 12 by the QR): the device route and the numpy route around the restatement."""
    rng = np.random.default_rng(41)
    V = fem.FunctionSpace(fem.BoxMesh(fem.Point(0, 0, 0), fem.Point(1, 1, 1), 40, 40, 40), "CG", 1)
    assert V.dim() == 68921 >= model.DEVICE_EVAL_MIN_DOFS
    Vps = [fem.FunctionSpace(fem.IntervalMesh(32, 0.0, 1.0), "CG", 1), fem.FunctionSpace(fem.IntervalMesh(16, -1.0, 1.0), "CG", 1)]
    K, modes = 12, []
    for i, W in enumerate([V] + Vps):
        F = rng.standard_normal((W.dim(), K)) * (1.0 if i == 0 else 0.5) + (0.0 if i == 0 else 1.0)
        fs = []
        for k in range(K):
            f = fem.Function(W)
            f.vector()._host = np.ascontiguousarray(F[:, k])
            f.vector().touched_host()
            fs.append(f)
        modes.append(fs)
    sol = PGD(name="synthetic", n_modes=K, fmeshes=[W.mesh() for W in [V] + Vps], pgd_modes=modes, name_coord=["x", "p", "q"],
              modes_info=["U", "Node", "Scalar"])
    pts = rng.uniform(0.05, 0.95, (20, 3))
    grids = [Vps[0].mesh().coordinates()[:, 0].copy(), Vps[1].mesh().coordinates()[:, 0].copy()]
    grids = [np.sort(g) for g in grids]
    truth = sol.evaluate_sensor_response_many(0, [1, 2], np.array([[grids[0][20], grids[1][5]]]), 0, pts, gradient=True).values[0]
    sigma = 3.0 * np.abs(truth).max()                    # (wide: the seeded modes jump from node to node, many nodes keep mass)
    data = truth + sigma * rng.standard_normal(truth.shape)
    kw = dict(grids=grids, sigma=sigma, gradient=True, keep_chi2=True, prior={2: lambda x: 1.0 + 0.5 * x * x})

    monkeypatch.setattr(model, "DEVICE_POSTERIOR_MIN_SAMPLES", 1)
    calls = fem.STATS.get("posterior_calls", 0)
    dev = sol.sensor_posterior(0, [1, 2], 0, pts, data, **kw)
    assert dev.path == "device" and fem.STATS.get("posterior_calls", 0) == calls + 1
    monkeypatch.setattr(model, "DEVICE_POSTERIOR_MIN_SAMPLES", 1 << 40)
    ref = sol.sensor_posterior(0, [1, 2], 0, pts, data, **kw)
    assert ref.path == "numpy" and fem.STATS.get("posterior_calls", 0) == calls + 1

    # the restatement from what both routes were given: the whitened sensor modes, reduced by the same host QR
    phi = sol.sensor_modes(pts, 0, 0, gradient=True).host()[:K].T / sigma
    Q, Rm = np.linalg.qr(phi)
    z = Q.T @ (data.reshape(-1) / sigma)
    rest = data.reshape(-1) / sigma - Q @ z
    tables = [np.ascontiguousarray(sol._free_modes_at(d, g, 0)) for d, g in zip((1, 2), grids)]
    chi2x, B2 = R.chi2_exact(Rm, z, tables)
    chi2x = chi2x + np.longdouble(rest @ rest)
    # ... the remainder |rest|^2 is a dot of 60 terms in double on both sides, and its addition rounds once
    tau = R.chi2_bound(K, K, 2, B2) + (2 * (60 + 2) + 1) * U53 * float(rest @ rest) + U53 * chi2x.astype(np.float64)
    shape = (33, 17)
    for name, res in (("device", dev), ("numpy", ref)):
        got = np.asarray(res.chi2.host() if name == "device" else res.chi2).reshape(-1)
        err = float((np.abs(got - chi2x) / tau).max())
        print(name, "chi2: max error / bound", err)
        assert err <= 1.0
        assert res.map_index == tuple(int(i) for i in np.unravel_index(int(np.argmin(got)), shape))
        assert res.chi2_min == got.min()
        # the reductions of this route from its own chi2 (shift = its minimum before the QR's remainder is added)
        own = got - float(rest @ rest)
        ex = R.posterior_exact(own, res.shift, tables, res.weights, res.grids)
        bd = R.posterior_bounds(ex, own, res.shift, 2 * U53 * np.abs(got), 2)
        Z, dZ = float(ex["Z"]), bd["Z"]

        def ratio(got, num, dN):
            """max error / bound of a quotient num / Z (a sum within dN, Z within dZ; two roundings of the quotient itself)"""
            q = (num / ex["Z"]).astype(np.float64)
            bound = (np.asarray(dN) + np.abs(q) * dZ) / (Z - dZ) + 2 * U53 * np.abs(q)
            err = np.abs(got - q)
            assert np.all((bound > 0.0) | (err == 0.0))
            return float((err / np.where(bound > 0.0, bound, 1.0)).max())

        worst = {"Z": abs(res.Z - Z) / dZ}
        for d in range(2):
            worst["marginal %d" % d] = ratio(res.marginals[d], ex["marginals"][d], bd["marginals"][d])
            assert np.count_nonzero(res.marginals[d] > 1e-6) >= 5                 # the posterior is spread over many nodes
        worst["mean"] = ratio(res.mean, ex["theta1"], bd["theta1"])
        worst["coef_mean"] = ratio(res.coef_mean, ex["coef1"], bd["coef1"])
        worst["coef_second"] = ratio(res.coef_second, ex["coef2"], bd["coef2"])
        print(name, "max error / bound", worst, "ess", res.ess)
        assert all(v <= 1.0 for v in worst.values())
    assert dev.map_index == ref.map_index
    assert abs(dev.log_evidence - ref.log_evidence) <= 1e-10 * abs(ref.log_evidence)

    # the predictive fields run through pgd_quad_forms (and the mean through pgd_eval_batch)
    quads = fem.STATS.get("quad_forms_calls", 0)
    mean, variance = sol.posterior_predictive(dev, 0, 0)
    assert fem.STATS.get("quad_forms_calls", 0) == quads + 1
    F = np.stack([f.vector().host() for f in modes[0]], axis=1)
    mbar, M = dev.coef_mean, dev.coef_second
    Qm = M - np.outer(mbar, mbar)
    vref = np.maximum(np.einsum("ik,kl,il->i", F.astype(np.longdouble), Qm.astype(np.longdouble), F.astype(np.longdouble)), 0).astype(np.float64)
    from tests import uq_reference as UQ
    vtol = UQ.bound(K, UQ.scale(F, Qm[None]))[0]
    mtol = (K + 2) * U53 * (np.abs(F) @ np.abs(mbar))
    assert np.all(np.abs(variance.vector().host() - vref) <= vtol) and variance.vector().host().min() >= 0.0
    assert np.all(np.abs(mean.vector().host() - F @ mbar) <= 2 * mtol)
