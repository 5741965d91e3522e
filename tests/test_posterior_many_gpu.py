"""pgd_grid_posterior_many on the MI355X through the C-ABI, and PGD.sensor_posterior_many end to end: the chained f64-MFMA kernel
and the plain fma kernel against the longdouble restatement of tests/posterior_many_reference.py inside its derived bounds; every
output bit-identical from run to run, for any grid, with and without the skip of underflowed tiles and wherever a data set sits;
ties, zero weights, underflow, data at a node and every refusal."""
import ctypes as C
import math

import numpy as np
import pytest

from pgdrome_amd import _lib, fem, model
from tests import posterior_many_reference as RM

pytestmark = pytest.mark.gpu

PD = C.POINTER(C.c_double)
POISON = -12345.678
THETA = _lib.POST_THETA


class Knobs:
    """variant (1 MFMA, 0 plain), grid cap and skip of the call."""

    def __init__(self, ctx, variant=1, grid_max=0, skip=1):
        self.ctx, self.values = ctx, (variant, grid_max, skip)

    def set(self, variant, grid_max, skip):
        for knob, v in ((_lib.TUNE_POSTMANY_VARIANT, variant), (_lib.TUNE_POSTMANY_GRID_MAX, grid_max), (_lib.TUNE_POSTMANY_SKIP, skip)):
            self.ctx.tune(knob, v)

    def __enter__(self):
        self.set(*self.values)

    def __exit__(self, *exc):
        self.set(1, 0, 1)


def block(ctx, ndim):
    """The data sets a wave holds: read from the library."""
    return ctx.postmany_data_block(ndim)


# (grid, k, m, nd, accumulate); nd = None: one more than the wave's data block of that ndim.  Zero padding of the mode and row fragments
# (k, m no multiples of 4 / 16), of the data tiles (nd = 1, 15, 17, 33) and blocks, 16-sample tiles that end inside a segment, a
# dimension of length 1, one and two feature tiles (ndim 1, 3, 6) and three segments (9207 samples)
CASES = [((5,), 1, 1, 1, False), ((16,), 4, 16, 15, False), ((17,), 5, 17, 16, True), ((5, 7, 3), 17, 64, 17, False),
         ((1, 9, 1), 48, 1, 33, True), ((2, 2, 2, 2, 2, 3), 64, 16, 33, False), ((2, 2, 2, 2, 2, 3), 5, 17, None, True),
         ((5, 7, 3), 4, 16, None, False), ((33, 31, 9), 17, 17, 3, True), ((33, 31, 9), 64, 64, 17, False)]
IDS = ["n%s-k%d-m%d-nd%s%s" % ("x".join(map(str, g)), k, m, "B" if nd is None else nd, "-acc" if acc else "") for g, k, m, nd, acc in CASES]

_cache = {}


def case(ctx, grid, k, m, nd, accumulate, noise=0.4, scale=1.0, ref=True):
    """Seeded inputs of a case with their restatement (``ref``), computed once."""
    nd = block(ctx, len(grid)) + 1 if nd is None else nd
    key = (grid, k, m, nd, accumulate, noise, scale, ref)
    if key not in _cache:
        rng = np.random.default_rng(1000 * len(grid) + 10 * k + m + sum(grid) + nd)
        tables = [1.0 + 0.5 * rng.standard_normal((k, n)) for n in grid]
        a = scale * rng.standard_normal((m, k)) / np.sqrt(k)
        node = int(rng.integers(0, int(np.prod(grid))))
        c = np.ones(k)
        for t, i in zip(tables, np.unravel_index(node, grid)):
            c = c * t[:, i]
        Y = (a @ c)[None, :] + noise * rng.standard_normal((nd, m))
        weights = [rng.uniform(0.2, 1.0, n) for n in grid]
        absc = [np.sort(rng.uniform(-1.0, 2.0, n)) for n in grid]
        u, alpha, beta = RM.data_sets(Y, accumulate)
        _cache[key] = dict(tables=tables, a=a, Y=Y, u=u, alpha=alpha, beta=beta, weights=weights, absc=absc, node=node, S=int(np.prod(grid)),
                           nd=nd, D=len(grid))
        if ref:
            chi2x, sc = RM.chi2_many_exact(a, Y, tables, accumulate)
            _cache[key].update(chi2x=chi2x, bound=RM.chi2_many_bound(k, m, len(grid), sc, accumulate))
    return _cache[key]


def run(ctx, cs, want=THETA, rows=None, weights=None):
    rows = slice(None) if rows is None else rows
    return ctx.grid_posterior_many(cs["a"], cs["u"][rows], cs["alpha"][rows], cs["beta"][rows], cs["tables"],
                                   cs["weights"] if weights is None else weights, abscissae=cs["absc"], want=want)


def flat(out):
    """Every number of a result as one array of bits."""
    return np.concatenate([np.asarray(out[key], dtype=np.float64).reshape(-1).view(np.int64) if key != "argmin" else out[key].reshape(-1)
                           for key in ("chi2_min", "argmin", "Z", "sum_e2", "theta1", "theta2") if key in out])


@pytest.mark.parametrize("grid,k,m,nd,accumulate", CASES, ids=IDS)
def test_against_the_restatement(ctx, grid, k, m, nd, accumulate):
    cs = case(ctx, grid, k, m, nd, accumulate)
    outs = {}
    for name, variant in (("mfma", 1), ("plain", 0)):
        with Knobs(ctx, variant):
            outs[name] = run(ctx, cs)
        worst = RM.check(outs[name], cs["chi2x"], cs["bound"], cs["weights"], cs["absc"])
        print(name, "max error / bound", worst)
        assert all(v <= 1.0 for v in worst.values())
    # the variants agree within the bound, not bit for bit
    j = np.arange(cs["nd"])
    tol = cs["bound"][j, outs["mfma"]["argmin"]] + cs["bound"][j, outs["plain"]["argmin"]]
    assert np.all(np.abs(outs["mfma"]["chi2_min"] - outs["plain"]["chi2_min"]) <= tol + np.abs(
        (cs["chi2x"][j, outs["mfma"]["argmin"]] - cs["chi2x"][j, outs["plain"]["argmin"]]).astype(np.float64)))
    # without the bit: the same minima and sums, no moments
    with Knobs(ctx):
        bare = run(ctx, cs, want=0)
    assert "theta1" not in bare
    for key in ("chi2_min", "argmin", "Z", "sum_e2"):
        assert np.array_equal(bare[key], outs["mfma"][key]), key


def sharp(ctx, grid, k, m, nd):
    """Misfits of the order 1e4 and more: most (sample tile, data tile) pairs lie beyond the skip threshold, the tiles near a data
    set's best sample do not."""
    return case(ctx, grid, k, m, nd, False, noise=3.0, scale=40.0)


@pytest.mark.parametrize("variant", [1, 0], ids=["mfma", "plain"])
@pytest.mark.parametrize("which", [3, 5, 8, "sharp"])
def test_bit_identical_from_run_to_run_for_any_grid_with_and_without_skip(ctx, which, variant):
    cs = sharp(ctx, (33, 31, 9), 17, 17, 20) if which == "sharp" else case(ctx, *CASES[which])
    runs = []
    for grid_max, skip in ((0, 1), (0, 1), (1, 1), (3, 1), (0, 0), (3, 0)):
        with Knobs(ctx, variant, grid_max, skip):
            runs.append(flat(run(ctx, cs)))
    for r in runs[1:]:
        assert np.array_equal(r, runs[0])
    if which == "sharp":                                      # the case does what it is for: far samples carry no mass at all
        with Knobs(ctx, variant):
            out = run(ctx, cs)
        d = (cs["chi2x"] - cs["chi2x"].min(axis=1)[:, None]).astype(np.float64)
        assert np.mean(d > 2000.0) > 0.9 and np.all(np.isfinite(out["Z"])) and np.all(out["Z"] > 0.0)
        worst = RM.check(out, cs["chi2x"], cs["bound"], cs["weights"], cs["absc"])
        print("sharp: max error / bound", worst)
        assert all(v <= 1.0 for v in worst.values())


@pytest.mark.parametrize("grid,k,m", [((5, 7, 3), 17, 64), ((2, 2, 2, 2, 2, 3), 5, 17), ((33, 31, 9), 17, 17)], ids=["3d", "6d", "segments"])
@pytest.mark.parametrize("variant", [1, 0], ids=["mfma", "plain"])
def test_a_data_set_is_the_same_bits_wherever_it_sits(ctx, grid, k, m, variant):
    nd = 2 * block(ctx, len(grid)) + 5
    cs = case(ctx, grid, k, m, nd, False, ref=False)
    with Knobs(ctx, variant):
        alone = flat(run(ctx, cs, rows=[7]))
        for pos in (0, 16, nd - 1):
            order = [j for j in range(nd) if j != 7]
            order.insert(pos, 7)
            out = run(ctx, cs, rows=order)
            one = {key: v[pos:pos + 1] for key, v in out.items()}
            assert np.array_equal(flat(one), alone), pos
        # two identical rows in one call
        out = run(ctx, cs, rows=[3, 7, 5, 7])
        assert np.array_equal(flat({key: v[1:2] for key, v in out.items()}), flat({key: v[3:4] for key, v in out.items()}))
        assert np.array_equal(flat({key: v[1:2] for key, v in out.items()}), alone)


def test_weights_with_zeros(ctx):
    cs = case(ctx, *CASES[3])
    weights = [w.copy() for w in cs["weights"]]
    weights[0][1] = 0.0
    weights[2][[0, 2]] = 0.0
    for variant in (1, 0):
        with Knobs(ctx, variant):
            out = run(ctx, cs, weights=weights)
        worst = RM.check(out, cs["chi2x"], cs["bound"], weights, cs["absc"])
        print("max error / bound", worst)
        assert all(v <= 1.0 for v in worst.values()) and np.all(out["Z"] > 0.0)


def test_a_tie_goes_to_the_lower_sample_and_data_at_a_node_give_zero_within_the_bound(ctx):
    rng = np.random.default_rng(77)
    k, m, grid = 17, 15, (5, 7)
    tables = [1.0 + 0.5 * rng.standard_normal((k, n)) for n in grid]
    tables[0][:, 3] = tables[0][:, 1]                     # abscissa 3 of the slow dimension repeats abscissa 1
    a = rng.standard_normal((m, k))
    nodes = [(1, 4), (0, 0), (4, 6), (2, 3)]
    Y = np.stack([a @ (tables[0][:, i] * tables[1][:, j]) for i, j in nodes])        # data exactly at nodes; (1, 4) = (3, 4)
    u, alpha, beta = RM.data_sets(Y)
    weights, absc = [np.ones(5), np.ones(7)], [np.arange(5.0), np.arange(7.0)]
    chi2x, sc = RM.chi2_many_exact(a, Y, tables)
    bound = RM.chi2_many_bound(k, m, 2, sc)
    gap = RM.gap(chi2x)
    assert gap[0] == 0.0 and np.all(gap[1:] > 4 * bound[1:].max(axis=1))      # the exact runner-up gap: 0 for the tie, wide elsewhere
    for variant in (1, 0):
        with Knobs(ctx, variant):
            out = ctx.grid_posterior_many(a, u, alpha, beta, tables, weights, abscissae=absc, want=THETA)
        assert list(out["argmin"]) == [1 * 7 + 4, 0, 4 * 7 + 6, 2 * 7 + 3]
        for j in range(4):
            assert abs(out["chi2_min"][j]) <= bound[j, out["argmin"][j]] + float(chi2x[j, out["argmin"][j]])   # (a @ c is rounded: ~ 1e-30)


def test_one_sample_far_from_all_others_keeps_its_weight_and_nothing_else(ctx):
    cs = dict(case(ctx, (16, 16), 16, 16, 3, False))
    Y = 1e6 * cs["Y"]                                      # misfits of the order 1e12, their differences far beyond -2 log(tiny)
    cs["u"], cs["alpha"], cs["beta"] = RM.data_sets(Y)
    for variant, skip in ((1, 1), (1, 0), (0, 1)):
        with Knobs(ctx, variant, 0, skip):
            out = run(ctx, cs)
        for j in range(3):
            i = np.unravel_index(out["argmin"][j], (16, 16))
            w = 1.0 * cs["weights"][0][i[0]] * cs["weights"][1][i[1]]
            assert out["Z"][j] == w and out["sum_e2"][j] == w * w          # exp(0) = 1 at the minimum, 0 everywhere else
            assert out["theta1"][j, 0] == w * cs["absc"][0][i[0]] and out["theta1"][j, 1] == w * cs["absc"][1][i[1]]
            assert np.all(np.isfinite(out["theta2"][j]))


def test_invalid_arguments_leave_the_outputs_untouched(ctx):
    cs = case(ctx, *CASES[3])
    p = lambda arr: None if arr is None else arr.ctypes.data_as(PD)
    cat = lambda xs: np.ascontiguousarray(np.concatenate([np.asarray(x, dtype=np.float64).reshape(-1) for x in xs]))
    base = dict(a=np.ascontiguousarray(cs["a"]), m=64, k=17, u=np.ascontiguousarray(cs["u"]), alpha=cs["alpha"], beta=cs["beta"], nd=17,
                t=cat(cs["tables"]), n=np.array([5, 7, 3], dtype=np.int32), ndim=3, w=cat(cs["weights"]), x=cat(cs["absc"]), want=THETA,
                outs=(True,) * 5)

    def call(**kw):
        g = {**base, **kw}
        bufs = [np.full(17, POISON), np.full(17, -77, dtype=np.int64), np.full(34, POISON), np.full(17 * 3, POISON), np.full(17 * 9, POISON)]
        ptr = [p(bufs[0]), bufs[1].ctypes.data_as(_lib.PI64), p(bufs[2]), p(bufs[3]), p(bufs[4])]
        ptr = [q if on else None for q, on in zip(ptr, g["outs"])]
        rc = ctx.lib.pgd_grid_posterior_many(ctx.h, p(g["a"]), g["m"], g["k"], p(g["u"]), p(g["alpha"]), p(g["beta"]), g["nd"], p(g["t"]),
                                             None if g["n"] is None else g["n"].ctypes.data_as(_lib.PI32), g["ndim"], p(g["w"]), p(g["x"]),
                                             g["want"], *ptr)
        return rc, bufs

    bad_w, bad_x = base["w"].copy(), base["x"].copy()
    bad_w[4], bad_x[9] = np.inf, np.nan
    huge = np.array([1 << 11, 1 << 10, 1 << 10], dtype=np.int32)                    # S = 2^31
    for kw in (dict(want=1), dict(want=4), dict(want=3), dict(want=-1), dict(k=0), dict(k=65), dict(m=0), dict(m=65), dict(ndim=0), dict(ndim=7),
               dict(nd=0), dict(nd=-3), dict(nd=1 << 31), dict(a=None), dict(u=None), dict(alpha=None), dict(beta=None), dict(t=None),
               dict(n=None), dict(w=None), dict(x=None), dict(n=np.array([5, 0, 3], dtype=np.int32)), dict(n=huge), dict(w=bad_w),
               dict(x=bad_x), dict(outs=(False, True, True, True, True)), dict(outs=(True, False, True, True, True)),
               dict(outs=(True, True, False, True, True)), dict(outs=(True, True, True, False, True)),
               dict(outs=(True, True, True, True, False))):
        rc, bufs = call(**kw)
        assert rc == -1, kw
        assert all(np.all(b == (POISON if b.dtype == np.float64 else -77)) for b in bufs), kw
    rc, _ = call(k=65)
    assert b"compress the solution first" in ctx.lib.pgd_last_error(ctx.h)
    # without the bit neither the abscissae nor the moment arrays are needed (and a bad abscissa is not looked at)
    rc, bufs = call(want=0, x=None, outs=(True, True, True, False, False))
    assert rc == 0 and np.all(bufs[2][0::2] > 0.0) and np.all(bufs[3] == POISON)
    rc, bufs = call()
    assert rc == 0 and np.array_equal(bufs[4].reshape(17, 3, 3), bufs[4].reshape(17, 3, 3).transpose(0, 2, 1))


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


@pytest.mark.parametrize("accumulate", [False, True], ids=["each", "accumulate"])
def test_sensor_posterior_many_on_the_device_and_in_numpy(hip, monkeypatch, accumulate):
    """Twelve seeded modes on a small box, parameter dimensions of 33 and 17 nodes, 20 sensor points with gradient=True (60 rows,
    reduced to 12 by the QR), 21 data sets: the device route and the numpy route around the restatement of the reduced problem."""
    from pgdrome_amd.model import PGD
    rng = np.random.default_rng(41)
    V = fem.FunctionSpace(fem.BoxMesh(fem.Point(0, 0, 0), fem.Point(1, 1, 1), 6, 6, 6), "CG", 1)
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
    grids = [np.sort(Vps[0].mesh().coordinates()[:, 0].copy()), np.sort(Vps[1].mesh().coordinates()[:, 0].copy())]
    truth = sol.evaluate_sensor_response_many(0, [1, 2], np.array([[grids[0][20], grids[1][5]]]), 0, pts, gradient=True).values[0]
    sigma = 3.0 * np.abs(truth).max()                    # (wide: the seeded modes jump from node to node, many nodes keep mass)
    N = 21
    data = truth[None] + sigma * rng.standard_normal((N,) + truth.shape)
    kw = dict(grids=grids, sigma=sigma, gradient=True, prior={2: lambda x: 1.0 + 0.5 * x * x}, accumulate=accumulate)

    calls = fem.STATS.get("posterior_many_calls", 0)
    dev = sol.sensor_posterior_many(0, [1, 2], 0, pts, data, device=True, **kw)
    assert dev.path == "device" and fem.STATS.get("posterior_many_calls", 0) == calls + 1
    monkeypatch.setattr(model, "DEVICE_POSTERIOR_MANY_MIN_WORK", 1)
    assert sol.sensor_posterior_many(0, [1, 2], 0, pts, data, data_chunk=8, **kw).path == "device"        # (the default route, 3 chunks)
    assert fem.STATS.get("posterior_many_calls", 0) == calls + 4
    monkeypatch.setattr(model, "DEVICE_POSTERIOR_MANY_MIN_WORK", 1 << 60)
    ref = sol.sensor_posterior_many(0, [1, 2], 0, pts, data, **kw)
    assert ref.path == "numpy" and fem.STATS.get("posterior_many_calls", 0) == calls + 4

    # the restatement from what both routes were given: the whitened sensor modes, reduced by the same host QR
    phi = sol.sensor_modes(pts, 0, 0, gradient=True).host()[:K].T / sigma
    Q, Rm = np.linalg.qr(phi)
    Yw = data.reshape(N, -1) / sigma
    Zr = Yw @ Q
    r = Yw - Zr @ Q.T
    rest = np.einsum("np,np->n", r, r)
    tables = [np.ascontiguousarray(sol._free_modes_at(d, g, 0)) for d, g in zip((1, 2), grids)]
    for name, res in (("device", dev), ("numpy", ref)):
        print(name)
        RM.check_result(res, Rm, Zr, tables, accumulate=accumulate, rest=np.cumsum(rest) if accumulate else rest,
                        logdet=60 * math.log(sigma), m=60)
    assert np.array_equal(dev.map_index, ref.map_index)
