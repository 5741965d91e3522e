"""pgd_design_update and pgd_design_gains on the MI355X through the C-ABI, and PGD.sensor_placement end to end: the f64-MFMA kernel and
the plain fma kernel against the longdouble restatement of tests/placement_reference.py inside its derived bounds; every output
bit-identical from run to run, for any grid and wherever a candidate sits; installed / exclude; every refusal.

The shape with 4100 candidates is held to the restatement on the candidates at both ends of the range (the longdouble product of all
4100 takes most of a minute); every candidate of it is held to the bit-identity of those against a call of their own."""
import ctypes as C

import numpy as np
import pytest

from pgdrome_amd import _lib, fem, model
from tests import placement_reference as PR

pytestmark = pytest.mark.gpu

PD = C.POINTER(C.c_double)
POISON = -12345.678

# (grid, k, M, R): zero padding in k and M, every R, ndim 1, 3 and 6, a dimension of length 1, 9207 samples (three segments, tiles that
# end inside a segment), more than one chunk of candidates
SHAPES = [((5,), 1, 3, 1), ((17,), 5, 17, 1), ((5, 7, 3), 17, 37, 1), ((5, 7, 3), 17, 37, 3), ((1, 9, 1), 48, 16, 2),
          ((2, 2, 2, 2, 2, 3), 64, 130, 2), ((33, 31, 9), 48, 130, 1), ((33, 31, 9), 64, 4100, 1)]
IDS = ["n%s-k%d-M%d-R%d" % ("x".join(map(str, s[0])), s[1], s[2], s[3]) for s in SHAPES]


class Knobs:
    """variant (1 MFMA, 0 plain) and grid cap of the calls."""

    def __init__(self, ctx, variant=1, grid_max=0):
        self.ctx, self.values = ctx, (variant, grid_max)

    def set(self, variant, grid_max):
        self.ctx.tune(_lib.TUNE_DESIGN_VARIANT, variant)
        self.ctx.tune(_lib.TUNE_DESIGN_GRID_MAX, grid_max)

    def __enter__(self):
        self.set(*self.values)

    def __exit__(self, *exc):
        self.set(1, 0)


_cache = {}


def case(grid, k, M, R):
    """Seeded inputs of a shape, a state (H0 plus two candidates, formed on the host) and the restatement of the gains at it, once."""
    key = (grid, k, M, R)
    if key not in _cache:
        cs = PR.recipe(grid, k, M, R)
        g = PR.grid_of(cs["tables"], cs["dtables"], cs["weights"])
        st = model.design_state_numpy(grid)
        model.design_update_numpy(st, cs["tables"], cs["dtables"], cs["weights"], rows=cs["a"][:2 * R], h0=cs["H0"])
        sub = np.arange(M) if M <= 256 else np.concatenate([np.arange(48), np.arange(M - 40, M)])
        rows = (sub[:, None] * R + np.arange(R)[None, :]).reshape(-1)
        gx, bound = PR.gains_exact(g, cs["a"][rows], R, st["W"])
        cs.update(g=g, H=st["H"], W=st["W"], packed=PR.pack_state(st["H"], st["W"]), sub=sub, sub_rows=rows, gx=gx, bound=bound)
        _cache[key] = cs
    return _cache[key]


def grid_args(cs):
    return cs["tables"], cs["dtables"], cs["weights"]


@pytest.mark.parametrize("grid,k,M,R", SHAPES, ids=IDS)
def test_gains_against_the_restatement(ctx, grid, k, M, R):
    cs = case(grid, k, M, R)
    state = ctx.vec_from(cs["packed"])
    try:
        outs = {}
        for name, variant in (("mfma", 1), ("plain", 0)):
            with Knobs(ctx, variant):
                outs[name] = ctx.design_gains(cs["a"], R, state, *grid_args(cs))
            ratio = np.abs(outs[name][cs["sub"]] - cs["gx"]).astype(np.float64) / cs["bound"]
            print(name, "gains: max error / bound", float(ratio.max()))
            assert np.all(ratio <= 1.0)
            assert np.all(np.isfinite(outs[name])) and np.all(outs[name] > 0.0)
        # the variants agree within the sum of their bounds, not bit for bit
        assert np.all(np.abs(outs["mfma"][cs["sub"]] - outs["plain"][cs["sub"]]) <= 2.0 * cs["bound"])
        if cs["sub"].size < M:
            # the candidates the restatement covers, in a call of their own: the same bits as among the 4100
            for name, variant in (("mfma", 1), ("plain", 0)):
                with Knobs(ctx, variant):
                    own = ctx.design_gains(cs["a"][cs["sub_rows"]], R, state, *grid_args(cs))
                assert np.array_equal(own, outs[name][cs["sub"]]), name
        # the call does not touch the state
        assert np.array_equal(ctx.vec_download(state), cs["packed"])
    finally:
        ctx.vec_free(state)


@pytest.mark.parametrize("grid,k,M,R", SHAPES[:7], ids=IDS[:7])
def test_update_against_the_restatement(ctx, grid, k, M, R):
    cs = case(grid, k, M, R)
    g, D, S = cs["g"], len(grid), int(np.prod(grid))
    state = ctx.design_state(grid)
    try:
        ctx.vec_fill(state, POISON)
        ld0, cov0 = ctx.design_update(state, *grid_args(cs), h0=cs["H0"])                      # R = 0 with h0: the reset
        Hk, Wk = PR.unpack_state(ctx.vec_download(state), D, S)
        assert np.all(Hk == cs["H0"][None])
        H, dH = PR.h_exact(g, cs["H0"], np.zeros((0, k)))
        ldx, b_ld, covx, b_cov = PR.sums_exact(g, H, dH)
        assert abs(ld0 - ldx) <= b_ld and np.all(np.abs(cov0 - covx) <= b_cov)
        rows = cs["a"][:2 * R]
        ld, cov = ctx.design_update(state, *grid_args(cs), rows=rows)                           # added to what is there
        Hk, Wk = PR.unpack_state(ctx.vec_download(state), D, S)
        H, dH = PR.h_exact(g, cs["H0"], rows)
        err = np.abs(Hk - H).astype(np.float64)
        print("H: max error / bound", float(np.max(err / dH)))
        assert np.all(err <= dH)
        E, bE = PR.w_backward_bound(Hk, Wk)
        print("W H W^T - I: max error / bound", float(np.max(np.abs(E) / bE)))
        assert np.all(np.abs(E) <= bE)
        ldx, b_ld, covx, b_cov = PR.sums_exact(g, H, dH)
        print("log det: error / bound", float(abs(ld - ldx) / b_ld), " covariance:", float(np.max(np.abs(cov - covx) / b_cov)))
        assert abs(ld - ldx) <= b_ld and np.all(np.abs(cov - covx) <= b_cov) and np.array_equal(cov, cov.T)
        # h0 and the rows in one call: the same bits as the two calls
        first = ctx.vec_download(state)
        ctx.vec_fill(state, POISON)
        ld2, cov2 = ctx.design_update(state, *grid_args(cs), rows=rows, h0=cs["H0"])
        assert ld2 == ld and np.array_equal(cov2, cov) and np.array_equal(ctx.vec_download(state), first)
    finally:
        ctx.vec_free(state)


@pytest.mark.parametrize("which", [3, 5, 6], ids=[IDS[3], IDS[5], IDS[6]])
def test_bit_identical_from_run_to_run_and_for_any_grid(ctx, which):
    cs = case(*SHAPES[which])
    grid, k, M, R = SHAPES[which]
    state = ctx.design_state(grid)
    try:
        runs = []
        for grid_max in (0, 0, 1, 3):
            with Knobs(ctx, 1, grid_max):
                ld, cov = ctx.design_update(state, *grid_args(cs), rows=cs["a"][:2 * R], h0=cs["H0"])
                st = ctx.vec_download(state)
                mf = ctx.design_gains(cs["a"], R, state, *grid_args(cs))
            with Knobs(ctx, 0, grid_max):
                pl = ctx.design_gains(cs["a"], R, state, *grid_args(cs))
            runs.append(np.concatenate([[ld], cov.reshape(-1), st, mf, pl]).view(np.int64))
        for r in runs[1:]:
            assert np.array_equal(r, runs[0])
    finally:
        ctx.vec_free(state)


@pytest.mark.parametrize("which", [3, 5, 7], ids=[IDS[3], IDS[5], IDS[7]])
@pytest.mark.parametrize("variant", [1, 0], ids=["mfma", "plain"])
def test_a_candidate_is_the_same_bits_wherever_it_sits(ctx, which, variant):
    cs = case(*SHAPES[which])
    grid, k, M, R = SHAPES[which]
    a = cs["a"].reshape(M, R * k)
    state = ctx.vec_from(cs["packed"])
    try:
        with Knobs(ctx, variant):
            full = ctx.design_gains(a.reshape(-1, k), R, state, *grid_args(cs))
            alone = ctx.design_gains(a[7].reshape(-1, k), R, state, *grid_args(cs))
            assert alone[0] == full[7]
            for pos in (0, 16, M - 1):
                order = [j for j in range(M) if j != 7]
                order.insert(pos, 7)
                out = ctx.design_gains(a[order].reshape(-1, k), R, state, *grid_args(cs))
                assert out[pos] == alone[0], pos
                assert np.array_equal(out, full[order])
            twice = ctx.design_gains(a[[3, 7, 5, 7]].reshape(-1, k), R, state, *grid_args(cs))
            assert twice[1] == twice[3] == alone[0]
    finally:
        ctx.vec_free(state)


def test_invalid_arguments_leave_the_outputs_untouched(ctx):
    grid, k, M, R = SHAPES[3]
    cs = case(grid, k, M, R)
    p = lambda arr: None if arr is None else arr.ctypes.data_as(PD)
    cat = lambda xs: np.ascontiguousarray(np.concatenate([np.asarray(x, dtype=np.float64).reshape(-1) for x in xs]))
    state = ctx.vec_from(cs["packed"])
    short = ctx.vec_alloc(cs["packed"].size - 1)
    base = dict(a=cs["a"], M=M, R=R, k=k, t=cat(cs["tables"]), dt=cat(cs["dtables"]), n=np.array(grid, dtype=np.int32), ndim=3, w=cat(cs["weights"]),
                state=state, out=True, h0=np.ascontiguousarray(cs["H0"]))
    bad_w = base["w"].copy()
    bad_w[4] = np.inf
    huge = np.array([1 << 11, 1 << 10, 1 << 10], dtype=np.int32)                    # S = 2^31
    common = (dict(k=0), dict(k=65), dict(ndim=0), dict(ndim=7), dict(t=None), dict(dt=None), dict(n=None), dict(w=None), dict(w=bad_w),
              dict(n=np.array([5, 0, 3], dtype=np.int32)), dict(n=huge), dict(state=short), dict(state=987654), dict(out=False), dict(a=None))

    def gains(**kw):
        q = {**base, **kw}
        buf = np.full(M, POISON)
        rc = ctx.lib.pgd_design_gains(ctx.h, p(q["a"]), q["M"], q["R"], q["k"], p(q["t"]), p(q["dt"]),
                                      None if q["n"] is None else q["n"].ctypes.data_as(_lib.PI32), q["ndim"], p(q["w"]), q["state"],
                                      p(buf) if q["out"] else None)
        return rc, buf

    def update(**kw):
        q = {**base, **kw}
        buf = np.full(7, POISON)
        rc = ctx.lib.pgd_design_update(ctx.h, p(q["h0"]), p(q["a"]), q["R"], q["k"], p(q["t"]), p(q["dt"]),
                                       None if q["n"] is None else q["n"].ctypes.data_as(_lib.PI32), q["ndim"], p(q["w"]), q["state"],
                                       p(buf) if q["out"] else None)
        return rc, buf

    try:
        for kw in common + (dict(R=0), dict(R=4), dict(M=0), dict(M=-2), dict(M=1 << 31)):
            rc, buf = gains(**kw)
            assert rc == -1 and np.all(buf == POISON), kw
        rc, _ = gains(k=65)
        assert b"compress the solution first" in ctx.lib.pgd_last_error(ctx.h)
        rc, _ = gains(R=4)
        assert b"group=\"entry\"" in ctx.lib.pgd_last_error(ctx.h)
        unsym, indef, nan = base["h0"].copy(), base["h0"].copy(), base["h0"].copy()
        unsym[0, 1] += 1e-9
        indef[2, 2] = -1.0
        nan[1, 1] = np.nan
        for kw in common + (dict(R=-1), dict(R=257), dict(h0=unsym), dict(h0=indef), dict(h0=nan)):
            rc, buf = update(**kw)
            assert rc == -1 and np.all(buf == POISON), kw
            assert np.array_equal(ctx.vec_download(state), cs["packed"]), kw             # nothing was launched
        rc, _ = update(h0=indef)
        assert b"symmetric positive definite" in ctx.lib.pgd_last_error(ctx.h)
        rc, buf = gains()
        assert rc == 0 and np.all(buf > 0.0)
        rc, buf = update(a=None, R=0)                                                   # no rows: none are needed
        assert rc == 0 and np.all(buf != POISON)
    finally:
        ctx.vec_free(state)
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


@pytest.fixture(scope="module")
def solved(hip):
    """Twelve seeded modes on a small box, parameter dimensions of 33 and 17 nodes (the model of tests/test_posterior_many_gpu.py),
    forty candidate points."""
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
    pts = rng.uniform(0.05, 0.95, (40, 3))
    grids = [np.sort(Vps[0].mesh().coordinates()[:, 0].copy()), np.sort(Vps[1].mesh().coordinates()[:, 0].copy())]
    return sol, pts, grids


def reference(sol, pts, grids, sigma, gradient, n_select, H0, prior=None, **kw):
    K = sol.used_numModes
    tables = [np.ascontiguousarray(sol._free_modes_at(d, x, 0)) for d, x in zip((1, 2), grids)]
    dtables = [np.ascontiguousarray(sol._free_mode_derivatives_at(d, x, 0)) for d, x in zip((1, 2), grids)]
    weights = []
    for d, x in zip((1, 2), grids):
        w = model.trapezoid_weights(x) * (prior[d](x) if prior and d in prior else 1.0)
        weights.append(w / w.sum())
    A = np.ascontiguousarray(sol.sensor_modes(pts, 0, 0, gradient=gradient).host()[:K].T / sigma)
    R = 3 if gradient else 1
    return PR.greedy(PR.grid_of(tables, dtables, weights), A, R, H0, n_select, **kw), R


@pytest.mark.parametrize("gradient", [False, True], ids=["R1", "R3"])
def test_sensor_placement_on_the_device_and_in_numpy(solved, monkeypatch, gradient):
    sol, pts, grids = solved
    sigma, n_select = 0.2, 6
    prior = {2: lambda x: 1.0 + 0.5 * x * x}
    kw = dict(grids=grids, sigma=sigma, gradient=gradient, prior=prior, keep_gains=True)
    calls = fem.STATS.get("placement_calls", 0)
    dev = sol.sensor_placement(0, [1, 2], 0, pts, n_select, device=True, **kw)
    assert dev.path == "device" and fem.STATS.get("placement_calls", 0) == calls + 1
    monkeypatch.setattr(model, "DEVICE_PLACEMENT_MIN_WORK", 1)
    assert sol.sensor_placement(0, [1, 2], 0, pts, 1, **kw).path == "device"                     # (the default route)
    monkeypatch.setattr(model, "DEVICE_PLACEMENT_MIN_WORK", 1 << 60)
    ref = sol.sensor_placement(0, [1, 2], 0, pts, n_select, **kw)
    assert ref.path == "numpy" and fem.STATS.get("placement_calls", 0) == calls + 2
    ex, R = reference(sol, pts, grids, sigma, gradient, n_select, dev.prior_precision, prior=prior)
    # the condition, on the reference: every gap is more than ten times the bound - so the selections must be the same
    for step, j in enumerate(ex["selected"]):
        print("step", step, "gap", ex["gap"][step], "bound / gain", float(ex["bounds"][step].max() / ex["gains"][step][j]))
        assert ex["gap"][step] * float(ex["gains"][step][j]) > 10.0 * ex["bounds"][step].max(), step
    assert list(dev.selected) == ex["selected"] and list(ref.selected) == ex["selected"]
    for name, res in (("device", dev), ("numpy", ref)):
        for step in range(n_select):
            ratio = np.abs(res.gain_history[step] - ex["gains"][step]).astype(np.float64) / ex["bounds"][step]
            print(name, "step", step, "gains: max error / bound", float(ratio.max()))
            assert np.all(ratio <= 1.0)
            tol = ex["bounds"][step][res.selected[step]] + 0.5 * (ex["logdet_bound"][step] + ex["logdet_bound"][step + 1])
            assert abs(res.gains[step] - (res.utility[step + 1] - res.utility[step])) <= tol
        for step in range(n_select + 1):
            assert np.all(np.abs(res.expected_cov[step] - ex["cov"][step]).astype(np.float64) <= ex["cov_bound"][step])
    assert np.all(np.abs(dev.gain_history - ref.gain_history) <= 2.0 * np.stack(ex["bounds"]))
    assert np.array_equal(dev.selected_points, pts[dev.selected])


def test_installed_and_exclude_on_the_device(solved):
    sol, pts, grids = solved
    kw = dict(grids=grids, sigma=0.2, keep_gains=True)
    free = sol.sensor_placement(0, [1, 2], 0, pts, 3, device=True, **kw)
    inst = sol.sensor_placement(0, [1, 2], 0, pts, 2, device=True, installed=[int(free.selected[0])], exclude=[int(free.selected[1])], **kw)
    host = sol.sensor_placement(0, [1, 2], 0, pts, 2, device=False, installed=[int(free.selected[0])], exclude=[int(free.selected[1])], **kw)
    assert inst.installed_gains[0] == free.gains[0]                     # (a candidate alone: the bits it has among the others)
    assert free.selected[1] not in inst.selected and free.selected[0] not in inst.selected
    assert np.array_equal(inst.gain_history[0], free.gain_history[1])   # the state after the installed one is the state after step 0
    ex, _ = reference(sol, pts, grids, 0.2, False, 2, free.prior_precision, installed=[int(free.selected[0])], exclude=[int(free.selected[1])])
    assert list(inst.selected) == ex["selected"] == list(host.selected)
    for res in (inst, host):
        assert abs(res.installed_gains[0] - float(ex["installed_gains"][0])) <= ex["installed_bounds"][0]
        for step in range(2):
            assert np.all(np.abs(res.gain_history[step] - ex["gains"][step]).astype(np.float64) <= ex["bounds"][step])
