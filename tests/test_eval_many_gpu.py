"""pgd_eval_batch on the MI355X, through the C-ABI: the f64-MFMA kernel and the plain fma kernel against the numpy
restatement of tests/eval_many_reference.py - exact on integer data (fragment map, tails, padding, chunk boundaries),
bit-identical across grid sizes and sample chunks, inside the derived rounding bound on floating-point data - and
PGD.evaluate_many through the frontend."""

import numpy as np
import pytest

from pgdrome_amd import _lib
from tests.eval_many_reference import bound, evaluate_many_reference

pytestmark = pytest.mark.gpu

VARIANTS = {"mfma": 1, "plain": 0}


class Knobs:
    """Set pgd_eval_batch's knobs, put the defaults back on the way out."""

    def __init__(self, ctx, variant=1, grid_max=0, chunk=0):
        self.ctx, self.values = ctx, (variant, grid_max, chunk)

    def __enter__(self):
        for knob, v in zip((_lib.TUNE_EVAL_VARIANT, _lib.TUNE_EVAL_GRID_MAX, _lib.TUNE_EVAL_SAMPLE_CHUNK), self.values):
            self.ctx.tune(knob, v)

    def __exit__(self, *exc):
        for knob, v in ((_lib.TUNE_EVAL_VARIANT, 1), (_lib.TUNE_EVAL_GRID_MAX, 0), (_lib.TUNE_EVAL_SAMPLE_CHUNK, 0)):
            self.ctx.tune(knob, v)


def run_all_outputs(ctx, modes, Cm, n, threshold):
    """Every output of one call: dict of numpy arrays (fields as (S, n))."""
    S = Cm.shape[1]
    emn, emx, exc, fld = ctx.vec_alloc(n), ctx.vec_alloc(n), ctx.vec_alloc(n), ctx.vec_alloc(n * S)
    try:
        # poison: an entry the kernel fails to write must not look like a result
        for v in (emn, emx, exc, fld):
            ctx.vec_fill(v, -12345.678)
        st = ctx.eval_batch(modes, Cm, stats=True, env_min=emn, env_max=emx, exceed=exc, threshold=threshold, fields=fld)
        return {"stats": st, "env_min": ctx.vec_download(emn), "env_max": ctx.vec_download(emx),
                "exceed": ctx.vec_download(exc), "fields": ctx.vec_download(fld).reshape(S, n)}
    finally:
        for v in (emn, emx, exc, fld):
            ctx.vec_free(v)


def upload_modes(ctx, F):
    return [ctx.vec_from(np.ascontiguousarray(F[:, k], dtype=np.float64)) for k in range(F.shape[1])]


def free_all(ctx, vs):
    for v in vs:
        ctx.vec_free(v)


# (n, K, S, grid_max): every n of {1, 15, 16, 17, 293, 1541}; every K of {1, 3, 4, 5, 50, 256} and one just above each k-size the
# MFMA kernel is compiled for (16, 32, 48, 64, 128 -> 17, 33, 49, 65, 129); every S of {1, 15, 16, 17, 100}, 65 (the four waves of a
# workgroup take 16 samples each: the fifth tile is a wave's second) and 1025 (one past the default sample chunk)
SHAPES = [
    (1, 1, 1, 0), (15, 3, 15, 0), (16, 4, 16, 0), (17, 5, 17, 0), (293, 50, 100, 0), (1541, 256, 17, 0), (1541, 17, 65, 2),
    (293, 33, 16, 0), (17, 49, 100, 0), (16, 65, 15, 0), (293, 129, 17, 3), (1541, 50, 100, 2), (15, 256, 1, 0),
    (1, 5, 1025, 0), (293, 4, 65, 0), (1541, 3, 16, 1), (17, 1, 100, 0), (16, 50, 17, 0), (293, 17, 1025, 0), (1541, 5, 15, 0),
]


@pytest.mark.parametrize("sign", ["mixed", "positive", "negative"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "n%d-K%d-S%d-g%d" % s)
def test_exact_layout_on_integer_data(ctx, shape, sign):
    """Small integers: every product and sum is an exact integer far below 2^53, so every output of both variants must EQUAL
    the int64 result.  All-positive / all-negative fields are what a padded row, sample or k would show up in (a padded zero
    is the minimum of one and the maximum of the other)."""
    n, K, S, grid_max = shape
    rng = np.random.default_rng(1000 * n + 10 * K + S)
    if sign == "mixed":
        F, Cm = rng.integers(-7, 8, size=(n, K)), rng.integers(-7, 8, size=(K, S))
    else:
        F, Cm = rng.integers(1, 8, size=(n, K)), rng.integers(1, 8, size=(K, S))
        if sign == "negative":
            F = -F
    ref = evaluate_many_reference(F, Cm, 0.5)
    spread = np.sort(ref["U"].reshape(-1))
    threshold = float(spread[len(spread) // 2]) + 0.5        # an integer + 0.5 near the median: both sides are populated
    ref = evaluate_many_reference(F, Cm, threshold)
    modes = upload_modes(ctx, F)
    try:
        for name, variant in VARIANTS.items():
            with Knobs(ctx, variant=variant, grid_max=grid_max):
                out = run_all_outputs(ctx, modes, Cm.astype(np.float64), n, threshold)
            assert np.array_equal(out["fields"], ref["U"].T.astype(np.float64)), name
            assert np.array_equal(out["stats"][0], ref["min"]) and np.array_equal(out["stats"][1], ref["max"]), name
            assert np.array_equal(out["stats"][2], ref["max_abs"]), name
            assert np.array_equal(out["env_min"], ref["env_min"]) and np.array_equal(out["env_max"], ref["env_max"]), name
            assert np.array_equal(out["exceed"], ref["exceed"]), name
    finally:
        free_all(ctx, modes)


@pytest.fixture(scope="module")
def float_case():
    """n = 1541, K = 50, S = 100 of seeded normal data and its long-double reference, computed once."""
    n, K, S = 1541, 50, 100
    rng = np.random.default_rng(20240517)
    F, Cm = rng.standard_normal((n, K)), rng.standard_normal((K, S))
    return n, K, S, F, Cm, evaluate_many_reference(F, Cm, 0.25)


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_knob_invariance_is_bitwise(ctx, float_case, variant):
    """Grid size and sample chunk change which workgroup and which launch sees a (row, sample) pair, never a bit of any output:
    each u comes from one accumulation chain over k, a min / max is order-independent, counts are integers - and envelopes
    and counts ACCUMULATE across chunks, which is what this case is about."""
    n, K, S, F, Cm, _ = float_case
    modes = upload_modes(ctx, F)
    try:
        base = None
        for grid_max in (0, 1, 2, 3):
            for chunk in (0, 16, 48):
                with Knobs(ctx, variant=VARIANTS[variant], grid_max=grid_max, chunk=chunk):
                    out = run_all_outputs(ctx, modes, Cm, n, 0.25)
                if base is None:
                    base = out
                    continue
                for key in base:
                    assert np.array_equal(out[key].view(np.uint64), base[key].view(np.uint64)), (key, grid_max, chunk)
    finally:
        free_all(ctx, modes)


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_floating_point_bound_on_fields(ctx, float_case, variant):
    """|u - exact| <= (K + 2) 2^-53 sum_k |c_k| |f_k|: holds for any summation order, fused or not - derived, not measured."""
    n, K, S, F, Cm, ref = float_case
    modes = upload_modes(ctx, F)
    try:
        with Knobs(ctx, variant=VARIANTS[variant], grid_max=3):
            out = run_all_outputs(ctx, modes, Cm, n, 0.25)
    finally:
        free_all(ctx, modes)
    err = np.abs(out["fields"].T.astype(np.longdouble) - ref["U"]).astype(np.float64)
    ratio = float((err / bound(K, ref["B"])).max())
    print("eval_batch %s: largest error / bound = %.4f" % (variant, ratio))
    assert ratio <= 1.0


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_statistics_and_fields_come_from_the_same_accumulators(ctx, float_case, variant):
    n, K, S, F, Cm, _ = float_case
    modes = upload_modes(ctx, F)
    try:
        with Knobs(ctx, variant=VARIANTS[variant], grid_max=2, chunk=48):
            out = run_all_outputs(ctx, modes, Cm, n, 0.25)
    finally:
        free_all(ctx, modes)
    U = out["fields"]                                   # (S, n)
    assert np.array_equal(out["stats"][0], U.min(axis=1)) and np.array_equal(out["stats"][1], U.max(axis=1))
    assert np.array_equal(out["stats"][2], np.abs(U).max(axis=1))
    assert np.array_equal(out["env_min"], U.min(axis=0)) and np.array_equal(out["env_max"], U.max(axis=0))
    assert np.array_equal(out["exceed"], (U > 0.25).sum(axis=0))


def test_partial_requests_write_only_what_was_asked(ctx, float_case):
    """Statistics alone, and envelopes alone (no host synchronisation inside the call): the same values as the all-outputs call."""
    n, K, S, F, Cm, _ = float_case
    modes = upload_modes(ctx, F)
    emn, emx = ctx.vec_alloc(n), ctx.vec_alloc(n)
    try:
        full = run_all_outputs(ctx, modes, Cm, n, 0.25)
        st = ctx.eval_batch(modes, Cm, stats=True)
        assert np.array_equal(st, full["stats"])
        assert ctx.eval_batch(modes, Cm, stats=False, env_min=emn, env_max=emx) is None
        assert np.array_equal(ctx.vec_download(emn), full["env_min"]) and np.array_equal(ctx.vec_download(emx), full["env_max"])
    finally:
        free_all(ctx, modes + [emn, emx])


def test_argument_errors_are_codes_and_messages(ctx):
    """Invalid calls only: each is refused with PGD_ERR_INVALID and a message before anything is launched."""
    n, K, S = 40, 3, 5
    modes = [ctx.vec_from(np.ones(n)) for _ in range(K)]
    short, emn, emx, exc, fld = ctx.vec_alloc(n - 1), ctx.vec_alloc(n), ctx.vec_alloc(n), ctx.vec_alloc(n), ctx.vec_alloc(n * S)
    cf = np.ones((K, S))
    st = np.full((3, S), -1.0)
    lib, PD = ctx.lib, _lib.PD

    def call(mlist, k, want, thr=0.0, stats=None, a=0, b=0, c=0, d=0, s=S):
        arr = (_lib.H * max(len(mlist), 1))(*mlist)
        rc = lib.pgd_eval_batch(ctx.h, arr, k, cf.ctypes.data_as(PD), s, want, thr,
                                stats.ctypes.data_as(PD) if stats is not None else None, a, b, c, d)
        return rc, lib.pgd_last_error(ctx.h).decode()

    try:
        for what, (rc, msg) in {
            "k = 0": call(modes, 0, 1, stats=st),
            "k = 257": call(modes * 86, 257, 1, stats=st),
            "s = 0": call(modes, K, 1, stats=st, s=0),
            "nothing requested": call(modes, K, 0),
            "missing stats": call(modes, K, 1),
            "missing envelope": call(modes, K, 2, a=emn),
            "missing exceed": call(modes, K, 4, thr=0.5),
            "missing fields": call(modes, K, 8),
            "unrequested stats": call(modes, K, 2, stats=st, a=emn, b=emx),
            "unrequested envelope": call(modes, K, 1, stats=st, a=emn, b=emx),
            "unrequested threshold": call(modes, K, 1, thr=0.5, stats=st),
            "mode of another size": call(modes[:2] + [short], K, 1, stats=st),
            "envelope of another size": call(modes, K, 2, a=short, b=emx),
            "fields of another size": call(modes, K, 8, d=emn),
            "output aliasing a mode": call(modes, K, 2, a=modes[1], b=emx),
            "outputs aliasing each other": call(modes, K, 2, a=emn, b=emn),
            "not a vector": call(modes[:2] + [987654], K, 1, stats=st),
        }.items():
            assert rc == -1 and msg.startswith("eval_batch:"), (what, rc, msg)
        assert np.all(st == -1.0)                        # nothing ran
        # and the valid call right after them works
        assert ctx.eval_batch(modes, cf).tolist() == [[3.0] * S] * 3
    finally:
        free_all(ctx, modes + [short, emn, emx, exc, fld])


def test_empty_vectors_are_ok_and_leave_the_statistics_alone(ctx):
    m = ctx.vec_alloc(0)
    st = np.full((3, 2), 7.0)
    try:
        arr = (_lib.H * 1)(m)
        cf = np.ones((1, 2))
        assert ctx.lib.pgd_eval_batch(ctx.h, arr, 1, cf.ctypes.data_as(_lib.PD), 2, 1, 0.0, st.ctypes.data_as(_lib.PD), 0, 0, 0, 0) == 0
        assert np.all(st == 7.0)
    finally:
        ctx.vec_free(m)


def test_evaluate_many_through_the_frontend(monkeypatch):
    """A small solved problem, the device path forced: evaluate_many agrees with a loop over evaluate() + numpy reductions
    within the rounding bound of the two summation orders, and the batched kernel is what ran."""
    from pgdrome_amd import fem, model, problems
    from pgdrome_amd.hip_backend import HipBackend
    from pgdrome_amd.solver import PGDProblem
    old = fem._backend
    fem.set_backend(HipBackend(0))
    fem.clear_caches()
    try:
        mesh = fem.BoxMesh(fem.Point(0, 0, 0), fem.Point(1, 1, 1), 8, 8, 8)
        p = PGDProblem(**problems.reaction_diffusion(mesh, 17, PGD_nmax=3))
        p.solve_PGD(_problem="linear")
        sol = p.return_PGD()
        monkeypatch.setattr(model, "DEVICE_EVAL_MIN_DOFS", 0)
        S = 37
        X = sol.mesh[1].dataX
        coords = np.random.default_rng(5).uniform(X.min(), X.max(), size=(S, 1))
        coords[0, 0], coords[1, 0] = X.min(), X.max()
        loop = np.array([sol.evaluate(0, [1], list(c), 0).vector().host() for c in coords])       # (S, n), vertex order
        Cm = sol.mode_factors_many([1], coords, 0)
        K = sol.used_numModes
        F = np.stack([sol.mesh[0].attributes[0].interpolationfct[k].vector().host() for k in range(K)], axis=1)
        B = bound(K, np.abs(F) @ np.abs(Cm)).T              # (S, n)
        threshold = float(np.median(loop))
        calls = fem.STATS.get("eval_batch_calls", 0)
        res = sol.evaluate_many(0, [1], coords, 0, stats=True, envelope=True, threshold=threshold, fields=True)
        assert fem.STATS.get("eval_batch_calls", 0) == calls + 1
        fields = np.array([f.vector().host() for f in res.fields])
        assert np.all(np.abs(fields - loop) <= B)
        assert np.all(np.abs(res.min - loop.min(axis=1)) <= B.max(axis=1))
        assert np.all(np.abs(res.max - loop.max(axis=1)) <= B.max(axis=1))
        assert np.all(np.abs(res.max_abs - np.abs(loop).max(axis=1)) <= B.max(axis=1))
        assert np.all(np.abs(res.envelope_min.vector().host() - loop.min(axis=0)) <= B.max(axis=0))
        assert np.all(np.abs(res.envelope_max.vector().host() - loop.max(axis=0)) <= B.max(axis=0))
        clear = np.abs(loop - threshold) > B                 # pairs whose side of the threshold rounding cannot change
        lo = (clear & (loop > threshold)).sum(axis=0) / S
        hi = lo + (~clear).sum(axis=0) / S
        ex = res.exceedance.vector().host()
        assert np.all(ex >= lo - 1e-15) and np.all(ex <= hi + 1e-15)
        # the statistics and the fields of the one call are the same numbers
        assert np.array_equal(res.min, fields.min(axis=1)) and np.array_equal(ex, (fields > threshold).sum(axis=0) / S)
    finally:
        fem.set_backend(old)
        fem.clear_caches()
