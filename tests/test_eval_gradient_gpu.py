"""pgd_cell_gradient and pgd_eval_batch_norm on the MI355X, through the C-ABI, against tests/eval_gradient_reference.py: exact on
integer data (cell records, blocked layouts, plane order; fragment map, tails, padding, chunk boundaries, every choice of the row
block), bit-identical across grid sizes and sample chunks, inside the derived rounding bounds on floating-point data - and
PGD.evaluate_gradient_many through the frontend."""

import numpy as np
import pytest

from pgdrome_amd import _lib, fem
from tests.eval_gradient_reference import (LD, evaluate_norm_reference, norm_bound, plane_bound, planes, product_bound, run_and_check,
                                           samples_of, two_valued)
from tests.test_eval_many_gpu import VARIANTS, Knobs, free_all

pytestmark = pytest.mark.gpu

POISON = -12345.678


# ------------------------------------------------------------------------------------------------ stage 1
def _meshes():
    P = fem.Point
    return {
        "interval7": fem.IntervalMesh(7, 0.0, 7.0),
        "rect-right": fem.RectangleMesh(P(0, 0), P(3, 2), 3, 2, "right"),
        "rect-left": fem.RectangleMesh(P(0, 0), P(3, 2), 3, 2, "left"),
        "rect-crossed": fem.RectangleMesh(P(0, 0), P(3, 2), 3, 2, "crossed"),
        "box72": fem.BoxMesh(P(0, 0, 0), P(2, 3, 2), 2, 3, 2),
        "box360": fem.BoxMesh(P(0, 0, 0), P(5, 4, 3), 5, 4, 3),            # more than one workgroup
    }


MESHES = _meshes()
STEPS = np.array([0.1, 0.37, 1.0 / 3.0])


def gradient_cases(ctx, name, X, integer):
    """Every (ncomp, q, scale or none) on one uploaded mesh: yields (got (q, cells), X, cells, U, L, scale)."""
    cells = MESHES[name].cells()
    nc, nv, G = cells.shape[0], X.shape[0], cells.shape[1] - 1
    rng = np.random.default_rng(nc)
    base = ctx.mesh_upload(X, cells)
    layouts = {1: base}
    try:
        for ncomp in (1, 2, 3):
            if ncomp > 1:
                layouts[ncomp] = ctx.mesh_blocked(base, ncomp)
            qin = ncomp * G
            for q in sorted({1} | {q for q in (3, 6, 9) if q <= qin}):
                for with_scale in (False, True):
                    if integer:
                        U, L = rng.integers(-7, 8, size=(nv, ncomp)), rng.integers(-4, 5, size=(q, qin))
                        scale = rng.integers(-3, 4, size=nc) if with_scale else None
                    else:
                        U, L = rng.standard_normal((nv, ncomp)), rng.standard_normal((q, qin))
                        scale = rng.standard_normal(nc) if with_scale else None
                    u, out = ctx.vec_from(U.astype(np.float64).reshape(-1)), ctx.vec_alloc(q * nc)
                    sc = ctx.vec_from(scale.astype(np.float64)) if with_scale else 0
                    try:
                        ctx.vec_fill(out, POISON)
                        ctx.cell_gradient(layouts[ncomp], u, L.astype(np.float64), out, sc)
                        yield ctx.vec_download(out).reshape(q, nc), cells, U, L, scale
                    finally:
                        free_all(ctx, [u, out] + ([sc] if with_scale else []))
    finally:
        for h in list(layouts.values())[::-1]:
            ctx.mesh_free(h)


@pytest.mark.parametrize("name", list(MESHES))
def test_cell_gradient_is_exact_on_unit_lattices(ctx, name):
    """Integer nodal values, integer L and scale on lattices of unit steps: every entry of the inverse Jacobian is an integer (0
    or +-1; +-2 around the midpoints of the crossed mesh), every intermediate is a small integer, so the planes must EQUAL the int64
    reference - scalar and blocked layouts, every q the layout allows, with and without a scale."""
    X = MESHES[name].coordinates()
    n = 0
    for got, cells, U, L, scale in gradient_cases(ctx, name, X, integer=True):
        ref = planes(X, cells, U, L, scale)
        assert ref.dtype == np.int64 and np.array_equal(got, ref.astype(np.float64)), (name, U.shape[1], L.shape[0], scale is not None)
        n += 1
    assert n >= 2


@pytest.mark.parametrize("name", list(MESHES))
def test_cell_gradient_bound_on_stretched_meshes(ctx, name):
    """Steps (0.1, 0.37, 1 / 3) and normal data: inside the stage-1 bound of the reference (operation counts of the cofactor
    inverse) against long double."""
    X0 = MESHES[name].coordinates()
    X = X0 * STEPS[None, :X0.shape[1]]
    worst = 0.0
    for got, cells, U, L, scale in gradient_cases(ctx, name, X, integer=False):
        ref, bd = planes(X, cells, U, L, scale), plane_bound(X, cells, U, L, scale)
        err = np.abs(got.astype(LD) - ref).astype(np.float64)
        assert np.all(err <= bd), (name, U.shape[1], L.shape[0], float((err / bd).max()))
        worst = max(worst, float((err[bd > 0] / bd[bd > 0]).max()))
    print("cell_gradient %s: largest error / bound = %.4f" % (name, worst))


def test_cell_gradient_argument_errors(ctx):
    mesh = MESHES["rect-right"]
    X, cells = mesh.coordinates(), mesh.cells()
    nc, nv = cells.shape[0], X.shape[0]
    base = ctx.mesh_upload(X, cells)
    blocked = ctx.mesh_blocked(base, 2)
    p2 = fem.FunctionSpace(mesh, "CG", 2)._lay
    p2h = ctx.mesh_upload(p2.coords, p2.cells)
    u, u2, out, scale, short = ctx.vec_from(np.ones(nv)), ctx.vec_from(np.ones(2 * nv)), ctx.vec_alloc(2 * nc), ctx.vec_from(np.ones(nc)), ctx.vec_alloc(nc - 1)
    up2 = ctx.vec_from(np.ones(p2.n))
    ctx.vec_fill(out, POISON)
    L = np.ones((2, 2))
    lib, PD = ctx.lib, _lib.PD

    def call(m, uh, q, sc, o, Lp=L):
        rc = lib.pgd_cell_gradient(ctx.h, m, uh, Lp.ctypes.data_as(PD) if Lp is not None else None, q, sc, o)
        return rc, lib.pgd_last_error(ctx.h).decode()

    try:
        for what, (rc, msg) in {
            "P2 layout": call(p2h, up2, 2, 0, out),
            "q = 0": call(base, u, 0, 0, out),
            "q = 10": call(base, u, 10, 0, out),
            "null L": call(base, u, 2, 0, out, None),
            "u of the scalar layout on the blocked one": call(blocked, u, 2, 0, out),
            "u of the blocked layout on the scalar one": call(base, u2, 2, 0, out),
            "out of another size": call(base, u, 2, 0, scale),
            "scale of another size": call(base, u, 2, short, out),
            "out aliases u": call(base, out, 2, 0, out),
            "out aliases scale": call(base, u, 1, scale, scale),
            "not a mesh": call(987654, u, 2, 0, out),
            "not a vector": call(base, 987654, 2, 0, out),
        }.items():
            assert rc == -1 and msg.startswith("cell_gradient:"), (what, rc, msg)
        assert np.all(ctx.vec_download(out) == POISON)            # nothing ran
    finally:
        free_all(ctx, [u, u2, out, scale, short, up2])
        for h in (p2h, blocked, base):
            ctx.mesh_free(h)


# ------------------------------------------------------------------------------------------------ stage 2
def upload_planes(ctx, P):
    """P: (K, q, m) -> one vector of q * m entries per mode, plane-major."""
    return [ctx.vec_from(np.ascontiguousarray(P[k], dtype=np.float64).reshape(-1)) for k in range(P.shape[0])]


def run_norm_outputs(ctx, modes, q, Cm, m, threshold):
    """Every output of one call: dict of numpy arrays (fields as (S, m))."""
    S = Cm.shape[1]
    emn, emx, exc, fld = ctx.vec_alloc(m), ctx.vec_alloc(m), ctx.vec_alloc(m), ctx.vec_alloc(m * S)
    try:
        for v in (emn, emx, exc, fld):
            ctx.vec_fill(v, POISON)
        st = ctx.eval_batch_norm(modes, q, Cm, stats=True, env_min=emn, env_max=emx, exceed=exc, threshold=threshold, fields=fld)
        return {"stats": st, "env_min": ctx.vec_download(emn), "env_max": ctx.vec_download(emx),
                "exceed": ctx.vec_download(exc), "fields": ctx.vec_download(fld).reshape(S, m)}
    finally:
        free_all(ctx, [emn, emx, exc, fld])


# (m, q, K, S, grid_max): every m of {1, 15, 16, 17, 293, 1541}, q of {1, 2, 3, 4, 6, 9}, K of {1, 5, 17, 33, 49, 65, 129, 256}, S of
# {1, 17, 65, 1025} (65: a wave's second sample tile; 1025: one past the default sample chunk).  With kp = K rounded up to 4 the
# matrix-unit kernel takes 64 rows per workgroup up to q kp of about 100, 32 up to about 165, 16 up to about 500, 16 rows in more than
# 64 KiB of LDS up to about 1250, and reads its fragments from global memory beyond: each of the five is here more than once.
SHAPES = [
    (1, 1, 1, 1, 0), (15, 2, 5, 17, 0), (16, 3, 17, 65, 0), (17, 4, 33, 17, 0), (293, 6, 49, 65, 2), (1541, 9, 65, 17, 0),
    (293, 4, 256, 17, 3), (1541, 6, 129, 17, 1), (293, 9, 256, 1, 0), (1541, 9, 129, 65, 2), (17, 6, 256, 1025, 0),
    (293, 3, 33, 1025, 0), (293, 1, 129, 65, 0), (16, 2, 1, 17, 0), (15, 9, 5, 65, 3), (1, 6, 17, 1, 0), (17, 3, 65, 1025, 1),
    (1541, 2, 49, 17, 2), (293, 4, 5, 17, 0), (1541, 1, 1, 65, 0), (16, 9, 256, 17, 0),
]


def expected_shape(q, K, S):
    """(rows, staged) the launcher must choose: the largest row block of 64, 32, 16 whose q planes (rows padded to 16 mod 32 doubles
    above 16) fit 64 KiB beside 2 x 8 bytes per sample of the chunk and 12 x 8 per row; else 16 rows in up to 160 KiB; else global."""
    kp, cs16 = 4 * ((K + 3) // 4), (min(S, 1024) + 15) // 16 * 16
    for rows, stride in ((64, 80), (32, 48), (16, 16)):
        if 8 * (q * kp * stride + 2 * cs16 + 12 * rows) <= 64 * 1024:
            return rows, 1
    return (16, 2) if 8 * (q * kp * 16 + 2 * cs16 + 12 * 16) <= 160 * 1024 else (16, 0)


def test_the_shapes_cover_every_value():
    assert {expected_shape(q, K, S) for _, q, K, S, _ in SHAPES} == {(64, 1), (32, 1), (16, 1), (16, 2), (16, 0)}
    for col, values in enumerate([{1, 15, 16, 17, 293, 1541}, {1, 2, 3, 4, 6, 9}, {1, 5, 17, 33, 49, 65, 129, 256}, {1, 17, 65, 1025},
                                  {0, 1, 2, 3}]):
        assert {s[col] for s in SHAPES} == values


@pytest.mark.parametrize("sign", ["mixed", "positive", "negative"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "m%d-q%d-K%d-S%d-g%d" % s)
def test_norm_exact_layout_on_integer_data(ctx, shape, sign):
    """Small integers: every u_i and every sum of squares is an exact integer below 2^53, so every field entry, statistic and
    envelope of both variants lies within one ulp of np.sqrt of the int64 value (the root is the one rounded operation), and with
    the threshold sqrt(N + 0.5), N an integer near the median of the sums of squares - at least about 0.25 / sqrt(N) away from
    every value - the exceedance counts must EQUAL the reference's."""
    m, q, K, S, grid_max = shape
    rng = np.random.default_rng(100000 * q + 1000 * m + 10 * K + S)
    if sign == "mixed":
        P, Cm = rng.integers(-7, 8, size=(K, q, m)), rng.integers(-7, 8, size=(K, S))
    else:
        P, Cm = rng.integers(1, 8, size=(K, q, m)), rng.integers(1, 8, size=(K, S))
        if sign == "negative":
            P = -P
    ref = evaluate_norm_reference(P, Cm, None)
    assert int(ref["SS"].max()) < 2 ** 53
    spread = np.sort(ref["SS"].reshape(-1))
    threshold = float(np.sqrt(float(spread[len(spread) // 2]) + 0.5))
    ref = evaluate_norm_reference(P, Cm, threshold)
    modes = upload_planes(ctx, P)

    def close(got, want):
        return np.all(np.abs(got - want) <= np.spacing(want))

    try:
        for name, variant in VARIANTS.items():
            with Knobs(ctx, variant=variant, grid_max=grid_max):
                out = run_norm_outputs(ctx, modes, q, Cm.astype(np.float64), m, threshold)
            assert ctx.eval_norm_last_shape() == (expected_shape(q, K, S) if variant else (64, 0)), name
            assert close(out["fields"], ref["V"].T), name
            assert close(out["stats"][0], ref["min"]) and close(out["stats"][1], ref["max"]), name
            assert np.array_equal(out["stats"][2], out["stats"][1]), name
            assert close(out["env_min"], ref["env_min"]) and close(out["env_max"], ref["env_max"]), name
            assert np.array_equal(out["exceed"], ref["exceed"]), name
    finally:
        free_all(ctx, modes)


@pytest.fixture(scope="module")
def float_case():
    """m = 1541, q = 6, K = 50, S = 100 of seeded normal data and its long-double reference, computed once."""
    m, q, K, S = 1541, 6, 50, 100
    rng = np.random.default_rng(20250911)
    P, Cm = rng.standard_normal((K, q, m)), rng.standard_normal((K, S))
    return m, q, K, S, P, Cm, evaluate_norm_reference(P, Cm, 7.0)


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_norm_knob_invariance_is_bitwise(ctx, float_case, variant):
    """Grid size and sample chunk change which workgroup and which launch sees a (row, sample) pair, never a bit of any output."""
    m, q, K, S, P, Cm, _ = float_case
    modes = upload_planes(ctx, P)
    try:
        base = None
        for grid_max in (0, 1, 2, 3):
            for chunk in (0, 16, 48):
                with Knobs(ctx, variant=VARIANTS[variant], grid_max=grid_max, chunk=chunk):
                    out = run_norm_outputs(ctx, modes, q, Cm, m, 7.0)
                if base is None:
                    base = out
                    continue
                for key in base:
                    assert np.array_equal(out[key].view(np.uint64), base[key].view(np.uint64)), (key, grid_max, chunk)
    finally:
        free_all(ctx, modes)


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_norm_floating_point_bound_and_agreement(ctx, float_case, variant):
    """|v - exact| inside the stage-2 bound of the reference (derived, not measured), and the statistics, envelopes and counts of
    the call are the extrema of the fields it returns."""
    m, q, K, S, P, Cm, ref = float_case
    modes = upload_planes(ctx, P)
    try:
        with Knobs(ctx, variant=VARIANTS[variant], grid_max=2, chunk=48):
            out = run_norm_outputs(ctx, modes, q, Cm, m, 7.0)
    finally:
        free_all(ctx, modes)
    bd = norm_bound(product_bound(K, ref["B"]), ref["V"])             # (m, S)
    err = np.abs(out["fields"].T.astype(LD) - ref["V"]).astype(np.float64)
    ratio = float((err / bd).max())
    print("eval_batch_norm %s: largest error / bound = %.4f" % (variant, ratio))
    assert ratio <= 1.0
    U = out["fields"]                                   # (S, m)
    assert np.array_equal(out["stats"][0], U.min(axis=1)) and np.array_equal(out["stats"][1], U.max(axis=1))
    assert np.array_equal(out["stats"][2], U.max(axis=1))
    assert np.array_equal(out["env_min"], U.min(axis=0)) and np.array_equal(out["env_max"], U.max(axis=0))
    assert np.array_equal(out["exceed"], (U > 7.0).sum(axis=0))


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_one_plane_is_the_absolute_value_of_eval_batch(ctx, variant):
    """q = 1: sqrt(u^2) of the very accumulators of pgd_eval_batch - within one ulp of |u| (the square and the root round)."""
    n, K, S = 293, 50, 37
    rng = np.random.default_rng(77)
    F, Cm = rng.standard_normal((K, 1, n)), rng.standard_normal((K, S))
    modes = upload_planes(ctx, F)
    fld, fld1 = ctx.vec_alloc(n * S), ctx.vec_alloc(n * S)
    try:
        with Knobs(ctx, variant=VARIANTS[variant]):
            ctx.eval_batch(modes, Cm, stats=False, fields=fld)
            ctx.eval_batch_norm(modes, 1, Cm, stats=False, fields=fld1)
        u, v = np.abs(ctx.vec_download(fld)), ctx.vec_download(fld1)
        assert np.all(np.abs(v - u) <= np.spacing(u))
    finally:
        free_all(ctx, modes + [fld, fld1])


def test_norm_partial_requests_write_only_what_was_asked(ctx, float_case):
    m, q, K, S, P, Cm, _ = float_case
    modes = upload_planes(ctx, P)
    emn, emx, exc = ctx.vec_alloc(m), ctx.vec_alloc(m), ctx.vec_alloc(m)
    try:
        full = run_norm_outputs(ctx, modes, q, Cm, m, 7.0)
        st = ctx.eval_batch_norm(modes, q, Cm, stats=True)
        assert np.array_equal(st, full["stats"])
        ctx.vec_fill(exc, POISON)
        assert ctx.eval_batch_norm(modes, q, Cm, stats=False, env_min=emn, env_max=emx) is None
        assert np.array_equal(ctx.vec_download(emn), full["env_min"]) and np.array_equal(ctx.vec_download(emx), full["env_max"])
        assert np.all(ctx.vec_download(exc) == POISON)
    finally:
        free_all(ctx, modes + [emn, emx, exc])


def test_norm_argument_errors_are_codes_and_messages(ctx):
    """Invalid calls only: each is refused with PGD_ERR_INVALID and a message before anything is launched."""
    m, q, K, S = 20, 2, 3, 5
    modes = [ctx.vec_from(np.ones(q * m)) for _ in range(K)]
    odd = [ctx.vec_from(np.ones(q * m + 1)) for _ in range(K)]
    short, emn, emx, exc, fld = ctx.vec_alloc(m - 1), ctx.vec_alloc(m), ctx.vec_alloc(m), ctx.vec_alloc(m), ctx.vec_alloc(m * S)
    cf = np.ones((K, S))
    st = np.full((3, S), -1.0)
    lib, PD = ctx.lib, _lib.PD

    def call(mlist, k, want, thr=0.0, stats=None, a=0, b=0, c=0, d=0, s=S, qq=q):
        arr = (_lib.H * max(len(mlist), 1))(*mlist)
        rc = lib.pgd_eval_batch_norm(ctx.h, arr, k, qq, cf.ctypes.data_as(PD), s, want, thr,
                                     stats.ctypes.data_as(PD) if stats is not None else None, a, b, c, d)
        return rc, lib.pgd_last_error(ctx.h).decode()

    try:
        for what, (rc, msg) in {
            "k = 0": call(modes, 0, 1, stats=st),
            "k = 257": call(modes * 86, 257, 1, stats=st),
            "s = 0": call(modes, K, 1, stats=st, s=0),
            "q = 0": call(modes, K, 1, stats=st, qq=0),
            "q = 10": call(modes, K, 1, stats=st, qq=10),
            "mode sizes not divisible by q": call(odd, K, 1, stats=st),
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
            "output aliasing a mode": call(modes, K, 2, a=modes[1], b=emx, qq=1),
            "outputs aliasing each other": call(modes, K, 2, a=emn, b=emn),
            "not a vector": call(modes[:2] + [987654], K, 1, stats=st),
        }.items():
            assert rc == -1 and msg.startswith("eval_batch_norm:"), (what, rc, msg)
        assert np.all(st == -1.0)                        # nothing ran
        # and the valid call right after them works: sqrt(2 * 3^2)
        assert np.allclose(ctx.eval_batch_norm(modes, q, cf), np.sqrt(18.0), rtol=2e-16, atol=0.0)
    finally:
        free_all(ctx, modes + odd + [short, emn, emx, exc, fld])


# ------------------------------------------------------------------------------------------------ frontend
@pytest.fixture()
def hip_frontend():
    from pgdrome_amd.hip_backend import HipBackend
    old = fem._backend
    fem.set_backend(HipBackend(0))
    fem.clear_caches()
    yield
    fem.set_backend(old)
    fem.clear_caches()


def frontend_case(monkeypatch, sol, quantity, scale):
    """The device path forced, then the host path forced: both inside the bound around the loop over evaluate()."""
    from pgdrome_amd import model
    coords = samples_of(sol, (1,), 17, 5)
    monkeypatch.setattr(model, "DEVICE_EVAL_MIN_DOFS", 0)
    calls = fem.STATS.get("eval_gradient_calls", 0)
    dev, _ = run_and_check(sol, [1], coords, quantity, scale)
    assert fem.STATS.get("eval_gradient_calls", 0) == calls + 1
    again = sol.evaluate_gradient_many(0, [1], coords, 0, quantity=quantity, scale=scale)
    assert fem.STATS.get("eval_gradient_calls", 0) == calls + 2 and np.array_equal(again.max, dev.max)
    monkeypatch.setattr(model, "DEVICE_EVAL_MIN_DOFS", 1 << 60)
    run_and_check(sol, [1], coords, quantity, scale)
    assert fem.STATS.get("eval_gradient_calls", 0) == calls + 2


def test_von_mises_of_the_elastic_block_through_the_frontend(hip_frontend, monkeypatch):
    from pgdrome_amd import problems
    from pgdrome_amd.solver import PGDProblem
    mesh = fem.BoxMesh(fem.Point(0, 0, 0), fem.Point(2, 1, 1), 4, 4, 4)
    p = PGDProblem(**problems.elastic_block(mesh, 7, PGD_nmax=3))
    p.solve_PGD(_problem="linear", settings={"relative_tolerance": 1e-11})
    frontend_case(monkeypatch, p.return_PGD(), "von_mises", two_valued(mesh, 1.0 / 1.3, 3.0 / 1.3))


def test_flux_of_reaction_diffusion_through_the_frontend(hip_frontend, monkeypatch):
    from pgdrome_amd import problems
    from pgdrome_amd.solver import PGDProblem
    mesh = fem.BoxMesh(fem.Point(0, 0, 0), fem.Point(1, 1, 1), 9, 9, 9)
    p = PGDProblem(**problems.reaction_diffusion(mesh, 17, PGD_nmax=3))
    p.solve_PGD(_problem="linear")
    frontend_case(monkeypatch, p.return_PGD(), "gradient_norm", None)
