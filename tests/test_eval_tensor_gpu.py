"""pgd_eval_batch_quantity, pgd_eval_batch_grad_quantity and pgd_eval_batch_grad_p2_quantity on the MI355X, through the C-ABI,
against tests/eval_tensor_reference.py: the eigenvalue kinds on hand-made planes of the tensor families (every tail of the row
block and the sample tile, both variants) inside the bound |e| + 48 u (|sigma|_F + |e|), kinds 0 and 1 bit for bit the calls they
restate, bitwise knob invariance, the fused calls on nodal data, the refusals - and PGD.evaluate_gradient_many through the frontend
for "max_principal", "min_principal", "tresca" and "stress_component"."""
import itertools

import numpy as np
import pytest

from pgdrome_amd import _lib, fem
from tests.eval_gradient_fused_reference import KEYS, POISON, Layouts, _outputs, run_fused, upload_nodal
from tests.eval_gradient_p2_reference import plane_bound_p2, planes_p2
from tests.eval_gradient_reference import plane_bound, planes, product_bound, samples_of, two_valued
from tests.eval_many_reference import U53
from tests.eval_tensor_reference import (EIG_MAX, EIG_MIN, EIG_SPREAD, NORM, VALUE, family_pool, frobenius, planes_of, run_and_check_tensor,
                                         tensor_bound, value_reference)
from tests.test_eval_gradient_gpu import run_norm_outputs, upload_planes
from tests.test_eval_many_gpu import VARIANTS, Knobs, free_all

pytestmark = pytest.mark.gpu

P = fem.Point
EIG_KINDS = (EIG_MAX, EIG_MIN, EIG_SPREAD)


def run_quantity(ctx, modes, q, kind, Cm, m, threshold):
    """Every output of one pgd_eval_batch_quantity call (fields as (S, m))."""
    Cm = np.asarray(Cm, dtype=np.float64)
    return _outputs(ctx, m, Cm.shape[1], lambda emn, emx, exc, fld: ctx.eval_batch_quantity(
        modes, q, kind, Cm, stats=True, env_min=emn, env_max=emx, exceed=exc, threshold=threshold, fields=fld))


def check_outputs(out, V, Bd, threshold, tag):
    """The outputs of one call against V (S, m) within Bd (S, m), and against each other: the statistics, envelopes and counts are
    those of the fields the call returns; row 2 of the statistics is max |v|."""
    assert not isinstance(out["stats"], Exception), (tag, out["stats"])
    F = out["fields"]
    assert F.shape == V.shape
    worst = np.abs(F - V) - Bd
    assert np.all(worst <= 0.0), (tag, float(worst.max()), np.unravel_index(np.argmax(worst), worst.shape))
    assert np.array_equal(out["stats"][0], F.min(axis=1)) and np.array_equal(out["stats"][1], F.max(axis=1)), tag
    assert np.array_equal(out["stats"][2], np.abs(F).max(axis=1)), tag
    assert np.array_equal(out["env_min"], F.min(axis=0)) and np.array_equal(out["env_max"], F.max(axis=0)), tag
    assert np.array_equal(out["exceed"], (F > threshold).sum(axis=0)), tag


# ------------------------------------------------------------------------------------------------ hand-made planes
@pytest.fixture(scope="module")
def pools():
    return {4: family_pool(4, True), 6: family_pool(6, False)}


@pytest.mark.parametrize("S", [1, 5, 33])
@pytest.mark.parametrize("q", [4, 6])
@pytest.mark.parametrize("m", [1, 17, 67, 130])
def test_eigenvalues_of_the_tensor_families(ctx, pools, m, q, S):
    """K = 1 and coefficients that are powers of two: the combined planes are exact, the bound is 48 u |sigma|_F (96 for the
    spread).  Entry e holds tensor e + shift of the pool (random, rotated uniaxial, close pairs at gaps 1e-3 .. 1e-15, hydrostatic
    + noise, offset 1e6, zero) times 1 + 3 e / 8, sample j the factor 2^(j - 16): a value at the wrong entry or sample is far
    outside the bound.  m: one entry, one past a 16-row tile, 67 = 4 tiles and 3, 130 = more than two plain workgroups' worth;
    S: one sample, a partial tile, a third tile.  All three kinds, the matrix unit and the plain kernels."""
    pool = pools[q]
    shift = 5 * q + S                                                # (m = 1: another tensor of the pool per case)
    T = pool[(np.arange(m) + shift) % len(pool)] * (1.0 + 0.375 * np.arange(m))[:, None, None]
    Pm = planes_of(T, q)[None]                                        # (1, q, m)
    Cm = (2.0 ** (np.arange(S) - 16.0))[None, :]
    U = Pm[0][:, :, None] * Cm[0][None, None, :]                      # (q, m, S), exact
    modes = upload_planes(ctx, Pm)
    try:
        for kind, (name, variant) in itertools.product(EIG_KINDS, VARIANTS.items()):
            V = value_reference(U, kind).T                            # (S, m)
            Bd = tensor_bound(np.zeros_like(U), U, kind).T
            threshold = float(np.median(V))
            with Knobs(ctx, variant=variant):
                out = run_quantity(ctx, modes, q, kind, Cm, m, threshold)
            assert ctx.eval_norm_last_shape() == ((16, 1) if variant else (64, 0)), (kind, name)
            check_outputs(out, V, Bd, threshold, (kind, name))
            if kind == EIG_SPREAD:
                assert np.all(out["fields"] >= 0.0)
    finally:
        free_all(ctx, modes)


def test_worst_error_in_units(ctx, pools):
    """Report: the largest |v - eigvalsh| / (u |sigma|_F) over the pool, per kind (the bound allows 48)."""
    pool = np.concatenate([pools[6]] * 8)
    Pm = planes_of(pool, 6)[None]
    modes = upload_planes(ctx, Pm)
    nf = frobenius(Pm[0])
    try:
        for kind in (EIG_MAX, EIG_MIN):
            out = run_quantity(ctx, modes, 6, kind, np.ones((1, 1)), len(pool), 0.0)
            err = np.abs(out["fields"][0] - value_reference(Pm[0], kind)) / (U53 * np.where(nf > 0, nf, 1.0))
            print("kind %d: largest error %.2f u |sigma|_F" % (kind, err.max()))
            assert err.max() <= 48.0
    finally:
        free_all(ctx, modes)


# ------------------------------------------------------------------------------------------------ bitwise
@pytest.fixture(scope="module")
def float_planes():
    m, q, K, S = 293, 6, 40, 50
    rng = np.random.default_rng(20261020)
    return m, q, K, S, rng.standard_normal((K, q, m)), rng.standard_normal((K, S))


def same_bits(a, b):
    return all(np.array_equal(a[k].view(np.uint64), b[k].view(np.uint64)) for k in KEYS)


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_kind_0_is_the_norm_call_and_kind_1_is_eval_batch(ctx, float_planes, variant):
    m, q, K, S, Pm, Cm = float_planes
    modes, one = upload_planes(ctx, Pm), upload_planes(ctx, Pm[:, :1])
    try:
        with Knobs(ctx, variant=VARIANTS[variant], grid_max=3, chunk=32):
            assert same_bits(run_quantity(ctx, modes, q, NORM, Cm, m, 2.0), run_norm_outputs(ctx, modes, q, Cm, m, 2.0))
            signed = run_quantity(ctx, one, 1, VALUE, Cm, m, 0.25)
            plain = _outputs(ctx, m, S, lambda a, b, c, d: ctx.eval_batch(one, Cm, stats=True, env_min=a, env_max=b, exceed=c,
                                                                           threshold=0.25, fields=d))
            assert same_bits(signed, plain)
            assert np.any(signed["fields"] < 0) and np.array_equal(signed["stats"][2], np.abs(signed["fields"]).max(axis=1))
    finally:
        free_all(ctx, modes + one)


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_kind_0_of_the_fused_calls_is_the_fused_calls(ctx, variant):
    mesh = fem.BoxMesh(P(0, 0, 0), P(0.5, 1.48, 1.0), 5, 4, 3)
    rng = np.random.default_rng(3)
    K, S = 7, 20
    Cm, L = rng.standard_normal((K, S)), rng.standard_normal((6, 9))
    for degree in (1, 2):
        lay = fem.DofLayout(mesh, degree)
        X, rec = (mesh.coordinates(), mesh.cells()) if degree == 1 else (lay.coords, lay.cells)
        nc = rec.shape[0]
        U = rng.standard_normal((K, X.shape[0], 3))
        lam = np.eye(4)
        with Layouts(ctx, X, rec) as lays:
            modes = upload_nodal(ctx, U)
            try:
                with Knobs(ctx, variant=VARIANTS[variant]):
                    if degree == 1:
                        old = run_fused(ctx, lays[3], modes, L, Cm, nc, 1.0)
                        new = _outputs(ctx, nc, S, lambda a, b, c, d: ctx.eval_batch_grad_quantity(
                            lays[3], modes, L, NORM, Cm, stats=True, env_min=a, env_max=b, exceed=c, threshold=1.0, fields=d))
                    else:
                        old = _outputs(ctx, 4 * nc, S, lambda a, b, c, d: ctx.eval_batch_grad_p2(
                            lays[3], modes, lam, L, Cm, stats=True, env_min=a, env_max=b, exceed=c, threshold=1.0, fields=d))
                        new = _outputs(ctx, 4 * nc, S, lambda a, b, c, d: ctx.eval_batch_grad_p2_quantity(
                            lays[3], modes, lam, L, NORM, Cm, stats=True, env_min=a, env_max=b, exceed=c, threshold=1.0, fields=d))
                assert not isinstance(old["stats"], Exception) and same_bits(old, new)
            finally:
                free_all(ctx, modes)


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_knob_invariance_is_bitwise(ctx, float_planes, variant):
    """Sample chunk and grid cap change which launch and workgroup sees a pair; modes of zeros appended up to K = 128 and 256 move
    the planes of a row block from 64 KiB of LDS to more and to global memory: never a bit of any output."""
    m, q, K, S, Pm, Cm = float_planes
    modes = upload_planes(ctx, Pm)
    zeros = [ctx.vec_from(np.zeros(q * m)) for _ in range(256 - K)]
    try:
        base = None
        for grid_max, chunk in ((0, 0), (1, 16), (3, 48), (2, 0)):
            with Knobs(ctx, variant=VARIANTS[variant], grid_max=grid_max, chunk=chunk):
                out = run_quantity(ctx, modes, q, EIG_MAX, Cm, m, 1.0)
            base = base or out
            assert same_bits(out, base), (grid_max, chunk)
        assert ctx.eval_norm_last_shape() == ((16, 1) if VARIANTS[variant] else (64, 0))
        for Kp, staged in ((128, 2), (256, 0)):
            Cp = np.concatenate([Cm, np.ones((Kp - K, S))])
            with Knobs(ctx, variant=VARIANTS[variant]):
                out = run_quantity(ctx, modes + zeros[:Kp - K], q, EIG_MAX, Cp, m, 1.0)
            assert ctx.eval_norm_last_shape() == ((16, staged) if VARIANTS[variant] else (64, 0))
            assert same_bits(out, base), Kp
    finally:
        free_all(ctx, modes + zeros)


# ------------------------------------------------------------------------------------------------ the fused calls
def fused_reference(P_modes, b_modes, Cm, kind):
    """V (S, entries) and the bound from the planes per mode P (K, q, entries; long double) and their stage-1 bounds b: a code that
    forms the planes per mode and combines them has u_i off by e_i = sum_t |c_t| b_t,i + product_bound(K, sum_t |c_t| (|P_t,i| + b_t,i))."""
    K = len(P_modes)
    Pf = np.asarray(P_modes).astype(np.float64)
    U = np.einsum("tie,ts->ies", np.asarray(P_modes), Cm.astype(np.longdouble)).astype(np.float64)
    ca = np.abs(Cm)
    e = np.einsum("tie,ts->ies", b_modes, ca) + product_bound(K, np.einsum("tie,ts->ies", np.abs(Pf) + b_modes, ca)) + U53 * np.abs(U)
    return value_reference(U, kind).T, tensor_bound(e, U, kind).T


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", ["box 5x4x3", "crossed 6x5"])
def test_fused_calls_on_nodal_data(ctx, name, variant):
    """Fused P1, fused P2 at the midpoint and at the G + 1 vertices, every eigenvalue kind and a signed component, on stretched
    meshes with a cell-wise scale: inside the bound built from the planes' bounds."""
    mesh = fem.BoxMesh(P(0, 0, 0), P(0.5, 1.48, 1.0), 5, 4, 3) if name.startswith("box") else \
        fem.RectangleMesh(P(0, 0), P(0.6, 1.85), 6, 5, "crossed")
    G = mesh.topology().dim()
    q = 4 if G == 2 else 6
    rng = np.random.default_rng(G)
    K, S = 5, 21
    Cm = rng.standard_normal((K, S))
    L = rng.standard_normal((q, G * G))
    for degree, lam in ((1, None), (2, np.full((1, G + 1), 1.0 / (G + 1))), (2, np.eye(G + 1))):
        lay = fem.DofLayout(mesh, degree)
        X, rec = (mesh.coordinates(), mesh.cells()) if degree == 1 else (lay.coords, lay.cells)
        nc = rec.shape[0]
        npt = 1 if lam is None else len(lam)
        U = rng.standard_normal((K, X.shape[0], G))
        scale = rng.uniform(0.5, 2.0, nc)
        flat = lambda p: np.asarray(p).reshape(p.shape[0], -1)
        with Layouts(ctx, X, rec) as lays:
            modes, sc = upload_nodal(ctx, U), ctx.vec_from(scale)
            try:
                for kind in EIG_KINDS + (VALUE,):
                    Lk = L if kind != VALUE else L[1:2]
                    if lam is None:
                        Pm = [planes(X, rec, U[k], Lk, scale) for k in range(K)]
                        bm = np.stack([plane_bound(X, rec, U[k], Lk, scale) for k in range(K)])
                        call = lambda a, b, c, d: ctx.eval_batch_grad_quantity(
                            lays[G], modes, Lk, kind, Cm, scale=sc, stats=True, env_min=a, env_max=b, exceed=c, threshold=thr, fields=d)
                    else:
                        Pm = [flat(planes_p2(X, rec, U[k], lam, Lk, scale)) for k in range(K)]
                        bm = np.stack([flat(plane_bound_p2(X, rec, U[k], lam, Lk, scale)) for k in range(K)])
                        call = lambda a, b, c, d: ctx.eval_batch_grad_p2_quantity(
                            lays[G], modes, lam, Lk, kind, Cm, scale=sc, stats=True, env_min=a, env_max=b, exceed=c, threshold=thr, fields=d)
                    V, Bd = fused_reference(Pm, bm, Cm, kind)
                    thr = float(np.median(V))
                    with Knobs(ctx, variant=VARIANTS[variant], grid_max=3, chunk=16):
                        out = _outputs(ctx, npt * nc, S, call)
                    check_outputs(out, V, Bd, thr, (degree, npt, kind))
            finally:
                free_all(ctx, modes + [sc])


# ------------------------------------------------------------------------------------------------ refusals
def test_argument_errors_are_codes_and_messages(ctx):
    mesh = fem.RectangleMesh(P(0, 0), P(3, 2), 3, 2)
    X, cells = mesh.coordinates(), mesh.cells()
    p2 = fem.DofLayout(mesh, 2)
    nc, nv, K, S, m = cells.shape[0], X.shape[0], 2, 3, 10
    lib, PD = ctx.lib, _lib.PD
    cf, st = np.ones((K, S)), np.full((3, S), -1.0)
    L, lam = np.ones((6, 4)), np.eye(3)
    ptr = lambda a: a.ctypes.data_as(PD)
    planes6, planes1 = [ctx.vec_from(np.ones(6 * m)) for _ in range(K)], [ctx.vec_from(np.ones(m)) for _ in range(K)]
    nodal, nodal2 = [ctx.vec_from(np.ones(2 * nv)) for _ in range(K)], [ctx.vec_from(np.ones(2 * p2.n)) for _ in range(K)]
    arr = lambda hs: (_lib.H * len(hs))(*hs)
    with Layouts(ctx, X, cells) as l1, Layouts(ctx, p2.coords, p2.cells) as l2:
        def stored(modes, q, kind):
            return lib.pgd_eval_batch_quantity(ctx.h, arr(modes), K, q, kind, ptr(cf), S, 1, 0.0, ptr(st), 0, 0, 0, 0)

        def fused(q, kind, want=1):
            return lib.pgd_eval_batch_grad_quantity(ctx.h, l1[2], arr(nodal), K, ptr(L), q, kind, 0, ptr(cf), S, want, 0.0, ptr(st), 0, 0, 0, 0)

        def fused_p2(q, kind, npt=3):
            return lib.pgd_eval_batch_grad_p2_quantity(ctx.h, l2[2], arr(nodal2), K, ptr(lam), npt, ptr(L), q, kind, 0, ptr(cf), S, 1, 0.0,
                                                       ptr(st), 0, 0, 0, 0)
        try:
            cases = {
                "eval_batch_quantity": [lambda: stored(planes6, 6, 5), lambda: stored(planes6, 6, -1), lambda: stored(planes6, 6, VALUE),
                                        lambda: stored(planes6, 3, EIG_MAX), lambda: stored(planes1, 1, EIG_SPREAD),
                                        lambda: stored(planes6, 0, NORM), lambda: stored(planes1, 4, EIG_MIN)],      # (m is no multiple of 4)
                "eval_batch_grad_quantity": [lambda: fused(6, 5), lambda: fused(4, VALUE), lambda: fused(5, EIG_MAX), lambda: fused(10, NORM),
                                             lambda: fused(6, EIG_MAX, want=0)],
                "eval_batch_grad_p2_quantity": [lambda: fused_p2(6, 7), lambda: fused_p2(6, VALUE), lambda: fused_p2(3, EIG_MIN),
                                                lambda: fused_p2(6, EIG_MAX, npt=5)],
            }
            for fn, calls in cases.items():
                for i, call in enumerate(calls):
                    rc = call()
                    msg = lib.pgd_last_error(ctx.h).decode()
                    assert rc == -1 and msg.startswith(fn + ":"), (fn, i, rc, msg)
            assert np.all(st == -1.0)                        # nothing ran
            # and valid calls right after them: sigma = 2 * (all-ones tensor) has the eigenvalues 6, 0, 0
            assert stored(planes6, 6, EIG_MAX) == 0 and np.allclose(st[:2], 6.0, rtol=1e-14)
            assert stored(planes6, 6, EIG_SPREAD) == 0 and np.allclose(st[:2], 6.0, rtol=1e-14)
            assert fused(4, EIG_MIN) == 0 and fused_p2(4, EIG_MAX) == 0
        finally:
            free_all(ctx, planes6 + planes1 + nodal + nodal2)


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


NU = 0.3
QUANTITIES = [("max_principal", None), ("min_principal", None), ("tresca", None), ("stress_component", (0, 1))]


def _elastic(degree, n=4):
    from pgdrome_amd import problems
    from pgdrome_amd.solver import PGDProblem
    mesh = fem.BoxMesh(P(0, 0, 0), P(2, 1, 1), n, n, n)                        # 5^3 vertices
    p = PGDProblem(**problems.elastic_block(mesh, 5, PGD_nmax=2, degree=degree))
    p.solve_PGD(_problem="linear", settings={"relative_tolerance": 1e-11})
    return mesh, p.return_PGD()


@pytest.mark.parametrize("degree", [1, 2])
def test_stress_quantities_through_the_frontend(hip_frontend, monkeypatch, degree):
    """elastic_block, every quantity, stored and fused on the device (P2: at the midpoint and at the vertices), a float E and a
    graded DG0 E, inside the bound around the loop evaluate -> gradient -> eigvalsh; the counters say the device ran."""
    from pgdrome_amd import model
    mesh, sol = _elastic(degree)
    monkeypatch.setattr(model, "DEVICE_EVAL_MIN_DOFS", 0)
    coords = samples_of(sol, (1,), 9, 5)
    graded = two_valued(mesh, 70.0, 210.0)
    for at in ((None,) if degree == 1 else ("midpoint", "vertices")):
        for quantity, comp in QUANTITIES:
            for planes_, counter in (("stored", "eval_gradient_calls"), ("fused", "eval_gradient_fused_calls")):
                n0, b0 = fem.STATS.get(counter, 0), fem.STATS.get("gradient_mode_builds", 0)
                run_and_check_tensor(sol, [1], coords, quantity, NU, 210.0, comp, at=at, planes=planes_)
                run_and_check_tensor(sol, [1], coords, quantity, NU, graded, comp, at=at, planes=planes_)
                assert fem.STATS.get(counter, 0) == n0 + 2
                assert fem.STATS.get("gradient_mode_builds", 0) == b0 + (2 if planes_ == "stored" else 0)
    # the host path gives the same numbers within the two bounds: checked against the same reference
    monkeypatch.setattr(model, "DEVICE_EVAL_MIN_DOFS", 1 << 60)
    n0 = fem.STATS.get("eval_gradient_calls", 0)
    run_and_check_tensor(sol, [1], coords, "max_principal", NU, graded, at=None if degree == 1 else "midpoint")
    assert fem.STATS.get("eval_gradient_calls", 0) == n0
