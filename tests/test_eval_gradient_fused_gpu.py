"""pgd_eval_batch_grad on the MI355X, through the C-ABI: the planes of pgd_cell_gradient formed inside the batch evaluation, never
stored.  Exact on integer data (cell records, blocked layouts, padded last block, mode rows beyond k, every row block, the refusal
beyond 160 KiB), inside the derived rounding bound on floating-point data, bit-identical across grid sizes and sample chunks, equal
to the two stored stages on integers - and PGD.evaluate_gradient_many(planes="fused" / "auto") through the frontend."""

import numpy as np
import pytest

from pgdrome_amd import _lib, fem
from tests.eval_gradient_fused_reference import (KEYS, POISON, Layouts, assert_integer_outputs, float_reference, integer_data,
                                                 integer_reference, run_fused, run_stored, upload_nodal)
from tests.eval_gradient_reference import LD, run_and_check, samples_of, two_valued
from tests.test_eval_gradient_gpu import MESHES, STEPS, expected_shape
from tests.test_eval_many_gpu import VARIANTS, Knobs, free_all

pytestmark = pytest.mark.gpu

KS = (1, 5, 17)
SS = (1, 17, 65)


def layout_cases(G):
    """(ncomp, q): ncomp 1, 2, 3 and every q of {1, 3, 6, 9} that ncomp * G allows."""
    return [(ncomp, q) for ncomp in (1, 2, 3) for q in (1, 3, 6, 9) if q == 1 or q <= ncomp * G]


# ------------------------------------------------------------------------------------------------ 1. exact on integers
@pytest.mark.parametrize("name", list(MESHES))
def test_exact_on_integer_data(ctx, name):
    """Unit-step meshes, small integers everywhere: the planes are exact integers (as the stage-1 test has them), so are the u_i and
    the sums of squares (< 2^53, asserted), and every field entry, statistic and envelope of both variants lies within one ulp of
    np.sqrt of the int64 value; the exceedance counts at sqrt(N + 0.5) must EQUAL the reference's.  72 cells (box72) and 7 (interval7)
    end in a padded block, K = 1, 5, 17 leave padded mode rows, box360 spans several workgroups."""
    X, cells = MESHES[name].coordinates(), MESHES[name].cells()
    nc, nv, G = cells.shape[0], X.shape[0], cells.shape[1] - 1
    rng = np.random.default_rng(7000 + nc)
    n = 0
    with Layouts(ctx, X, cells) as lay:
        for ncomp, q in layout_cases(G):
            for with_scale in (False, True):
                U, L, scale, Cm = integer_data(rng, nv, nc, G, ncomp, q, max(KS), max(SS), with_scale)
                modes = upload_nodal(ctx, U)
                sc = ctx.vec_from(scale.astype(np.float64)) if with_scale else 0
                try:
                    for K in KS:
                        for S in SS:
                            ref, thr = integer_reference(X, cells, U[:K], L, scale, Cm[:K, :S])
                            for vname, variant in VARIANTS.items():
                                for grid_max in (0, 2):
                                    with Knobs(ctx, variant=variant, grid_max=grid_max):
                                        out = run_fused(ctx, lay[ncomp], modes[:K], L, Cm[:K, :S], nc, thr, sc)
                                    assert_integer_outputs(out, ref, (name, ncomp, q, with_scale, K, S, vname, grid_max))
                                    n += 1
                finally:
                    free_all(ctx, modes + ([sc] if with_scale else []))
    assert n == len(layout_cases(G)) * 2 * 9 * 4


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_exact_one_sample_past_the_default_chunk(ctx, variant):
    X, cells = MESHES["box72"].coordinates(), MESHES["box72"].cells()
    nc, nv = cells.shape[0], X.shape[0]
    U, L, scale, Cm = integer_data(np.random.default_rng(1025), nv, nc, 3, 3, 6, 5, 1025, True)
    ref, thr = integer_reference(X, cells, U, L, scale, Cm)
    with Layouts(ctx, X, cells) as lay:
        modes, sc = upload_nodal(ctx, U), ctx.vec_from(scale.astype(np.float64))
        try:
            with Knobs(ctx, variant=VARIANTS[variant]):
                out = run_fused(ctx, lay[3], modes, L, Cm, nc, thr, sc)
            assert_integer_outputs(out, ref, variant)
        finally:
            free_all(ctx, modes + [sc])


# ------------------------------------------------------------------------------------------------ 2. every row block
ROW_BLOCKS = {(3, 17): (64, 1), (6, 21): (32, 1), (9, 49): (16, 1), (9, 129): (16, 2)}


def box360_integer_case(ctx, lay, q, K, S=17):
    X, cells = MESHES["box360"].coordinates(), MESHES["box360"].cells()
    nc, nv = cells.shape[0], X.shape[0]
    U, L, scale, Cm = integer_data(np.random.default_rng(100 * q + K), nv, nc, 3, 3, q, K, S, True)
    ref, thr = integer_reference(X, cells, U, L, scale, Cm)
    return nc, U, L, scale, Cm, ref, thr


@pytest.mark.parametrize("qk", list(ROW_BLOCKS), ids=lambda qk: "q%d-K%d" % qk)
def test_every_row_block(ctx, qk):
    """64, 32, 16 cells in at most 64 KiB and 16 cells in more (the kernel's own LDS attribute): the rule of the stored path."""
    q, K = qk
    assert expected_shape(q, K, 17) == ROW_BLOCKS[qk]
    X, cells = MESHES["box360"].coordinates(), MESHES["box360"].cells()
    with Layouts(ctx, X, cells) as lay:
        nc, U, L, scale, Cm, ref, thr = box360_integer_case(ctx, lay, q, K)
        modes, sc = upload_nodal(ctx, U), ctx.vec_from(scale.astype(np.float64))
        try:
            for grid_max in (0, 2):
                with Knobs(ctx, variant=1, grid_max=grid_max):
                    out = run_fused(ctx, lay[3], modes, L, Cm, nc, thr, sc)
                assert ctx.eval_norm_last_shape() == ROW_BLOCKS[qk]
                assert_integer_outputs(out, ref, (qk, grid_max))
        finally:
            free_all(ctx, modes + [sc])


def test_beyond_the_lds_limit_is_refused_and_the_plain_variant_runs(ctx):
    """q = 9, K = 256: q * kp = 2304 rows of 16 cells are 295 KiB.  The matrix-unit variant refuses with PGD_ERR_LIMIT and a message
    naming q and k before anything is launched (every output still poisoned); the plain variant has no such limit and is exact."""
    q, K = 9, 256
    assert expected_shape(q, K, 17) == (16, 0)
    X, cells = MESHES["box360"].coordinates(), MESHES["box360"].cells()
    with Layouts(ctx, X, cells) as lay:
        nc, U, L, scale, Cm, ref, thr = box360_integer_case(ctx, lay, q, K)
        modes, sc = upload_nodal(ctx, U), ctx.vec_from(scale.astype(np.float64))
        try:
            with Knobs(ctx, variant=1):
                out = run_fused(ctx, lay[3], modes, L, Cm, nc, thr, sc)
            err = out["stats"]
            assert isinstance(err, _lib.PgdError) and err.code == -4, err
            assert "eval_batch_grad:" in str(err) and "q = 9" in str(err) and "k = 256" in str(err) and str(160 * 1024) in str(err)
            for key in KEYS[1:]:
                assert np.all(out[key] == POISON), key
            with Knobs(ctx, variant=0):
                out = run_fused(ctx, lay[3], modes, L, Cm, nc, thr, sc)
            assert ctx.eval_norm_last_shape() == (64, 0)
            assert_integer_outputs(out, ref, "plain")
        finally:
            free_all(ctx, modes + [sc])


# ------------------------------------------------------------------------------------------------ 3. - 5. floating point
THR = 20.0


@pytest.fixture(scope="module")
def float_case():
    """box360 stretched by (0.1, 0.37, 1 / 3), ncomp = 3, q = 6, K = 50, S = 100 of seeded normal data with a normal scale, and its
    long-double reference with the bound, computed once."""
    cells = MESHES["box360"].cells()
    X = MESHES["box360"].coordinates() * STEPS[None, :]
    nc, nv, K, S, q = cells.shape[0], X.shape[0], 50, 100, 6
    rng = np.random.default_rng(20251019)
    U, L = rng.standard_normal((K, nv, 3)), rng.standard_normal((q, 9))
    scale, Cm = rng.standard_normal(nc), rng.standard_normal((K, S))
    ref, bd = float_reference(X, cells, U, L, scale, Cm, THR)
    return {"X": X, "cells": cells, "nc": nc, "U": U, "L": L, "scale": scale, "Cm": Cm, "ref": ref, "bd": bd}


class FloatOnDevice:
    def __init__(self, ctx, case):
        self.ctx, self.case = ctx, case

    def __enter__(self):
        ctx, c = self.ctx, self.case
        self.lay = Layouts(ctx, c["X"], c["cells"])
        self.modes, self.sc = upload_nodal(ctx, c["U"]), ctx.vec_from(c["scale"])
        return self

    def __exit__(self, *exc):
        free_all(self.ctx, self.modes + [self.sc])
        self.lay.__exit__()

    def fused(self):
        c = self.case
        return run_fused(self.ctx, self.lay[3], self.modes, c["L"], c["Cm"], c["nc"], THR, self.sc)

    def stored(self):
        c = self.case
        return run_stored(self.ctx, self.lay[3], self.modes, c["L"], c["Cm"], c["nc"], THR, self.sc)


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_floating_point_bound_and_consistency(ctx, float_case, variant):
    """Every field entry inside the derived bound around the long-double reference; the statistics, envelopes and counts of the call
    are the extrema of the fields it returns."""
    with FloatOnDevice(ctx, float_case) as dev:
        with Knobs(ctx, variant=VARIANTS[variant], grid_max=2, chunk=48):
            out = dev.fused()
    ref, bd = float_case["ref"], float_case["bd"]
    err = np.abs(out["fields"].T.astype(LD) - ref["V"]).astype(np.float64)
    ratio = float((err / bd).max())
    print("eval_batch_grad %s: largest error / bound = %.4f" % (variant, ratio))
    assert ratio <= 1.0
    F = out["fields"]                                   # (S, cells)
    assert np.array_equal(out["stats"][0], F.min(axis=1)) and np.array_equal(out["stats"][1], F.max(axis=1))
    assert np.array_equal(out["stats"][2], F.max(axis=1))
    assert np.array_equal(out["env_min"], F.min(axis=0)) and np.array_equal(out["env_max"], F.max(axis=0))
    assert np.array_equal(out["exceed"], (F > THR).sum(axis=0))
    assert 0 < out["exceed"].sum() < F.size             # (the threshold separates something)


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_knob_invariance_is_bitwise(ctx, float_case, variant):
    """Grid size and sample chunk change which workgroup and which launch sees a (cell, sample) pair, never a bit of any output."""
    with FloatOnDevice(ctx, float_case) as dev:
        base = None
        for grid_max in (0, 1, 2, 3):
            for chunk in (0, 16, 48):
                with Knobs(ctx, variant=VARIANTS[variant], grid_max=grid_max, chunk=chunk):
                    out = dev.fused()
                if base is None:
                    base = out
                    continue
                for key in KEYS:
                    assert np.array_equal(out[key].view(np.uint64), base[key].view(np.uint64)), (key, grid_max, chunk)


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name,ncomp,q", [("interval7", 3, 3), ("rect-crossed", 3, 6), ("box72", 3, 9), ("box360", 2, 6)])
def test_fused_equals_stored_on_integer_data(ctx, name, ncomp, q, variant):
    X, cells = MESHES[name].coordinates(), MESHES[name].cells()
    nc, nv, G = cells.shape[0], X.shape[0], cells.shape[1] - 1
    U, L, scale, Cm = integer_data(np.random.default_rng(nc + q), nv, nc, G, ncomp, q, 17, 65, True)
    with Layouts(ctx, X, cells) as lay:
        modes, sc = upload_nodal(ctx, U), ctx.vec_from(scale.astype(np.float64))
        try:
            with Knobs(ctx, variant=VARIANTS[variant]):
                a, b = run_fused(ctx, lay[ncomp], modes, L, Cm, nc, 100.5, sc), run_stored(ctx, lay[ncomp], modes, L, Cm, nc, 100.5, sc)
            for key in KEYS:
                assert np.array_equal(a[key], b[key]), key
        finally:
            free_all(ctx, modes + [sc])


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_fused_against_stored_on_floating_point_data(ctx, float_case, variant):
    """Both paths derive the planes per mode and combine them: each lies inside the same bound around the reference, so they differ
    by at most its double.  Whether they are bit-identical is printed, not asserted (the compiler may contract the per-cell
    arithmetic differently in the two kernels)."""
    with FloatOnDevice(ctx, float_case) as dev:
        with Knobs(ctx, variant=VARIANTS[variant]):
            a, b = dev.fused(), dev.stored()
    bd = float_case["bd"]                               # (cells, S)
    print("eval_batch_grad %s: fused and stored bit-identical: %s" % (variant, all(np.array_equal(a[k], b[k]) for k in KEYS)))
    assert np.all(np.abs(a["fields"] - b["fields"]) <= 2.0 * bd.T)
    assert np.all(np.abs(a["stats"][:2] - b["stats"][:2]) <= 2.0 * bd.max(axis=0)[None, :])
    for key in ("env_min", "env_max"):
        assert np.all(np.abs(a[key] - b[key]) <= 2.0 * bd.max(axis=1))


# ------------------------------------------------------------------------------------------------ 6. partial requests, errors
def test_partial_requests_write_only_what_was_asked(ctx, float_case):
    c = float_case
    nc = c["nc"]
    with FloatOnDevice(ctx, c) as dev:
        full = dev.fused()
        emn, emx, exc = ctx.vec_alloc(nc), ctx.vec_alloc(nc), ctx.vec_alloc(nc)
        try:
            st = ctx.eval_batch_grad(dev.lay[3], dev.modes, c["L"], c["Cm"], scale=dev.sc, stats=True)
            assert np.array_equal(st, full["stats"])
            for v in (emn, emx, exc):
                ctx.vec_fill(v, POISON)
            assert ctx.eval_batch_grad(dev.lay[3], dev.modes, c["L"], c["Cm"], scale=dev.sc, stats=False, env_min=emn, env_max=emx) is None
            assert np.array_equal(ctx.vec_download(emn), full["env_min"]) and np.array_equal(ctx.vec_download(emx), full["env_max"])
            assert np.all(ctx.vec_download(exc) == POISON)
            for v in (emn, emx):
                ctx.vec_fill(v, POISON)
            assert ctx.eval_batch_grad(dev.lay[3], dev.modes, c["L"], c["Cm"], scale=dev.sc, stats=False, exceed=exc, threshold=THR) is None
            assert np.array_equal(ctx.vec_download(exc), full["exceed"])
            assert np.all(ctx.vec_download(emn) == POISON) and np.all(ctx.vec_download(emx) == POISON)
        finally:
            free_all(ctx, [emn, emx, exc])


def test_argument_errors_are_codes_and_messages(ctx):
    """Invalid calls only: each is refused with PGD_ERR_INVALID and a message before anything is launched.  rect-right 3 x 2 has as
    many nodes as cells (12), so a scalar mode has the size of an output and can alias one."""
    mesh = MESHES["rect-right"]
    X, cells = mesh.coordinates(), mesh.cells()
    nc, nv, K, S, q = cells.shape[0], X.shape[0], 3, 5, 2
    assert nc == nv
    base = ctx.mesh_upload(X, cells)
    blocked = ctx.mesh_blocked(base, 2)
    p2 = fem.FunctionSpace(mesh, "CG", 2)._lay
    p2h = ctx.mesh_upload(p2.coords, p2.cells)
    modes = [ctx.vec_from(np.ones(nv)) for _ in range(K)]
    modes2 = [ctx.vec_from(np.ones(2 * nv)) for _ in range(K)]
    modesp2 = [ctx.vec_from(np.ones(p2.n)) for _ in range(K)]
    short, emn, emx, exc, fld, scale = (ctx.vec_alloc(nc - 1), ctx.vec_alloc(nc), ctx.vec_alloc(nc), ctx.vec_alloc(nc),
                                        ctx.vec_alloc(nc * S), ctx.vec_from(np.ones(nc)))
    outs = (emn, emx, exc, fld)
    for v in outs:
        ctx.vec_fill(v, POISON)
    cf = np.ones((K, S))
    st = np.full((3, S), -1.0)
    L = np.ones((q, 4))
    lib, PD = ctx.lib, _lib.PD

    def call(k, want, m=base, mlist=modes, thr=0.0, stats=None, a=0, b=0, c=0, d=0, s=S, qq=q, Lp=L, sc=0):
        arr = (_lib.H * max(len(mlist), 1))(*mlist)
        rc = lib.pgd_eval_batch_grad(ctx.h, m, arr, k, Lp.ctypes.data_as(PD) if Lp is not None else None, qq, sc, cf.ctypes.data_as(PD), s,
                                     want, thr, stats.ctypes.data_as(PD) if stats is not None else None, a, b, c, d)
        return rc, lib.pgd_last_error(ctx.h).decode()

    try:
        for what, (rc, msg) in {
            # what pgd_eval_batch refuses
            "k = 0": call(0, 1, stats=st),
            "k = 257": call(257, 1, mlist=modes * 86, stats=st),
            "s = 0": call(K, 1, stats=st, s=0),
            "nothing requested": call(K, 0),
            "missing stats": call(K, 1),
            "missing envelope": call(K, 2, a=emn),
            "missing exceed": call(K, 4, thr=0.5),
            "missing fields": call(K, 8),
            "unrequested stats": call(K, 2, stats=st, a=emn, b=emx),
            "unrequested envelope": call(K, 1, stats=st, a=emn, b=emx),
            "unrequested threshold": call(K, 1, thr=0.5, stats=st),
            "NaN threshold": call(K, 4, thr=float("nan"), c=exc),
            "mode of another size": call(K, 1, mlist=modes[:2] + [short], stats=st),
            "envelope of another size": call(K, 2, a=short, b=emx),
            "fields of another size": call(K, 8, d=emn),
            "outputs aliasing each other": call(K, 2, a=emn, b=emn),
            "mode that is no vector": call(K, 1, mlist=modes[:2] + [987654], stats=st),
            # what pgd_cell_gradient refuses
            "P2 layout": call(K, 1, m=p2h, mlist=modesp2, stats=st),
            "not a mesh": call(K, 1, m=987654, stats=st),
            "q = 0": call(K, 1, stats=st, qq=0),
            "q = 10": call(K, 1, stats=st, qq=10),
            "null L": call(K, 1, stats=st, Lp=None),
            "scalar modes on the blocked layout": call(K, 1, m=blocked, stats=st),
            "blocked modes on the scalar layout": call(K, 1, mlist=modes2, stats=st),
            "scale of another size": call(K, 1, stats=st, sc=short),
            "scale that is no vector": call(K, 1, stats=st, sc=987654),
            # and the aliases of this call
            "output aliasing a mode": call(K, 2, a=modes[1], b=emx),
            "output aliasing the scale": call(K, 2, a=emn, b=scale, sc=scale),
        }.items():
            assert rc == -1 and msg.startswith("eval_batch_grad:"), (what, rc, msg)
        assert np.all(st == -1.0)                        # nothing ran
        for v in outs:
            assert np.all(ctx.vec_download(v) == POISON)
        assert np.all(ctx.vec_download(modes[1]) == 1.0) and np.all(ctx.vec_download(scale) == 1.0)
        # and the valid call right after them works: nodal values 1 everywhere have no gradient
        assert np.array_equal(ctx.eval_batch_grad(base, modes, L[:, :2], cf, scale=scale), np.zeros((3, S)))
    finally:
        free_all(ctx, modes + modes2 + modesp2 + [short, emn, emx, exc, fld, scale])
        for h in (p2h, blocked, base):
            ctx.mesh_free(h)


# ------------------------------------------------------------------------------------------------ 7. frontend
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
    from pgdrome_amd import model
    coords = samples_of(sol, (1,), 17, 5)
    monkeypatch.setattr(model, "DEVICE_EVAL_MIN_DOFS", 0)
    count = lambda: tuple(fem.STATS.get(k, 0) for k in ("eval_gradient_fused_calls", "gradient_mode_builds", "eval_gradient_calls"))
    att = sol.mesh[0].attributes[0]
    before, c0 = getattr(att, "_gradient_modes", None), count()
    dev, _ = run_and_check(sol, [1], coords, quantity, scale, planes="fused")
    assert count() == (c0[0] + 1, c0[1], c0[2]) and getattr(att, "_gradient_modes", None) is before
    auto = sol.evaluate_gradient_many(0, [1], coords, 0, quantity=quantity, scale=scale, planes="auto", modes_max_bytes=1)
    assert count() == (c0[0] + 2, c0[1], c0[2]) and np.array_equal(auto.max, dev.max)
    # the host path of the same request (no device call is counted apart: the counter is the request's)
    monkeypatch.setattr(model, "DEVICE_EVAL_MIN_DOFS", 1 << 60)
    run_and_check(sol, [1], coords, quantity, scale, planes="fused")
    assert count() == (c0[0] + 3, c0[1], c0[2])


def test_fused_von_mises_of_the_elastic_block_through_the_frontend(hip_frontend, monkeypatch):
    from pgdrome_amd import problems
    from pgdrome_amd.solver import PGDProblem
    mesh = fem.BoxMesh(fem.Point(0, 0, 0), fem.Point(2, 1, 1), 4, 4, 4)
    p = PGDProblem(**problems.elastic_block(mesh, 7, PGD_nmax=3))
    p.solve_PGD(_problem="linear", settings={"relative_tolerance": 1e-11})
    frontend_case(monkeypatch, p.return_PGD(), "von_mises", two_valued(mesh, 1.0 / 1.3, 3.0 / 1.3))


def test_fused_flux_of_reaction_diffusion_through_the_frontend(hip_frontend, monkeypatch):
    from pgdrome_amd import problems
    from pgdrome_amd.solver import PGDProblem
    mesh = fem.BoxMesh(fem.Point(0, 0, 0), fem.Point(1, 1, 1), 9, 9, 9)
    p = PGDProblem(**problems.reaction_diffusion(mesh, 17, PGD_nmax=3))
    p.solve_PGD(_problem="linear")
    frontend_case(monkeypatch, p.return_PGD(), "gradient_norm", None)


def test_the_kernel_limit_is_a_value_error_through_the_frontend(hip_frontend, monkeypatch):
    """150 modes of a vector field in 3-D, gradient_norm: q * kp = 9 * 152 is beyond what 160 KiB hold."""
    from pgdrome_amd import model
    from pgdrome_amd.model import PGD
    monkeypatch.setattr(model, "DEVICE_EVAL_MIN_DOFS", 0)
    K = 150
    mesh, pm = MESHES["box72"], fem.IntervalMesh(2, 0.0, 1.0)
    V, Vp = fem.VectorFunctionSpace(mesh, "CG", 1), fem.FunctionSpace(pm, "CG", 1)
    rng = np.random.default_rng(150)
    fs, ones = [], []
    for _ in range(K):
        f, one = fem.Function(V), fem.Function(Vp)
        f.vector().set_local(rng.standard_normal(V.dim()))
        one.vector().set_local(np.ones(3))
        fs.append(f)
        ones.append(one)
    sol = PGD(name="synthetic", n_modes=K, fmeshes=[mesh, pm], pgd_modes=[fs, ones], name_coord=["x", "p"])
    with pytest.raises(ValueError, match="q = 9 planes of K = 150"):
        sol.evaluate_gradient_many(0, [1], [[0.5]], 0, planes="fused")
    res = sol.evaluate_gradient_many(0, [1], [[0.5]], 0, planes="stored")       # the stored path holds such a shape
    assert res.max.shape == (1,) and res.max[0] > 0.0
