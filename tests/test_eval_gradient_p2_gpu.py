"""pgd_cell_gradient_p2 and pgd_eval_batch_grad_p2 on the MI355X, through the C-ABI, against tests/eval_gradient_p2_reference.py:
stage 1 exact on integer data (records, blocked layouts, point-major plane order, every point count), inside the derived bound on
stretched meshes, the argument errors; the fused call equal to the two stored stages and to the int64 reference on integers (every
row block, entry counts that end in a padded block, two sample chunks), inside the bound and bit-identical across grids and chunks
on floating-point data, the LDS limit - and PGD.evaluate_gradient_many(at=...) through the frontend."""

import numpy as np
import pytest

from pgdrome_amd import _lib, fem
from tests.eval_gradient_fused_reference import KEYS, POISON, Layouts, _outputs, assert_integer_outputs, integer_data, upload_nodal
from tests.eval_gradient_p2_reference import plane_bound_p2, planes_p2, points_of, run_and_check_p2
from tests.eval_gradient_reference import LD, evaluate_norm_reference, norm_bound, product_bound, samples_of, two_valued
from tests.eval_many_reference import U53
from tests.test_eval_gradient_fused_gpu import ROW_BLOCKS
from tests.test_eval_gradient_gpu import expected_shape
from tests.test_eval_many_gpu import VARIANTS, Knobs, free_all

pytestmark = pytest.mark.gpu

P = fem.Point
STEPS = np.array([0.1, 0.37, 1.0 / 3.0])


def _layouts():
    meshes = {
        "rect-right": fem.RectangleMesh(P(0, 0), P(3, 2), 3, 2, "right"),
        "rect-left": fem.RectangleMesh(P(0, 0), P(3, 2), 3, 2, "left"),
        "rect-crossed": fem.RectangleMesh(P(0, 0), P(3, 2), 3, 2, "crossed"),
        "box72": fem.BoxMesh(P(0, 0, 0), P(2, 3, 2), 2, 3, 2),
        "box360": fem.BoxMesh(P(0, 0, 0), P(5, 4, 3), 5, 4, 3),            # more than one workgroup
    }
    return {name: fem.DofLayout(m, 2) for name, m in meshes.items()}


LAYOUTS = _layouts()                     # .coords (nodes, G), .cells (cells, 6 | 10): the frontend's own P2 layouts

# integer 4 lam: the vertices, an edge midpoint, (1/2, 1/4, 1/4) resp. the barycentre (1/4 each), and sets of 2, 3 and 4 points
POINTS = {
    2: [np.eye(3), np.array([[0.5, 0.5, 0.0]]), np.array([[0.5, 0.25, 0.25]]), np.array([[0.0, 0.5, 0.5], [0.25, 0.25, 0.5]]),
        np.array([[0.5, 0.25, 0.25], [1.0, 0.0, 0.0], [0.5, 0.0, 0.5], [0.25, 0.5, 0.25]])],
    3: [np.eye(4), np.array([[0.0, 0.5, 0.0, 0.5]]), np.full((1, 4), 0.25), np.array([[0.25] * 4, [0.5, 0.0, 0.5, 0.0]]),
        np.array([[0.5, 0.25, 0.25, 0.0], [0.0, 0.0, 0.0, 1.0], [0.25, 0.25, 0.0, 0.5]])],
}


def sub_layout(lay, ncells):
    """(coords, records) of the first ``ncells`` cells of a layout, the nodes renumbered to those they use (order kept)."""
    rec = lay.cells[:ncells]
    used, inv = np.unique(rec, return_inverse=True)
    return lay.coords[used], inv.reshape(rec.shape).astype(np.int32)


# ------------------------------------------------------------------------------------------------ stage 1
def gradient_cases(ctx, X, rec, integer, point_sets):
    """Every (ncomp, q, scale or none, point set) on one uploaded P2 layout: yields (got (q, npt, cells), U, lam, L, scale)."""
    nc, nv, G = rec.shape[0], X.shape[0], X.shape[1]
    rng = np.random.default_rng(nc)
    with Layouts(ctx, X, rec) as lay:
        for ncomp in (1, 2, 3):
            qin = ncomp * G
            for q in sorted({1} | {q for q in (3, 6, 9) if q <= qin}):
                for with_scale in (False, True):
                    if integer:
                        U, L = rng.integers(-7, 8, size=(nv, ncomp)), rng.integers(-4, 5, size=(q, qin))
                        scale = rng.integers(-3, 4, size=nc) if with_scale else None
                    else:
                        U, L = rng.standard_normal((nv, ncomp)), rng.standard_normal((q, qin))
                        scale = rng.standard_normal(nc) if with_scale else None
                    u = ctx.vec_from(U.astype(np.float64).reshape(-1))
                    sc = ctx.vec_from(scale.astype(np.float64)) if with_scale else 0
                    try:
                        for lam in point_sets:
                            out = ctx.vec_alloc(q * len(lam) * nc)
                            try:
                                ctx.vec_fill(out, POISON)
                                ctx.cell_gradient_p2(lay[ncomp], u, lam, L.astype(np.float64), out, sc)
                                yield ctx.vec_download(out).reshape(q, len(lam), nc), U, lam, L, scale
                            finally:
                                ctx.vec_free(out)
                    finally:
                        free_all(ctx, [u] + ([sc] if with_scale else []))


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_cell_gradient_p2_is_exact_on_unit_lattices(ctx, name):
    """Integer nodal values, L and scale on lattices of unit steps, points with integer 4 lam: every coefficient d N_j / d xi_a and
    every entry of the inverse Jacobian is an integer, so the planes must EQUAL the int64 reference - scalar and blocked layouts,
    every q the layout allows, with and without a scale, 1 .. 4 points.  The output is poisoned first: every entry is written."""
    lay = LAYOUTS[name]
    X, rec = lay.coords, lay.cells
    n, npts = 0, set()
    for got, U, lam, L, scale in gradient_cases(ctx, X, rec, True, POINTS[X.shape[1]]):
        ref = planes_p2(X, rec, U, lam, L, scale)
        assert ref.dtype == np.int64 and np.array_equal(got, ref.astype(np.float64)), (name, U.shape[1], L.shape[0], scale is not None, lam)
        n += 1
        npts.add(len(lam))
    G = X.shape[1]
    assert n == sum(len({1} | {q for q in (3, 6, 9) if q <= ncomp * G}) for ncomp in (1, 2, 3)) * 2 * 5 and npts == {1, 2, 3, 4}


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_cell_gradient_p2_bound_on_stretched_meshes(ctx, name):
    """Steps (0.1, 0.37, 1 / 3), normal data, the barycentre (1/3 resp. 1/4 each: the coefficient of the shared edge vanishes
    there), a point off every symmetry and the vertices: inside the stage-1 bound of the reference against long double."""
    lay = LAYOUTS[name]
    X, rec = lay.coords * STEPS[None, :lay.coords.shape[1]], lay.cells
    G = X.shape[1]
    off = np.array([[0.1, 0.2, 0.7]]) if G == 2 else np.array([[0.1, 0.2, 0.3, 0.4]])
    worst = 0.0
    for got, U, lam, L, scale in gradient_cases(ctx, X, rec, False, [np.full((1, G + 1), 1.0 / (G + 1)), np.concatenate([off, np.eye(G + 1)[:2]])]):
        ref, bd = planes_p2(X, rec, U, lam, L, scale), plane_bound_p2(X, rec, U, lam, L, scale)
        assert ref.dtype == LD
        err = np.abs(got.astype(LD) - ref).astype(np.float64)
        assert np.all(err <= bd), (name, U.shape[1], L.shape[0], float((err / bd).max()))
        worst = max(worst, float((err[bd > 0] / bd[bd > 0]).max()))
    print("cell_gradient_p2 %s: largest error / bound = %.4f" % (name, worst))


def test_cell_gradient_p2_argument_errors(ctx):
    lay = LAYOUTS["rect-right"]
    X, rec = lay.coords, lay.cells
    nc, nv = rec.shape[0], X.shape[0]
    mesh = lay.mesh
    base = ctx.mesh_upload(X, rec)
    blocked = ctx.mesh_blocked(base, 2)
    p1h = ctx.mesh_upload(mesh.coordinates(), mesh.cells())
    iv = fem.DofLayout(fem.IntervalMesh(7, 0.0, 7.0), 2)
    ivh = ctx.mesh_upload(iv.coords, iv.cells)
    npt, q = 2, 2
    u, u2, out, scale, short = (ctx.vec_from(np.ones(nv)), ctx.vec_from(np.ones(2 * nv)), ctx.vec_alloc(q * npt * nc), ctx.vec_from(np.ones(nc)),
                                ctx.vec_alloc(nc - 1))
    up1, uiv, big = ctx.vec_from(np.ones(mesh.num_vertices())), ctx.vec_from(np.ones(iv.n)), ctx.vec_alloc(q * npt * nc)
    ctx.vec_fill(out, POISON)
    ctx.vec_fill(big, POISON)
    # three cells of 12 nodes: a nodal vector has the size of the output of one plane at four points, so it can alias it
    Xs, recs = sub_layout(LAYOUTS["rect-left"], 3)
    assert Xs.shape[0] == 4 * recs.shape[0]
    small = ctx.mesh_upload(Xs, recs)
    us, outs, scs = ctx.vec_from(np.ones(12)), ctx.vec_alloc(12), ctx.vec_from(np.ones(3))
    ctx.vec_fill(outs, POISON)
    L = np.ones((2, 2))
    lam = np.array([[0.5, 0.5, 0.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.25, 0.25, 0.5]])
    lib, PD = ctx.lib, _lib.PD

    def call(m, uh, sc, o, n=npt, qq=q, Lp=L, lp=lam):
        rc = lib.pgd_cell_gradient_p2(ctx.h, m, uh, lp.ctypes.data_as(PD) if lp is not None else None, n,
                                      Lp.ctypes.data_as(PD) if Lp is not None else None, qq, sc, o)
        return rc, lib.pgd_last_error(ctx.h).decode()

    try:
        for what, (rc, msg) in {
            "P1 layout": call(p1h, up1, 0, out),
            "interval P2 layout": call(ivh, uiv, 0, out),
            "npt = 0": call(base, u, 0, out, n=0),
            "npt = 5": call(base, u, 0, out, n=5),
            "null lam": call(base, u, 0, out, lp=None),
            "null L": call(base, u, 0, out, Lp=None),
            "q = 0": call(base, u, 0, out, qq=0),
            "q = 10": call(base, u, 0, out, qq=10),
            "u of the scalar layout on the blocked one": call(blocked, u, 0, out),
            "u of the blocked layout on the scalar one": call(base, u2, 0, out),
            "out of q * cells entries (one point's)": call(base, u, 0, scale, qq=1),
            "out for another point count": call(base, u, 0, out, n=3),
            "scale of another size": call(base, u, short, out),
            "scale of one entry per point and cell": call(base, u, big, out),
            "out aliases u": call(small, outs, 0, outs, n=4, qq=1),
            "out aliases scale": call(base, u, scale, scale, n=1, qq=1),
            "not a mesh": call(987654, u, 0, out),
            "not a vector": call(base, 987654, 0, out),
            "scale that is no vector": call(base, u, 987654, out),
        }.items():
            assert rc == -1 and msg.startswith("cell_gradient_p2:"), (what, rc, msg)
        assert np.all(ctx.vec_download(out) == POISON) and np.all(ctx.vec_download(scale) == 1.0)        # nothing ran
        assert np.all(ctx.vec_download(outs) == POISON)
        ctx.cell_gradient_p2(small, us, lam[:4], L[:1], outs, scs)               # (the same call with u and out apart)
        assert np.all(ctx.vec_download(outs) == 0.0)
        # the valid call right after them: nodal values 1 everywhere have no gradient
        ctx.cell_gradient_p2(base, u, lam[:npt], L, out, scale)
        assert np.all(ctx.vec_download(out) == 0.0)
    finally:
        free_all(ctx, [u, u2, out, scale, short, up1, uiv, big, us, outs, scs])
        for h in (small, ivh, p1h, blocked, base):
            ctx.mesh_free(h)


# ------------------------------------------------------------------------------------------------ fused against stored
def run_fused_p2(ctx, lay, modes, lam, L, Cm, m, threshold, scale=0):
    """Every output of one pgd_eval_batch_grad_p2 call (fields as (S, entries)); where the call raises, "stats" is the exception."""
    Cm = np.asarray(Cm, dtype=np.float64)
    return _outputs(ctx, m, Cm.shape[1], lambda emn, emx, exc, fld: ctx.eval_batch_grad_p2(
        lay, modes, lam, np.asarray(L, dtype=np.float64), Cm, scale=scale, stats=True, env_min=emn, env_max=emx, exceed=exc,
        threshold=threshold, fields=fld))


def run_stored_p2(ctx, lay, modes, lam, L, Cm, m, threshold, scale=0):
    """The same outputs from pgd_cell_gradient_p2 per mode and pgd_eval_batch_norm on the planes."""
    L, Cm = np.asarray(L, dtype=np.float64), np.asarray(Cm, dtype=np.float64)
    q = L.shape[0]
    pl = [ctx.vec_alloc(q * m) for _ in modes]
    try:
        for f, p in zip(modes, pl):
            ctx.cell_gradient_p2(lay, f, lam, L, p, scale)
        return _outputs(ctx, m, Cm.shape[1], lambda emn, emx, exc, fld: ctx.eval_batch_norm(
            pl, q, Cm, stats=True, env_min=emn, env_max=emx, exceed=exc, threshold=threshold, fields=fld))
    finally:
        free_all(ctx, pl)


def integer_reference_p2(X, rec, U, lam, L, scale, Cm):
    """``integer_reference`` of the P1 tests on the planes of the P2 restatement, entries point-major."""
    Pm = np.stack([planes_p2(X, rec, U[k], lam, L, scale).reshape(L.shape[0], -1) for k in range(U.shape[0])])      # (K, q, entries)
    assert Pm.dtype == np.int64
    ref = evaluate_norm_reference(Pm, Cm, None)
    assert ref["SS"].dtype == np.int64 and int(ref["SS"].max()) < 2 ** 53
    spread = np.sort(ref["SS"].reshape(-1))
    threshold = float(np.sqrt(float(spread[len(spread) // 2]) + 0.5))
    return evaluate_norm_reference(Pm, Cm, threshold), threshold


# (layout, cells or None for all, point set index, ncomp, q): 24 = 12 cells x 2 points, 72 x 1, 17 x 1, 12 x 1 (below a block of
# 16), 72 x 4 and 17 x 3 (a block that spans the seam of two points), 360 x 4 (several workgroups)
ENTRY_CASES = [("rect-right", None, 3, 2, 3), ("box72", None, 2, 3, 6), ("box72", 17, 2, 1, 3), ("rect-left", None, 1, 1, 1),
               ("box72", None, 0, 3, 9), ("box72", 17, 4, 2, 6), ("rect-crossed", 17, 0, 3, 6), ("box360", None, 0, 1, 3)]
SS = (1, 17, 65, 1025)


@pytest.mark.parametrize("case", ENTRY_CASES, ids=lambda c: "%s-%s-p%d-c%d-q%d" % c)
def test_fused_equals_stored_and_the_reference_on_integer_data(ctx, case):
    """Small integers everywhere: the planes, the u_i and the sums of squares are exact integers, so every output of the fused call
    lies within one ulp of np.sqrt of the int64 value with equal counts, and EQUALS what the two stored stages give - both
    variants, two grids, S = 1, 17, 65 and 1025 (one past the default chunk: two launches)."""
    name, ncells, pset, ncomp, q = case
    lay = LAYOUTS[name]
    X, rec = (lay.coords, lay.cells) if ncells is None else sub_layout(lay, ncells)
    G, nc, nv = X.shape[1], rec.shape[0], X.shape[0]
    lam = POINTS[G][pset]
    m, K = len(lam) * nc, 5
    U, L, scale, Cm = integer_data(np.random.default_rng(m + q), nv, nc, G, ncomp, q, K, max(SS), True)
    with Layouts(ctx, X, rec) as lh:
        modes, sc = upload_nodal(ctx, U), ctx.vec_from(scale.astype(np.float64))
        try:
            for S in SS:
                ref, thr = integer_reference_p2(X, rec, U, lam, L, scale, Cm[:, :S])
                for vname, variant in VARIANTS.items():
                    with Knobs(ctx, variant=variant):
                        stored = run_stored_p2(ctx, lh[ncomp], modes, lam, L, Cm[:, :S], m, thr, sc)
                    assert_integer_outputs(stored, ref, (case, S, vname, "stored"))
                    for grid_max in ((0, 2) if S <= 65 else (0,)):
                        with Knobs(ctx, variant=variant, grid_max=grid_max):
                            out = run_fused_p2(ctx, lh[ncomp], modes, lam, L, Cm[:, :S], m, thr, sc)
                        assert_integer_outputs(out, ref, (case, S, vname, grid_max))
                        for key in KEYS:
                            assert np.array_equal(out[key], stored[key]), (case, S, vname, grid_max, key)
        finally:
            free_all(ctx, modes + [sc])


@pytest.mark.parametrize("qk", list(ROW_BLOCKS), ids=lambda qk: "q%d-K%d" % qk)
def test_every_row_block(ctx, qk):
    """64, 32, 16 entries in at most 64 KiB and 16 entries in more (the kernel's own LDS attribute): the rule of the stored path, on
    box72 at its vertices (288 entries) and its first 17 cells at 3 points (51)."""
    q, K = qk
    assert expected_shape(q, K, 17) == ROW_BLOCKS[qk]
    for ncells, pset in ((None, 0), (17, 4)):
        lay = LAYOUTS["box72"]
        X, rec = (lay.coords, lay.cells) if ncells is None else sub_layout(lay, ncells)
        lam = POINTS[3][pset]
        nc, nv, m = rec.shape[0], X.shape[0], len(lam) * rec.shape[0]
        U, L, scale, Cm = integer_data(np.random.default_rng(100 * q + K), nv, nc, 3, 3, q, K, 17, True)
        ref, thr = integer_reference_p2(X, rec, U, lam, L, scale, Cm)
        with Layouts(ctx, X, rec) as lh:
            modes, sc = upload_nodal(ctx, U), ctx.vec_from(scale.astype(np.float64))
            try:
                for grid_max in (0, 2):
                    with Knobs(ctx, variant=1, grid_max=grid_max):
                        out = run_fused_p2(ctx, lh[3], modes, lam, L, Cm, m, thr, sc)
                    assert ctx.eval_norm_last_shape() == ROW_BLOCKS[qk]
                    assert_integer_outputs(out, ref, (qk, ncells, grid_max))
            finally:
                free_all(ctx, modes + [sc])


def test_beyond_the_lds_limit_is_refused_and_the_plain_variant_runs(ctx):
    """q = 9, K = 256: the matrix-unit variant refuses with PGD_ERR_LIMIT before anything is launched (every output still
    poisoned); the plain variant has no such limit and is exact."""
    q, K = 9, 256
    assert expected_shape(q, K, 17) == (16, 0)
    X, rec = sub_layout(LAYOUTS["box72"], 17)
    lam = POINTS[3][3]
    nc, nv, m = rec.shape[0], X.shape[0], 2 * rec.shape[0]
    U, L, scale, Cm = integer_data(np.random.default_rng(9256), nv, nc, 3, 3, q, K, 17, True)
    ref, thr = integer_reference_p2(X, rec, U, lam, L, scale, Cm)
    with Layouts(ctx, X, rec) as lh:
        modes, sc = upload_nodal(ctx, U), ctx.vec_from(scale.astype(np.float64))
        try:
            with Knobs(ctx, variant=1):
                out = run_fused_p2(ctx, lh[3], modes, lam, L, Cm, m, thr, sc)
            err = out["stats"]
            assert isinstance(err, _lib.PgdError) and err.code == -4, err
            assert "eval_batch_grad_p2:" in str(err) and "q = 9" in str(err) and "k = 256" in str(err) and str(160 * 1024) in str(err)
            for key in KEYS[1:]:
                assert np.all(out[key] == POISON), key
            with Knobs(ctx, variant=0):
                out = run_fused_p2(ctx, lh[3], modes, lam, L, Cm, m, thr, sc)
            assert ctx.eval_norm_last_shape() == (64, 0)
            assert_integer_outputs(out, ref, "plain")
        finally:
            free_all(ctx, modes + [sc])


THR = 25.0


@pytest.fixture(scope="module")
def float_case():
    """box72 stretched by (0.1, 0.37, 1 / 3) at its vertices (288 entries), ncomp = 3, q = 6, K = 21, S = 65 of seeded normal data
    with a normal scale, and its long-double reference with the bound, computed once: with P_t the planes of mode t and b_t =
    ``plane_bound_p2`` of mode t, a code that forms the planes per mode and combines them has u_i off by at most
    e_i = sum_t |c_t| b_t,i + product_bound(K, sum_t |c_t| (|P_t,i| + b_t,i)), and the value by ``norm_bound(e, V)``."""
    lay = LAYOUTS["box72"]
    X, rec = lay.coords * STEPS[None, :], lay.cells
    lam = np.eye(4)
    nc, nv, K, S, q = rec.shape[0], X.shape[0], 21, 65, 6
    rng = np.random.default_rng(20261020)
    U, L = rng.standard_normal((K, nv, 3)), rng.standard_normal((q, 9))
    scale, Cm = rng.standard_normal(nc), rng.standard_normal((K, S))
    Pm = np.stack([planes_p2(X, rec, U[k], lam, L, scale).reshape(q, -1) for k in range(K)])
    b = np.stack([plane_bound_p2(X, rec, U[k], lam, L, scale).reshape(q, -1) for k in range(K)])
    assert Pm.dtype == LD
    ref = evaluate_norm_reference(Pm, Cm, THR)
    ca = np.abs(Cm)
    e = np.einsum("tie,ts->ies", b, ca) + product_bound(K, np.einsum("tie,ts->ies", np.abs(Pm.astype(np.float64)) + b, ca))
    return {"X": X, "rec": rec, "lam": lam, "m": 4 * nc, "U": U, "L": L, "scale": scale, "Cm": Cm, "ref": ref, "bd": norm_bound(e, ref["V"])}


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_floating_point_bound_and_knob_invariance(ctx, float_case, variant):
    """Every field entry of the fused call inside the derived bound around the long-double reference; the statistics, envelopes
    and counts are the extrema of the fields it returns; grid size (0, 1, 3) and sample chunk (0, 16, 48) change no bit of any
    output; the stored stages lie inside the same bound."""
    c = float_case
    with Layouts(ctx, c["X"], c["rec"]) as lh:
        modes, sc = upload_nodal(ctx, c["U"]), ctx.vec_from(c["scale"])
        try:
            base = None
            for grid_max in (0, 1, 3):
                for chunk in (0, 16, 48):
                    with Knobs(ctx, variant=VARIANTS[variant], grid_max=grid_max, chunk=chunk):
                        out = run_fused_p2(ctx, lh[3], modes, c["lam"], c["L"], c["Cm"], c["m"], THR, sc)
                    if base is None:
                        base = out
                        continue
                    for key in KEYS:
                        assert np.array_equal(out[key].view(np.uint64), base[key].view(np.uint64)), (key, grid_max, chunk)
            with Knobs(ctx, variant=VARIANTS[variant]):
                stored = run_stored_p2(ctx, lh[3], modes, c["lam"], c["L"], c["Cm"], c["m"], THR, sc)
        finally:
            free_all(ctx, modes + [sc])
    ref, bd = c["ref"], c["bd"]
    for name, out in (("fused", base), ("stored", stored)):
        err = np.abs(out["fields"].T.astype(LD) - ref["V"]).astype(np.float64)
        ratio = float((err / bd).max())
        print("eval_batch_grad_p2 %s %s: largest error / bound = %.4f" % (variant, name, ratio))
        assert ratio <= 1.0
    F = base["fields"]                                  # (S, entries)
    assert np.array_equal(base["stats"][0], F.min(axis=1)) and np.array_equal(base["stats"][1], F.max(axis=1))
    assert np.array_equal(base["stats"][2], F.max(axis=1))
    assert np.array_equal(base["env_min"], F.min(axis=0)) and np.array_equal(base["env_max"], F.max(axis=0))
    assert np.array_equal(base["exceed"], (F > THR).sum(axis=0))
    assert 0 < base["exceed"].sum() < F.size            # (the threshold separates something)


def test_eval_batch_grad_p2_argument_errors(ctx):
    """What the fused call refuses of its own (the layout, the points) and that pgd_eval_batch's checks name this entry point."""
    lay = LAYOUTS["rect-right"]
    X, rec = lay.coords, lay.cells
    nc, nv, K, S, q, npt = rec.shape[0], X.shape[0], 3, 5, 2, 2
    mesh = lay.mesh
    base = ctx.mesh_upload(X, rec)
    p1h = ctx.mesh_upload(mesh.coordinates(), mesh.cells())
    iv = fem.DofLayout(fem.IntervalMesh(7, 0.0, 7.0), 2)
    ivh = ctx.mesh_upload(iv.coords, iv.cells)
    modes = [ctx.vec_from(np.ones(nv)) for _ in range(K)]
    modesp1 = [ctx.vec_from(np.ones(mesh.num_vertices())) for _ in range(K)]
    modesiv = [ctx.vec_from(np.ones(iv.n)) for _ in range(K)]
    emn, emx, percell, scale = ctx.vec_alloc(npt * nc), ctx.vec_alloc(npt * nc), ctx.vec_alloc(nc), ctx.vec_from(np.ones(nc))
    for v in (emn, emx, percell):
        ctx.vec_fill(v, POISON)
    Xs, recs = sub_layout(LAYOUTS["rect-left"], 3)       # 3 cells of 12 nodes: a mode has the size of an output at four points
    assert Xs.shape[0] == 4 * recs.shape[0]
    small = ctx.mesh_upload(Xs, recs)
    modess = [ctx.vec_from(np.ones(12)) for _ in range(K)]
    cf, st, L = np.ones((K, S)), np.full((3, S), -1.0), np.ones((q, 2))
    lam = np.array([[0.5, 0.5, 0.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.25, 0.25, 0.5]])
    lib, PD = ctx.lib, _lib.PD

    def call(want, m=base, mlist=modes, stats=None, a=0, b=0, n=npt, qq=q, Lp=L, lp=lam, sc=0, k=K):
        arr = (_lib.H * max(len(mlist), 1))(*mlist)
        rc = lib.pgd_eval_batch_grad_p2(ctx.h, m, arr, k, lp.ctypes.data_as(PD) if lp is not None else None, n,
                                        Lp.ctypes.data_as(PD) if Lp is not None else None, qq, sc, cf.ctypes.data_as(PD), S, want, 0.0,
                                        stats.ctypes.data_as(PD) if stats is not None else None, a, b, 0, 0)
        return rc, lib.pgd_last_error(ctx.h).decode()

    try:
        for what, (rc, msg) in {
            "P1 layout": call(1, m=p1h, mlist=modesp1, stats=st),
            "interval P2 layout": call(1, m=ivh, mlist=modesiv, stats=st),
            "not a mesh": call(1, m=987654, stats=st),
            "npt = 0": call(1, stats=st, n=0),
            "npt = 5": call(1, stats=st, n=5),
            "null lam": call(1, stats=st, lp=None),
            "null L": call(1, stats=st, Lp=None),
            "q = 0": call(1, stats=st, qq=0),
            "q = 10": call(1, stats=st, qq=10),
            "scale of one entry per point and cell": call(1, stats=st, sc=emn),
            "modes of the P1 layout": call(1, mlist=modesp1, stats=st),
            "k = 0": call(1, stats=st, k=0),
            "missing stats": call(1),
            "envelope of one entry per cell": call(2, a=percell, b=emx),
            "output aliasing a mode": call(2, m=small, mlist=modess, a=modess[1], b=modess[2], n=4),
            "outputs aliasing each other": call(2, a=emn, b=emn),
            "output aliasing the scale": call(2, a=emn, b=scale, sc=scale, n=1),
        }.items():
            assert rc == -1 and msg.startswith("eval_batch_grad_p2:"), (what, rc, msg)
        assert np.all(st == -1.0)                        # nothing ran
        for v in (emn, emx, percell):
            assert np.all(ctx.vec_download(v) == POISON)
        assert np.array_equal(ctx.eval_batch_grad_p2(base, modes, lam[:npt], L, cf, scale=scale), np.zeros((3, S)))
    finally:
        assert np.all(ctx.vec_download(modess[1]) == 1.0)
        free_all(ctx, modes + modesp1 + modesiv + modess + [emn, emx, percell, scale])
        for h in (small, ivh, p1h, base):
            ctx.mesh_free(h)


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
    """Both ``at``, stored, fused and auto on the device inside the reference bound (``run_and_check_p2``: for "vertices" the
    reduced envelopes against the per-entry reference), the host path of the same request inside it too, and the two within the sum
    of both bounds of each other."""
    from pgdrome_amd import model
    coords = samples_of(sol, (1,), 9, 5)
    count = lambda: tuple(fem.STATS.get(k, 0) for k in ("eval_gradient_fused_calls", "gradient_mode_builds", "eval_gradient_calls"))
    nc = sol.mesh[0].attributes[0].interpolationfct[0].function_space().mesh().num_cells()
    for at in ("midpoint", "vertices"):
        monkeypatch.setattr(model, "DEVICE_EVAL_MIN_DOFS", 0)
        c0 = count()
        dev, ref, Bd = run_and_check_p2(sol, [1], coords, quantity, scale, at, planes="stored")
        assert count() == (c0[0], c0[1] + 1, c0[2] + 1)                         # planes built on the device, one device product
        fused = run_and_check_p2(sol, [1], coords, quantity, scale, at, planes="fused")[0]
        auto = run_and_check_p2(sol, [1], coords, quantity, scale, at, planes="auto")[0]
        assert count() == (c0[0] + 1, c0[1] + 1, c0[2] + 2)                     # auto: stored, from the cache
        assert np.array_equal(auto.max, dev.max) and np.array_equal(auto.min, dev.min)
        small = sol.evaluate_gradient_many(0, [1], coords, 0, quantity=quantity, scale=scale, at=at, planes="auto", modes_max_bytes=1)
        assert count()[0] == c0[0] + 2 and np.array_equal(small.max, fused.max)      # auto: fused where the planes do not fit
        monkeypatch.setattr(model, "DEVICE_EVAL_MIN_DOFS", 1 << 60)
        host = run_and_check_p2(sol, [1], coords, quantity, scale, at, planes="stored")[0]
        # each statistic lies within the largest slack of its sample around the reference's (check_result): the sum of both bounds
        tol = 2.0 * (Bd + 2 * U53 * ref.astype(np.float64)).max(axis=1)
        for a in (dev, fused):
            assert np.all(np.abs(a.max - host.max) <= tol) and np.all(np.abs(a.min - host.min) <= tol)
        assert dev.envelope_max.vector().host().shape == (nc,)


def test_von_mises_of_the_p2_elastic_block_through_the_frontend(hip_frontend, monkeypatch):
    from pgdrome_amd import problems
    from pgdrome_amd.solver import PGDProblem
    mesh = fem.BoxMesh(P(0, 0, 0), P(2, 1, 1), 3, 3, 3)
    p = PGDProblem(**problems.elastic_block(mesh, 5, PGD_nmax=2, degree=2))
    p.solve_PGD(_problem="linear", settings={"relative_tolerance": 1e-11})
    frontend_case(monkeypatch, p.return_PGD(), "von_mises", two_valued(mesh, 1.0 / 1.3, 3.0 / 1.3))


def test_flux_of_p2_reaction_diffusion_through_the_frontend(hip_frontend, monkeypatch):
    from pgdrome_amd import problems
    from pgdrome_amd.solver import PGDProblem
    mesh = fem.RectangleMesh(P(0, 0), P(1.5, 1), 6, 5)
    p = PGDProblem(**problems.reaction_diffusion(mesh, 9, PGD_nmax=3, degree=2))
    p.solve_PGD(_problem="linear")
    frontend_case(monkeypatch, p.return_PGD(), "gradient_norm", None)
