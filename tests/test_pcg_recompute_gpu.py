"""Single-sync PCG on one-stencil grids with q = A p formed again by the update instead of stored (PGD_TUNE_PCG_RECOMPUTE_Q,
knob 53): the product keeps only its dots, the update is an epilogue of the stencil march over p (k_spmv_stencil_march, EPI 3)
that writes the new direction to a second buffer.

The reference is always the existing loop (knob 53 = 0: the product stores q, k_pcg1_update reads it) in the same process.  The
path is forced onto small grids: PGD_TUNE_PCG_SMALL_SINGLE_SYNC = 0 and PGD_TUNE_PCG_FOLD_REDUCE = 0 select the three-launch
recurrence of large systems, PGD_TUNE_SPMV_ZCHUNK_FORCE = 4 and PGD_TUNE_SPMV_ZCHUNK_STENCIL = L the stencil march with marches
of L planes.

Bounds.  alpha_0 and beta_0 come from identical inputs (the same product launch shape leaves the same partial sums) and the
per-row arithmetic is the same, so after ONE iteration x and the reported residual are bit-identical.  From the second
iteration on only the grouping of the residual's partial sums differs (per 64 x 16 patch and march instead of per 256-row
block): the bounds are those of test_two_launch_recurrence_of_small_systems for the same kind of change - equal iteration
counts and 1e-10 relative at a cut-off, counts within 2 and 1e-9 relative at convergence (rtol 1e-10), the true residual
through the CSR kernel at 1.05e-10 |b|.
"""
import numpy as np
import pytest

from oracle import fem_numpy as F
from tests import pcg_form_cases as PC

pytestmark = pytest.mark.gpu

GRIDS = {"130x37x41": (130, 37, 41), "65x4x9": (65, 4, 9)}     # several x-tiles with a partial last one, partial y-tiles, odd plane counts
KNOBS = (25, 12, 7, 36, 48, 22, 23, 53, 3, 38)
DEFAULTS = {25: 1, 12: 1, 7: 0, 36: 0, 48: 0, 22: 1, 23: 1, 53: 1, 3: 1, 38: 0}


def boundary_dofs(coords):
    lo, hi = coords.min(axis=0), coords.max(axis=0)
    return np.where(np.any((coords <= lo + 1e-12) | (coords >= hi - 1e-12), axis=1))[0].astype(np.int32)


@pytest.fixture(scope="module", params=sorted(GRIDS))
def grid(request, ctx):
    nx, ny, nz = GRIDS[request.param]
    coords, cells = F.box_mesh((0, 0, 0), (1.0, 0.7, 1.3), nx - 1, ny - 1, nz - 1)
    h = ctx.mesh_upload(coords, cells)
    n = coords.shape[0]
    ak, am = ctx.atom_assemble(h, F.STIFF), ctx.atom_assemble(h, F.MASS)
    hull = boundary_dofs(coords)
    ix, iy = min(5, nx - 2), min(2, ny - 2)
    column = (ix + nx * iy + nx * ny * np.arange(nz)).astype(np.int32)      # an interior Dirichlet column through all planes
    face = np.where(coords[:, 2] <= 1e-12)[0].astype(np.int32)              # natural boundaries elsewhere: not one stencil
    rng = np.random.default_rng(31)
    b = rng.uniform(-1, 1, n)
    x0 = 0.01 * rng.uniform(-1, 1, n)
    yield {"name": request.param, "h": h, "n": n, "ak": ak, "am": am, "b": b, "x0": x0,
           "bc": {"hull": hull, "hull+column": np.union1d(hull, column).astype(np.int32), "face": face}}
    for a in (ak, am):
        ctx.atom_free(a)
    ctx.mesh_free(h)


def forced(ctx, L, rows=0, lag=1, hints=1, depth=0):
    ctx.tune(38, depth)
    ctx.tune(25, 0)
    ctx.tune(12, 0)
    ctx.tune(7, 4)
    ctx.tune(36, L)
    ctx.tune(48, rows)
    ctx.tune(22, lag)
    ctx.tune(23, hints)


def restore(ctx):
    for k in KNOBS:
        ctx.tune(k, DEFAULTS[k])


def solves(ctx, g, bc, knob, keys):
    """The solves of `keys` (a maxit, or "again": a second solve from the converged x) with knob 53 = `knob`:
    key -> (iterations, reported residual, x, launches of the recomputing update, stencil_march launches)."""
    b = g["b"].copy()
    b[bc] = 0.0
    x0 = g["x0"].copy()
    x0[bc] = 0.0
    bv = ctx.vec_from(b)
    ctx.tune(53, knob)
    out = {}
    for key in keys:
        if key == "again":
            continue
        op = ctx.op_combine(g["h"], [g["ak"], g["am"]], [1.0, 3.0], bc)
        xv = ctx.vec_from(x0)
        u0, k0 = ctx.pcg_recompute_updates(), ctx.kernel_counts()
        it, rel = ctx.pcg_solve(op, bv, xv, 1e-10, 0.0, key)
        u1, k1 = ctx.pcg_recompute_updates(), ctx.kernel_counts()
        out[key] = (it, rel, ctx.vec_download(xv), u1 - u0, k1["stencil_march"] - k0["stencil_march"])
        if key == 10000:
            if "again" in keys:
                it2, rel2 = ctx.pcg_solve(op, bv, xv, 1e-10, 0.0, key)
                out["again"] = (it2, rel2, ctx.vec_download(xv), 0, 0)
            # the true residual through the plain CSR product of the unscaled operator
            yv = ctx.vec_alloc(g["n"])
            ctx.tune(3, 0)
            ctx.spmv(op, xv, yv)
            ctx.tune(3, 1)
            res_csr = np.linalg.norm(b - ctx.vec_download(yv)) / np.linalg.norm(b)
            # afterwards the operator is usable as before: its ordinary product with the fused dot
            ctx.flags_reset()
            ctx.spmv_dot_slot(op, xv, yv, xv, 0, g["n"], 30)
            res_own = np.linalg.norm(b - ctx.vec_download(yv)) / np.linalg.norm(b)
            out["residuals"] = (res_csr, res_own)
            ctx.vec_free(yv)
        ctx.vec_free(xv)
        ctx.atom_free(op)
    ctx.vec_free(bv)
    return out


def compare(new, ref, again):
    # one iteration: identical bits
    a, r = new[1], ref[1]
    print("maxit 1: it %d / %d, reported residual %.17g / %.17g, max |x - x_ref| %.3g" % (a[0], r[0], a[1], r[1], np.abs(a[2] - r[2]).max()))
    assert a[0] == r[0] == 1 and a[1] == r[1] and np.array_equal(a[2], r[2])
    assert a[3] == 1 and a[4] == 2 and r[3] == 0 and r[4] == 2       # one recomputing update; the initial residual's product and the iteration's
    for maxit in (2, 23, 24):
        a, r = new[maxit], ref[maxit]
        err = np.linalg.norm(a[2] - r[2]) / np.linalg.norm(r[2])
        print("maxit %d: it %d / %d, |x - x_ref| / |x_ref| %.3g" % (maxit, a[0], r[0], err))
        assert a[0] == r[0] and err <= 1e-10
        assert a[3] > 0 and a[4] > 0 and r[3] == 0
    a, r = new[10000], ref[10000]
    err = np.linalg.norm(a[2] - r[2]) / np.linalg.norm(r[2])
    print("convergence: it %d / %d, reported %.3g / %.3g, |x - x_ref| / |x_ref| %.3g, true residuals %s / %s" %
          (a[0], r[0], a[1], r[1], err, new["residuals"], ref["residuals"]))
    assert abs(a[0] - r[0]) <= 2 and err <= 1e-9 and a[1] <= 1e-10
    assert a[3] > 0 and a[4] > 0 and r[3] == 0
    assert new["residuals"][0] <= 1.05e-10 and new["residuals"][1] <= 1.05e-10
    if again:
        print("second solve from the converged x: it %d / %d" % (new["again"][0], ref["again"][0]))
        assert new["again"][0] <= 1
        assert np.linalg.norm(new["again"][2] - r[2]) <= 1e-9 * np.linalg.norm(r[2])


CASES = [(bc, L, 0, 1, 1) for bc in ("hull", "hull+column") for L in (3, 7, 1000)]
CASES += [("hull+column", 7, 2, 1, 1)]            # two rows per thread
CASES += [("hull+column", 7, 0, 0, 1)]            # x updated in every iteration
CASES += [("hull+column", 7, 0, 1, 0)]            # no stream hints


@pytest.mark.parametrize("bc,L,rows,lag,hints", CASES)
def test_update_that_forms_q_walks_the_iterates_of_the_stored_q(ctx, grid, bc, L, rows, lag, hints):
    """Marches of 3 and 7 planes (halo planes that belong to another workgroup, an incomplete last group of steps) and one march
    over the grid; Dirichlet hull, and hull + an interior column; cut off after 1 iteration (bit-identical), after 2, 23 and 24
    (odd and even counts inside a chunk: with a lagged x term outstanding and without), to convergence, and again from the
    converged x.  Two runs with the knob on are bit-identical."""
    keys = (1, 2, 23, 24, 10000, "again")
    try:
        forced(ctx, L, rows, lag, hints)
        ref = solves(ctx, grid, grid["bc"][bc], 0, keys)
        new = solves(ctx, grid, grid["bc"][bc], 1, keys)
        rep = solves(ctx, grid, grid["bc"][bc], 1, (23, 10000))
    finally:
        restore(ctx)
    compare(new, ref, True)
    for key in (23, 10000):
        assert new[key][0] == rep[key][0] and new[key][1] == rep[key][1] and np.array_equal(new[key][2], rep[key][2]), key


DEPTH6_CASES = [(bc, L, 0) for bc in ("hull", "hull+column") for L in (3, 7, 1000)]
DEPTH6_CASES += [("hull+column", 7, 2)]           # two rows per thread asked for: the product of depth 6 has four, the update two


@pytest.mark.parametrize("bc,L,rows", DEPTH6_CASES)
def test_update_at_depth_3_under_a_product_at_depth_6(ctx, grid, bc, L, rows):
    """PGD_TUNE_STENCIL_DEPTH = 6: the product marches with six plane fetches in flight, the update that forms q again is planned at
    three.  Knob 53 on against off at that depth, held to what the knob's comment promises - the same q and per-row operations, another
    grouping of the residual's partial sums - i.e. to the bounds of compare().  Marches of 3 planes become marches of 6 in the product
    only (other workgroup counts in the two launches, no fused march); 7 planes and one march over the grid keep one shape.  Whether
    the fused march runs is read from the two plans, never assumed."""
    keys = (1, 2, 23, 24, 10000, "again")
    try:
        forced(ctx, L, rows, depth=6)
        op = ctx.op_combine(grid["h"], [grid["ak"], grid["am"]], [1.0, 3.0], grid["bc"][bc])
        assert 1 <= ctx.op_classify(op) <= 255
        product, update = PC.product_and_update_plans(ctx, op, 6)
        ctx.atom_free(op)
        print(grid["name"], bc, L, rows, "product", product, "update", update)
        assert product["family"] == update["family"] == "stencil_march"
        assert product["depth"] == 6 and product["rows_per_thread"] == 4 and product["zchunk"] >= 6
        assert update["depth"] == 3 and update["rows_per_thread"] == (2 if rows == 2 else 4) and update["zchunk"] == max(3, L)
        ref = solves(ctx, grid, grid["bc"][bc], 0, keys)
        f0 = ctx.pcg_fused_marches()
        new = solves(ctx, grid, grid["bc"][bc], 1, keys)
        fused = ctx.pcg_fused_marches() - f0
        rep = solves(ctx, grid, grid["bc"][bc], 1, (23, 10000))
    finally:
        restore(ctx)
    assert (fused > 0) == PC.plans_agree(product, update), (fused, product, update)
    compare(new, ref, True)
    for key in (23, 10000):
        assert new[key][0] == rep[key][0] and new[key][1] == rep[key][1] and np.array_equal(new[key][2], rep[key][2]), key


def test_operators_that_are_not_one_stencil_keep_the_stored_q(ctx, grid):
    """Natural boundaries (a Dirichlet face only): the products run on the row-class dictionary, the solve goes through
    k_pcg1_update with the knob on - no launch of the recomputing update, the same bits as with the knob off."""
    try:
        forced(ctx, 7)
        ref = solves(ctx, grid, grid["bc"]["face"], 0, (23, 10000))
        new = solves(ctx, grid, grid["bc"]["face"], 1, (23, 10000))
    finally:
        restore(ctx)
    for key in (23, 10000):
        assert new[key][3] == 0 and new[key][4] == 0
        assert new[key][0] == ref[key][0] and new[key][1] == ref[key][1] and np.array_equal(new[key][2], ref[key][2])
    assert new["residuals"][0] <= 1.05e-10 and new["residuals"][1] <= 1.05e-10
