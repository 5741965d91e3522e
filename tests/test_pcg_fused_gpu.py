"""PGD_PCG_FORM_SINGLE_SYNC_RECOMPUTE with ONE march per iteration (PGD_TUNE_PCG_FUSED_MARCH, knob 57: k_pcg1_fused_march forms the update
on overlapped tiles - a one-cell ring of q, r' and p' recomputed per workgroup, r in two alternating buffers - and the dots of the
direction it has just written; the solve issues a single stand-alone dot-only product, of p0).

The reference is always the same process with knob 57 = 0: the three-launch loop.  Systems and knob forcing are those of
test_pcg_fold_gpu.py (PGD_TUNE_PCG_SMALL_SINGLE_SYNC = 0, PGD_TUNE_PCG_FOLD_REDUCE = 0, PGD_TUNE_SPMV_ZCHUNK_FORCE = 4,
PGD_TUNE_SPMV_ZCHUNK_STENCIL = L).

Bounds.  The knob keeps every operation and every summation order: the comparison is BITWISE - iteration count, reported residual
and np.array_equal on x.  At convergence (rtol 1e-10) the true residual through the plain CSR product is at most 1.05e-10 |b|, the
bound of the existing PCG tests.
"""
import numpy as np
import pytest

from oracle import fem_numpy as F
from tests import pcg_form_cases as PC

pytestmark = pytest.mark.gpu

GRIDS = {"130x37x41": (130, 37, 41), "65x4x9": (65, 4, 9)}
KNOBS = (25, 12, 7, 36, 48, 22, 23, 53, 3, 55, 56, 57, 38)
DEFAULTS = {25: 1, 12: 1, 7: 0, 36: 0, 48: 0, 22: 1, 23: 1, 53: 1, 3: 1, 55: 0, 56: 1, 57: 1, 38: 0}
# below a chunk of 16 iterations, exactly one, just past one (graph replay + a pipelined chunk behind it), odd and even cut-offs
# (with and without a lagged x term outstanding; the live r and p in either buffer), more than two chunks, convergence
MAXITS = (1, 2, 15, 16, 17, 23, 24, 37, 10000)
# launches are counted where they are queued, a replayed chunk is counted once (at its capture): exact up to one replay
COUNTED = (1, 2, 15, 16, 17, 23, 24)


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


def solves(ctx, g, bc, k57, keys, k56=1, k55=0, on_bc=False):
    """The solves of `keys` (a maxit, or "again": a second solve from the converged x) with knob 57 = k57:
    key -> (iterations, reported residual, x, launches of the recomputing update, stencil_march launches, fused marches); "residual": the true
    residual of the converged x through the plain CSR product.  on_bc: right-hand side and start vector keep their (different)
    values on the eliminated rows, so the residual is non-zero there."""
    b = g["b"].copy()
    x0 = g["x0"].copy()
    if not on_bc:
        b[bc] = 0.0
        x0[bc] = 0.0
    bv = ctx.vec_from(b)
    ctx.tune(55, k55)
    ctx.tune(56, k56)
    ctx.tune(57, k57)
    out = {}
    for key in keys:
        if key == "again":
            continue
        op = ctx.op_combine(g["h"], [g["ak"], g["am"]], [1.0, 3.0], bc)
        xv = ctx.vec_from(x0)
        u0, k0, f0 = ctx.pcg_recompute_updates(), ctx.kernel_counts(), ctx.pcg_fused_marches()
        it, rel = ctx.pcg_solve(op, bv, xv, 1e-10, 0.0, key)
        u1, k1, f1 = ctx.pcg_recompute_updates(), ctx.kernel_counts(), ctx.pcg_fused_marches()
        out[key] = (it, rel, ctx.vec_download(xv), u1 - u0, k1["stencil_march"] - k0["stencil_march"], f1 - f0)
        if key == 10000:
            yv = ctx.vec_alloc(g["n"])
            ctx.tune(3, 0)
            ctx.spmv(op, xv, yv)
            ctx.tune(3, 1)
            out["residual"] = np.linalg.norm(b - ctx.vec_download(yv)) / np.linalg.norm(b)
            ctx.vec_free(yv)
            if "again" in keys:
                it2, rel2 = ctx.pcg_solve(op, bv, xv, 1e-10, 0.0, key)
                out["again"] = (it2, rel2, ctx.vec_download(xv), 0, 0, 0)
        ctx.vec_free(xv)
        ctx.atom_free(op)
    ctx.vec_free(bv)
    return out


def same_bits(new, ref, keys, what):
    for key in keys:
        a, r = new[key], ref[key]
        print("%s, %s: it %d / %d, reported residual %.17g / %.17g, max |x - x_ref| %.3g" %
              (what, key, a[0], r[0], a[1], r[1], np.abs(a[2] - r[2]).max()))
    for key in keys:
        a, r = new[key], ref[key]
        assert a[0] == r[0] and a[1] == r[1] and np.array_equal(a[2], r[2]), (what, key)


CASES = [(bc, L, 0, 1, 1) for bc in ("hull", "hull+column") for L in (3, 7, 1000)]
CASES += [("hull+column", 7, 2, 1, 1), ("hull+column", 3, 2, 1, 1)]      # two rows per thread
CASES += [("hull+column", 7, 0, 0, 1)]            # x updated in every iteration
CASES += [("hull+column", 7, 0, 1, 0)]            # no stream hints
CASES += [("hull", 3, 2, 0, 0)]


@pytest.mark.parametrize("bc,L,rows,lag,hints", CASES)
def test_one_march_per_iteration_keeps_every_bit(ctx, grid, bc, L, rows, lag, hints):
    """Knob 57 on against off: marches of 3 and 7 planes (3: two of every five computed planes are redundant, chunk seams lie next
    to identity planes) and one march over the grid, Dirichlet hull and hull + an interior column (ring cells are masked), every
    cut-off of MAXITS, convergence, and a second solve from the converged x - whose very first scalar step sets the done flag, so
    that every march is a no-op.  A cut solve of k iterations is k updates and k + 1 products.  Two runs with the knob on are
    bit-identical."""
    keys = MAXITS + ("again",)
    try:
        forced(ctx, L, rows, lag, hints)
        ref = solves(ctx, grid, grid["bc"][bc], 0, keys)
        new = solves(ctx, grid, grid["bc"][bc], 1, keys)
        rep = solves(ctx, grid, grid["bc"][bc], 1, (23, 10000))
    finally:
        restore(ctx)
    same_bits(new, ref, keys, "57 on / off")
    same_bits(rep, new, (23, 10000), "57 on, twice")
    for k in COUNTED:
        assert new[k][3] == k and new[k][4] == k + 1 and new[k][5] == k, (k, new[k][0], new[k][3], new[k][4], new[k][5])
        assert ref[k][3] == k and ref[k][4] == k + 1 and ref[k][5] == 0, (k, ref[k][0], ref[k][3], ref[k][4], ref[k][5])
    for k in (1, 2, 15):
        assert new[k][0] == k
    assert new[10000][3] > 0 and new[10000][1] <= 1e-10 and new["residual"] <= 1.05e-10
    assert new["again"][0] == ref["again"][0] <= 1


DEPTH6_CASES = [(bc, L, 0) for bc in ("hull", "hull+column") for L in (3, 7, 1000)]
DEPTH6_CASES += [("hull+column", 7, 2)]           # two rows per thread asked for: the product of depth 6 has four, the update two


@pytest.mark.parametrize("bc,L,rows", DEPTH6_CASES)
def test_one_march_per_iteration_under_a_product_at_depth_6(ctx, grid, bc, L, rows):
    """PGD_TUNE_STENCIL_DEPTH = 6: the stand-alone product of p0 marches with six plane fetches in flight, the fused march is planned
    like the update, at three.  Its workgroups leave the product's pairs where a product launch would, so it may run only where the two
    plans have one shape (stencil_fused_ok): read from pgd_product_plan here, never assumed.  Where they agree knob 57 on must run one
    fused march per iteration; where they differ - marches of 3 planes are 6 in the product, two rows per thread exist at depth 3 only -
    none at all, in the same recurrence.  Either way knob 57 on against off is BITWISE, as its comment promises, at every cut-off of
    MAXITS, at convergence and from the converged x."""
    keys = MAXITS + ("again",)
    try:
        forced(ctx, L, rows, depth=6)
        op = ctx.op_combine(grid["h"], [grid["ak"], grid["am"]], [1.0, 3.0], grid["bc"][bc])
        assert 1 <= ctx.op_classify(op) <= 255
        product, update = PC.product_and_update_plans(ctx, op, 6)
        ctx.atom_free(op)
        agree = PC.plans_agree(product, update)
        print(grid["name"], bc, L, rows, "plans agree" if agree else "plans differ", "product", product, "update", update)
        assert product["family"] == update["family"] == "stencil_march" and product["depth"] == 6 and update["depth"] == 3
        assert product["rows_per_thread"] == 4 and update["rows_per_thread"] == (2 if rows == 2 else 4)
        ref = solves(ctx, grid, grid["bc"][bc], 0, keys)
        new = solves(ctx, grid, grid["bc"][bc], 1, keys)
        assert ctx.pcg_last_form()[0] == "SINGLE_SYNC_RECOMPUTE"
        rep = solves(ctx, grid, grid["bc"][bc], 1, (23, 10000))
    finally:
        restore(ctx)
    same_bits(new, ref, keys, "depth 6, 57 on / off")
    same_bits(rep, new, (23, 10000), "depth 6, 57 on, twice")
    for k in COUNTED:
        assert new[k][3] == k and new[k][4] == k + 1 and new[k][5] == (k if agree else 0), (agree, k, new[k][3], new[k][4], new[k][5])
        assert ref[k][3] == k and ref[k][4] == k + 1 and ref[k][5] == 0, (k, ref[k][3], ref[k][4], ref[k][5])
    assert (new[10000][5] > 0) == agree
    for k in (1, 2, 15):
        assert new[k][0] == k
    assert new[10000][3] > 0 and new[10000][1] <= 1e-10 and new["residual"] <= 1.05e-10
    assert new["again"][0] == ref["again"][0] <= 1


@pytest.mark.parametrize("bc,L,on_bc", [("hull", 7, False), ("hull", 7, True), ("hull+column", 3, False), ("hull+column", 3, True)])
def test_exact_phase_on_eliminated_rows_keeps_every_bit(ctx, grid, bc, L, on_bc):
    """Knob 57 on against off with knob 56 at both settings, solved to rtol 1e-10 so that the exact phase (the last two decades of the
    residual) runs for several iterations; a cut at 23 for the phase before it.  on_bc: right-hand side and start vector are non-zero on
    the eliminated rows - the residual is non-zero there and those rows divide by 1."""
    keys = (23, 10000)
    try:
        forced(ctx, L)
        ref = {k56: solves(ctx, grid, grid["bc"][bc], 0, keys, k56, 0, on_bc) for k56 in (0, 1)}
        new = {k56: solves(ctx, grid, grid["bc"][bc], 1, keys, k56, 0, on_bc) for k56 in (0, 1)}
    finally:
        restore(ctx)
    for k56 in (0, 1):
        same_bits(new[k56], ref[k56], keys, "57 on / off with 56 = %d" % k56)
        assert new[k56][10000][5] > 0 and ref[k56][10000][5] == 0 and new[k56][10000][1] <= 1e-10
        print("true residual %.4g" % new[k56]["residual"])
        assert new[k56]["residual"] <= 1.05e-10


def test_the_fused_march_takes_precedence_over_the_folded_scalar_step(ctx, grid):
    """Knobs 55 and 57 both on: the fused march runs (k_pcg1_scalars stays a launch), the same bits as with both off."""
    keys = (17, 24, 10000)
    try:
        forced(ctx, 7)
        ref = solves(ctx, grid, grid["bc"]["hull+column"], 0, keys)
        new = solves(ctx, grid, grid["bc"]["hull+column"], 1, keys, 1, 1)
    finally:
        restore(ctx)
    same_bits(new, ref, keys, "55 + 57 on / both off")
    assert new[17][3] == 17 and new[17][4] == 18 and new[17][5] == 17
    assert new["residual"] <= 1.05e-10


def test_operators_that_are_not_one_stencil_are_left_alone(ctx, grid):
    """Natural boundaries (a Dirichlet face only): the solve goes through k_pcg1_scalars + k_pcg1_update with the knob on - no launch
    of the recomputing update, the same bits as with it off."""
    try:
        forced(ctx, 7)
        ref = solves(ctx, grid, grid["bc"]["face"], 0, (23, 10000))
        new = solves(ctx, grid, grid["bc"]["face"], 1, (23, 10000))
    finally:
        restore(ctx)
    for key in (23, 10000):
        assert new[key][3] == 0 and new[key][4] == 0 and new[key][5] == 0
    same_bits(new, ref, (23, 10000), "face only")
    assert new["residual"] <= 1.05e-10


def test_first_solve_of_a_fresh_context_keeps_the_dots_of_p0():
    """The stand-alone product of p0 leaves its pairs before the loop allocates what its chunks need: on a context whose reduction
    scratch is still small (the first solve, more than 2^18 rows) that allocation must not move them.  130 x 37 x 66 = 317 460 rows,
    a context of its own per knob setting, marches of 7 planes; same bits."""
    from pgdrome_amd import _lib
    nx, ny, nz = 130, 37, 66
    coords, cells = F.box_mesh((0, 0, 0), (1.0, 0.7, 1.3), nx - 1, ny - 1, nz - 1)
    hull = boundary_dofs(coords)
    rng = np.random.default_rng(57)
    b = rng.uniform(-1, 1, coords.shape[0])
    b[hull] = 0.0
    out = {}
    for k57 in (0, 1):
        c = _lib.Context(0)
        try:
            c.tune(25, 0)
            c.tune(12, 0)
            c.tune(7, 4)
            c.tune(36, 7)
            c.tune(57, k57)
            h = c.mesh_upload(coords, cells)
            ak, am = c.atom_assemble(h, F.STIFF), c.atom_assemble(h, F.MASS)
            op = c.op_combine(h, [ak, am], [1.0, 3.0], hull)
            bv, xv = c.vec_from(b), c.vec_from(np.zeros_like(b))
            it, rel = c.pcg_solve(op, bv, xv, 1e-10, 0.0, 10000)
            out[k57] = (it, rel, c.vec_download(xv), c.pcg_fused_marches(), c.pcg_last_form()[0])
        finally:
            c.close()
    print("fresh contexts: it %d / %d, residual %.17g / %.17g, form %s" % (out[1][0], out[0][0], out[1][1], out[0][1], out[1][4]))
    assert out[1][3] > 0 and out[0][3] == 0
    assert out[1][0] == out[0][0] and out[1][1] == out[0][1] <= 1e-10 and np.array_equal(out[1][2], out[0][2])
