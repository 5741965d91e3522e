"""The product plan (pgd_product_plan, Context.product_plan): the kernel family and launch shape a product with an operator in symmetric
storage gets are decided in ONE place, and launch_spmv_op, the predicates of the solves and the update launchers of the single-sync
recurrence all read that decision.  Here: what the plan reports is what a launch does, under every knob the decision reads.

Operators and reference are those of test_stencil_form_is_lossless (test_kernels_gpu.py): K + 0.37 M on a box lattice with five Dirichlet
sets, y of the march over the slot values (PGD_TUNE_SPMV_ZCHUNK_FORCE = 4, row classes off) as the reference.  Every form of the product
computes the same 15 fused multiply-adds per row in the same order, so y is compared BITWISE.  The fused dot is a sum of at most
197 210 products in per-workgroup partial sums of at most 16 384 rows, reduced in a tree: 1e-12 |w| . |y| is above its rounding error
(16 384 * 2^-53 = 1.8e-12 would be the bound of one serial chain of that length; the lanes of a workgroup carry 64 to 256 of them) and
far below any wrong row.
"""
import numpy as np
import pytest

from oracle import fem_numpy as F
from tests import pcg_form_cases as PC

pytestmark = pytest.mark.gpu

SHAPES = {"65x4x9": (65, 4, 9), "64x8x5": (64, 8, 5), "130x37x41": (130, 37, 41)}
# knob numbers (include/pgd_amd.h)
SYM, FORCE, VARIANT, CLASSES, STENCIL, ZSTENCIL, DEPTH, MARCH3, ROWS = 3, 7, 13, 19, 35, 36, 38, 47, 48
DEFAULTS = {SYM: 1, FORCE: 0, VARIANT: 0, CLASSES: 1, STENCIL: 1, ZSTENCIL: 0, DEPTH: 0, MARCH3: 0, ROWS: 0}
SETTINGS = {
    "defaults": {},
    "force4": {FORCE: 4},
    "force4+zstencil1": {FORCE: 4, ZSTENCIL: 1},
    "force4+zstencil3": {FORCE: 4, ZSTENCIL: 3},
    "force4+zstencil7": {FORCE: 4, ZSTENCIL: 7},
    "stencil0": {STENCIL: 0},
    "classes0": {CLASSES: 0},
    "variant0": {VARIANT: 0},
    "variant1": {VARIANT: 1},
    "variant2": {VARIANT: 2},
    "march3": {MARCH3: 1},
    "rows2": {ROWS: 2},
    "rows4": {ROWS: 4},
    "depth3": {DEPTH: 3},
    "depth6": {DEPTH: 6},
    "sym0": {SYM: 0},
    # the same knobs where the march is forced onto these small grids, so that they decide something
    "force4+stencil0": {FORCE: 4, STENCIL: 0},
    "force4+classes0": {FORCE: 4, CLASSES: 0},
    "force4+classes0+march3": {FORCE: 4, CLASSES: 0, MARCH3: 1},
    "force4+variant1": {FORCE: 4, VARIANT: 1},
    "force4+variant2": {FORCE: 4, VARIANT: 2},
    "force4+zstencil3+rows2": {FORCE: 4, ZSTENCIL: 3, ROWS: 2},
    "force4+zstencil7+depth6": {FORCE: 4, ZSTENCIL: 7, DEPTH: 6},
}
BOUNDARIES = ("hull", "hull + column", "hull + one interior node", "natural", "one face")


def boundary_dofs(coords):
    lo, hi = coords.min(axis=0), coords.max(axis=0)
    return np.where(np.any((coords <= lo + 1e-12) | (coords >= hi - 1e-12), axis=1))[0].astype(np.int32)


def restore(ctx):
    for k, v in DEFAULTS.items():
        ctx.tune(k, v)


@pytest.fixture(scope="module", params=sorted(SHAPES))
def lattice(request, ctx):
    """Mesh, vectors and the five classified operators of one shape, each with the y of the march over its slot values."""
    nx, ny, nz = SHAPES[request.param]
    coords, cells = F.box_mesh((0, 0, 0), (1.0, 0.7, 1.3), nx - 1, ny - 1, nz - 1)
    h = ctx.mesh_upload(coords, cells)
    n = coords.shape[0]
    plane = nx * ny
    ak, am = ctx.atom_assemble(h, F.STIFF), ctx.atom_assemble(h, F.MASS)
    bnd = boundary_dofs(coords)
    face = np.where(coords[:, 2] <= 1e-12)[0].astype(np.int32)
    ix, iy = min(5, nx - 2), min(2, ny - 2)
    column = (ix + nx * iy + plane * np.arange(nz)).astype(np.int32)
    single = np.array([ix + nx * iy + plane * (nz // 2)], dtype=np.int32)
    bcs = dict(zip(BOUNDARIES, (bnd, np.union1d(bnd, column).astype(np.int32), np.union1d(bnd, single).astype(np.int32),
                                np.zeros(0, dtype=np.int32), face)))
    rng = np.random.default_rng(7)
    x, w = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    xv, wv, yv = ctx.vec_from(x), ctx.vec_from(w), ctx.vec_alloc(n)
    ctx.flags_reset()
    ops, y_ref = {}, {}
    try:
        for name in BOUNDARIES:
            op = ctx.op_combine(h, [ak, am], [1.0, 0.37], bcs[name])
            assert ctx.op_symmetrize(op) is True
            ctx.tune(FORCE, 4)
            ctx.tune(CLASSES, 0)
            k0 = ctx.kernel_counts()
            ctx.spmv_dot_slot(op, xv, yv, xv, 0, n, 30)                  # the march over the slot values
            assert ctx.kernel_counts()["dia_march"] == k0["dia_march"] + 1
            restore(ctx)
            y_ref[name] = ctx.vec_download(yv)
            assert 1 <= ctx.op_classify(op) <= 255
            ops[name] = op
    finally:
        restore(ctx)
    nzs = nz - 1
    ranges = {"whole": (0, n), "slab": (plane, nzs * plane), "one plane": ((nz // 2) * plane, (nz // 2 + 1) * plane),
              "not plane-aligned": (plane + 7, 3 * plane - 5)}
    yield {"shape": request.param, "n": n, "h": h, "x": x, "w": w, "xv": xv, "wv": wv, "yv": yv, "ops": ops, "y_ref": y_ref, "ranges": ranges,
           "bcs": bcs, "ak": ak, "am": am}
    for v in (xv, wv, yv):
        ctx.vec_free(v)
    for a in list(ops.values()) + [ak, am]:
        ctx.atom_free(a)
    ctx.mesh_free(h)


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_plan_is_what_the_launch_does(ctx, lattice, setting):
    """For five operators x four row ranges x (PCG-like, dot against a third vector) under one knob setting:
    (a) the family the plan reports is exactly the one kernel counter that moves in spmv_dot_slot (-1: the CSR kernels);
    (b) y is bit-identical to the march over the slot values inside the range and untouched outside, the dot is the range's;
    (c) asking twice gives the same plan and moves no counter, kernel or classification."""
    g = lattice
    x, w, xv, wv, yv = g["x"], g["w"], g["xv"], g["wv"], g["yv"]
    try:
        for k, v in SETTINGS[setting].items():
            ctx.tune(k, v)
        for name in BOUNDARIES:
            op, y_ref = g["ops"][name], g["y_ref"][name]
            for rname, (r0, r1) in g["ranges"].items():
                for pcg_like in (True, False):
                    what = (g["shape"], setting, name, rname, pcg_like)
                    k0, c0 = ctx.kernel_counts(), ctx.classify_counts()
                    plan = ctx.product_plan(op, r0, r1, pcg_like)
                    assert ctx.product_plan(op, r0, r1, pcg_like) == plan, what                            # (c)
                    assert ctx.kernel_counts() == k0 and ctx.classify_counts() == c0, what
                    ctx.vec_fill(yv, -7.0)
                    ctx.spmv_dot_slot(op, xv, yv, xv if pcg_like else wv, r0, r1, 31)
                    k1 = ctx.kernel_counts()
                    ran = {k for k in k1 if k1[k] != k0[k]}
                    print(what, plan, sorted(ran))
                    if plan["form"] < 0:                                                                   # (a)
                        assert ran and ran <= {"csr", "csr_dict"}, what
                    else:
                        assert ran == {plan["family"]} and k1[plan["family"]] == k0[plan["family"]] + 1, (what, plan, ran)
                    y = ctx.vec_download(yv)                                                               # (b)
                    assert np.array_equal(y[r0:r1], y_ref[r0:r1]), (what, plan, np.where(y[r0:r1] != y_ref[r0:r1])[0][:8])
                    assert np.all(y[:r0] == -7.0) and np.all(y[r1:] == -7.0), what
                    d_ref = (x if pcg_like else w)[r0:r1] @ y_ref[r0:r1]
                    assert abs(ctx.slots_download(31, 1)[0] - d_ref) <= 1e-12 * (np.abs(w if not pcg_like else x) @ np.abs(y_ref)), what
                    assert ctx.product_plan(op, r0, r1, pcg_like) == plan, what
    finally:
        restore(ctx)


@pytest.mark.parametrize("bc", ["hull", "hull + column"])
def test_fused_solve_where_the_plans_say_so(ctx, lattice, bc):
    """(d) An operator whose whole-grid plan is the stencil march, product and update of one shape, no ghost planes: pgd_pcg_solve in the
    single-sync recurrence that forms A p again runs the fused march.  (Knobs as in test_pcg_fused_gpu.py: the recurrence and the
    march forced onto a small grid, marches of 7 planes.)"""
    g = lattice
    knobs = {25: (0, 1), 12: (0, 1), FORCE: (4, 0), ZSTENCIL: (7, 0)}
    b = np.random.default_rng(31).uniform(-1, 1, g["n"])
    b[g["bcs"][bc]] = 0.0
    bv, sv = ctx.vec_from(b), ctx.vec_alloc(g["n"])
    op = ctx.op_combine(g["h"], [g["ak"], g["am"]], [1.0, 3.0], g["bcs"][bc])
    try:
        for k, (v, _) in knobs.items():
            ctx.tune(k, v)
        assert 1 <= ctx.op_classify(op) <= 255
        plan = ctx.product_plan(op)
        print(g["shape"], bc, plan)
        assert plan["family"] == "stencil_march" and plan["depth"] == 3          # depth 3: the update's own plan
        ctx.vec_fill(sv, 0.0)
        f0 = ctx.pcg_fused_marches()
        its, rel = ctx.pcg_solve(op, bv, sv, 1e-10, 0.0, 40)
        assert ctx.pcg_last_form()[0] == "SINGLE_SYNC_RECOMPUTE"
        assert ctx.pcg_fused_marches() > f0, (its, rel)
    finally:
        for k, (_, d) in knobs.items():
            ctx.tune(k, d)
        restore(ctx)
        ctx.atom_free(op)
        for v in (bv, sv):
            ctx.vec_free(v)


@pytest.mark.parametrize("rows", [0, 2])
@pytest.mark.parametrize("L", [3, 5, 6, 7, 13])
@pytest.mark.parametrize("bc", ["hull", "hull + column"])
def test_fused_solve_at_depth_6_only_where_the_two_plans_agree(ctx, lattice, bc, L, rows):
    """(d) with the product at fetch depth 6 (PGD_TUNE_STENCIL_DEPTH): the update that forms A p again and the fused march are planned at
    depth 3 (plan_stencil_update), so the product's launch can have another shape - marches of at least 6 planes, four rows per thread
    whatever PGD_TUNE_STENCIL_ROWS asks.  Both plans are read through pgd_product_plan.  Where they differ in wgs, zchunk,
    rows_per_thread or tiles_y the fused march must not run (its workgroups would leave the product's pairs in another count or
    order than the scalar step sums), the recurrence stays SINGLE_SYNC_RECOMPUTE and the solve meets the residual bar of the PCG
    tests; where they agree the fused march runs."""
    g = lattice
    knobs = {25: (0, 1), 12: (0, 1), FORCE: (4, 0), ZSTENCIL: (L, 0), ROWS: (rows, 0), DEPTH: (6, 0)}
    b = np.random.default_rng(31).uniform(-1, 1, g["n"])
    b[g["bcs"][bc]] = 0.0
    bv, sv, yv = ctx.vec_from(b), ctx.vec_alloc(g["n"]), ctx.vec_alloc(g["n"])
    op = ctx.op_combine(g["h"], [g["ak"], g["am"]], [1.0, 3.0], g["bcs"][bc])
    try:
        for k, (v, _) in knobs.items():
            ctx.tune(k, v)
        assert 1 <= ctx.op_classify(op) <= 255
        product, update = PC.product_and_update_plans(ctx, op, 6)
        agree = PC.plans_agree(product, update)
        print(g["shape"], bc, L, rows, "plans agree" if agree else "plans differ", "product", product, "update", update)
        assert product["family"] == update["family"] == "stencil_march"
        assert product["depth"] == 6 and product["rows_per_thread"] == 4 and product["zchunk"] >= 6
        assert update["depth"] == 3 and update["rows_per_thread"] == (2 if rows == 2 else 4) and update["zchunk"] == max(3, L)
        ctx.vec_fill(sv, 0.0)
        f0, u0 = ctx.pcg_fused_marches(), ctx.pcg_recompute_updates()
        its, rel = ctx.pcg_solve(op, bv, sv, 1e-10, 0.0, 10000)
        assert ctx.pcg_last_form()[0] == "SINGLE_SYNC_RECOMPUTE"
        fused, updates = ctx.pcg_fused_marches() - f0, ctx.pcg_recompute_updates() - u0
        assert updates > 0 and (fused > 0 if agree else fused == 0), (its, rel, fused, updates, product, update)
        ctx.tune(SYM, 0)
        ctx.spmv(op, sv, yv)
        ctx.tune(SYM, 1)
        res = np.linalg.norm(b - ctx.vec_download(yv)) / np.linalg.norm(b)
        print("iterations %d, reported %.3g, true residual %.3g, fused marches %d of %d updates" % (its, rel, res, fused, updates))
        assert its < 10000 and rel <= 1e-10 and res <= 1.05e-10
    finally:
        for k, (_, d) in knobs.items():
            ctx.tune(k, d)
        restore(ctx)
        ctx.atom_free(op)
        for v in (bv, sv, yv):
            ctx.vec_free(v)
