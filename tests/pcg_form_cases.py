"""The case table of tests/test_pcg_forms_gpu.py: one knob setting + system per row of the two tables by which pgd_pcg_solve picks
its recurrence and its preconditioner (pcg_choose / pcg_precond_prepare in pgdrome_amd/csrc/pgd_pcg.hip).  tools/pcg_forms_dump.py
runs the same table and dumps every result, for comparing two builds bit by bit.

Inputs of the choice: scaled = symmetric storage && knob 10 && n >= 2; grid = the mesh is a full structured vertex grid;
whole = the operator's products run in the stencil march over the whole grid.  Form, the first line that applies:
  a cycle preconditions -> PRECOND | !scaled -> TEXTBOOK | knob 18 && knob 25 && (n <= 2^20 || (grid && n <= knob 26)) -> TWO_LAUNCH |
  knob 12 && n <= 2^20 -> FOLDED | knob 18 && grid -> SINGLE_SYNC (_RECOMPUTE with knob 53 && whole) | knob 16 -> DEFERRED_X | PLAIN.
Preconditioner (knob 40): 1 -> MG and 2 -> VMG (grid only) on the scaled branch, 3 -> CMG on the unscaled branch of a blocked
layout, each only where its hierarchy can be built; everything else is Jacobi and counted as a fallback of the cycle asked for.
The fetch depth of the stencil march (knob 38) is no input of either table: the rows at depth 6 must report what their depth-3 twins do.

The expected names are literals from those tables, not read back from the library.  (The second way into TWO_LAUNCH - a grid of
more than 2^20 rows - has no case: a system of that size does not solve in a test's few seconds.)

Systems.  "lattice": the 65 x 4 x 9 box of tests/test_pcg_recompute_gpu.py, stiffness + 3 mass; Dirichlet hull + an interior column
(one stencil on the whole grid once the march is forced onto it: knobs 7 and 36) or the face z = 0 only (not one stencil).
"rect": a 64 x 64 triangulated rectangle - symmetric storage, but no structured 3-D grid.  "permuted": a 10^3 box with its nodes
renumbered at random - no column dictionary, hence no symmetric storage.  "mg32": a 32^3 unit box with the hull eliminated, the
smallest lattice of the multigrid tests; "vmg17" / "cmg17": the 17^3 lattices of tests/test_vmg_gpu.py ("constant" family) and
tests/test_cmg_gpu.py (clamped elasticity, three components, through the frontend)."""
import numpy as np

from oracle import fem_numpy as F

KNOB_DEFAULTS = {10: 1, 12: 1, 16: 1, 18: 1, 25: 1, 53: 1, 7: 0, 36: 0, 38: 0, 40: 0}
LARGE = {25: 0, 12: 0}                         # the recurrences of large systems on a small one
MARCH = {25: 0, 12: 0, 7: 4, 36: 7}            # ... with the stencil march (7 planes per march) forced onto the small grid
CUT = 37                                        # inside a chunk and odd: a lagged or deferred x term is outstanding

# (name, system, Dirichlet set, knobs, form, preconditioner, the fallback counter that moves or None)
CASES = [
    ("two_launch_lattice", "lattice", "hull+column", {}, "TWO_LAUNCH", "JACOBI", None),
    ("folded_lattice", "lattice", "hull+column", {25: 0}, "FOLDED", "JACOBI", None),
    ("single_sync_recompute", "lattice", "hull+column", MARCH, "SINGLE_SYNC_RECOMPUTE", "JACOBI", None),
    ("single_sync_not_one_stencil", "lattice", "face", MARCH, "SINGLE_SYNC", "JACOBI", None),
    ("single_sync_knob_off", "lattice", "hull+column", {**MARCH, 53: 0}, "SINGLE_SYNC", "JACOBI", None),
    # the product with six plane fetches in flight (knob 38): the update that forms A p again stays at three, the choice is the same
    ("single_sync_recompute_depth6", "lattice", "hull+column", {**MARCH, 38: 6}, "SINGLE_SYNC_RECOMPUTE", "JACOBI", None),
    ("single_sync_knob_off_depth6", "lattice", "hull+column", {**MARCH, 38: 6, 53: 0}, "SINGLE_SYNC", "JACOBI", None),
    ("deferred_x_lattice", "lattice", "hull+column", {**LARGE, 18: 0}, "DEFERRED_X", "JACOBI", None),
    ("plain_lattice", "lattice", "hull+column", {**LARGE, 18: 0, 16: 0}, "PLAIN", "JACOBI", None),
    ("textbook_knob", "lattice", "hull+column", {10: 0}, "TEXTBOOK", "JACOBI", None),
    ("two_launch_no_grid", "rect", "hull", {}, "TWO_LAUNCH", "JACOBI", None),
    ("folded_no_grid", "rect", "hull", {25: 0}, "FOLDED", "JACOBI", None),
    ("single_sync_needs_a_grid", "rect", "hull", LARGE, "DEFERRED_X", "JACOBI", None),
    ("deferred_x_no_grid", "rect", "hull", {**LARGE, 18: 0}, "DEFERRED_X", "JACOBI", None),
    ("plain_no_grid", "rect", "hull", {**LARGE, 18: 0, 16: 0}, "PLAIN", "JACOBI", None),
    ("textbook_no_symmetric_storage", "permuted", "hull", {}, "TEXTBOOK", "JACOBI", None),
    ("mg", "mg32", "hull", {40: 1}, "PRECOND", "MG", None),
    ("vmg", "vmg17", "hull", {40: 2}, "PRECOND", "VMG", None),
    ("cmg", "cmg17", "clamped", {40: 3}, "PRECOND", "CMG", None),
    ("mg_request_not_a_hull", "lattice", "face", {40: 1}, "TWO_LAUNCH", "JACOBI", "mg"),
    ("vmg_request_no_grid", "rect", "hull", {40: 2}, "TWO_LAUNCH", "JACOBI", "vmg"),
    ("cmg_request_scalar_scaled", "lattice", "hull+column", {40: 3}, "TWO_LAUNCH", "JACOBI", "cmg"),
    ("mg_request_unscaled", "lattice", "hull+column", {10: 0, 40: 1}, "TEXTBOOK", "JACOBI", "mg"),
    ("vmg_request_unscaled", "lattice", "hull+column", {10: 0, 40: 2}, "TEXTBOOK", "JACOBI", "vmg"),
    ("cmg_request_scalar_unscaled", "lattice", "hull+column", {10: 0, 40: 3}, "TEXTBOOK", "JACOBI", "cmg"),
]


def _hull(coords):
    lo, hi = coords.min(axis=0), coords.max(axis=0)
    return np.where(np.any((coords <= lo + 1e-12) | (coords >= hi - 1e-12), axis=1))[0].astype(np.int32)


def _scalar_system(ctx, coords, cells, mass, bcs, seed):
    """Stiffness + mass * mass matrix on an uploaded mesh; every solve combines a fresh operator (a solve may leave the operator's
    symmetric copy scaled)."""
    h = ctx.mesh_upload(coords, cells.astype(np.int32))
    n = coords.shape[0]
    ak, am = ctx.atom_assemble(h, F.STIFF), ctx.atom_assemble(h, F.MASS)
    rng = np.random.default_rng(seed)

    def free():
        for a in (ak, am):
            ctx.atom_free(a)
        ctx.mesh_free(h)
    return {"n": n, "b": rng.uniform(-1, 1, n), "x0": 0.01 * rng.uniform(-1, 1, n), "bc": bcs,
            "op": lambda bc: ctx.op_combine(h, [ak, am], [1.0, mass], bc), "free": free}


def build_system(ctx, name):
    """ctx: the _lib.Context of the HIP backend the frontend is set to ("cmg17" assembles through the frontend)."""
    if name == "lattice":
        nx, ny, nz = 65, 4, 9
        coords, cells = F.box_mesh((0, 0, 0), (1.0, 0.7, 1.3), nx - 1, ny - 1, nz - 1)
        hull = _hull(coords)
        column = (5 + nx * 2 + nx * ny * np.arange(nz)).astype(np.int32)      # an interior Dirichlet column through all planes
        face = np.where(coords[:, 2] <= 1e-12)[0].astype(np.int32)            # natural boundaries elsewhere: not one stencil
        return _scalar_system(ctx, coords, cells, 3.0, {"hull+column": np.union1d(hull, column).astype(np.int32), "face": face}, 31)
    if name == "rect":
        coords, cells = F.rectangle_mesh((0, 0), (1, 1), 63, 63)
        return _scalar_system(ctx, coords, cells, 3.0, {"hull": _hull(coords)}, 32)
    if name == "permuted":
        coords, cells = F.box_mesh((0, 0, 0), (1, 1, 1), 9, 9, 9)
        perm = np.random.default_rng(5).permutation(coords.shape[0])
        coords, cells = coords[perm], np.argsort(perm)[cells]
        return _scalar_system(ctx, coords, cells, 3.0, {"hull": _hull(coords)}, 33)
    if name == "mg32":
        coords, cells = F.box_mesh((0, 0, 0), (1, 1, 1), 31, 31, 31)
        return _scalar_system(ctx, coords, cells, 3.0, {"hull": _hull(coords)}, 34)
    if name == "vmg17":
        from tests import vmg_reference as V
        coords, cells = V.box((17, 17, 17))
        return _scalar_system(ctx, coords, cells, 3.0, {"hull": _hull(coords)}, 35)
    if name == "cmg17":
        from tests import cmg_reference as CM
        shape, nc = (17, 17, 17), 3
        bc = CM.dirichlet_dofs(shape, nc, "clamped")
        A, _ = CM.frontend_operator(CM.vector_space(shape), "elastic", bc, k_found=2.0)
        n = A.lay.n
        rng = np.random.default_rng(36)
        return {"n": n, "b": rng.uniform(-1, 1, n), "x0": 0.01 * rng.uniform(-1, 1, n), "bc": {"clamped": np.asarray(bc, dtype=np.int32)},
                "op": lambda bc: A.op(), "free": lambda: None, "keep": A}
    raise KeyError(name)


# The fused march of PGD_PCG_FORM_SINGLE_SYNC_RECOMPUTE exists only where the product's launch and the update's have one shape
# (stencil_fused_ok, pgdrome_amd/csrc/pgd_spmv.hip): these fields of the two plans
PLAN_SHAPE = ("wgs", "zchunk", "rows_per_thread", "tiles_y")


def product_and_update_plans(ctx, op, depth):
    """(plan of the whole-grid product of `op` under the knobs as set and PGD_TUNE_STENCIL_DEPTH = depth, plan of the update that forms
    A p again), both through pgd_product_plan.  The update's plan is the product's at fetch depth 3 whatever knob 38 says
    (plan_stencil_update), read here with the knob at 3; apart from the depth the two calls can differ only in the rows-per-thread rule
    of marches whose length the launcher chooses, so march lengths must be forced (PGD_TUNE_SPMV_ZCHUNK_STENCIL > 0) around this call.
    Knob 38 is left at `depth`."""
    ctx.tune(38, depth)
    product = ctx.product_plan(op)
    ctx.tune(38, 3)
    update = ctx.product_plan(op)
    ctx.tune(38, depth)
    return product, update


def plans_agree(product, update):
    return all(product[k] == update[k] for k in PLAN_SHAPE)


def set_knobs(ctx, knobs):
    for k, v in KNOB_DEFAULTS.items():
        ctx.tune(k, knobs.get(k, v))


def solve(ctx, system, bc_name, maxit, rtol, residual=False):
    """One solve from the system's start vector with the knobs as they are set: (iterations, reported residual, x, true residual
    relative to |b| through the plain CSR product of the unscaled operator or None)."""
    bc = system["bc"][bc_name]
    b, x0 = system["b"].copy(), system["x0"].copy()
    b[bc] = 0.0
    x0[bc] = 0.0
    op = system["op"](bc)
    bv, xv = ctx.vec_from(b), ctx.vec_from(x0)
    try:
        it, rel = ctx.pcg_solve(op, bv, xv, rtol, 0.0, maxit)
        x = ctx.vec_download(xv)
        res = None
        if residual:
            yv = ctx.vec_alloc(system["n"])
            ctx.tune(3, 0)
            try:
                ctx.spmv(op, xv, yv)
            finally:
                ctx.tune(3, 1)
            res = np.linalg.norm(b - ctx.vec_download(yv)) / np.linalg.norm(b)
            ctx.vec_free(yv)
        return it, rel, x, res
    finally:
        ctx.vec_free(bv)
        ctx.vec_free(xv)
        ctx.atom_free(op)
