"""Every launch variant of the products on box lattices, at the seams of its tiles and marches.

launch_product_diac, launch_product_stencil and launch_product_dia (pgdrome_amd/csrc/pgd_spmv.hip) pick a template instance from the plan
(plan_product, pgd_product_plan.h) and the PGD_TUNE_* knobs.  SETTINGS lists one knob setting per instance and march length that matters,
with the kernel-count family that must move for it; the shapes (tests/product_variant_reference.py) are each the smallest case of a seam:
a second x tile of one column, fewer rows than any y patch, one row more than a patch, exactly one patch and one group of six planes, a
last group of planes that is incomplete, marches longer than the grid.

Every setting runs on K + 0.37 M with the five Dirichlet sets of test_stencil_form_is_lossless, over the whole grid, the slab [1, nz - 1)
and the plane nz // 2, as a PCG-like product (w = x), with a third vector as w, and as a plain pgd_spmv (store, no dot).  Per run:
 (a) y meets the longdouble product of the operator's own CSR values within 4e-15 (|A||x|)_i per row;
 (b) y is the y of the CSR kernel (PGD_TUNE_SPMV_SYM = 0), bit for bit, as include/pgd_amd.h promises for every form of the product;
 (c) rows outside the range keep the value the vector was filled with;
 (d) the fused dot meets math.fsum of w_i y_i over the kernel's own y within 1e-12 sum |w_i y_i|, and at least 95 % of the rows of the
     range carry a term above that bar (so a row left out or added twice would be seen);
 (e) exactly the expected kernel counter moves, by one - pgd_product_plan names the same family, the fetch depth 6 of the stencil march
     always reports four rows per thread, and no stencil march is shorter than its fetch depth;
 (f) every knob is back at its default afterwards, whatever happened.
A product whose w is a third vector is no march (the marches fuse the dot with x only): it must run in row order, k_spmv_dia_rows.
The NTY instances (non-temporal y) are launched only inside the single-sync recurrence: tests/pcg_form_cases.py, test_pcg_*_gpu.py.

Run with -s for one line per setting: the largest error / bound of (a) and (d), the smallest share of (d) and the whole-grid plan."""
import numpy as np
import pytest

from oracle import fem_numpy as F
from tests import product_variant_reference as R

pytestmark = pytest.mark.gpu

# knob numbers (include/pgd_amd.h)
SYM, FORCE, PLANE_BYTES, VARIANT, CLASSES, FETCH, STENCIL, ZSTENCIL, DEPTH, MARCH3, ROWS = 3, 7, 8, 13, 19, 24, 35, 36, 38, 47, 48
DEFAULTS = {SYM: 1, FORCE: 0, PLANE_BYTES: 0, VARIANT: 0, CLASSES: 1, FETCH: 6, STENCIL: 1, ZSTENCIL: 0, DEPTH: 0, MARCH3: 0, ROWS: 0}
POISON = -7.0


def _dictionary(fetch):
    """k_spmv_diac_march2 at forced march lengths in whole sixes: six plane fetches in flight unless PGD_TUNE_SPMV_FETCH_DEPTH = 3."""
    return [{"name": "march%d fetch%d" % (L, fetch), "knobs": {FORCE: L, FETCH: fetch}, "family": "diac_march",
             "instance": "k_spmv_diac_march2<D=%d>" % fetch} for L in (12, 18, 24, 1002)]


def _stencil(depth):
    """k_spmv_stencil_march: the operators that are one stencil take it, the other three keep the dictionary march (of 4 planes)."""
    out = []
    for rows in (0, 2, 4):
        for L in (1, 5, 6, 7, 12, 13, 1000):
            rwt = 2 if (rows == 2 and depth == 3) else 4
            out.append({"name": "depth%d rows%d march%d" % (depth, rows, L), "knobs": {FORCE: 4, ZSTENCIL: L, DEPTH: depth, ROWS: rows},
                        "family": "stencil_march", "other": "diac_march", "depth": depth, "rows_per_thread": rwt,
                        "instance": "k_spmv_stencil_march<D=%d, RWT=%d>" % (depth, rwt)})
    return out


def _plain():
    """The marches over the slot values themselves (row classes off)."""
    names = {(0, 0): "k_spmv_dia_march2", (0, 1): "k_spmv_dia_march3", (1, 0): "k_spmv_dia_march<8>", (1, 1): "k_spmv_dia_march<8>",
             (2, 0): "k_spmv_dia_march<4>", (2, 1): "k_spmv_dia_march<4>"}
    return [{"name": "variant%d march3=%d march%d" % (v, m3, L), "knobs": {CLASSES: 0, VARIANT: v, MARCH3: m3, FORCE: L},
             "family": "dia_march", "instance": names[(v, m3)]} for v in (0, 1, 2) for m3 in (0, 1) for L in (1, 3, 16)]


# one setting per reachable instance and march length; "family": the kernel counter that must move for a PCG-like or plain product
# ("other": for the operators that are not one stencil)
SETTINGS = {
    "dictionary six-deep": _dictionary(6),
    "dictionary three-deep": _dictionary(3) + [
        # above DIAC_MAXCHUNK = 1024 planes per march the plan must leave the dictionary march
        {"name": "march1026", "knobs": {FORCE: 1026, FETCH: 6}, "family": "dia_march", "instance": "k_spmv_dia_march2 (no dictionary march)"}],
    "stencil depth 3": _stencil(3),
    "stencil depth 6": _stencil(6),
    "plain": _plain(),
}


def restore(ctx):
    for k, v in DEFAULTS.items():
        ctx.tune(k, v)


@pytest.fixture(scope="module", params=sorted(R.SHAPES))
def lattice(request, ctx):
    """Mesh, vectors and the five classified operators of one shape; per operator the longdouble reference from its own CSR values and
    the y of the CSR kernel."""
    shape = R.SHAPES[request.param]
    nx, ny, nz = shape
    coords, cells = F.box_mesh((0, 0, 0), R.BOX, nx - 1, ny - 1, nz - 1)
    h = ctx.mesh_upload(coords, cells)
    n = coords.shape[0]
    assert n == nx * ny * nz
    rp, cols = ctx.mesh_pattern(h)
    nnz = ctx.mesh_info(h)["nnz"]
    ak, am = ctx.atom_assemble(h, F.STIFF), ctx.atom_assemble(h, F.MASS)
    bcs = R.boundary_sets(coords, shape)
    x, w = R.vectors(n)
    xv, wv, yv = ctx.vec_from(x), ctx.vec_from(w), ctx.vec_alloc(n)
    ctx.flags_reset()
    ops, ref, y_csr = {}, {}, {}
    try:
        restore(ctx)
        for name in R.BOUNDARIES:
            op = ctx.op_combine(h, [ak, am], list(R.COEFS), bcs[name])
            ref[name] = R.csr_product(rp, cols, ctx.atom_download(op, nnz), x)
            assert ctx.op_symmetrize(op) is True
            assert 1 <= ctx.op_classify(op) <= 255
            ctx.tune(SYM, 0)
            k0 = ctx.kernel_counts()
            ctx.vec_fill(yv, POISON)
            ctx.spmv_dot_slot(op, xv, yv, xv, 0, n, 30)
            k1 = ctx.kernel_counts()
            ctx.tune(SYM, 1)
            assert {k for k in k1 if k1[k] != k0[k]} <= {"csr", "csr_dict"}, name
            y_csr[name] = ctx.vec_download(yv)
            assert R.row_excess(y_csr[name], ref[name][0], ref[name][1], 0, n) <= 1.0, name
            ops[name] = op
    finally:
        restore(ctx)
    yield {"shape": request.param, "n": n, "x": x, "w": w, "xv": xv, "wv": wv, "yv": yv, "ops": ops, "ref": ref, "y_csr": y_csr,
           "ranges": R.row_ranges(shape)}
    for v in (xv, wv, yv):
        ctx.vec_free(v)
    for a in list(ops.values()) + [ak, am]:
        ctx.atom_free(a)
    ctx.mesh_free(h)


def expected_family(setting, boundary, kind):
    if kind == "third vector":
        return "dia_rows"
    if "other" in setting and boundary not in R.ONE_STENCIL:
        return setting["other"]
    return setting["family"]


def run_setting(ctx, g, setting):
    """(a) - (e) for one setting, under the knobs already set: (largest row error / bound, largest dot error / bar, smallest share)."""
    x, xv, wv, yv, n = g["x"], g["xv"], g["wv"], g["yv"], g["n"]
    worst_row = worst_dot = 0.0
    least_share = 1.0
    for bname in R.BOUNDARIES:
        op, (y_ref, rowabs), y_csr = g["ops"][bname], g["ref"][bname], g["y_csr"][bname]
        for rname, (r0, r1) in g["ranges"].items():
            for kind in ("w = x", "third vector", "store only"):
                what = (g["shape"], setting["name"], bname, rname, kind)
                family = expected_family(setting, bname, kind)
                plan = ctx.product_plan(op, r0, r1, kind != "third vector")
                assert plan["family"] == family, (what, plan)                                              # (e)
                if family == "stencil_march":
                    assert plan["depth"] == setting["depth"] and plan["rows_per_thread"] == setting["rows_per_thread"], (what, plan)
                    assert plan["depth"] != 6 or plan["rows_per_thread"] == 4, (what, plan)
                    assert plan["zchunk"] >= plan["depth"], (what, plan)
                elif family != "dia_rows":
                    assert plan["zchunk"] == setting["knobs"][FORCE], (what, plan)
                ctx.vec_fill(yv, POISON)
                k0 = ctx.kernel_counts()
                if kind == "store only":
                    ctx.spmv(op, xv, yv, r0, r1)
                else:
                    ctx.spmv_dot_slot(op, xv, yv, xv if kind == "w = x" else wv, r0, r1, 31)
                k1 = ctx.kernel_counts()
                assert {k: k1[k] - k0[k] for k in k1 if k1[k] != k0[k]} == {family: 1}, (what, plan)
                y = ctx.vec_download(yv)
                row = R.row_excess(y, y_ref, rowabs, r0, r1)                                               # (a)
                worst_row = max(worst_row, row)
                assert row <= 1.0, (what, plan, row)
                assert np.array_equal(y[r0:r1], y_csr[r0:r1]), (what, plan, (r0 + np.where(y[r0:r1] != y_csr[r0:r1])[0])[:8])   # (b)
                assert np.all(y[:r0] == POISON) and np.all(y[r1:] == POISON), (what, plan)                 # (c)
                if kind != "store only":                                                                   # (d)
                    wh = x if kind == "w = x" else g["w"]
                    share = R.dot_share(wh, y, r0, r1)
                    least_share = min(least_share, share)
                    assert share >= R.DOT_SHARE, (what, share)
                    d_ref, bar = R.dot_reference(wh, y, r0, r1)
                    err = abs(ctx.slots_download(31, 1)[0] - d_ref)
                    worst_dot = max(worst_dot, err / bar)
                    assert err <= bar, (what, plan, err, bar)
    return worst_row, worst_dot, least_share


@pytest.mark.parametrize("group", list(SETTINGS))
def test_every_instance_at_the_seams(ctx, lattice, group):
    g = lattice
    hull = g["ops"]["hull"]
    for setting in SETTINGS[group]:
        try:
            for k, v in setting["knobs"].items():
                ctx.tune(k, v)
            plan = ctx.product_plan(hull)
            worst_row, worst_dot, share = run_setting(ctx, g, setting)
            print("%-9s %-22s %-28s %-44s row error / bound %.3f  dot error / bar %.2e  share %.3f  plan %s" % (
                g["shape"], group, setting["name"], setting["instance"], worst_row, worst_dot, share,
                {k: plan[k] for k in ("family", "wgs", "zchunk", "tiles_x", "tiles_y", "rows_per_thread", "depth")}))
        finally:
            restore(ctx)                                                                                   # (f)


def test_planes_below_the_size_threshold_run_in_row_order(ctx, lattice):
    """PGD_TUNE_SPMV_GRID_MIN_BYTES: the marches are for grids whose planes of slot values (64 bytes per row) have at least that many
    bytes.  At exactly the plane's size the forced march still runs; one byte more and every product is k_spmv_dia_rows - with the
    same y, dots and untouched rows, (a) - (e) as for every other setting."""
    g = lattice
    plane = g["ranges"]["one plane"][1] - g["ranges"]["one plane"][0]
    for threshold, family in ((64 * plane, "diac_march"), (64 * plane + 1, "dia_rows")):
        setting = {"name": "plane bytes %d" % threshold, "knobs": {FORCE: 4}, "family": family}
        try:
            ctx.tune(FORCE, 4)
            ctx.tune(PLANE_BYTES, threshold)
            worst_row, worst_dot, share = run_setting(ctx, g, setting)
            print("%-9s %-22s %-28s %-44s row error / bound %.3f  dot error / bar %.2e  share %.3f" % (
                g["shape"], "plane-size threshold", setting["name"], "k_spmv_dia_rows" if family == "dia_rows" else "k_spmv_diac_march2<D=3>",
                worst_row, worst_dot, share))
        finally:
            restore(ctx)


def test_the_table_reaches_every_instance():
    """SETTINGS names every instance the product launchers can select by form, depth, rows per thread and variant."""
    reached = {s["instance"] for group in SETTINGS.values() for s in group}
    assert reached >= {"k_spmv_diac_march2<D=6>", "k_spmv_diac_march2<D=3>", "k_spmv_stencil_march<D=3, RWT=2>",
                       "k_spmv_stencil_march<D=3, RWT=4>", "k_spmv_stencil_march<D=6, RWT=4>", "k_spmv_dia_march2", "k_spmv_dia_march3",
                       "k_spmv_dia_march<8>", "k_spmv_dia_march<4>"}
    # six plane fetches need a march of at least 12 planes in whole sixes (plan_product), and the depth 6 of the stencil march has no
    # two-row instance
    for s in SETTINGS["dictionary six-deep"]:
        assert s["knobs"][FORCE] >= 12 and s["knobs"][FORCE] % 6 == 0 and s["knobs"][FETCH] == 6
    assert all(s["rows_per_thread"] == 4 for s in SETTINGS["stencil depth 6"])
    assert {s["rows_per_thread"] for s in SETTINGS["stencil depth 3"]} == {2, 4}
