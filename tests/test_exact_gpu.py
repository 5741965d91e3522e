"""Every assembled atom, product kernel, facet atom, blocked layout and the frontend on the MI355X against the exact rational
reference (tests/exact_reference.py), through the C-ABI.

Tolerances (per row, against the exact cell contributions S_ij = sum over cells |K_e,ij|):
- atoms: |got_ij - exact_ij| <= 1e-14 max_j S_ij;
- products: |y_i - (A_exact x)_i| <= 1e-14 sum_j S_ij |x_j|.
Run with -s to see the largest error per kernel family as a fraction of its bound.
"""
from fractions import Fraction

import numpy as np
import pytest

from tests import exact_reference as X
from tests import test_exact_cpu as T

pytestmark = pytest.mark.gpu

MESHES = X.mesh_matrix()
TOL = 1e-14
WORST = {}                     # kernel family -> largest error / bound seen
FAMILIES = ("csr", "csr_dict", "sym_rows", "dia_rows", "dia_march", "multi", "diac_march", "stencil_march")
_LAYOUTS = {}


def exact_layout(name):
    if name not in _LAYOUTS:
        _LAYOUTS[name] = X.ExactLayout(*MESHES[name]())
    return _LAYOUTS[name]


def note(family, q):
    WORST[family] = max(WORST.get(family, 0.0), float(q))


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    print("\nlargest error / bound per family:")
    for k in sorted(WORST):
        print("  %-28s %.4f" % (k, WORST[k]))


def asm_family(lay, lattice=None):
    if lay.degree == 2:
        return "assemble_p2_interval" if lay.D == 1 else "assemble_p2_simplex<%d>" % lay.D
    return "assemble_p1<%d>" % lay.D + ("" if lattice is None else " lattice knob %d" % lattice)


def check_atom(ctx, h, lay, kind, a, b, w, family):
    wv = ctx.vec_from(w) if kind in (X.WMASS, X.WSTIFF) else 0
    try:
        at = ctx.atom_assemble(h, kind, a, b, wv)
        got = ctx.atom_download(at, lay.nnz)
        ctx.atom_free(at)
    finally:
        if wv:
            ctx.vec_free(wv)
    vals, S = lay.atom(kind, a, b, w if kind in (X.WMASS, X.WSTIFF) else None)
    q = X.entry_excess(lay, got, vals, S, TOL)
    note(family, q)
    assert q <= 1.0, (family, X.KIND_NAMES[kind], a, b, q)
    return got


@pytest.mark.parametrize("name", sorted(MESHES))
def test_atoms_are_exact(ctx, name):
    lay = exact_layout(name)
    h = ctx.mesh_upload(lay.coords, lay.cells.astype(np.int32))
    try:
        rp, cols = ctx.mesh_pattern(h)
        assert np.array_equal(rp, lay.rp) and np.array_equal(cols, lay.cols)
        w = X.weight_of(lay.coords)
        for kind, a, b in X.kinds_and_pairs(lay.D):
            check_atom(ctx, h, lay, kind, a, b, w, asm_family(lay))
    finally:
        ctx.mesh_free(h)


def lattice_layout(shape):
    return X.ExactLayout(*X.lattice_box(shape))


@pytest.mark.parametrize("name", sorted(X.LATTICE_SHAPES))
def test_lattice_boxes_are_exact_under_every_lattice_form(ctx, name):
    """Axis-aligned dyadic boxes (non-zero origin, a different step per axis; 2 vertices along x; 2 planes along z):
    detected as lattices with the exact steps, and every kind / pair within the exact bound under PGD_TUNE_ASM_LATTICE
    1 (index steps, the regular kernel for unweighted kinds on the 6-tetrahedra numbering), 3 (index steps in the general
    kernel) and 2 (steps rounded from the coordinates)."""
    shape = X.LATTICE_SHAPES[name]
    lay = lattice_layout(shape)
    h = ctx.mesh_upload(lay.coords, lay.cells.astype(np.int32))
    w = X.weight_of(lay.coords)
    try:
        is_lat, steps = ctx.mesh_lattice(h)
        # detect_lattice: a 3-D structured vertex grid with origin + index * step coordinates; planes of 2 x n vertices
        # qualify (the unit-cell form, which needs 3 x 3, is not observable through the ABI - its atoms must be the same)
        assert is_lat and np.array_equal(steps, [0.25, 0.5, 0.125])
        for knob in (1, 3, 2):
            ctx.tune(20, knob)
            for kind, a, b in X.kinds_and_pairs(3):
                check_atom(ctx, h, lay, kind, a, b, w, "assemble_p1<3> lattice knob %d" % knob)
    finally:
        ctx.tune(20, 1)
        ctx.mesh_free(h)


def test_near_lattices(ctx):
    """One interior vertex moved by 2^-30 (about 1e-9 relative): NOT a lattice, so the exact geometry is used - the
    index-derived one is off by far more than the bound.  Moved by 2 ulp: within the 8-ulp test, it may stay on the
    lattice path; only the bound is asserted."""
    coords, cells = X.lattice_box(X.LATTICE_SHAPES["lattice_4x3x3"])
    nx, ny = 5, 4
    v = 2 + nx * (1 + ny * 1)                                           # vertex (2, 1, 1): interior
    far = coords.copy()
    far[v, 0] += 2.0 ** -30
    near = coords.copy()
    near[v, 0] = np.nextafter(np.nextafter(near[v, 0], np.inf), np.inf)
    w = X.weight_of(coords)
    for label, c in (("moved 2^-30", far), ("moved 2 ulp", near)):
        lay = X.ExactLayout(c, cells)
        h = ctx.mesh_upload(c, cells)
        try:
            if label == "moved 2^-30":
                assert not ctx.mesh_lattice(h)[0]
            for knob in (1, 3, 2):
                ctx.tune(20, knob)
                for kind, a, b in X.kinds_and_pairs(3):
                    check_atom(ctx, h, lay, kind, a, b, w, "assemble_p1<3> %s" % label)
        finally:
            ctx.tune(20, 1)
            ctx.mesh_free(h)


# ------------------------------------------------------------------------------------------------- products
SYMMETRIC = {X.MASS, X.STIFF, X.WMASS, X.WSTIFF}
REACHED_ALL = set()            # product kernel families reached over the mesh matrix


def counts_delta(ctx, before):
    after = ctx.kernel_counts()
    return [k for k in FAMILIES if after[k] > before[k]]


def check_product(lay, S, vals, x, y, rows, family):
    bound = X.product_bound(lay, S, x, TOL)[rows]
    ex = lay.matvec(vals, x)
    err = X.exact_errors(y[rows], ex[rows])
    q = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    note(family, q)
    assert np.all(err <= bound), (family, q)


@pytest.mark.parametrize("name", sorted(MESHES))
def test_products_are_exact(ctx, name):
    """y = A x for every atom at x = a polynomial's nodal values and at a random dyadic x, all rows and [r0, r1), under
    PGD_TUNE_SPMV_DICT 0 / 1 / 2; the symmetric kinds also through pgd_op_combine + pgd_op_symmetrize and the products of
    the SPD solves under PGD_TUNE_SPMV_SYM 0 / 1."""
    lay = exact_layout(name)
    n = lay.n
    h = ctx.mesh_upload(lay.coords, lay.cells.astype(np.int32))
    w = X.weight_of(lay.coords)
    xs = [np.array([float(v) for v in T.exact_nodal(T.polys(lay.D, lay.degree)[0], lay.coords)]),
          np.random.default_rng(n).integers(-64, 65, n) / 64.0]
    r0, r1 = n // 3, max(n // 3 + 1, 2 * n // 3)
    wv = ctx.vec_from(w)
    yv = ctx.vec_alloc(n)
    reached = set()
    try:
        for kind, a, b in X.kinds_and_pairs(lay.D):
            weighted = kind in (X.WMASS, X.WSTIFF)
            at = ctx.atom_assemble(h, kind, a, b, wv if weighted else 0)
            vals, S = lay.atom(kind, a, b, w if weighted else None)
            sym = kind in SYMMETRIC or (kind == X.DUDV and a == b)
            op = ctx.op_combine(h, [at], [1.0], np.zeros(0, dtype=np.int32)) if sym else 0
            if op:
                ctx.op_symmetrize(op)
            try:
                for x in xs:
                    xv = ctx.vec_from(x)
                    try:
                        for d in (0, 1, 2):
                            ctx.tune(2, d)
                            before = ctx.kernel_counts()
                            ctx.spmv(at, xv, yv)
                            fam = counts_delta(ctx, before)
                            reached.update(fam)
                            check_product(lay, S, vals, x, ctx.vec_download(yv), np.arange(n), "spmv " + "+".join(fam))
                            ctx.vec_fill(yv, -7.0)
                            ctx.spmv(at, xv, yv, r0, r1)
                            y = ctx.vec_download(yv)
                            assert np.all(y[:r0] == -7.0) and np.all(y[r1:] == -7.0)
                            check_product(lay, S, vals, x, y, np.arange(r0, r1), "spmv " + "+".join(fam))
                        ctx.tune(2, 1)
                        if op:
                            for s in (0, 1):
                                ctx.tune(3, s)
                                ctx.flags_reset()
                                before = ctx.kernel_counts()
                                ctx.spmv_dot_slot(op, xv, yv, xv, 0, n, 40)
                                fam = counts_delta(ctx, before)
                                reached.update(fam)
                                check_product(lay, S, vals, x, ctx.vec_download(yv), np.arange(n), "op " + "+".join(fam))
                            ctx.tune(3, 1)
                    finally:
                        ctx.vec_free(xv)
            finally:
                ctx.tune(2, 1)
                ctx.tune(3, 1)
                ctx.atom_free(at)
                if op:
                    ctx.atom_free(op)
    finally:
        ctx.vec_free(wv)
        ctx.vec_free(yv)
        ctx.mesh_free(h)
    assert "csr" in reached
    REACHED_ALL.update(reached)



def test_product_families_were_reached():
    """Over the mesh matrix the products went through the streaming CSR kernel, the column-dictionary kernels and the
    symmetric half storage (row order on 2-D grids; its diagonal forms on 3-D grids)."""
    if not REACHED_ALL:
        pytest.skip("run together with test_products_are_exact")
    assert {"csr", "csr_dict", "sym_rows"} <= REACHED_ALL, REACHED_ALL


# ------------------------------------------------------------------------------------------------ facet atom
FACET_LAYOUTS = ["p1_interval_nonuniform", "p1_tri_jitter", "p1_tri_shear", "p1_tet_jitter", "p1_tet_shear",
                 "p2_interval_nonuniform", "p2_tri_jitter", "p2_tri_shear", "p2_tet_jitter", "p2_tet_shear"]


def reversed_facets(tup, D, degree):
    """The same facets with their vertices in reversed order (P2: the edge nodes follow, edge e is opposite vertex e)."""
    if D == 1:
        return tup.copy()
    if D == 2:
        return np.concatenate([tup[:, 1::-1], tup[:, 2:]], axis=1)
    return np.concatenate([tup[:, 2::-1], tup[:, 3:][:, ::-1]], axis=1)


@pytest.mark.parametrize("name", FACET_LAYOUTS)
def test_facet_atom_is_exact(ctx, name):
    lay = exact_layout(name)
    h = ctx.mesh_upload(lay.coords, lay.cells.astype(np.int32))
    try:
        allf, right = T.exterior_facets(lay, lay.D)
        assert right.shape[0] > 0
        for label, tup in (("exterior", allf), ("tagged", right), ("reversed", reversed_facets(allf, lay.D, lay.degree))):
            at = ctx.atom_assemble_facets(h, tup)
            got = ctx.atom_download(at, lay.nnz)
            ctx.atom_free(at)
            vals, S = X.facet_mass(lay, tup)
            q = X.entry_excess(lay, got, vals, S, TOL)
            note("assemble_facets", q)
            assert q <= 1.0, (label, q)
    finally:
        ctx.mesh_free(h)


# ------------------------------------------------------------------------------------------------ blocked layouts
@pytest.mark.parametrize("name,ncomp", [("p2_tri_shear", 2), ("p2_tet_jitter", 3)])
def test_blocked_elasticity_sum_is_exact(ctx, name, ncomp):
    """pgd_mesh_blocked + pgd_atom_embed: an elasticity-like sum of embedded dudv atoms (every (a, b) into block (b, a))
    and a mass block, against the exact scalar blocks (dof = ncomp node + component)."""
    lay = exact_layout(name)
    D = lay.D
    h = ctx.mesh_upload(lay.coords, lay.cells.astype(np.int32))
    bh = ctx.mesh_blocked(h, ncomp)
    coefs = [2.0, 0.5, 0.75, 1.0, 0.25, 1.5]
    terms = [(X.DUDV, a, b, b % ncomp, a % ncomp, coefs[(a + 2 * b) % 6]) for a in range(D) for b in range(D)]
    terms.append((X.MASS, 0, 0, ncomp - 1, 0, 0.25))
    try:
        dst = 0
        for kind, a, b, cv, cu, coef in terms:
            at = ctx.atom_assemble(h, kind, a, b, 0)
            dst = ctx.atom_embed(bh, at, cv, cu, coef, dst)
            ctx.atom_free(at)
        rp, cols = ctx.mesh_pattern(bh)
        got = ctx.atom_download(dst, int(rp[-1]))
        ctx.atom_free(dst)
    finally:
        ctx.mesh_free(bh)
        ctx.mesh_free(h)
    rows = np.repeat(np.arange(rp.size - 1), np.diff(rp))
    i, cv, j, cu = rows // ncomp, rows % ncomp, cols // ncomp, cols % ncomp
    key_pat = np.repeat(np.arange(lay.n, dtype=np.int64), np.diff(lay.rp)) * lay.n + lay.cols
    pos = np.searchsorted(key_pat, i.astype(np.int64) * lay.n + j)
    assert np.array_equal(key_pat[pos], i.astype(np.int64) * lay.n + j)
    exact = np.empty(rows.size, dtype=object)
    exact[:] = [0] * rows.size
    S = np.zeros(rows.size)
    for kind, a, b, tv, tu, coef in terms:
        vals, Sk = lay.atom(kind, a, b)
        m = (cv == tv) & (cu == tu)
        exact[m] = exact[m] + vals[pos[m]] * Fraction(coef)
        S[m] += abs(coef) * Sk[pos[m]]
    err = X.exact_errors(got, exact)
    rmax = np.repeat(np.maximum.reduceat(S, rp[:-1]), np.diff(rp))
    q = float((err / np.maximum(TOL * rmax, 1e-300)).max())
    note("atom_embed (blocked)", q)
    assert np.all(err <= TOL * rmax), q


# ------------------------------------------------------------------------------------------ frontend on the device
@pytest.fixture(scope="module")
def hip_backend():
    from pgdrome_amd import fem
    from pgdrome_amd.hip_backend import HipBackend
    old = fem._backend
    be = fem.set_backend(HipBackend(0))
    fem.clear_caches()
    yield be
    fem.set_backend(old)
    fem.clear_caches()


@pytest.mark.parametrize("case", sorted(T.FRONTEND))
def test_frontend_is_exact_on_the_device(hip_backend, case):
    name, degree = T.FRONTEND[case]
    note("frontend functionals", T.check_frontend_functionals(T.frontend_mesh(name), degree))
    note("frontend matrices", T.check_frontend_matrices(T.frontend_mesh(name), degree))


@pytest.mark.parametrize("name,degree", [("p1_tri_shear", 1), ("p1_tri_reversed", 2), ("p1_tet_reordered", 1),
                                         ("small_tet_shear", 2)])
def test_frontend_elasticity_is_exact_on_the_device(hip_backend, name, degree):
    note("frontend elasticity", T.check_elasticity(T.frontend_mesh(name), degree))
