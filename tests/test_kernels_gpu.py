"""Parity of every HIP kernel against the oracle, called through the C-ABI.

Index data (CSR pattern) must be bit-exact; float64 results are compared with
the tolerances written next to each assertion (summation order differs between
scipy and the owner-computes kernels, nothing else does).
"""
import numpy as np
import pytest
import scipy.sparse as sps

from oracle import fem_numpy as F

pytestmark = pytest.mark.gpu

MESHES = {
    "interval33": lambda: F.interval_mesh(32, 0.0, 2.0),
    "interval2": lambda: F.interval_mesh(1, 0.0, 1.0),
    "interval1000": lambda: F.interval_mesh(999, -1.0, 3.0),
    "rect17x9": lambda: F.rectangle_mesh((0, 0), (2, 1), 16, 8),
    "rect64": lambda: F.rectangle_mesh((0, 0), (1, 1), 63, 63),
    "box6x5x4": lambda: F.box_mesh((0, 0, 0), (1, 2, 3), 5, 4, 3),
    "box20": lambda: F.box_mesh((0, 0, 0), (1, 1, 1), 19, 19, 19),
    # quadratic elements on triangles / tetrahedra (6 / 10 nodes per cell); geometry jittered below
    "p2tri9x7": lambda: F.rectangle_mesh((0, 0), (2, 1), 9, 7),
    "p2tet4x3x3": lambda: F.box_mesh((0, 0, 0), (1, 2, 1), 4, 3, 3),
    "p2tet9": lambda: F.box_mesh((0, 0, 0), (1, 1, 1), 9, 9, 9),
}


def jitter(coords, cells, seed=7):
    """Unstructured-like geometry on the same topology: move interior vertices."""
    rng = np.random.default_rng(seed)
    lo, hi = coords.min(axis=0), coords.max(axis=0)
    h = (hi - lo).min() / (round(coords.shape[0] ** (1.0 / coords.shape[1])) + 1)
    out = coords.copy()
    interior = np.all((coords > lo + 1e-12) & (coords < hi - 1e-12), axis=1)
    out[interior] += rng.uniform(-0.2 * h, 0.2 * h, size=(interior.sum(), coords.shape[1]))
    return out


@pytest.fixture(scope="module", params=sorted(MESHES))
def mesh(request, ctx):
    coords, cells = MESHES[request.param]()
    if request.param in ("rect17x9", "box6x5x4", "p2tri9x7", "p2tet4x3x3"):
        coords = jitter(coords, cells)
    if request.param.startswith("p2"):
        coords, cells = F.p2_simplex_nodes(coords, cells)     # straight-sided: edge nodes at the midpoints
    h = ctx.mesh_upload(coords, cells)
    yield request.param, coords, cells, h
    ctx.mesh_free(h)


def test_pattern_bit_exact(ctx, mesh):
    name, coords, cells, h = mesh
    rp, cols = ctx.mesh_pattern(h)
    rp_o, cols_o = F.csr_pattern(coords.shape[0], cells)
    assert np.array_equal(rp, rp_o)
    assert np.array_equal(cols, cols_o)
    info = ctx.mesh_info(h)
    assert info["nnz"] == rp_o[-1] and info["nv"] == coords.shape[0]
    rows = np.repeat(np.arange(coords.shape[0]), np.diff(rp_o))
    assert info["kl"] == (rows - cols_o).max() and info["ku"] == (cols_o - rows).max()


def test_pattern_sizes_match_survey_formulas(ctx):
    c, e = F.box_mesh((0, 0, 0), (1, 1, 1), 11, 11, 11)
    h = ctx.mesh_upload(c, e)
    assert ctx.mesh_info(h)["nnz"] == F.nnz_p1_box(12)
    ctx.mesh_free(h)
    c, e = F.rectangle_mesh((0, 0), (1, 1), 30, 30)
    h = ctx.mesh_upload(c, e)
    assert ctx.mesh_info(h)["nnz"] == F.nnz_p1_rect(31)
    ctx.mesh_free(h)


@pytest.mark.parametrize("kind", ["mass", "stiff", "dudv", "conv", "convt", "wmass", "wstiff"])
def test_atoms_match_oracle(ctx, mesh, kind):
    name, coords, cells, h = mesh
    gdim = coords.shape[1]
    k = F.KIND_NAMES.index(kind)
    da, db = (gdim - 1, 0) if kind in ("dudv", "conv", "convt") else (0, 0)
    w = None
    wv = 0
    if kind in ("wmass", "wstiff"):
        w = 1.0 + coords[:, 0] ** 2 + 0.5 * np.sin(coords.sum(axis=1))
        wv = ctx.vec_from(w)
    a = ctx.atom_assemble(h, k, da, db, wv)
    ref = F.assemble_atom(coords, cells, k, da, db, w)
    vals = ctx.atom_download(a, ref.nnz)
    scale = np.abs(ref.data).max()
    # float64, same closed forms, different summation order over <= 24 cells
    assert np.abs(vals - ref.data).max() <= 5e-14 * scale
    ctx.atom_free(a)
    if wv:
        ctx.vec_free(wv)


@pytest.mark.parametrize("shape", [(12, 9, 7), (5, 4, 3), (33, 20, 17)])
def test_lattice_assembly_from_vertex_indices_is_the_one_from_coordinates(ctx, shape):
    """On a uniform lattice whose cells span at most one step per axis k_assemble_p1<3> reads the edge vectors off the vertex
    INDICES (no coordinate gather, r04): bit for bit the atoms of the r03 form, which rounds coordinate differences to whole steps
    (PGD_TUNE_ASM_LATTICE = 2) - all seven kinds, different steps per axis, an origin that is not zero; and within the oracle's bar."""
    coords, cells = F.box_mesh((0.25, -1.0, 3.0), (1.0, 1.5, 3.7), *shape)
    h = ctx.mesh_upload(coords, cells)
    assert ctx.mesh_lattice(h)[0]
    nnz = ctx.mesh_info(h)["nnz"]
    w = 1.0 + coords[:, 0] ** 2 + 0.5 * np.sin(coords.sum(axis=1))
    wv = ctx.vec_from(w)
    try:
        for kind in range(7):
            for da, db in ((0, 0), (2, 1)) if F.KIND_NAMES[kind] in ("dudv", "conv", "convt") else ((0, 0),):
                weighted = F.KIND_NAMES[kind] in ("wmass", "wstiff")
                got = {}
                for knob in (1, 3, 2):         # nothing gathered (regular numbering, unweighted kinds) / index steps in the general kernel / r03
                    ctx.tune(20, knob)
                    a = ctx.atom_assemble(h, kind, da, db, wv if weighted else 0)
                    got[knob] = ctx.atom_download(a, nnz)
                    ctx.atom_free(a)
                assert np.array_equal(got[1], got[2]), (F.KIND_NAMES[kind], da, db, np.abs(got[1] - got[2]).max())
                assert np.array_equal(got[3], got[2]), (F.KIND_NAMES[kind], da, db, np.abs(got[3] - got[2]).max())
                ref = F.assemble_atom(coords, cells, kind, da, db, w if weighted else None)
                assert np.abs(got[1] - ref.data).max() <= 5e-14 * np.abs(ref.data).max()
        # the same lattice with its cells in another order (and their vertices rotated): not the regular numbering - the general
        # kernel takes it, the atoms are those of the oracle
        rng = np.random.default_rng(8)
        perm = rng.permutation(cells.shape[0])
        shuffled = np.roll(cells[perm], 1, axis=1).copy()
        h2 = ctx.mesh_upload(coords, shuffled)
        try:
            assert ctx.mesh_lattice(h2)[0]
            for kind in (F.STIFF, F.MASS):
                a = ctx.atom_assemble(h2, kind)
                ref = F.assemble_atom(coords, shuffled, kind)
                assert np.abs(ctx.atom_download(a, nnz) - ref.data).max() <= 5e-14 * np.abs(ref.data).max()
                ctx.atom_free(a)
        finally:
            ctx.mesh_free(h2)
    finally:
        ctx.tune(20, 1)
        ctx.vec_free(wv)
        ctx.mesh_free(h)


def test_assembly_is_bitwise_reproducible(ctx, mesh):
    name, coords, cells, h = mesh
    nnz = ctx.mesh_info(h)["nnz"]
    a1 = ctx.atom_assemble(h, F.STIFF)
    a2 = ctx.atom_assemble(h, F.STIFF)
    assert np.array_equal(ctx.atom_download(a1, nnz), ctx.atom_download(a2, nnz))
    ctx.atom_free(a1)
    ctx.atom_free(a2)


def test_spmv_bilinear_dot(ctx, mesh):
    name, coords, cells, h = mesh
    n = coords.shape[0]
    rng = np.random.default_rng(1234)
    K = F.assemble_atom(coords, cells, F.STIFF) + 0.3 * F.assemble_atom(coords, cells, F.MASS)
    a = ctx.atom_upload(h, K.data)
    x, w = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    xv, wv, yv = ctx.vec_from(x), ctx.vec_from(w), ctx.vec_alloc(n)
    ctx.spmv(a, xv, yv)
    y = ctx.vec_download(yv)
    y_ref = K @ x
    rowabs = np.abs(K) @ np.abs(x)
    assert np.all(np.abs(y - y_ref) <= 4e-15 * rowabs + 1e-300)        # <= a few ulp per row
    # sub-range (row-sharded SpMV): rows outside [r0, r1) untouched
    r0, r1 = n // 3, 2 * n // 3 + 1
    ctx.vec_fill(yv, -7.0)
    ctx.spmv(a, xv, yv, r0, r1)
    y2 = ctx.vec_download(yv)
    assert np.array_equal(y2[r0:r1], y[r0:r1]) and np.all(y2[:r0] == -7.0) and np.all(y2[r1:] == -7.0)
    bl = ctx.bilinear(a, wv, xv)
    assert abs(bl - w @ y_ref) <= 1e-13 * (np.abs(w) @ rowabs)
    blr = ctx.bilinear(a, wv, xv, r0, r1)
    assert abs(blr - w[r0:r1] @ y_ref[r0:r1]) <= 1e-13 * (np.abs(w) @ rowabs)
    d = ctx.vec_dot(xv, wv)
    assert abs(d - x @ w) <= 1e-13 * (np.abs(x) @ np.abs(w))
    d2 = ctx.vec_dot(xv, wv, r0, r1)
    assert abs(d2 - x[r0:r1] @ w[r0:r1]) <= 1e-13 * (np.abs(x) @ np.abs(w))
    assert ctx.vec_dot(xv, wv) == d                                        # deterministic
    # batched functionals: 11 modes in one pass over the matrix
    Y = rng.uniform(-1, 1, (11, n))
    ys = [ctx.vec_from(Y[m]) for m in range(11)]
    many = ctx.bilinear_many(a, wv, ys)
    ref = np.array([w @ (K @ Y[m]) for m in range(11)])
    assert np.all(np.abs(many - ref) <= 1e-13 * (np.abs(w) @ (np.abs(K) @ np.abs(Y).max(axis=0))))
    for v in ys + [xv, wv, yv]:
        ctx.vec_free(v)
    ctx.atom_free(a)


@pytest.mark.parametrize("rows", [64, 128, 256])
def test_spmv_workgroup_shapes_agree(ctx, rows):
    """Every tile height of k_spmv_csr gives the same product (only the dot's partial order differs)."""
    coords, cells = F.box_mesh((0, 0, 0), (1, 1, 1), 30, 17, 23)
    h = ctx.mesh_upload(coords, cells)
    n = coords.shape[0]
    K = F.assemble_atom(coords, cells, F.STIFF)
    a = ctx.atom_upload(h, K.data)
    x = np.random.default_rng(8).uniform(-1, 1, n)
    xv, yv = ctx.vec_from(x), ctx.vec_alloc(n)
    from pgdrome_amd._lib import PgdError
    with pytest.raises(PgdError):
        ctx.tune(1, 100)
    ctx.tune(1, rows)
    try:
        ctx.spmv(a, xv, yv)
        y = ctx.vec_download(yv)
        assert np.all(np.abs(y - K @ x) <= 4e-15 * (np.abs(K) @ np.abs(x)))
        r0, r1 = 1000, n - 777
        bl = ctx.bilinear(a, xv, xv, r0, r1)
        assert abs(bl - x[r0:r1] @ (K @ x)[r0:r1]) <= 1e-12 * (np.abs(x) @ (np.abs(K) @ np.abs(x)))
    finally:
        ctx.tune(1, 64)
    ctx.mesh_free(h)


def test_column_dictionary_is_lossless(ctx):
    """k_spmv_csr_dict (column ids decoded from the relative-pattern dictionary) is bit-identical to the
    streaming kernel; an irregularly numbered mesh has no dictionary and takes the plain kernel."""
    rng = np.random.default_rng(21)
    for name, (coords, cells) in {"box": F.box_mesh((0, 0, 0), (1, 1, 1), 21, 13, 17),
                                  "rect": F.rectangle_mesh((0, 0), (1, 1), 50, 37),
                                  "interval": F.interval_mesh(1000, 0.0, 1.0)}.items():
        h = ctx.mesh_upload(coords, cells)
        n = coords.shape[0]
        count = ctx.mesh_dict_count(h)
        assert 1 <= count <= 64, (name, count)        # interior pattern + boundary variants
        K = F.assemble_atom(coords, cells, F.STIFF) + F.assemble_atom(coords, cells, F.MASS)
        a = ctx.atom_upload(h, K.data)
        x = rng.uniform(-1, 1, n)
        xv, y1, y2 = ctx.vec_from(x), ctx.vec_alloc(n), ctx.vec_alloc(n)
        out = {}
        for rows in (64, 128, 256):
            ctx.tune(1, rows)
            for d in (1, 0, 2):
                ctx.tune(2, d)
                ctx.spmv(a, xv, y1)
                out[(rows, d)] = (ctx.vec_download(y1), ctx.bilinear(a, xv, xv, 3, n - 2))
            for d in (1, 2):
                assert np.array_equal(out[(rows, d)][0], out[(rows, 0)][0])
                assert out[(rows, d)][1] == out[(rows, 0)][1]
        ctx.tune(1, 64)
        ctx.tune(2, 1)
        assert np.all(np.abs(out[(64, 1)][0] - K @ x) <= 4e-15 * (np.abs(K) @ np.abs(x)))
        ctx.mesh_free(h)
    # random renumbering of the vertices: every row has its own relative pattern -> no dictionary
    coords, cells = F.box_mesh((0, 0, 0), (1, 1, 1), 9, 9, 9)
    perm = rng.permutation(coords.shape[0])
    inv = np.argsort(perm)
    h = ctx.mesh_upload(coords[perm], inv[cells].astype(np.int32))
    assert ctx.mesh_dict_count(h) == 0
    K = F.assemble_atom(coords[perm], inv[cells].astype(np.int32), F.STIFF)
    a = ctx.atom_assemble(h, F.STIFF)
    x = rng.uniform(-1, 1, coords.shape[0])
    xv, yv = ctx.vec_from(x), ctx.vec_alloc(coords.shape[0])
    ctx.spmv(a, xv, yv)
    assert np.all(np.abs(ctx.vec_download(yv) - K @ x) <= 1e-13 * (np.abs(K) @ np.abs(x)))
    ctx.mesh_free(h)


@pytest.mark.parametrize("ncomp", [2, 3])
def test_blocked_layout_and_embedded_atoms(ctx, ncomp):
    """pgd_mesh_blocked / pgd_atom_embed against scipy's Kronecker product (dof = ncomp * node + component)."""
    coords, cells = F.rectangle_mesh((0, 0), (2, 1), 7, 5)
    coords = jitter(coords, cells)
    nodes, tab = F.p2_simplex_nodes(coords, cells)
    h = ctx.mesh_upload(nodes, tab)
    bh = ctx.mesh_blocked(h, ncomp)
    n = nodes.shape[0]
    rp, cols = ctx.mesh_pattern(bh)
    rp_s, cols_s = F.csr_pattern(n, tab)
    P = sps.kron(sps.csr_matrix((np.ones(cols_s.size), cols_s, rp_s), shape=(n, n)), np.ones((ncomp, ncomp))).tocsr()
    P.sort_indices()
    assert np.array_equal(rp, P.indptr) and np.array_equal(cols, P.indices)          # index data: bit-exact
    info = ctx.mesh_info(bh)
    rows = np.repeat(np.arange(n * ncomp), np.diff(rp))
    assert info["nv"] == n * ncomp and info["nnz"] == P.nnz
    assert info["kl"] >= (rows - cols).max() and info["ku"] >= (cols - rows).max()
    # an elasticity-like sum of embedded atoms
    terms = [(F.DUDV, 0, 0, 0, 0, 2.0), (F.DUDV, 1, 1, 0, 0, 0.5), (F.DUDV, 1, 1, 1, 1, 2.0), (F.DUDV, 0, 0, 1, 1, 0.5),
             (F.DUDV, 1, 0, 0, 1, 1.0), (F.DUDV, 0, 1, 1, 0, 1.0), (F.MASS, 0, 0, ncomp - 1, ncomp - 1, 0.3)]
    ref = sps.csr_matrix((n * ncomp, n * ncomp))
    dst = 0
    for kind, da, db, cv, cu, coef in terms:
        a = ctx.atom_assemble(h, kind, da, db, 0)
        dst = ctx.atom_embed(bh, a, cv, cu, coef, dst)
        E = np.zeros((ncomp, ncomp))
        E[cv, cu] = coef
        ref = ref + sps.kron(F.assemble_atom(nodes, tab, kind, da, db), E)
        ctx.atom_free(a)
    full = ref.tocsr()
    dense = full.toarray()
    vals = ctx.atom_download(dst, P.nnz)
    assert np.abs(vals - dense[rows, cols]).max() <= 1e-13 * np.abs(dense).max()
    # the blocked layout is a layout like any other: SpMV and PCG apply
    rng = np.random.default_rng(5)
    x = rng.uniform(-1, 1, n * ncomp)
    xv, yv = ctx.vec_from(x), ctx.vec_alloc(n * ncomp)
    ctx.spmv(dst, xv, yv)
    assert np.abs(ctx.vec_download(yv) - full @ x).max() <= 1e-12 * np.abs(full @ x).max()
    assert abs(full - full.T).max() < 1e-12 * np.abs(full.data).max()
    bc = np.where(np.repeat(nodes[:, 0] < 1e-9, ncomp))[0].astype(np.int32)
    op = ctx.op_combine(bh, [dst], [1.0], bc)
    A, b = F.apply_dirichlet((full + 0.7 * sps.identity(n * ncomp)).tocsr(), rng.uniform(-1, 1, n * ncomp), bc)
    ctx.atom_free(op)
    ident = ctx.atom_upload(bh, (rows == cols).astype(np.float64))
    op = ctx.op_combine(bh, [dst, ident], [1.0, 0.7], bc)
    bv, sv = ctx.vec_from(b), ctx.vec_alloc(n * ncomp)
    its, rel = ctx.pcg_solve(op, bv, sv, 1e-12, 0.0, 5000)
    sol = F.direct_solve(A, b)
    assert rel <= 1e-12 and np.linalg.norm(ctx.vec_download(sv) - sol) <= 1e-9 * np.linalg.norm(sol)
    with pytest.raises(RuntimeError):
        ctx.atom_assemble(bh, F.MASS)                      # blocked layouts have no geometry of their own
    for v in (xv, yv, bv, sv):
        ctx.vec_free(v)
    for a in (op, ident, dst):
        ctx.atom_free(a)
    ctx.mesh_free(bh)
    ctx.mesh_free(h)


@pytest.mark.parametrize("name", ["interval33", "rect17x9", "box6x5x4", "box20"])
def test_symmetric_half_storage_products(ctx, name):
    """k_spmv_sym (every off-diagonal value stored once, lower entries read from the neighbours' slots) against the
    oracle product, on full and partial row ranges, with Dirichlet rows eliminated; a non-symmetric operator is
    refused and keeps the CSR kernel."""
    coords, cells = MESHES[name]()
    if name in ("rect17x9", "box6x5x4"):
        coords = jitter(coords, cells)
    h = ctx.mesh_upload(coords, cells)
    n = coords.shape[0]
    K, M = F.assemble_atom(coords, cells, F.STIFF), F.assemble_atom(coords, cells, F.MASS)
    ak, am = ctx.atom_assemble(h, F.STIFF), ctx.atom_assemble(h, F.MASS)
    bc = boundary_dofs(coords)[::2].astype(np.int32)
    op = ctx.op_combine(h, [ak, am], [1.0, 0.37], bc)
    A, _ = F.apply_dirichlet((K + 0.37 * M).tocsr(), np.zeros(n), bc)
    rng = np.random.default_rng(99)
    x, w = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    xv, wv, yv = ctx.vec_from(x), ctx.vec_from(w), ctx.vec_alloc(n)
    ctx.flags_reset()
    ctx.tune(3, 0)                         # CSR kernels
    ctx.spmv_dot_slot(op, xv, yv, wv, 0, n, 30)
    ctx.tune(3, 1)
    y_csr, d_csr = ctx.vec_download(yv), ctx.slots_download(30, 1)[0]
    assert ctx.op_symmetrize(op) is True
    ctx.vec_fill(yv, -3.0)
    ctx.spmv_dot_slot(op, xv, yv, wv, 0, n, 31)
    y_sym, d_sym = ctx.vec_download(yv), ctx.slots_download(31, 1)[0]
    ref = A @ x
    rowabs = np.abs(A) @ np.abs(x)
    assert np.all(np.abs(y_sym - ref) <= 4e-15 * rowabs + 1e-300) and np.all(np.abs(y_csr - ref) <= 4e-15 * rowabs + 1e-300)
    assert abs(d_sym - w @ ref) <= 1e-13 * (np.abs(w) @ rowabs) and abs(d_sym - d_csr) <= 1e-13 * (np.abs(w) @ rowabs)
    r0, r1 = n // 3, 2 * n // 3 + 1
    ctx.vec_fill(yv, -7.0)
    ctx.spmv_dot_slot(op, xv, yv, wv, r0, r1, 32)
    y2 = ctx.vec_download(yv)
    assert np.array_equal(y2[r0:r1], y_sym[r0:r1]) and np.all(y2[:r0] == -7.0) and np.all(y2[r1:] == -7.0)
    assert abs(ctx.slots_download(32, 1)[0] - w[r0:r1] @ ref[r0:r1]) <= 1e-13 * (np.abs(w) @ rowabs)
    if name.startswith("box"):
        # structured vertex grids: the z-marching kernel with x planes in LDS, on the whole grid and on a slab of
        # planes as a row-sharded rank calls it
        nxy = {"box6x5x4": 6 * 5, "box20": 20 * 20}[name]
        for zc in (1, 3, 16):        # planes per workgroup march (forced: grids this small take the row-order kernel)
            ctx.tune(7, zc)
            ctx.vec_fill(yv, -5.0)
            ctx.spmv_dot_slot(op, xv, yv, xv, 0, n, 35)
            assert np.array_equal(ctx.vec_download(yv), y_sym)              # same per-row arithmetic, bit for bit
            assert abs(ctx.slots_download(35, 1)[0] - x @ ref) <= 1e-13 * (np.abs(x) @ rowabs)
        ctx.tune(7, 2)
        ctx.vec_fill(yv, -5.0)
        ctx.spmv_dot_slot(op, xv, yv, xv, nxy, 3 * nxy, 36)
        y3 = ctx.vec_download(yv)
        assert np.array_equal(y3[nxy:3 * nxy], y_sym[nxy:3 * nxy]) and np.all(y3[:nxy] == -5.0) and np.all(y3[3 * nxy:] == -5.0)
        assert abs(ctx.slots_download(36, 1)[0] - x[nxy:3 * nxy] @ ref[nxy:3 * nxy]) <= 1e-13 * (np.abs(x) @ rowabs)
        ctx.tune(7, 0)               # adaptive again: the row-order kernel gives the same rows
        ctx.vec_fill(yv, -5.0)
        ctx.spmv_dot_slot(op, xv, yv, xv, 0, n, 37)
        assert np.array_equal(ctx.vec_download(yv), y_sym)
    # the solve: same solution with and without the symmetric storage
    b = A @ rng.uniform(-1, 1, n)
    sols = []
    for sym in (1, 0):
        ctx.tune(3, sym)
        bv, sv = ctx.vec_from(b), ctx.vec_alloc(n)
        its, rel = ctx.pcg_solve(op, bv, sv, 1e-12, 0.0, 5000)
        sols.append((ctx.vec_download(sv), its))
        assert rel <= 1e-12
        ctx.vec_free(bv)
        ctx.vec_free(sv)
    ctx.tune(3, 1)
    assert np.linalg.norm(sols[0][0] - sols[1][0]) <= 1e-9 * np.linalg.norm(sols[1][0]) and abs(sols[0][1] - sols[1][1]) <= 2
    # ... and on the symmetrically scaled system (default) vs the unscaled recurrence on the same storage: the same
    # Krylov iterates up to rounding, the same stop test on the true residual
    ctx.tune(10, 0)
    bv, sv = ctx.vec_from(b), ctx.vec_from(0.1 * np.ones(n))
    its_u, rel_u = ctx.pcg_solve(op, bv, sv, 1e-12, 0.0, 5000)
    x_u = ctx.vec_download(sv)
    ctx.tune(10, 1)
    ctx.vec_upload(sv, 0.1 * np.ones(n))
    its_s, rel_s = ctx.pcg_solve(op, bv, sv, 1e-12, 0.0, 5000)
    x_s = ctx.vec_download(sv)
    assert rel_u <= 1e-12 and rel_s <= 1e-12 and abs(its_u - its_s) <= 2
    assert np.linalg.norm(x_s - x_u) <= 1e-9 * np.linalg.norm(x_u)
    assert np.linalg.norm(A @ x_s - b) <= 1.01e-12 * np.linalg.norm(b)            # the reported residual is the true one
    its0, rel0 = ctx.pcg_solve(op, bv, sv, 1e-12, 0.0, 5000)                        # converged start: nothing to do
    assert its0 == 0 and np.array_equal(ctx.vec_download(sv), x_s) or its0 <= 1
    ctx.vec_free(bv)
    ctx.vec_free(sv)
    # new values through the same handle: the copy is rebuilt
    op = ctx.op_combine(h, [ak, am], [2.0, 0.1], bc, op=op)
    assert ctx.op_symmetrize(op) is True
    ctx.flags_reset()                      # the solves above left the done flag set: later launches would be no-ops
    ctx.spmv_dot_slot(op, xv, yv, wv, 0, n, 33)
    A2, _ = F.apply_dirichlet((2.0 * K + 0.1 * M).tocsr(), np.zeros(n), bc)
    assert np.all(np.abs(ctx.vec_download(yv) - A2 @ x) <= 4e-15 * (np.abs(A2) @ np.abs(x)) + 1e-300)
    # not symmetric -> refused, CSR kernel keeps the result right
    ac = ctx.atom_assemble(h, F.CONV, 0, 0, 0)
    opn = ctx.op_combine(h, [ak, ac], [1.0, 0.5], np.zeros(0, dtype=np.int32))
    assert ctx.op_symmetrize(opn) is False
    ctx.spmv_dot_slot(opn, xv, yv, wv, 0, n, 34)
    An = (K + 0.5 * F.assemble_atom(coords, cells, F.CONV, 0, 0)).tocsr()
    assert np.all(np.abs(ctx.vec_download(yv) - An @ x) <= 4e-15 * (np.abs(An) @ np.abs(x)) + 1e-300)
    for v in (xv, wv, yv):
        ctx.vec_free(v)
    for a in (op, opn, ak, am, ac):
        ctx.atom_free(a)
    ctx.mesh_free(h)


GRID_SHAPES = {                      # vertices per axis: >= 2 x-tiles with a partial last tile, partial y-tiles, odd plane counts
    "130x37x41": (130, 37, 41),
    "65x4x9": (65, 4, 9),
    "257x9x33": (257, 9, 33),
    "64x8x5": (64, 8, 5),             # exactly one full tile in x
}


@pytest.mark.parametrize("shape", sorted(GRID_SHAPES))
def test_grid_march_in_multi_tile_launch_shapes(ctx, shape):
    """k_spmv_dia_march in the launch shapes the bench uses (several x-tiles, halo cells fetched from a neighbouring
    tile, partial last tiles, several chunks per column with the prologue at za > 0, plane-aligned slabs) against the
    oracle's product: <= 4e-15 * (|A| |x|) per row, and bit-identical to the row-order kernel of the same storage and to
    the CSR kernels (same products, same order; absent couplings add an exact zero)."""
    nx, ny, nz = GRID_SHAPES[shape]
    coords, cells = F.box_mesh((0, 0, 0), (1.0, 0.7, 1.3), nx - 1, ny - 1, nz - 1)
    h = ctx.mesh_upload(coords, cells)
    n = coords.shape[0]
    info = ctx.mesh_sym_info(h)
    assert (info["slots"], info["nx"], info["ny"]) == (8, nx, ny)
    K, M = F.assemble_atom(coords, cells, F.STIFF), F.assemble_atom(coords, cells, F.MASS)
    ctx.tune(20, 0)               # entries from the coordinate differences, like the oracle's: the 4e-15 bounds below are on the PRODUCT
    ak, am = ctx.atom_assemble(h, F.STIFF), ctx.atom_assemble(h, F.MASS)
    ctx.tune(20, 1)
    bc = boundary_dofs(coords)[::3].astype(np.int32)                 # a scattered part of the boundary is Dirichlet
    op = ctx.op_combine(h, [ak, am], [1.0, 0.37], bc)
    A, _ = F.apply_dirichlet((K + 0.37 * M).tocsr(), np.zeros(n), bc)
    rng = np.random.default_rng(1234)
    x = rng.uniform(-1, 1, n)
    ref, rowabs = A @ x, np.abs(A) @ np.abs(x)
    xv, yv = ctx.vec_from(x), ctx.vec_alloc(n)
    ctx.flags_reset()
    k0 = ctx.kernel_counts()
    ctx.tune(3, 0)                                                   # the CSR (dictionary) kernel
    ctx.spmv_dot_slot(op, xv, yv, xv, 0, n, 30)
    ctx.tune(3, 1)
    assert ctx.kernel_counts()["csr_dict"] == k0["csr_dict"] + 1
    y_csr = ctx.vec_download(yv)
    assert np.all(np.abs(y_csr - ref) <= 4e-15 * rowabs + 1e-300)
    assert ctx.op_symmetrize(op) is True           # already there: op_combine formed it from the atoms' diagonal forms
    # ... and it is the same, bit for bit, as the diagonal form converted from the operator's CSR values
    ctx.tune(14, 0)
    op_conv = ctx.op_combine(h, [ak, am], [1.0, 0.37], bc)
    ctx.tune(14, 1)
    assert ctx.op_symmetrize(op_conv) is True
    ctx.spmv_dot_slot(op_conv, xv, yv, xv, 0, n, 30)
    y_conv = ctx.vec_download(yv)
    ctx.atom_free(op_conv)
    k0 = ctx.kernel_counts()
    ctx.tune(7, 0)                                                   # adaptive: grids this small take the row-order kernel
    ctx.spmv_dot_slot(op, xv, yv, xv, 0, n, 31)
    y_rows, d_rows = ctx.vec_download(yv), ctx.slots_download(31, 1)[0]
    k1 = ctx.kernel_counts()
    assert k1["dia_rows"] == k0["dia_rows"] + 1 and k1["dia_march"] == k0["dia_march"]
    assert np.all(np.abs(y_rows - ref) <= 4e-15 * rowabs + 1e-300)
    assert np.array_equal(y_rows, y_csr) and np.array_equal(y_rows, y_conv)
    assert abs(d_rows - x @ ref) <= 1e-13 * (np.abs(x) @ rowabs)
    plane = nx * ny
    try:
        for zc, patch in ((1, 0), (4, 0), (16, 0), (1000, 0), (1, 1), (5, 1), (1000, 1), (1, 2), (3, 2), (8, 2), (1000, 2)):
            ctx.tune(7, zc)                                          # planes per march (forced)
            ctx.tune(13, patch)                                      # 0: 64 x 8, two rows per thread (default), 1: 64 x 8 (512 threads), 2: 64 x 4
            ctx.vec_fill(yv, -5.0)
            ctx.spmv_dot_slot(op, xv, yv, xv, 0, n, 32)
            y = ctx.vec_download(yv)
            assert ctx.kernel_counts()["dia_march"] > k1["dia_march"]
            k1 = ctx.kernel_counts()
            assert np.array_equal(y, y_rows), (shape, zc, np.abs(y - y_rows).max())
            assert abs(ctx.slots_download(32, 1)[0] - x @ ref) <= 1e-13 * (np.abs(x) @ rowabs)
            # a slab of whole planes, as a row-sharded rank calls it: rows outside untouched, halo planes read
            z0, z1 = 1, nz - 2
            ctx.vec_fill(yv, -7.0)
            ctx.spmv_dot_slot(op, xv, yv, xv, z0 * plane, z1 * plane, 33)
            y2 = ctx.vec_download(yv)
            assert np.array_equal(y2[z0 * plane:z1 * plane], y_rows[z0 * plane:z1 * plane])
            assert np.all(y2[:z0 * plane] == -7.0) and np.all(y2[z1 * plane:] == -7.0)
            assert abs(ctx.slots_download(33, 1)[0] - x[z0 * plane:z1 * plane] @ ref[z0 * plane:z1 * plane]) <= \
                1e-13 * (np.abs(x) @ rowabs)
        ctx.tune(13, 0)
        ctx.tune(7, 4)
        # the scaled operator inside the PCG: D^-1/2 A D^-1/2 through k_dia_scale, checked through the solve
        b = A @ rng.uniform(-1, 1, n)
        bv, sv = ctx.vec_from(b), ctx.vec_alloc(n)
        its, rel = ctx.pcg_solve(op, bv, sv, 1e-12, 0.0, 5000)
        xs = ctx.vec_download(sv)
        assert rel <= 1e-12 and np.linalg.norm(A @ xs - b) <= 1.01e-12 * np.linalg.norm(b)
        ctx.tune(3, 0)                                               # ... and the same solve on the CSR kernels
        ctx.vec_fill(sv, 0.0)
        its_c, rel_c = ctx.pcg_solve(op, bv, sv, 1e-12, 0.0, 5000)
        assert abs(its - its_c) <= 2 and np.linalg.norm(ctx.vec_download(sv) - xs) <= 1e-9 * np.linalg.norm(xs)
    finally:
        ctx.tune(7, 0)
        ctx.tune(13, 0)
        ctx.tune(3, 1)
    for v in (xv, yv, bv, sv):
        ctx.vec_free(v)
    for a in (op, ak, am):
        ctx.atom_free(a)
    ctx.mesh_free(h)


@pytest.mark.parametrize("npts", [128, 256])
def test_products_agree_at_bench_size(ctx, npts):
    """The BENCH configuration's operator (256^3 P1 dofs, 255^3 x 6 tetrahedra; 128^3 = config 3's) through every product
    kernel: k_spmv_dia_march with its adaptive march (8 planes at 256^3 and 128^3), the row-order kernel, the
    dictionary CSR kernel and the plain CSR kernel give the same y bit for bit; at 128^3 the CSR arrays are downloaded
    and the oracle's C product and scipy's agree to rounding; at both sizes the size-independent properties hold
    (K annihilates linear fields, M 1 sums to the volume, symmetry x.(A w) = w.(A x))."""
    from pgdrome_amd import fem
    from oracle import c_oracle
    mesh = fem.BoxMesh(fem.Point(0, 0, 0), fem.Point(1, 1, 1), npts - 1, npts - 1, npts - 1)
    coords, cells = mesh.coordinates(), mesh.cells()
    n = coords.shape[0]
    h = ctx.mesh_upload(coords, cells)
    del cells
    assert ctx.mesh_sym_info(h) == {"slots": 8, "nx": npts, "ny": npts}
    ak, am = ctx.atom_assemble(h, F.STIFF), ctx.atom_assemble(h, F.MASS)
    on_bnd = np.any((coords <= 1e-12) | (coords >= 1 - 1e-12), axis=1)
    bc = np.where(on_bnd)[0].astype(np.int32)
    op = ctx.op_combine(h, [ak, am], [1.0, 5.5], bc)
    rng = np.random.default_rng(1234)
    x = rng.uniform(-1, 1, n)
    xv, yv, wv = ctx.vec_from(x), ctx.vec_alloc(n), ctx.vec_from(rng.uniform(-1, 1, n))
    ys = {}
    try:
        ctx.flags_reset()
        for name, knobs in (("csr", [(3, 0), (2, 0)]), ("csr_dict", [(3, 0), (2, 1)])):
            for k, v in knobs:
                ctx.tune(k, v)
            c0 = ctx.kernel_counts()
            ctx.spmv_dot_slot(op, xv, yv, xv, 0, n, 30)
            assert ctx.kernel_counts()[name] == c0[name] + 1
            ys[name] = (ctx.vec_download(yv), ctx.slots_download(30, 1)[0])
        ctx.tune(3, 1)
        assert ctx.op_symmetrize(op) is True
        # (dia_march: k_spmv_dia_march3 - buffer addressing, the next plane's slots prefetched; dia_march2: the r02 form of it)
        for name, knobs in (("dia_march", [(6, 8), (47, 1)]), ("dia_march2", [(6, 8), (47, 0)]), ("dia_rows", [(6, 0)])):
            for k, v in knobs:
                ctx.tune(k, v)
            c0 = ctx.kernel_counts()
            ctx.vec_fill(yv, -1.0)
            ctx.spmv_dot_slot(op, xv, yv, xv, 0, n, 30)
            counter = "dia_march" if name == "dia_march2" else name
            assert ctx.kernel_counts()[counter] == c0[counter] + 1
            ys[name] = (ctx.vec_download(yv), ctx.slots_download(30, 1)[0])
        ctx.tune(47, 0)
        # ... and the march on the row-class dictionary (one code byte per row), several chunk lengths
        assert 1 <= ctx.op_classify(op) <= 64
        ctx.tune(6, 8)
        # (s) the STENCIL form (the hull is Dirichlet: one tuple + eliminated nodes) in the launch shape the solves take by default -
        # marches that fill every workgroup slot once (256^3: 8 marches of 32 planes, an incomplete last group of steps) - and
        # with marches of 7 / 33 planes
        for L in (0, 7, 33):
            ctx.tune(36, L)
            c0 = ctx.kernel_counts()
            ctx.vec_fill(yv, -1.0)
            ctx.spmv_dot_slot(op, xv, yv, xv, 0, n, 30)
            assert ctx.kernel_counts()["stencil_march"] == c0["stencil_march"] + 1
            ys["stencil_march_%d" % L] = (ctx.vec_download(yv), ctx.slots_download(30, 1)[0])
        ctx.tune(36, 0)
        # (s2) ... and with TWO rows per thread (64 x 8 patches: what a thin z-slab of a sharded solve takes), default march and 9 planes
        ctx.tune(48, 2)
        for L in (0, 9):
            ctx.tune(36, L)
            c0 = ctx.kernel_counts()
            ctx.vec_fill(yv, -1.0)
            ctx.spmv_dot_slot(op, xv, yv, xv, 0, n, 30)
            assert ctx.kernel_counts()["stencil_march"] == c0["stencil_march"] + 1
            ys["stencil_march_rows2_%d" % L] = (ctx.vec_download(yv), ctx.slots_download(30, 1)[0])
        ctx.tune(36, 0)
        ctx.tune(48, 0)
        ctx.tune(35, 0)                               # ... and the dictionary form of the same classes from here on
        # (a) the launch shape the solves take by DEFAULT: as many planes per march as fill every resident workgroup slot exactly
        # once (PGD_TUNE_SPMV_ZCHUNK_CODED2 = 96: 256^3 -> 4 marches of 66 planes, 128^3 -> marches of 9) ...
        c0 = ctx.kernel_counts()
        ctx.vec_fill(yv, -1.0)
        ctx.spmv_dot_slot(op, xv, yv, xv, 0, n, 30)
        assert ctx.kernel_counts()["diac_march"] == c0["diac_march"] + 1
        ys["diac_march_default_rule"] = (ctx.vec_download(yv), ctx.slots_download(30, 1)[0])
        # (b) ... and, with that rule OFF (it would override knob 21 at these sizes), marches of at most 24 / 12 / 5 planes
        ctx.tune(32, 0)
        for zc in (24, 12, 5):                        # most planes per march (whole threes: 5 -> 3)
            ctx.tune(21, zc)
            c0 = ctx.kernel_counts()
            ctx.vec_fill(yv, -1.0)
            ctx.spmv_dot_slot(op, xv, yv, xv, 0, n, 30)
            assert ctx.kernel_counts()["diac_march"] == c0["diac_march"] + 1
            ys["diac_march_%d" % zc] = (ctx.vec_download(yv), ctx.slots_download(30, 1)[0])
    finally:
        ctx.tune(3, 1)
        ctx.tune(2, 1)
        ctx.tune(6, 8)
        ctx.tune(21, 24)
        ctx.tune(32, 96)
        ctx.tune(35, 1)
        ctx.tune(36, 0)
        ctx.tune(48, 0)
    base = ys["csr"][0]
    # (the dot's partial sums are grouped per workgroup: different march lengths give different last bits of the DOT, never of y)
    assert len({ys["diac_march_%d" % zc][1] for zc in (24, 12, 5)} | {ys["diac_march_default_rule"][1]}) >= 2
    for name in ("csr_dict", "dia_march", "dia_march2", "dia_rows", "stencil_march_0", "stencil_march_7", "stencil_march_33", "stencil_march_rows2_0", "stencil_march_rows2_9", "diac_march_default_rule",
                 "diac_march_24", "diac_march_12", "diac_march_5"):
        assert np.array_equal(ys[name][0], base), (name, np.abs(ys[name][0] - base).max())
        assert abs(ys[name][1] - ys["csr"][1]) <= 1e-12 * np.abs(x) @ np.abs(base)
    assert np.all(base[bc] == x[bc])                                   # Dirichlet rows are identity rows
    # symmetry of the eliminated operator: w.(A x) = x.(A w)
    ctx.spmv_dot_slot(op, xv, yv, wv, 0, n, 31)
    d1 = ctx.slots_download(31, 1)[0]
    tv = ctx.vec_alloc(n)
    ctx.spmv_dot_slot(op, wv, tv, xv, 0, n, 32)
    d2 = ctx.slots_download(32, 1)[0]
    assert abs(d1 - d2) <= 1e-12 * np.abs(x) @ np.abs(base)
    # size-independent properties of the atoms: K (a + b.x) = 0 in the interior, sum(M 1) = |Omega| = 1
    lin = ctx.vec_from(0.3 + coords @ np.array([1.0, -2.0, 0.5]))
    ctx.spmv(ak, lin, tv)
    kl = ctx.vec_download(tv)
    scale = 3.0 * (1.0 / (npts - 1))                                    # |K| |x| per interior row is O(h)
    assert np.abs(kl[~on_bnd]).max() <= 1e-12 * scale
    ones = ctx.vec_from(np.ones(n))
    assert abs(ctx.bilinear(am, ones, ones) - 1.0) <= 1e-12
    if npts == 128:
        rp, cols = ctx.mesh_pattern(h)
        vals = ctx.atom_download(op, cols.size)
        y_c = c_oracle.spmv(rp, cols, vals, x)
        A = sps.csr_matrix((vals, cols, rp), shape=(n, n))
        rowabs = np.abs(A) @ np.abs(x)
        assert np.all(np.abs(base - y_c) <= 4e-15 * rowabs + 1e-300)
        assert np.all(np.abs(base - A @ x) <= 4e-15 * rowabs + 1e-300)
        assert abs(A - A.T).max() <= 1e-12 * np.abs(vals).max()
    for v in (xv, yv, wv, tv, lin, ones):
        ctx.vec_free(v)
    for a in (op, ak, am):
        ctx.atom_free(a)
    ctx.mesh_free(h)


@pytest.mark.parametrize("name", ["rect17x9", "box20"])
def test_start_gram_matches_oracle(ctx, name):
    """pgd_start_gram (Galerkin start of a PCG solve): G[i, j] = v_i . (A v_j), g[j] = v_j . b, full and partial row
    ranges, 1 .. 17 vectors, products from the symmetric storage (diagonal form on the box grid)."""
    coords, cells = MESHES[name]()
    h = ctx.mesh_upload(coords, cells)
    n = coords.shape[0]
    K, M = F.assemble_atom(coords, cells, F.STIFF), F.assemble_atom(coords, cells, F.MASS)
    ak, am = ctx.atom_assemble(h, F.STIFF), ctx.atom_assemble(h, F.MASS)
    bc = boundary_dofs(coords)
    op = ctx.op_combine(h, [ak, am], [1.0, 2.0], bc)
    A, _ = F.apply_dirichlet((K + 2.0 * M).tocsr(), np.zeros(n), bc)
    rng = np.random.default_rng(77)
    V = rng.uniform(-1, 1, (17, n))
    b = rng.uniform(-1, 1, n)
    vs, bv = [ctx.vec_from(v) for v in V], ctx.vec_from(b)
    for k, (r0, r1) in ((1, (0, n)), (4, (0, n)), (9, (0, n)), (17, (0, n)), (3, (n // 4, 3 * n // 4))):
        G, g = ctx.start_gram(op, vs[:k], bv, r0, r1)
        W = (A @ V[:k].T)[r0:r1]                                   # columns A v_j on the row range
        G_ref = V[:k, r0:r1] @ W
        scale = (np.abs(V[:k, r0:r1]) @ (np.abs(A) @ np.abs(V[:k].T))[r0:r1]).max()
        # the upper triangle is computed (i <= j) and mirrored: on a row sub-range only the SUM over the ranges is symmetric
        assert np.abs(np.triu(G - G_ref)).max() <= 1e-13 * scale and np.array_equal(G, G.T)
        assert np.abs(g - V[:k, r0:r1] @ b[r0:r1]).max() <= 1e-13 * n
    from pgdrome_amd._lib import PgdError
    with pytest.raises(PgdError):
        ctx.start_gram(op, vs + [bv], bv)                          # more than 17 vectors
    # pgd_start_residual: b - sum_j c_j (A v_j) from the products the call right before left in the library (k <= 9, all rows)
    rv = ctx.vec_alloc(n)
    for k in (1, 5, 9):
        ctx.start_gram(op, vs[:k], bv, 0, n)
        cf = rng.uniform(-1, 1, k)
        ctx.start_residual(op, cf, bv, rv)
        ref = b - (A @ V[:k].T) @ cf
        assert np.abs(ctx.vec_download(rv) - ref).max() <= 1e-13 * (np.abs(b) + np.abs(A) @ np.abs(V[:k].T) @ np.abs(cf)).max()
    with pytest.raises(PgdError):
        ctx.start_residual(op, np.ones(4), bv, rv)                 # not the number of products held
    with pytest.raises(PgdError):
        ctx.start_residual(am, np.ones(9), bv, rv)                 # not the operator they belong to
    ctx.start_gram(op, vs[:12], bv, 0, n)
    with pytest.raises(PgdError):
        ctx.start_residual(op, np.ones(12), bv, rv)                # more than 9 vectors: the products are not kept
    ctx.start_gram(op, vs[:3], bv, n // 4, n // 2)
    with pytest.raises(PgdError):
        ctx.start_residual(op, np.ones(3), bv, rv)                 # products over a row range only
    ctx.vec_free(rv)
    for v in vs + [bv]:
        ctx.vec_free(v)
    for a in (op, ak, am):
        ctx.atom_free(a)
    ctx.mesh_free(h)


def test_pcg_with_the_x_update_in_the_p_kernel_is_bit_identical(ctx):
    """Above 2^20 rows the scaled recurrence lets the p kernel apply x += alpha p (8 vector passes per iteration instead of
    9; the last update is applied after the loop when the solve converges): same iterates, bit for bit, as the x / r
    kernel + p kernel pair - also when the loop ends on maxit, and on a converged start."""
    from pgdrome_amd import fem
    npts = 104                                        # 104^3 = 1 124 864 rows > 2^20
    mesh = fem.BoxMesh(fem.Point(0, 0, 0), fem.Point(1, 1, 1), npts - 1, npts - 1, npts - 1)
    coords = mesh.coordinates()
    h = ctx.mesh_upload(coords, mesh.cells())
    n = coords.shape[0]
    ak, am = ctx.atom_assemble(h, F.STIFF), ctx.atom_assemble(h, F.MASS)
    bc = np.where(np.any((coords <= 1e-12) | (coords >= 1 - 1e-12), axis=1))[0].astype(np.int32)
    rng = np.random.default_rng(5)
    b = rng.uniform(-1, 1, n)
    b[bc] = 0.0
    x0 = 0.01 * rng.uniform(-1, 1, n)
    x0[bc] = 0.0
    bv = ctx.vec_from(b)
    out = {}
    try:
        ctx.tune(18, 0)                               # (the single-sync recurrence has its own test below)
        for defer in (1, 0):
            ctx.tune(16, defer)
            for maxit in (10000, 37):                 # to convergence; cut off in the middle of a 16-iteration chunk
                op = ctx.op_combine(h, [ak, am], [1.0, 3.0], bc)
                xv = ctx.vec_from(x0)
                try:
                    it, rel = ctx.pcg_solve(op, bv, xv, 1e-10, 0.0, maxit)
                except Exception:
                    raise
                out[(defer, maxit)] = (it, rel, ctx.vec_download(xv))
                if maxit == 10000:
                    it2, rel2 = ctx.pcg_solve(op, bv, xv, 1e-10, 0.0, maxit)          # converged start: nothing pending
                    out[(defer, "again")] = (it2, rel2, ctx.vec_download(xv))
                ctx.vec_free(xv)
                ctx.atom_free(op)
    finally:
        ctx.tune(16, 1)
        ctx.tune(18, 1)
    for key in (10000, 37, "again"):
        a, c = out[(1, key)], out[(0, key)]
        assert a[0] == c[0] and a[1] == c[1], key
        assert np.array_equal(a[2], c[2]), (key, np.abs(a[2] - c[2]).max())
    assert out[(1, 10000)][1] <= 1e-10 and out[(1, 37)][0] == 37 and out[(1, "again")][0] <= 1
    ctx.vec_free(bv)
    for a in (ak, am):
        ctx.atom_free(a)
    ctx.mesh_free(h)


def test_single_sync_recurrence_walks_the_textbook_iterates(ctx):
    """One reduction + one vector kernel per iteration (beta from r'.r' = alpha^2 q.q - r.r; every alpha and the stop test
    from the measured r.r): against the two-reduction recurrence on the same storage and against the oracle's textbook
    Jacobi-PCG - same iteration counts (+-1: the rounding of beta), same solution, the TRUE residual at the tolerance, a
    cut-off solve with the same iterate, a converged start, and run-to-run bitwise reproducibility."""
    from pgdrome_amd import fem
    npts = 104                                        # 1 124 864 rows > 2^20
    mesh = fem.BoxMesh(fem.Point(0, 0, 0), fem.Point(1, 1, 1), npts - 1, npts - 1, npts - 1)
    coords = mesh.coordinates()
    h = ctx.mesh_upload(coords, mesh.cells())
    n = coords.shape[0]
    ak, am = ctx.atom_assemble(h, F.STIFF), ctx.atom_assemble(h, F.MASS)
    bc = np.where(np.any((coords <= 1e-12) | (coords >= 1 - 1e-12), axis=1))[0].astype(np.int32)
    rng = np.random.default_rng(11)
    b = rng.uniform(-1, 1, n)
    b[bc] = 0.0
    bv = ctx.vec_from(b)
    res = {}
    try:
        for ss in (1, 0, 1):
            ctx.tune(18, ss)
            for maxit in (10000, 23):
                op = ctx.op_combine(h, [ak, am], [1.0, 3.0], bc)
                xv = ctx.vec_alloc(n)
                k0 = ctx.kernel_counts()
                it, rel = ctx.pcg_solve(op, bv, xv, 1e-10, 0.0, maxit)
                k1 = ctx.kernel_counts()
                assert sum(k1[k] for k in ("dia_march", "diac_march", "stencil_march")) > sum(k0[k] for k in ("dia_march", "diac_march", "stencil_march"))
                x = ctx.vec_download(xv)
                if maxit == 10000:
                    it2, _ = ctx.pcg_solve(op, bv, xv, 1e-10, 0.0, maxit)
                    assert it2 <= 1
                    # the true residual through an independent kernel (plain CSR product of the unscaled operator)
                    yv = ctx.vec_alloc(n)
                    ctx.tune(3, 0)
                    ctx.spmv(op, ctx.vec_from(x), yv)
                    ctx.tune(3, 1)
                    r = b - ctx.vec_download(yv)
                    assert np.linalg.norm(r) <= 1.05e-10 * np.linalg.norm(b)
                    ctx.vec_free(yv)
                res.setdefault((ss, maxit), []).append((it, rel, x))
                ctx.vec_free(xv)
                ctx.atom_free(op)
    finally:
        ctx.tune(18, 1)
    # a residual that vanishes EXACTLY (identity operator: every row a Dirichlet row): one iteration, no 0 / 0 in beta
    allrows = np.arange(n, dtype=np.int32)
    op = ctx.op_combine(h, [ak, am], [1.0, 3.0], allrows)
    xv, bv2 = ctx.vec_alloc(n), ctx.vec_from(np.arange(1, n + 1, dtype=np.float64))
    it, rel = ctx.pcg_solve(op, bv2, xv, 1e-10, 0.0, 100)
    assert it == 1 and rel == 0.0 and np.array_equal(ctx.vec_download(xv), np.arange(1, n + 1, dtype=np.float64))
    ctx.vec_free(xv)
    ctx.vec_free(bv2)
    ctx.atom_free(op)
    a, t = res[(1, 10000)], res[(0, 10000)][0]
    assert a[0][0] == a[1][0] and a[0][1] == a[1][1] and np.array_equal(a[0][2], a[1][2])      # reproducible run to run
    assert abs(a[0][0] - t[0]) <= 1 and a[0][1] <= 1e-10 and t[1] <= 1e-10
    assert np.linalg.norm(a[0][2] - t[2]) <= 1e-9 * np.linalg.norm(t[2])
    c1, c0 = res[(1, 23)][0], res[(0, 23)][0]
    assert c1[0] == c0[0] == 23 and np.linalg.norm(c1[2] - c0[2]) <= 1e-11 * np.linalg.norm(c0[2])   # same 23rd iterate
    ctx.vec_free(bv)
    for at in (ak, am):
        ctx.atom_free(at)
    ctx.mesh_free(h)


@pytest.mark.parametrize("shape", sorted(GRID_SHAPES))
def test_row_class_dictionary_is_lossless(ctx, shape):
    """k_spmv_diac_march2: the z-march that reads one class code per row and the classes' slot tuples from LDS.  On
    uniform grids with constant coefficients (all-Dirichlet, all-Neumann, one Dirichlet face) the operator has a few dozen
    row classes; the product must be bit-identical to the march that streams the slot values (several tiles, partial
    tiles, chunk prologues at za > 0, plane-aligned slabs), dots included.  A variable coefficient gives no dictionary
    and the plain march; new operator values drop the dictionary."""
    nx, ny, nz = GRID_SHAPES[shape]
    coords, cells = F.box_mesh((0, 0, 0), (1.0, 0.7, 1.3), nx - 1, ny - 1, nz - 1)
    h = ctx.mesh_upload(coords, cells)
    n = coords.shape[0]
    plane = nx * ny
    # the vertices sit on a uniform lattice: the assembly takes edge vectors as whole steps, congruent cells get identical
    # local matrices (entries within the oracle's own rounding noise - it differences the rounded coordinates)
    lat, steps = ctx.mesh_lattice(h)
    assert lat and np.allclose(steps, [1.0 / (nx - 1), 0.7 / (ny - 1), 1.3 / (nz - 1)], rtol=1e-14)
    ak, am = ctx.atom_assemble(h, F.STIFF), ctx.atom_assemble(h, F.MASS)
    for atom, kind in ((ak, F.STIFF), (am, F.MASS)):
        ref = F.assemble_atom(coords, cells, kind)
        # (a difference of two rounded coordinates of size ~1 carries ulp(1) / h = n * eps of relative error: the oracle's noise)
        assert np.abs(ctx.atom_download(atom, ref.nnz) - ref.data).max() <= 16 * max(nx, ny, nz) * 2.3e-16 * np.abs(ref.data).max()
    bnd = boundary_dofs(coords).astype(np.int32)
    face = np.where(coords[:, 2] <= 1e-12)[0].astype(np.int32)
    rng = np.random.default_rng(99)
    x = rng.uniform(-1, 1, n)
    xv, yv = ctx.vec_from(x), ctx.vec_alloc(n)
    ctx.flags_reset()
    try:
        for bc in (bnd, np.zeros(0, dtype=np.int32), face):
            op = ctx.op_combine(h, [ak, am], [1.0, 0.37], bc)
            assert ctx.op_symmetrize(op) is True
            ctx.tune(7, 4)
            ctx.spmv_dot_slot(op, xv, yv, xv, 0, n, 30)                  # the march over the slot values
            y_ref, d_ref = ctx.vec_download(yv), ctx.slots_download(30, 1)[0]
            ncls = ctx.op_classify(op)
            assert 1 <= ncls <= 255, ncls
            for zc in (1, 3, 4, 16, 1000):
                ctx.tune(7, zc)
                k0 = ctx.kernel_counts()
                ctx.vec_fill(yv, -5.0)
                ctx.spmv_dot_slot(op, xv, yv, xv, 0, n, 31)
                k1 = ctx.kernel_counts()
                assert k1["diac_march"] == k0["diac_march"] + 1 and k1["dia_march"] == k0["dia_march"]
                y = ctx.vec_download(yv)
                assert np.array_equal(y, y_ref), (shape, zc, np.abs(y - y_ref).max())
                if zc == 4:
                    assert ctx.slots_download(31, 1)[0] == d_ref      # same partial sums in the same order
                z0, z1 = 1, nz - 1
                ctx.vec_fill(yv, -7.0)
                ctx.spmv_dot_slot(op, xv, yv, xv, z0 * plane, z1 * plane, 32)
                y2 = ctx.vec_download(yv)
                assert np.array_equal(y2[z0 * plane:z1 * plane], y_ref[z0 * plane:z1 * plane])
                assert np.all(y2[:z0 * plane] == -7.0) and np.all(y2[z1 * plane:] == -7.0)
            # switched off: the plain march again
            ctx.tune(19, 0)
            k0 = ctx.kernel_counts()
            ctx.spmv_dot_slot(op, xv, yv, xv, 0, n, 31)
            ctx.tune(19, 1)
            k1 = ctx.kernel_counts()
            assert k1["diac_march"] == k0["diac_march"] and k1["dia_march"] == k0["dia_march"] + 1
            # new values through the same handle: no stale dictionary
            op = ctx.op_combine(h, [ak, am], [2.0, 0.1], bc, op=op)
            k0 = ctx.kernel_counts()
            ctx.spmv_dot_slot(op, xv, yv, xv, 0, n, 31)
            k1 = ctx.kernel_counts()
            assert k1["diac_march"] == k0["diac_march"] and k1["dia_march"] == k0["dia_march"] + 1
            y_new = ctx.vec_download(yv)
            assert 1 <= ctx.op_classify(op) <= 255
            ctx.spmv_dot_slot(op, xv, yv, xv, 0, n, 31)
            assert np.array_equal(ctx.vec_download(yv), y_new)
            ctx.atom_free(op)
        # a scattered Dirichlet set (every third boundary vertex): many more classes, or none - either way the same y
        op = ctx.op_combine(h, [ak, am], [1.0, 0.37], bnd[::3])
        assert ctx.op_symmetrize(op) is True
        ctx.tune(7, 4)
        ctx.spmv_dot_slot(op, xv, yv, xv, 0, n, 30)
        y_ref = ctx.vec_download(yv)
        ncls = ctx.op_classify(op)
        assert 0 <= ncls <= 255
        k0 = ctx.kernel_counts()
        ctx.vec_fill(yv, -3.0)
        ctx.spmv_dot_slot(op, xv, yv, xv, 0, n, 31)
        k1 = ctx.kernel_counts()
        assert (k1["diac_march"] - k0["diac_march"], k1["dia_march"] - k0["dia_march"]) == ((1, 0) if ncls else (0, 1))
        assert np.array_equal(ctx.vec_download(yv), y_ref)
        ctx.atom_free(op)
        # a coefficient that varies from vertex to vertex: more than 255 classes (or none that verify) -> no dictionary
        wv = ctx.vec_from(1.0 + coords[:, 0] ** 2 + 0.5 * np.sin(coords.sum(axis=1)))
        aw = ctx.atom_assemble(h, F.KIND_NAMES.index("wmass"), 0, 0, wv)
        opw = ctx.op_combine(h, [ak, aw], [1.0, 0.5], bnd)
        assert ctx.op_symmetrize(opw) is True
        ctx.tune(7, 4)
        assert ctx.op_classify(opw) == 0
        k0 = ctx.kernel_counts()
        ctx.spmv_dot_slot(opw, xv, yv, xv, 0, n, 31)
        k1 = ctx.kernel_counts()
        assert k1["diac_march"] == k0["diac_march"] and k1["dia_march"] == k0["dia_march"] + 1
        ctx.atom_free(opw)
        ctx.atom_free(aw)
        ctx.vec_free(wv)
        # a grid whose planes are not equally spaced is no lattice: coordinate differences as they are, and (here) no classes
        c2 = coords.copy()
        c2[:, 2] = c2[:, 2] ** 1.5
        h2 = ctx.mesh_upload(c2, cells)
        assert ctx.mesh_lattice(h2)[0] is False and ctx.mesh_sym_info(h2)["nx"] == nx
        ctx.mesh_free(h2)
    finally:
        ctx.tune(7, 0)
        ctx.tune(19, 1)
    for v in (xv, yv):
        ctx.vec_free(v)
    for a in (ak, am):
        ctx.atom_free(a)
    ctx.mesh_free(h)


def test_deferred_csr_values_and_atom_products(ctx):
    """pgd_op_combine on a structured grid forms the operator's diagonal form and leaves the CSR values to the first reader
    (PGD_TUNE_LAZY_CSR): whoever asks later - a download, a CSR product after the solve has scaled the slot arrays, the
    band / diagonal helpers - gets exactly what the eager combine gives, and an operator whose atoms have gone says so.
    Products with an ATOM whose diagonal form exists take the z-march over the atom's own row classes
    (PGD_TUNE_ATOM_FAST, pgd_atom_product_form): bit-identical y, plane-aligned ranges only."""
    from pgdrome_amd._lib import PgdError
    nx, ny, nz = 70, 19, 23
    coords, cells = F.box_mesh((0, 0, 0), (1.0, 0.7, 1.3), nx - 1, ny - 1, nz - 1)
    h = ctx.mesh_upload(coords, cells)
    n, plane = coords.shape[0], nx * ny
    nnz = ctx.mesh_info(h)["nnz"]
    ak, am = ctx.atom_assemble(h, F.STIFF), ctx.atom_assemble(h, F.MASS)
    bnd = boundary_dofs(coords).astype(np.int32)
    rng = np.random.default_rng(5)
    x = rng.uniform(-1, 1, n)
    xv, yv, bv = ctx.vec_from(x), ctx.vec_alloc(n), ctx.vec_from(rng.uniform(-1, 1, n))
    try:
        # before any operator: the atoms have no diagonal form yet, products read the CSR values
        assert ctx.atom_product_form(ak) == 0
        ctx.spmv(ak, xv, yv)
        yk_csr = ctx.vec_download(yv)
        ctx.spmv(am, xv, yv, 2 * plane, 9 * plane)
        ym_csr = ctx.vec_download(yv, 2 * plane, 7 * plane)
        for bc in (bnd, np.zeros(0, dtype=np.int32)):
            ctx.tune(28, 0)
            eager = ctx.op_combine(h, [ak, am], [1.3, 0.37], bc)
            v_eager = ctx.atom_download(eager, nnz)
            ctx.tune(28, 1)
            k0 = ctx.kernel_counts()
            lazy = ctx.op_combine(h, [ak, am], [1.3, 0.37], bc)
            # the solve reads the diagonal form only ...
            xs = ctx.vec_alloc(n)
            ctx.vec_fill(xs, 0.0)
            ctx.vec_set(bv, bc, np.zeros(bc.size)) if bc.size else None
            it, rel = ctx.pcg_solve(lazy, bv, xs, 1e-10, 0.0, 4000)
            k1 = ctx.kernel_counts()
            assert rel <= 1e-10 and k1["csr"] == k0["csr"] and k1["csr_dict"] == k0["csr_dict"]
            # ... and afterwards (slot arrays scaled and given up) the CSR values appear on request, bit for bit
            assert np.array_equal(ctx.atom_download(lazy, nnz), v_eager)
            ctx.spmv(lazy, xs, yv)
            r = ctx.vec_download(yv) - ctx.vec_download(bv)
            assert np.linalg.norm(r) <= 2e-10 * np.linalg.norm(ctx.vec_download(bv))
            ctx.vec_free(xs)
            # new values through the same handle, read through the diagonal helper
            lazy = ctx.op_combine(h, [ak, am], [0.5, 2.0], bc, op=lazy)
            eager = ctx.op_combine(h, [ak, am], [0.5, 2.0], bc, op=eager)
            dv = ctx.vec_alloc(n)
            ctx.op_diag_inv(lazy, dv)
            d_lazy = ctx.vec_download(dv)
            ctx.op_diag_inv(eager, dv)
            assert np.array_equal(d_lazy, ctx.vec_download(dv))
            ctx.vec_free(dv)
            ctx.atom_free(lazy)
            ctx.atom_free(eager)
        # the atoms went through combine_dia: they have their diagonal form now, and on this uniform grid row classes
        assert ctx.atom_product_form(ak) == 2 and ctx.atom_product_form(am) == 2
        ctx.tune(7, 4)            # (a grid this small would take the row-order kernel over the slot values otherwise)
        k0 = ctx.kernel_counts()
        ctx.vec_fill(yv, -1.0)
        ctx.spmv(ak, xv, yv)
        assert np.array_equal(ctx.vec_download(yv), yk_csr)
        ctx.vec_fill(yv, -1.0)
        ctx.spmv(am, xv, yv, 2 * plane, 9 * plane)
        y = ctx.vec_download(yv)
        assert np.array_equal(y[2 * plane:9 * plane], ym_csr) and np.all(y[:2 * plane] == -1.0) and np.all(y[9 * plane:] == -1.0)
        k1 = ctx.kernel_counts()
        assert k1["diac_march"] == k0["diac_march"] + 2 and k1["csr"] == k0["csr"] and k1["csr_dict"] == k0["csr_dict"]
        # a range that is not plane-aligned, and the knob switched off: the CSR kernels, same bits
        ctx.spmv(ak, xv, yv, 5, n - 3)
        assert np.array_equal(ctx.vec_download(yv, 5, n - 8), yk_csr[5:n - 3])
        ctx.tune(27, 0)
        assert ctx.atom_product_form(ak) == 0
        k0 = ctx.kernel_counts()
        ctx.spmv(ak, xv, yv)
        k1 = ctx.kernel_counts()
        assert k1["diac_march"] == k0["diac_march"] and np.array_equal(ctx.vec_download(yv), yk_csr)
        ctx.tune(27, 1)
        # an operator left pending whose atom is freed (its handle taken by another atom): an error, not a wrong product
        a2 = ctx.atom_assemble(h, F.MASS)
        op = ctx.op_combine(h, [ak, a2], [1.0, 1.0], bnd)
        ctx.atom_free(a2)
        a3 = ctx.atom_assemble(h, F.STIFF)
        with pytest.raises(PgdError):
            ctx.atom_download(op, nnz)
        ctx.atom_free(a3)
        ctx.atom_free(op)
    finally:
        ctx.tune(7, 0)
        ctx.tune(27, 1)
        ctx.tune(28, 1)
    for v in (xv, yv, bv):
        ctx.vec_free(v)
    for a in (ak, am):
        ctx.atom_free(a)
    ctx.mesh_free(h)


@pytest.mark.parametrize("shape", sorted(GRID_SHAPES))
def test_stencil_form_is_lossless(ctx, shape):
    """k_spmv_stencil_march: where the row classes of an operator are ONE 8-tuple plus the rows it becomes next to eliminated
    nodes and the rim of the grid - every row and slot verified bit by bit on the device - the z-march takes the couplings
    from scalar registers (four rows per thread, 64 x 16 patches, buffer addressing, identity rows stored out of a register
    ring).  y must be bit-identical to the march over the slot values for ANY x (non-zero entries on the Dirichlet rows
    included): all march lengths incl. incomplete last groups, several tiles with partial last tiles, plane-aligned slabs.
    Operators that are not of that form (natural boundaries, a Dirichlet face only, a Dirichlet node that exists in one
    plane only) must keep the dictionary kernel; a Dirichlet column that runs through all planes keeps the stencil form."""
    nx, ny, nz = GRID_SHAPES[shape]
    coords, cells = F.box_mesh((0, 0, 0), (1.0, 0.7, 1.3), nx - 1, ny - 1, nz - 1)
    h = ctx.mesh_upload(coords, cells)
    n = coords.shape[0]
    plane = nx * ny
    ak, am = ctx.atom_assemble(h, F.STIFF), ctx.atom_assemble(h, F.MASS)
    bnd = boundary_dofs(coords).astype(np.int32)
    face = np.where(coords[:, 2] <= 1e-12)[0].astype(np.int32)
    ix, iy = min(5, nx - 2), min(2, ny - 2)
    column = (ix + nx * iy + plane * np.arange(nz)).astype(np.int32)             # an interior Dirichlet column through all planes
    single = np.array([ix + nx * iy + plane * (nz // 2)], dtype=np.int32)       # ... and a single interior Dirichlet node
    rng = np.random.default_rng(7)
    x = rng.uniform(-1, 1, n)
    xv, yv = ctx.vec_from(x), ctx.vec_alloc(n)
    ctx.flags_reset()
    cases = (("hull", bnd, True), ("hull + column", np.union1d(bnd, column).astype(np.int32), True),
             ("hull + one interior node", np.union1d(bnd, single).astype(np.int32), False),
             ("natural", np.zeros(0, dtype=np.int32), False), ("one face", face, False))
    try:
        for name, bc, expect in cases:
            op = ctx.op_combine(h, [ak, am], [1.0, 0.37], bc)
            assert ctx.op_symmetrize(op) is True
            ctx.tune(7, 4)
            ctx.tune(36, 0)
            ctx.tune(19, 0)
            ctx.spmv_dot_slot(op, xv, yv, xv, 0, n, 30)                  # the march over the slot values
            ctx.tune(19, 1)
            y_ref, d_ref = ctx.vec_download(yv), ctx.slots_download(30, 1)[0]
            assert 1 <= ctx.op_classify(op) <= 255
            if len(bc):
                assert np.array_equal(y_ref[bc], x[bc])                   # identity rows
            for L in (1, 2, 3, 4, 7, 16, 1000):
                ctx.tune(36, L)
                k0 = ctx.kernel_counts()
                ctx.vec_fill(yv, -5.0)
                ctx.spmv_dot_slot(op, xv, yv, xv, 0, n, 31)
                k1 = ctx.kernel_counts()
                ran = {k for k in k1 if k1[k] != k0[k]}
                assert ran == ({"stencil_march"} if expect else {"diac_march"}), (name, L, ran)
                y = ctx.vec_download(yv)
                assert np.array_equal(y, y_ref), (shape, name, L, np.abs(y - y_ref).max(), np.where(y != y_ref)[0][:8])
                assert abs(ctx.slots_download(31, 1)[0] - d_ref) <= 1e-12 * np.abs(x) @ np.abs(y_ref)
                if nz >= 5:
                    z0, z1 = 1, nz - 1                                    # a plane-aligned slab: rows outside it untouched
                    ctx.vec_fill(yv, -7.0)
                    ctx.spmv_dot_slot(op, xv, yv, xv, z0 * plane, z1 * plane, 32)
                    y2 = ctx.vec_download(yv)
                    assert np.array_equal(y2[z0 * plane:z1 * plane], y_ref[z0 * plane:z1 * plane]), (shape, name, L)
                    assert np.all(y2[:z0 * plane] == -7.0) and np.all(y2[z1 * plane:] == -7.0)
                    s_ref = x[z0 * plane:z1 * plane] @ y_ref[z0 * plane:z1 * plane]
                    assert abs(ctx.slots_download(32, 1)[0] - s_ref) <= 1e-12 * np.abs(x) @ np.abs(y_ref)
            # the plain product without the fused dot (no w), and switched off
            ctx.tune(36, 5)
            ctx.vec_fill(yv, -1.0)
            ctx.spmv(op, xv, yv)
            assert np.array_equal(ctx.vec_download(yv), y_ref), (shape, name)
            ctx.tune(35, 0)
            k0 = ctx.kernel_counts()
            ctx.spmv_dot_slot(op, xv, yv, xv, 0, n, 31)
            k1 = ctx.kernel_counts()
            ctx.tune(35, 1)
            assert k1["stencil_march"] == k0["stencil_march"] and k1["diac_march"] == k0["diac_march"] + 1
            assert np.array_equal(ctx.vec_download(yv), y_ref)
            # new values through the same handle: no stale stencil
            op = ctx.op_combine(h, [ak, am], [2.0, 0.1], bc, op=op)
            k0 = ctx.kernel_counts()
            ctx.spmv_dot_slot(op, xv, yv, xv, 0, n, 31)
            k1 = ctx.kernel_counts()
            assert k1["stencil_march"] == k0["stencil_march"] and k1["diac_march"] == k0["diac_march"]
            ctx.atom_free(op)
    finally:
        ctx.tune(7, 0)
        ctx.tune(36, 0)
        ctx.tune(35, 1)
        ctx.tune(19, 1)
    for v in (xv, yv):
        ctx.vec_free(v)
    for a in (ak, am):
        ctx.atom_free(a)
    ctx.mesh_free(h)


def test_classification_cache_is_verified_not_trusted(ctx):
    """A mesh remembers the class codes of the operators classified on it; the next operator with that structure (other
    coefficients: every solve of a fixed-point pass) gets the codes copied and EVERY row verified against its class
    (pgd_classify_counts: served by the cache).  Same product bit for bit with the cache on and off; an operator with the same
    signature but another structure - the hint is a sample of the Dirichlet list - must fall back to the full classification
    and still give the right product; new coefficients must give new couplings, not the cached operator's."""
    nx, ny, nz = 130, 37, 41
    coords, cells = F.box_mesh((0, 0, 0), (1.0, 0.7, 1.3), nx - 1, ny - 1, nz - 1)
    h = ctx.mesh_upload(coords, cells)
    n = coords.shape[0]
    ak, am = ctx.atom_assemble(h, F.STIFF), ctx.atom_assemble(h, F.MASS)
    bnd = boundary_dofs(coords).astype(np.int32)
    rng = np.random.default_rng(3)
    x = rng.uniform(-1, 1, n)
    xv, yv = ctx.vec_from(x), ctx.vec_alloc(n)
    ctx.flags_reset()

    def product(op, L=5):
        ctx.tune(7, 4)
        ctx.tune(36, L)
        ctx.vec_fill(yv, -2.0)
        ctx.spmv_dot_slot(op, xv, yv, xv, 0, n, 30)
        return ctx.vec_download(yv)

    def reference(op):
        ctx.tune(3, 0)
        ctx.vec_fill(yv, -2.0)
        ctx.spmv_dot_slot(op, xv, yv, xv, 0, n, 30)
        ctx.tune(3, 1)
        assert ctx.op_symmetrize(op)
        return ctx.vec_download(yv)
    try:
        c0 = ctx.classify_counts()
        ys = {}
        for cache in (1, 0):
            ctx.tune(39, cache)
            for coefs in ((1.0, 0.37), (2.5, 0.01), (1.0, 0.37)):
                op = ctx.op_combine(h, [ak, am], list(coefs), bnd)
                ref = reference(op)
                assert ctx.op_classify(op) > 0
                k0 = ctx.kernel_counts()
                y = product(op)
                assert ctx.kernel_counts()["stencil_march"] == k0["stencil_march"] + 1
                assert np.array_equal(y, ref), (cache, coefs)
                ys[(cache, coefs)] = y
                ctx.atom_free(op)
        c1 = ctx.classify_counts()
        assert c1["cached"] - c0["cached"] == 2 and c1["full"] - c0["full"] == 4      # cache on: 1 full + 2 served; off: 3 full
        assert not np.array_equal(ys[(1, (1.0, 0.37))], ys[(1, (2.5, 0.01))])
        for coefs in ((1.0, 0.37), (2.5, 0.01)):
            assert np.array_equal(ys[(1, coefs)], ys[(0, coefs)])
        # the same sampled signature, another Dirichlet set: every 4096th entry of the list is kept, one in between is dropped -
        # the vertex becomes a free node on the rim, its row and its neighbours' rows change
        ctx.tune(39, 1)
        step = max(1, bnd.size // 4096)
        drop = 1 if step > 1 else None
        if drop is not None:
            bnd2 = np.delete(bnd, drop)
            op = ctx.op_combine(h, [ak, am], [1.0, 0.37], bnd2)
            ref = reference(op)
            c2 = ctx.classify_counts()
            ncls = ctx.op_classify(op)
            c3 = ctx.classify_counts()
            assert c3["full"] == c2["full"] + 1 and c3["cached"] == c2["cached"]       # the cached structure did not verify
            y = product(op)
            assert np.array_equal(y, ref) and ncls > 0
            ctx.atom_free(op)
    finally:
        ctx.tune(7, 0)
        ctx.tune(36, 0)
        ctx.tune(39, 1)
        ctx.tune(3, 1)
    for v in (xv, yv):
        ctx.vec_free(v)
    for a in (ak, am):
        ctx.atom_free(a)
    ctx.mesh_free(h)


def test_classification_cache_evicts_least_recently_used(ctx):
    """A mesh keeps at most four remembered structures and drops the least recently USED one.  Five Dirichlet lists on one fresh
    mesh - the hull plus 0 .. 4 interior vertices: the signature mixes the list's length - are classified in order, then S4, S0, S2,
    S1 again; pgd_classify_counts around every classification says whether the cache served it.  Every operator's product from
    its classes equals the CSR product bit for bit, whichever way the classes came."""
    nx, ny, nz = 12, 9, 7
    coords, cells = F.box_mesh((0, 0, 0), (1.0, 0.7, 1.3), nx - 1, ny - 1, nz - 1)
    h = ctx.mesh_upload(coords, cells)
    n = coords.shape[0]
    plane = nx * ny
    ak, am = ctx.atom_assemble(h, F.STIFF), ctx.atom_assemble(h, F.MASS)
    bnd = boundary_dofs(coords).astype(np.int32)
    interior = np.array([(2 + 2 * k) + nx * (2 + k) + plane * (1 + k) for k in range(4)], dtype=np.int32)
    assert np.intersect1d(bnd, interior).size == 0 and np.unique(interior).size == 4
    lists = [np.union1d(bnd, interior[:k]).astype(np.int32) for k in range(5)]
    rng = np.random.default_rng(11)
    x = rng.uniform(-1, 1, n)
    xv, yv = ctx.vec_from(x), ctx.vec_alloc(n)
    ctx.flags_reset()

    def product(op):
        ctx.tune(7, 4)
        ctx.tune(36, 5)
        ctx.vec_fill(yv, -2.0)
        ctx.spmv_dot_slot(op, xv, yv, xv, 0, n, 30)
        return ctx.vec_download(yv)

    def reference(op):
        ctx.tune(3, 0)
        ctx.vec_fill(yv, -2.0)
        ctx.spmv_dot_slot(op, xv, yv, xv, 0, n, 30)
        ctx.tune(3, 1)
        assert ctx.op_symmetrize(op)
        return ctx.vec_download(yv)
    # (list, full, cached): the fifth insert evicts S0; S4 is served; S0 is classified in full again and evicts S1 - S4 was used
    # after it -; S2 is served; S1 is gone
    steps = [(0, 1, 0), (1, 1, 0), (2, 1, 0), (3, 1, 0), (4, 1, 0), (4, 0, 1), (0, 1, 0), (2, 0, 1), (1, 1, 0)]
    try:
        ctx.tune(39, 1)
        for step, (k, full, cached) in enumerate(steps):
            op = ctx.op_combine(h, [ak, am], [1.0, 0.37], lists[k])
            ref = reference(op)
            c0 = ctx.classify_counts()
            ncls = ctx.op_classify(op)
            c1 = ctx.classify_counts()
            print("step %d: S%d classes %d full +%d cached +%d" % (step + 1, k, ncls, c1["full"] - c0["full"], c1["cached"] - c0["cached"]))
            assert ncls > 0, (step, k)
            assert (c1["full"] - c0["full"], c1["cached"] - c0["cached"]) == (full, cached), (step, k)
            k0 = ctx.kernel_counts()
            y = product(op)
            k1 = ctx.kernel_counts()
            assert k1["stencil_march"] + k1["diac_march"] == k0["stencil_march"] + k0["diac_march"] + 1, (step, k)
            assert np.array_equal(y, ref), (step, k)
            ctx.atom_free(op)
    finally:
        ctx.tune(7, 0)
        ctx.tune(36, 0)
        ctx.tune(39, 1)
        ctx.tune(3, 1)
    for v in (xv, yv):
        ctx.vec_free(v)
    for a in (ak, am):
        ctx.atom_free(a)
    ctx.mesh_free(h)


def test_pcg_on_the_stencil_form_walks_the_same_iterates(ctx):
    """The library's PCG with the scaled operator in its stencil form (k_spmv_stencil_march) against the same solve on the
    row-class dictionary: y is bit-identical, the fused dots are grouped per workgroup (64 x 16 patches instead of 64 x 8), so
    the iterates agree to rounding - iteration counts within one, the solution to 1e-9, the true residual at the tolerance."""
    from pgdrome_amd import fem
    npts = 104
    mesh = fem.BoxMesh(fem.Point(0, 0, 0), fem.Point(1, 1, 1), npts - 1, npts - 1, npts - 1)
    coords = mesh.coordinates()
    h = ctx.mesh_upload(coords, mesh.cells())
    n = coords.shape[0]
    ak, am = ctx.atom_assemble(h, F.STIFF), ctx.atom_assemble(h, F.MASS)
    bc = np.where(np.any((coords <= 1e-12) | (coords >= 1 - 1e-12), axis=1))[0].astype(np.int32)
    rng = np.random.default_rng(21)
    b = rng.uniform(-1, 1, n)
    b[bc] = rng.uniform(-1, 1, bc.size)                  # non-zero Dirichlet values: the identity rows carry them
    bv = ctx.vec_from(b)
    out = {}
    try:
        for stencil in (1, 0):
            ctx.tune(35, stencil)
            op = ctx.op_combine(h, [ak, am], [1.0, 3.0], bc)
            xv = ctx.vec_alloc(n)
            k0 = ctx.kernel_counts()
            it, rel = ctx.pcg_solve(op, bv, xv, 1e-10, 0.0, 10000)
            k1 = ctx.kernel_counts()
            st, coded = k1["stencil_march"] - k0["stencil_march"], k1["diac_march"] - k0["diac_march"]
            # (launches replayed from the captured chunk are not counted: the eager first chunk and the capture are)
            assert (st > 10 and coded == 0) if stencil else (st == 0 and coded > 10), (stencil, st, coded)
            assert it > 100
            xs = ctx.vec_download(xv)
            out[stencil] = (it, rel, xs)
            assert np.abs(xs[bc] - b[bc]).max() <= 1e-9        # identity rows: solved by the iteration like every other row
            # the true residual through the CSR kernel of the unscaled operator
            yv = ctx.vec_alloc(n)
            ctx.flags_reset()
            ctx.tune(3, 0)
            ctx.spmv_dot_slot(op, xv, yv, xv, 0, n, 30)
            ctx.tune(3, 1)
            assert np.linalg.norm(b - ctx.vec_download(yv)) <= 1.05e-10 * np.linalg.norm(b)
            for v in (yv, xv):
                ctx.vec_free(v)
            ctx.atom_free(op)
    finally:
        ctx.tune(35, 1)
        ctx.tune(3, 1)
    assert abs(out[1][0] - out[0][0]) <= 1 and np.linalg.norm(out[1][2] - out[0][2]) <= 1e-9 * np.linalg.norm(out[0][2])
    ctx.vec_free(bv)
    for a in (ak, am):
        ctx.atom_free(a)
    ctx.mesh_free(h)


def test_pcg_on_row_classes_is_bit_identical(ctx):
    """The library's PCG classifies the scaled operator per solve: with and without the dictionary the solve walks the same
    iterates bit for bit (single-sync recurrence and the two-reduction one) when both kernels march equally far - y is
    bit-identical anyway, the fused dots are summed per workgroup - and it really ran on the coded kernel."""
    from pgdrome_amd import fem
    npts = 104
    mesh = fem.BoxMesh(fem.Point(0, 0, 0), fem.Point(1, 1, 1), npts - 1, npts - 1, npts - 1)
    coords = mesh.coordinates()
    h = ctx.mesh_upload(coords, mesh.cells())
    n = coords.shape[0]
    ak, am = ctx.atom_assemble(h, F.STIFF), ctx.atom_assemble(h, F.MASS)
    bc = np.where(np.any((coords <= 1e-12) | (coords >= 1 - 1e-12), axis=1))[0].astype(np.int32)
    rng = np.random.default_rng(21)
    b = rng.uniform(-1, 1, n)
    b[bc] = 0.0
    bv = ctx.vec_from(b)
    out = {}
    try:
        ctx.tune(7, 6)        # the same march length for both kernels: the same workgroups, the same partial sums of the fused dots
        for ss in (1, 0):
            ctx.tune(18, ss)
            for classes in (1, 0):
                ctx.tune(19, classes)
                op = ctx.op_combine(h, [ak, am], [1.0, 3.0], bc)
                xv = ctx.vec_alloc(n)
                k0 = ctx.kernel_counts()
                it, rel = ctx.pcg_solve(op, bv, xv, 1e-10, 0.0, 10000)
                k1 = ctx.kernel_counts()
                coded, plain = k1["diac_march"] - k0["diac_march"], k1["dia_march"] - k0["dia_march"]
                assert (coded > 0 and plain == 0) if classes else (coded == 0 and plain > 0)
                out[(ss, classes)] = (it, rel, ctx.vec_download(xv))
                # afterwards the operator is usable as before: products of the UNSCALED operator through the plain kernels
                yv = ctx.vec_alloc(n)
                ctx.flags_reset()
                ctx.spmv_dot_slot(op, xv, yv, xv, 0, n, 30)
                r = b - ctx.vec_download(yv)
                assert np.linalg.norm(r) <= 1.05e-10 * np.linalg.norm(b)
                ctx.vec_free(yv)
                ctx.vec_free(xv)
                ctx.atom_free(op)
    finally:
        ctx.tune(7, 0)
        ctx.tune(18, 1)
        ctx.tune(19, 1)
    for ss in (1, 0):
        a, c = out[(ss, 1)], out[(ss, 0)]
        assert a[0] == c[0] and a[1] == c[1] and np.array_equal(a[2], c[2]), (ss, a[0], c[0])
    ctx.vec_free(bv)
    for a in (ak, am):
        ctx.atom_free(a)
    ctx.mesh_free(h)


def test_derived_scaled_stencil_is_the_classified_one(ctx):
    """pgd_pcg_solve on an operator that is one stencil + eliminated nodes: the couplings of D^-1/2 A D^-1/2 DERIVED from A's
    (PGD_TUNE_PCG_DERIVE_SCALED: no scaling pass, no second classification) against those of the scaled and classified slot
    arrays - iteration counts, reported residuals and x IDENTICAL (the same eight numbers go into the same kernel); with the
    diagonal set to 1 and not, under the multigrid preconditioner as well; the operator multiplies as A afterwards; an operator
    with a natural boundary keeps the scaling pass either way."""
    from pgdrome_amd import fem
    npts = 104
    mesh = fem.BoxMesh(fem.Point(0, 0, 0), fem.Point(1, 1, 1), npts - 1, npts - 1, npts - 1)
    coords = mesh.coordinates()
    h = ctx.mesh_upload(coords, mesh.cells())
    n = coords.shape[0]
    ak, am = ctx.atom_assemble(h, F.STIFF), ctx.atom_assemble(h, F.MASS)
    hull = np.where(np.any((coords <= 1e-12) | (coords >= 1 - 1e-12), axis=1))[0].astype(np.int32)
    face = np.where(coords[:, 2] <= 1e-12)[0].astype(np.int32)          # natural boundaries elsewhere: not one stencil
    rng = np.random.default_rng(51)
    b = rng.uniform(-1, 1, n)
    bv = ctx.vec_from(b)
    x0 = 0.01 * rng.uniform(-1, 1, n)
    out = {}
    try:
        for derive in (1, 0):
            ctx.tune(43, derive)
            for key, bc, unit, mg in (("hull", hull, 1, 0), ("hull-nounit", hull, 0, 0), ("hull-mg", hull, 1, 1), ("face", face, 1, 0)):
                ctx.tune(17, unit)
                ctx.tune(40, mg)
                op = ctx.op_combine(h, [ak, am], [1.0, 3.0], bc)
                xs = x0.copy(); xs[bc] = 0.0
                xv = ctx.vec_from(xs)
                cc0 = sum(ctx.classify_counts().values())
                k0 = ctx.kernel_counts()
                it, rel = ctx.pcg_solve(op, bv, xv, 1e-10, 0.0, 10000)
                k1 = ctx.kernel_counts()
                ncls = sum(ctx.classify_counts().values()) - cc0
                st = k1["stencil_march"] - k0["stencil_march"]
                assert (st > 0) == (key != "face"), (key, st)
                # derived: A is classified (here: nobody has before), and that is all; an operator that turns out not to be one
                # stencil has its scaled slot arrays classified as well.  Not derived: the scaled slot arrays only
                assert ncls == (2 if derive and key == "face" else 1), (key, derive, ncls)
                xsol = ctx.vec_download(xv)
                out[(derive, key)] = (it, rel, xsol)
                assert rel <= 1e-10 and it > 5
                # afterwards the operator multiplies as A: the true residual through the CSR kernel
                yv = ctx.vec_alloc(n)
                ctx.tune(3, 0)
                ctx.spmv(op, xv, yv)
                ctx.tune(3, 1)
                rhs = b.copy()
                assert np.linalg.norm(rhs - ctx.vec_download(yv)) <= 1.05e-10 * np.linalg.norm(rhs)
                # ... and through its own fast form
                ctx.spmv(op, xv, yv)
                assert np.linalg.norm(rhs - ctx.vec_download(yv)) <= 1.05e-10 * np.linalg.norm(rhs)
                for v in (xv, yv):
                    ctx.vec_free(v)
                ctx.atom_free(op)
    finally:
        ctx.tune(43, 1)
        ctx.tune(17, 1)
        ctx.tune(40, 0)
        ctx.tune(3, 1)
    for key in ("hull", "hull-nounit", "hull-mg", "face"):
        a, c = out[(1, key)], out[(0, key)]
        assert a[0] == c[0] and a[1] == c[1] and np.array_equal(a[2], c[2]), (key, a[0], c[0], a[1], c[1])
    ctx.vec_free(bv)
    for a in (ak, am):
        ctx.atom_free(a)
    ctx.mesh_free(h)


def test_lagged_x_update_leaves_the_recurrence_alone(ctx):
    """Single-sync recurrence with x updated every other iteration (two terms, the earlier direction reconstructed from
    p = r + beta' p'): iteration counts and reported residuals are IDENTICAL to the every-iteration update - nothing of the
    recurrence reads x - and x agrees to rounding; also when the solve stops between the two halves of a pair (odd maxit:
    the outstanding term is applied on the way out), on an even maxit, and on a converged start."""
    from pgdrome_amd import fem
    npts = 104
    mesh = fem.BoxMesh(fem.Point(0, 0, 0), fem.Point(1, 1, 1), npts - 1, npts - 1, npts - 1)
    coords = mesh.coordinates()
    h = ctx.mesh_upload(coords, mesh.cells())
    n = coords.shape[0]
    ak, am = ctx.atom_assemble(h, F.STIFF), ctx.atom_assemble(h, F.MASS)
    bc = np.where(np.any((coords <= 1e-12) | (coords >= 1 - 1e-12), axis=1))[0].astype(np.int32)
    rng = np.random.default_rng(31)
    b = rng.uniform(-1, 1, n)
    b[bc] = 0.0
    x0 = 0.01 * rng.uniform(-1, 1, n)
    x0[bc] = 0.0
    bv = ctx.vec_from(b)
    out = {}
    try:
        for lag in (1, 0):
            ctx.tune(22, lag)
            for maxit in (10000, 23, 24, 1, 2):
                op = ctx.op_combine(h, [ak, am], [1.0, 3.0], bc)
                xv = ctx.vec_from(x0)
                it, rel = ctx.pcg_solve(op, bv, xv, 1e-10, 0.0, maxit)
                out[(lag, maxit)] = (it, rel, ctx.vec_download(xv))
                if maxit == 10000:
                    it2, rel2 = ctx.pcg_solve(op, bv, xv, 1e-10, 0.0, maxit)
                    out[(lag, "again")] = (it2, rel2, ctx.vec_download(xv))
                    if lag:          # the true residual of the lagged solve through an independent kernel
                        yv = ctx.vec_alloc(n)
                        ctx.tune(3, 0)
                        ctx.spmv(op, xv, yv)
                        ctx.tune(3, 1)
                        assert np.linalg.norm(b - ctx.vec_download(yv)) <= 1.05e-10 * np.linalg.norm(b)
                        ctx.vec_free(yv)
                ctx.vec_free(xv)
                ctx.atom_free(op)
        # the cache hints of the recurrence (q, r, x streamed, p cached) change no bit
        ctx.tune(22, 1)
        ctx.tune(23, 0)
        op = ctx.op_combine(h, [ak, am], [1.0, 3.0], bc)
        xv = ctx.vec_from(x0)
        it, rel = ctx.pcg_solve(op, bv, xv, 1e-10, 0.0, 10000)
        a = out[(1, 10000)]
        assert it == a[0] and rel == a[1] and np.array_equal(ctx.vec_download(xv), a[2])
        ctx.vec_free(xv)
        ctx.atom_free(op)
    finally:
        ctx.tune(22, 1)
        ctx.tune(23, 1)
    for key in (10000, 23, 24, 1, 2, "again"):
        a, c = out[(1, key)], out[(0, key)]
        if key == "again":       # starts from the solution of the run before, which differs in the last bits
            assert a[0] == c[0] and abs(a[1] - c[1]) <= 1e-6 * c[1], (key, a[:2], c[:2])
        else:
            assert a[0] == c[0] and a[1] == c[1], (key, a[:2], c[:2])
        assert np.linalg.norm(a[2] - c[2]) <= 1e-13 * np.linalg.norm(c[2]), (key, np.linalg.norm(a[2] - c[2]) / np.linalg.norm(c[2]))
    assert out[(1, 23)][0] == 23 and out[(1, 24)][0] == 24 and out[(1, "again")][0] <= 1 and out[(1, 10000)][1] <= 1e-10
    ctx.vec_free(bv)
    for a in (ak, am):
        ctx.atom_free(a)
    ctx.mesh_free(h)


@pytest.mark.parametrize("name", ["rect129", "box40"])
def test_two_launch_recurrence_of_small_systems(ctx, name):
    """Systems of up to 2^20 rows: single-sync recurrence in TWO launches per iteration - the product, and k_pcg1_step, whose
    every workgroup sums the partial sums and forms alpha, beta and the stop decision itself (alternating buffers).  Against
    the two-reduction recurrence in three launches (PGD_TUNE_PCG_SMALL_SINGLE_SYNC = 0): iteration counts +0 .. +2 (the stop
    test sees a residual one iteration later), the same solution, the TRUE residual at the tolerance through the CSR kernel,
    the same iterate when cut off at an odd and an even count, a converged start, bitwise reproducible."""
    if name == "rect129":
        coords, cells = F.rectangle_mesh((0, 0), (1.0, 0.8), 128, 128)
    else:
        coords, cells = F.box_mesh((0, 0, 0), (1.0, 0.7, 1.3), 39, 39, 39)
    h = ctx.mesh_upload(coords, cells)
    n = coords.shape[0]
    ak, am = ctx.atom_assemble(h, F.STIFF), ctx.atom_assemble(h, F.MASS)
    bc = boundary_dofs(coords).astype(np.int32)
    rng = np.random.default_rng(3)
    b = rng.uniform(-1, 1, n)
    b[bc] = 0.0
    bv = ctx.vec_from(b)
    res = {}
    try:
        for two in (1, 0, 1):
            ctx.tune(25, two)
            for maxit in (10000, 23, 24):
                op = ctx.op_combine(h, [ak, am], [1.0, 3.0], bc)
                xv = ctx.vec_alloc(n)
                it, rel = ctx.pcg_solve(op, bv, xv, 1e-10, 0.0, maxit)
                x = ctx.vec_download(xv)
                if maxit == 10000:
                    it2, _ = ctx.pcg_solve(op, bv, xv, 1e-10, 0.0, maxit)
                    assert it2 <= 1
                    yv = ctx.vec_alloc(n)
                    ctx.tune(3, 0)
                    ctx.spmv(op, ctx.vec_from(x), yv)
                    ctx.tune(3, 1)
                    assert np.linalg.norm(b - ctx.vec_download(yv)) <= 1.05e-10 * np.linalg.norm(b)
                    ctx.vec_free(yv)
                res.setdefault((two, maxit), []).append((it, rel, x))
                ctx.vec_free(xv)
                ctx.atom_free(op)
    finally:
        ctx.tune(25, 1)
    a, t = res[(1, 10000)], res[(0, 10000)][0]
    assert a[0][0] == a[1][0] and a[0][1] == a[1][1] and np.array_equal(a[0][2], a[1][2])      # reproducible run to run
    assert 0 <= a[0][0] - t[0] <= 2 and a[0][1] <= 1e-10 and t[1] <= 1e-10
    assert np.linalg.norm(a[0][2] - t[2]) <= 1e-9 * np.linalg.norm(t[2])
    for maxit in (23, 24):
        c1, c0 = res[(1, maxit)][0], res[(0, maxit)][0]
        assert c1[0] == c0[0] == maxit and np.linalg.norm(c1[2] - c0[2]) <= 1e-10 * np.linalg.norm(c0[2])
    ctx.vec_free(bv)
    for at in (ak, am):
        ctx.atom_free(at)
    ctx.mesh_free(h)


def test_vector_ops(ctx):
    rng = np.random.default_rng(5)
    for n in (1, 63, 64, 257, 100_003):
        x, y = rng.standard_normal(n), rng.standard_normal(n)
        xv, yv = ctx.vec_from(x), ctx.vec_from(y)
        ctx.vec_axpy(yv, -0.75, xv)
        assert np.allclose(ctx.vec_download(yv), y - 0.75 * x, rtol=1e-15, atol=1e-15)
        ctx.vec_scale(xv, 3.0)
        assert np.array_equal(ctx.vec_download(xv), 3.0 * x)
        ctx.vec_fill(yv, 2.5)
        assert np.all(ctx.vec_download(yv) == 2.5)
        idx = np.unique(rng.integers(0, n, size=min(n, 17))).astype(np.int32)
        ctx.vec_set(yv, idx, np.arange(idx.size, dtype=np.float64))
        got = ctx.vec_download(yv)
        assert np.array_equal(got[idx], np.arange(idx.size)) and np.sum(got != 2.5) <= idx.size
        ctx.vec_copy(yv, xv)
        assert np.array_equal(ctx.vec_download(yv), 3.0 * x)
        assert ctx.vec_size(xv) == n
        ctx.vec_free(xv)
        ctx.vec_free(yv)


def test_kept_index_lists_are_compared_not_trusted(ctx):
    """pgd_vec_set keeps a large index list and its values on the device, pgd_op_combine the Dirichlet list of the last operator
    on a mesh (the same lists come back in every solve of a fixed-point pass): a call is served from what is kept only when its
    arrays equal the kept ones word by word - one changed index or value, another length, a vector too short for a kept index
    must all be seen."""
    from pgdrome_amd import _lib, fem
    rng = np.random.default_rng(77)
    n = 50_000
    idx = np.sort(rng.choice(n, size=9000, replace=False)).astype(np.int32)
    val = rng.standard_normal(idx.size)
    xv = ctx.vec_alloc(n)

    def check(i, v):
        ctx.vec_fill(xv, 2.5)
        ctx.vec_set(xv, i, v)
        want = np.full(n, 2.5)
        want[i] = v
        assert np.array_equal(ctx.vec_download(xv), want)

    check(idx, val)
    check(idx, val)                                   # served from the kept lists
    v2 = val.copy(); v2[4321] += 1.0
    check(idx, v2)                                    # one value differs
    i2 = idx.copy(); i2[-1] = n - 1 if idx[-1] != n - 1 else n - 2
    check(i2, v2)                                     # one index differs
    check(idx[:8000], val[:8000])                     # another length
    check(idx[:17], val[:17])                         # a small list in between (its own scratch) ...
    check(idx[:8000], val[:8000])                     # ... leaves the kept one intact
    short = ctx.vec_alloc(int(idx[7999]))             # the kept list's largest index is out of range for this vector
    with pytest.raises(_lib.PgdError):
        ctx.vec_set(short, idx[:8000], val[:8000])
    ctx.vec_free(short)
    ctx.vec_free(xv)
    # the Dirichlet list of pgd_op_combine
    mesh = fem.BoxMesh(fem.Point(0, 0, 0), fem.Point(1, 1, 1), 15, 13, 11)
    coords = mesh.coordinates()
    h = ctx.mesh_upload(coords, mesh.cells())
    nv = coords.shape[0]
    ak, am = ctx.atom_assemble(h, F.STIFF), ctx.atom_assemble(h, F.MASS)
    bc = np.where(np.any((coords <= 1e-12) | (coords >= 1 - 1e-12), axis=1))[0].astype(np.int32)
    x = rng.standard_normal(nv)
    xv, yv = ctx.vec_from(x), ctx.vec_alloc(nv)

    def product(bcs, coefs):
        op = ctx.op_combine(h, [ak, am], coefs, bcs)
        ctx.spmv(op, xv, yv)
        y = ctx.vec_download(yv)
        ctx.atom_free(op)
        return y

    y0 = product(bc, [1.0, 3.0])
    assert np.array_equal(y0[bc], x[bc])
    assert np.array_equal(product(bc, [1.0, 3.0]), y0)               # the kept list
    y1 = product(bc, [2.0, 0.5])                                     # ... with other coefficients
    assert np.array_equal(y1[bc], x[bc]) and not np.array_equal(y1, y0)
    free = np.setdiff1d(np.arange(nv), bc)
    bc2 = bc.copy(); bc2[bc.size // 2] = free[free.size // 2]; bc2.sort()      # same length, one node swapped
    y2 = product(bc2, [1.0, 3.0])
    assert np.array_equal(y2[bc2], x[bc2]) and not np.array_equal(y2, y0)
    assert np.array_equal(product(bc, [1.0, 3.0]), y0)
    with pytest.raises(_lib.PgdError):
        bad = bc.copy(); bad[-1] = nv
        product(bad, [1.0, 3.0])
    assert np.array_equal(product(bc, [1.0, 3.0]), y0)
    for v in (xv, yv):
        ctx.vec_free(v)
    for a in (ak, am):
        ctx.atom_free(a)
    ctx.mesh_free(h)


def test_multidot_matches_single_dots(ctx):
    """pgd_vec_multidot: x . y_j for 1 .. 40 vectors (chunks of 17) and a partial range, against numpy and against
    pgd_vec_dot (the functionals of one iterate against all stored modes go through it, fem._dots_with_stored_products)."""
    from pgdrome_amd._lib import PgdError
    rng = np.random.default_rng(77)
    for n, lo, hi in ((1, 0, -1), (257, 3, 200), (100_003, 0, -1), (100_003, 999, 54_321)):
        x = rng.standard_normal(n)
        ys = [rng.standard_normal(n) for _ in range(40)]
        xv, yv = ctx.vec_from(x), [ctx.vec_from(y) for y in ys]
        stop = n if hi < 0 else hi
        for k in (1, 2, 16, 17, 18, 34, 35, 40):
            got = ctx.vec_multidot(xv, yv[:k], lo, hi)
            want = np.array([x[lo:stop] @ y[lo:stop] for y in ys[:k]])
            scale = np.array([np.abs(x[lo:stop]) @ np.abs(y[lo:stop]) for y in ys[:k]])
            assert np.all(np.abs(got - want) <= 4e-16 * np.sqrt(max(stop - lo, 1)) * scale + 1e-300), (n, k)
            one = np.array([ctx.vec_dot(xv, v, lo, hi) for v in yv[:k]])
            assert np.all(np.abs(got - one) <= 1e-14 * scale + 1e-300)
            assert np.array_equal(got, ctx.vec_multidot(xv, yv[:k], lo, hi))          # fixed summation order
        assert np.array_equal(ctx.vec_multidot(xv, yv[:3], 0, 0), np.zeros(3))
        with pytest.raises(PgdError):
            ctx.vec_multidot(xv, [yv[0], 999999], lo, hi)
        with pytest.raises(PgdError):
            ctx.vec_multidot(xv, yv[:2], 5, n + 1)
        for v in [xv] + yv:
            ctx.vec_free(v)


def test_multidot_pair_matches_single_dots(ctx):
    """pgd_vec_multidot_pair: x0 . y_j and x1 . y_j for 1 .. 40 vectors (chunks of 16), every y_j read once for both, against
    numpy and pgd_vec_dot (fem._prefetch_functionals: (K F) . m_j and (M F) . m_j of an iterate against the stored modes)."""
    from pgdrome_amd._lib import PgdError
    rng = np.random.default_rng(78)
    for n, lo, hi in ((1, 0, -1), (257, 3, 200), (100_003, 0, -1), (100_003, 999, 54_321)):
        x0, x1 = rng.standard_normal(n), rng.standard_normal(n)
        ys = [rng.standard_normal(n) for _ in range(40)]
        v0, v1, yv = ctx.vec_from(x0), ctx.vec_from(x1), [ctx.vec_from(y) for y in ys]
        stop = n if hi < 0 else hi
        for k in (1, 2, 15, 16, 17, 32, 33, 40):
            g0, g1 = ctx.vec_multidot_pair(v0, v1, yv[:k], lo, hi)
            for got, x, xv in ((g0, x0, v0), (g1, x1, v1)):
                want = np.array([x[lo:stop] @ y[lo:stop] for y in ys[:k]])
                scale = np.array([np.abs(x[lo:stop]) @ np.abs(y[lo:stop]) for y in ys[:k]])
                assert np.all(np.abs(got - want) <= 4e-16 * np.sqrt(max(stop - lo, 1)) * scale + 1e-300), (n, k)
                one = np.array([ctx.vec_dot(xv, v, lo, hi) for v in yv[:k]])
                assert np.all(np.abs(got - one) <= 1e-14 * scale + 1e-300)
            h0, h1 = ctx.vec_multidot_pair(v0, v1, yv[:k], lo, hi)
            assert np.array_equal(g0, h0) and np.array_equal(g1, h1)                  # fixed summation order
        # the same vector on both sides, and as a right-hand vector
        s0, s1 = ctx.vec_multidot_pair(v0, v0, [v0, yv[0]], lo, hi)
        assert np.array_equal(s0, s1) and s0[0] > 0.0 or stop == lo
        z0, z1 = ctx.vec_multidot_pair(v0, v1, yv[:3], 0, 0)
        assert np.array_equal(z0, np.zeros(3)) and np.array_equal(z1, np.zeros(3))
        with pytest.raises(PgdError):
            ctx.vec_multidot_pair(v0, v1, [yv[0], 999999], lo, hi)
        with pytest.raises(PgdError):
            ctx.vec_multidot_pair(v0, v1, yv[:2], 5, n + 1)
        for v in [v0, v1] + yv:
            ctx.vec_free(v)


@pytest.mark.parametrize("kind", ["mass", "stiff", "conv", "convt", "wmass", "wstiff"])
def test_p2_interval_atoms_match_oracle(ctx, kind):
    """Quadratic elements on a non-uniform interval mesh: pattern bit-exact, values to rounding."""
    rng = np.random.default_rng(4)
    x = np.sort(np.concatenate([[0.0, 3.0], rng.uniform(0, 3, 37)]))
    coords, cells = x.reshape(-1, 1), np.stack([np.arange(38), np.arange(1, 39)], axis=1).astype(np.int32)
    nodes, tab = F.p2_interval_nodes(coords, cells)
    h = ctx.mesh_upload(nodes, tab)
    rp, cols = ctx.mesh_pattern(h)
    rp_o, cols_o = F.csr_pattern(nodes.shape[0], tab)
    assert np.array_equal(rp, rp_o) and np.array_equal(cols, cols_o)
    assert ctx.mesh_info(h)["kl"] == 2 and ctx.mesh_info(h)["ku"] == 2
    k = F.KIND_NAMES.index(kind)
    w, wv = None, 0
    if kind in ("wmass", "wstiff"):
        w = 1.0 + nodes[:, 0] ** 2
        wv = ctx.vec_from(w)
    a = ctx.atom_assemble(h, k, 0, 0, wv)
    ref = F.assemble_atom(nodes, tab, k, 0, 0, w)
    vals = ctx.atom_download(a, ref.nnz)
    assert np.abs(vals - ref.data).max() <= 1e-13 * np.abs(ref.data).max()
    ctx.mesh_free(h)


def test_lincomb(ctx):
    """y = sum_k c_k x_k (online reconstruction): exact against the same fma chain in numpy order."""
    rng = np.random.default_rng(17)
    n = 100_003
    X = rng.standard_normal((11, n))
    xs = [ctx.vec_from(X[k]) for k in range(11)]
    y = ctx.vec_from(rng.standard_normal(n))
    for k in (0, 1, 8, 11):
        c = rng.uniform(-2, 2, k)
        ctx.vec_lincomb(y, xs[:k], c)
        ref = (c[:, None] * X[:k]).sum(axis=0) if k else np.zeros(n)
        assert np.abs(ctx.vec_download(y) - ref).max() <= 1e-14 * max(1.0, np.abs(ref).max()) * max(k, 1)
    from pgdrome_amd._lib import PgdError
    with pytest.raises(PgdError):
        ctx.vec_lincomb(y, [y], [1.0])
    for v in xs + [y]:
        ctx.vec_free(v)


def boundary_dofs(coords):
    lo, hi = coords.min(axis=0), coords.max(axis=0)
    return np.where(np.any((coords <= lo + 1e-12) | (coords >= hi - 1e-12), axis=1))[0].astype(np.int32)


def test_combine_dirichlet_and_pcg(ctx, mesh):
    name, coords, cells, h = mesh
    n = coords.shape[0]
    if n < 3:
        pytest.skip("needs interior dofs")
    rng = np.random.default_rng(99)
    K, M = F.assemble_atom(coords, cells, F.STIFF), F.assemble_atom(coords, cells, F.MASS)
    ak, am = ctx.atom_assemble(h, F.STIFF), ctx.atom_assemble(h, F.MASS)
    bc = boundary_dofs(coords)
    c1, c2 = 0.7, 2.5
    op = ctx.op_combine(h, [ak, am], [c1, c2], bc)
    nnz = K.nnz
    A_ref, _ = F.apply_dirichlet(c1 * K + c2 * M, np.zeros(n), bc)
    # apply_dirichlet drops structural zeros: compare as dense-equivalent via the shared pattern
    A_dev = sps.csr_matrix((ctx.atom_download(op, nnz), K.indices, K.indptr), shape=(n, n))
    assert abs(A_dev - A_ref).max() <= 1e-13 * abs(A_ref).max()
    b = rng.uniform(-1, 1, n)
    b[bc] = 0.0
    bv, xv = ctx.vec_from(b), ctx.vec_alloc(n)
    it, rel = ctx.pcg_solve(op, bv, xv, rtol=1e-12, maxit=5000)
    x = ctx.vec_download(xv)
    x_ref = F.direct_solve(A_ref, b)
    assert rel <= 1e-12
    assert np.linalg.norm(x - x_ref) <= 1e-9 * np.linalg.norm(x_ref)
    x_o, it_o, _ = F.pcg_jacobi(A_ref, b, rtol=1e-12, maxit=5000)
    assert abs(it - it_o) <= max(2, it_o // 50)          # same recurrence, summation order differs
    # reusing the operator storage, no Dirichlet rows, warm start converges at once
    op2 = ctx.op_combine(h, [ak, am], [c1, c2], None, op)
    assert op2 == op
    A2 = c1 * K + c2 * M
    bv2 = ctx.vec_from(A2 @ x_ref)
    ctx.vec_upload(xv, x_ref)
    it2, rel2 = ctx.pcg_solve(op, bv2, xv, rtol=1e-10, maxit=50)
    assert it2 == 0 and rel2 <= 1e-10
    for v in (bv, xv, bv2):
        ctx.vec_free(v)
    for a in (ak, am, op):
        ctx.atom_free(a)


def test_pcg_is_bitwise_reproducible(ctx):
    coords, cells = F.box_mesh((0, 0, 0), (1, 1, 1), 15, 15, 15)
    h = ctx.mesh_upload(coords, cells)
    n = coords.shape[0]
    ak, am = ctx.atom_assemble(h, F.STIFF), ctx.atom_assemble(h, F.MASS)
    op = ctx.op_combine(h, [ak, am], [1.0, 1.0], boundary_dofs(coords))
    b = np.random.default_rng(3).uniform(-1, 1, n)
    b[boundary_dofs(coords)] = 0
    bv = ctx.vec_from(b)
    out = []
    for _ in range(2):
        xv = ctx.vec_alloc(n)
        it, _ = ctx.pcg_solve(op, bv, xv, rtol=1e-10)
        out.append((it, ctx.vec_download(xv)))
        ctx.vec_free(xv)
    assert out[0][0] == out[1][0] and np.array_equal(out[0][1], out[1][1])
    ctx.mesh_free(h)


@pytest.mark.parametrize("n", [2, 5, 33, 257, 1500, 4000])
def test_band_solve_nonsymmetric(ctx, n):
    """Time-dimension systems: c1 * (u' v) + c2 * (u v) with an initial condition row."""
    coords, cells = F.interval_mesh(n - 1, 0.0, 1.0)
    h = ctx.mesh_upload(coords, cells)
    C, M = F.assemble_atom(coords, cells, F.CONV), F.assemble_atom(coords, cells, F.MASS)
    ac, am = ctx.atom_assemble(h, F.CONV), ctx.atom_assemble(h, F.MASS)
    bc = np.array([0], dtype=np.int32)
    op = ctx.op_combine(h, [ac, am], [1.3, 0.4], bc)
    A_ref, _ = F.apply_dirichlet(1.3 * C + 0.4 * M, np.zeros(n), bc)
    b = np.random.default_rng(n).uniform(-1, 1, n)
    b[0] = 0.0
    bv, xv = ctx.vec_from(b), ctx.vec_alloc(n)
    ctx.band_solve(op, bv, xv)
    x = ctx.vec_download(xv)
    x_ref = F.direct_solve(A_ref, b)
    assert np.linalg.norm(x - x_ref) <= 1e-10 * np.linalg.norm(x_ref)
    ctx.mesh_free(h)


def test_error_paths(ctx):
    from pgdrome_amd._lib import PgdError
    with pytest.raises(PgdError):
        ctx.vec_download(999999)
    coords, cells = F.interval_mesh(4)
    bad = cells.copy()
    bad[0, 0] = 77
    with pytest.raises(PgdError):
        ctx.mesh_upload(coords, bad)
    # tetrahedra are validated on the device, before any kernel follows a vertex id
    c3, t3 = F.box_mesh((0, 0, 0), (1, 1, 1), 3, 2, 2)
    for wrong in (c3.shape[0], -1):
        bad3 = t3.copy()
        bad3[5, 2] = wrong
        with pytest.raises(PgdError, match="out of range"):
            ctx.mesh_upload(c3, bad3)
    ctx.mesh_free(ctx.mesh_upload(c3, t3))
    h = ctx.mesh_upload(coords, cells)
    v = ctx.vec_alloc(3)
    a = ctx.atom_assemble(h, F.MASS)
    with pytest.raises(PgdError):
        ctx.spmv(a, v, v)
    with pytest.raises(PgdError):
        ctx.atom_assemble(h, F.WMASS, 0, 0, 0)
    with pytest.raises(PgdError):
        ctx.atom_assemble(h, 42)
    ctx.mesh_free(h)


@pytest.mark.parametrize("npts", [40, 65, 104])
def test_multigrid_pcg_solves_the_same_system(ctx, npts):
    """PGD_TUNE_PCG_PRECOND = 1: the V-cycle of pgd_mg.hip as the preconditioner of pgd_pcg_solve where the scaled operator is one
    stencil on a lattice with an eliminated hull (even and odd node counts: the far faces with and without a coarse counterpart).
    Same system, same stop test: the solution agrees with the Jacobi form's to the tolerance of the solves, non-zero Dirichlet
    values are met exactly, the true residual through the CSR kernel is at the tolerance, in a number of iterations that does not
    grow with the lattice.  An operator whose eliminated nodes are not the hull falls back to Jacobi (counted)."""
    from pgdrome_amd import fem
    mesh = fem.BoxMesh(fem.Point(0, 0, 0), fem.Point(1, 1, 1), npts - 1, npts - 1, npts - 1)
    coords = mesh.coordinates()
    h = ctx.mesh_upload(coords, mesh.cells())
    n = coords.shape[0]
    ak, am = ctx.atom_assemble(h, F.STIFF), ctx.atom_assemble(h, F.MASS)
    bc = np.where(np.any((coords <= 1e-12) | (coords >= 1 - 1e-12), axis=1))[0].astype(np.int32)
    rng = np.random.default_rng(22)
    b = rng.uniform(-1, 1, n)
    b[bc] = rng.uniform(-1, 1, bc.size)
    bv = ctx.vec_from(b)
    out = {}
    try:
        for prec in (0, 1, 2):                                   # 2: the V-cycle with every level in the plain kernels of pgd_mg.hip
            ctx.tune(40, min(prec, 1))
            ctx.tune(42, 0 if prec == 2 else 64)
            op = ctx.op_combine(h, [ak, am], [1.0, 3.0], bc)
            xv = ctx.vec_from(rng.uniform(-1, 1, n))             # a start that violates the Dirichlet values
            it, rel = ctx.pcg_solve(op, bv, xv, 1e-10, 0.0, 10000)
            xs = ctx.vec_download(xv)
            out[prec] = (it, rel, xs)
            assert np.abs(xs[bc] - b[bc]).max() <= (0.0 if prec else 1e-9)
            yv = ctx.vec_alloc(n)
            ctx.flags_reset()
            ctx.tune(3, 0)
            ctx.spmv_dot_slot(op, xv, yv, xv, 0, n, 30)
            ctx.tune(3, 1)
            assert np.linalg.norm(b - ctx.vec_download(yv)) <= 1.05e-10 * np.linalg.norm(b)
            assert rel <= 1e-10
            for v in (yv, xv):
                ctx.vec_free(v)
            ctx.atom_free(op)
        assert out[1][0] <= 26 and out[0][0] > 3 * out[1][0], (out[0][0], out[1][0])
        assert np.linalg.norm(out[1][2] - out[0][2]) <= 2e-8 * np.linalg.norm(out[0][2])
        # the march kernel's epilogues against the plain passes: the same cycle up to the order of the sums
        assert abs(out[2][0] - out[1][0]) <= 1 and np.linalg.norm(out[2][2] - out[1][2]) <= 2e-8 * np.linalg.norm(out[1][2])
        st = ctx.mg_stats()
        assert st["solves"] >= 1
        # eliminated nodes on one face only: not the structure the hierarchy is built for -> Jacobi, and it says so
        face = np.where(coords[:, 2] <= 1e-12)[0].astype(np.int32)
        op = ctx.op_combine(h, [ak, am], [1.0, 3.0], face)
        xv = ctx.vec_alloc(n)
        b2 = b.copy(); b2[bc] = 0.0
        b2v = ctx.vec_from(b2)
        it2, rel2 = ctx.pcg_solve(op, b2v, xv, 1e-10, 0.0, 10000)
        assert rel2 <= 1e-10 and ctx.mg_stats()["fallbacks"] == st["fallbacks"] + 1
        for v in (xv, b2v):
            ctx.vec_free(v)
        ctx.atom_free(op)
    finally:
        ctx.tune(40, 0)
        ctx.tune(42, 64)
        ctx.tune(3, 1)
    ctx.vec_free(bv)
    for a in (ak, am):
        ctx.atom_free(a)
    ctx.mesh_free(h)


@pytest.mark.parametrize("npts", [32, 41])
def test_multigrid_pcg_walks_like_its_cpu_restatement(ctx, npts):
    """The HIP path against oracle/mg_numpy.py (the same hierarchy, cycle and stop test in numpy): the same system from a zero
    start takes the same number of iterations (+-1: the sums are grouped differently) and ends at the same solution."""
    from oracle import mg_numpy as MG
    from pgdrome_amd import fem
    mesh = fem.BoxMesh(fem.Point(0, 0, 0), fem.Point(1, 1, 1), npts - 1, npts - 1, npts - 1)
    coords = mesh.coordinates()
    h = ctx.mesh_upload(coords, mesh.cells())
    n = coords.shape[0]
    ak, am = ctx.atom_assemble(h, F.STIFF), ctx.atom_assemble(h, F.MASS)
    bc = np.where(np.any((coords <= 1e-12) | (coords >= 1 - 1e-12), axis=1))[0].astype(np.int32)
    rng = np.random.default_rng(23)
    b = rng.uniform(-1, 1, n)
    bv = ctx.vec_from(b)
    # the stencil of the unscaled operator from the atoms' rows of a node in the middle
    Ko, Mo = F.assemble_atom(coords, mesh.cells(), F.STIFF).tocsr(), F.assemble_atom(coords, mesh.cells(), F.MASS).tocsr()
    mid = (npts // 2) * npts * npts + (npts // 2) * npts + npts // 2
    c = np.array([Ko[mid, mid + dx + npts * dy + npts * npts * dz] + 3.0 * Mo[mid, mid + dx + npts * dy + npts * npts * dz]
                  for dx, dy, dz in MG.OFFS])
    try:
        ctx.tune(40, 1)
        op = ctx.op_combine(h, [ak, am], [1.0, 3.0], bc)
        xv = ctx.vec_alloc(n)
        s0 = ctx.mg_stats()
        it, rel = ctx.pcg_solve(op, bv, xv, 1e-10, 0.0, 1000)
        assert ctx.mg_stats()["solves"] == s0["solves"] + 1
        xs = ctx.vec_download(xv)
        ctx.vec_free(xv)
        ctx.atom_free(op)
    finally:
        ctx.tune(40, 0)
    shape = (npts, npts, npts)
    xo, ito, relo = MG.pcg(shape, c, b.reshape(shape))
    assert abs(it - ito) <= 1, (it, ito)
    assert np.linalg.norm(xs - xo.ravel()) <= 1e-8 * np.linalg.norm(xo)
    ctx.vec_free(bv)
    for a in (ak, am):
        ctx.atom_free(a)
    ctx.mesh_free(h)
