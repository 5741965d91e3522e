"""Cell-subdomain atoms (pgd_atom_assemble_cells) and dx(id) forms on the MI355X, against the exact rational reference
restricted to the marked cells (tests/subdomain_reference.py).

Atoms: |got_ij - exact_ij| <= 1e-14 max_j S_ij per row, S summed over the MARKED cells (the bound of tests/test_exact_gpu.py);
every cell marked: bit-identical to pgd_atom_assemble; none: all zeros.  Run with -s for the largest error per family."""
import ctypes as ct
from fractions import Fraction

import numpy as np
import pytest
import scipy.sparse as sps
import scipy.sparse.linalg as spla

from oracle import fem_numpy as FN
from pgdrome_amd import fem, problems
from pgdrome_amd._lib import PgdError
from tests import exact_reference as X
from tests import subdomain_reference as SR
from tests import test_subdomain_cpu as C
from tests import weighted_reference as W

pytestmark = pytest.mark.gpu
P = fem.Point
TOL = 1e-14
WORST = {}

MESHES = X.mesh_matrix()
LAYOUTS = {
    "p1_interval": ("p1_interval_nonuniform", None),
    "p1_tri_right": ("p1_tri_right", None),
    "p1_tri_crossed": ("p1_tri_crossed", None),
    "p1_tet_general": ("p1_tet_jitter", None),
    "p1_lattice_knob1": ("lattice_4x3x3", 1),
    "p1_lattice_knob2": ("lattice_4x3x3", 2),
    "p1_lattice_knob3": ("lattice_4x3x3", 3),
    "p2_interval": ("p2_interval_nonuniform", None),
    "p2_triangle": ("p2_tri_jitter", None),
    "p2_tetrahedron": ("p2_tet_jitter", None),
}
_EXACT = {}


def exact_layout(name):
    if name not in _EXACT:
        c, e = X.lattice_box(X.LATTICE_SHAPES[name]) if name in X.LATTICE_SHAPES else MESHES[name]()
        _EXACT[name] = W.WeightedExactLayout(c, e)
    return _EXACT[name]


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    print("\nlargest error / bound per family (masked atoms):")
    for k in sorted(WORST):
        print("  %-28s %.4f" % (k, WORST[k]))


def excess(lay, got, vals, S, S_full):
    """Largest |got_ij - exact_ij| / (TOL max_j S_ij), S over the marked cells.  A row on which every marked contribution is
    exactly zero (a gradient component that vanishes in exact arithmetic: a cell's own rounding leaves ~1e-19 there, as it does
    in the unmasked atom) takes the scale of the row on the whole mesh instead of a bound of 0."""
    err = X.exact_errors(got, vals)
    rm = lay.row_max(S)
    bound = TOL * np.where(rm > 0, rm, lay.row_max(S_full))
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    return float(q.max()) if q.size else 0.0


def _family(lay, knob):
    if lay.degree == 2:
        return "assemble_p2_interval" if lay.D == 1 else "assemble_p2_simplex<%d>" % lay.D
    return "assemble_p1<%d>" % lay.D + ("" if knob is None else " lattice knob %d" % knob)


@pytest.mark.parametrize("case", sorted(LAYOUTS))
def test_masked_atoms_are_exact(ctx, case):
    name, knob = LAYOUTS[case]
    lay = exact_layout(name)
    h = ctx.mesh_upload(lay.coords, lay.cells.astype(np.int32))
    w = X.weight_of(lay.coords)
    wv = ctx.vec_from(w)
    fam = _family(lay, knob)
    try:
        if knob is not None:
            assert ctx.mesh_lattice(h)[0]
            ctx.tune(20, knob)
        nc = lay.cells.shape[0]
        for kind, a, b in X.kinds_and_pairs(lay.D) + W.kinds_and_pairs(lay.D):
            weighted = kind >= X.WMASS
            full = ctx.atom_assemble(h, kind, a, b, wv if weighted else 0)
            ref_full = ctx.atom_download(full, lay.nnz)
            ctx.atom_free(full)
            for mname, mask in SR.masks(nc, seed=kind * 16 + 4 * a + b).items():
                at = ctx.atom_assemble_cells(h, kind, a, b, wv if weighted else 0, mask)
                got = ctx.atom_download(at, lay.nnz)
                ctx.atom_free(at)
                if mname == "all":
                    assert np.array_equal(got.view(np.int64), ref_full.view(np.int64)), (fam, kind, a, b)
                if mname == "none":
                    assert not got.any(), (fam, kind, a, b)
                vals, S = SR.subset_atom(lay, kind, a, b, w if weighted else None, mask)
                q = excess(lay, got, vals, S, SR.subset_atom(lay, kind, a, b, w if weighted else None)[1])
                WORST[fam] = max(WORST.get(fam, 0.0), q)
                assert q <= 1.0, (fam, mname, kind, a, b, q)
                assert not got[~SR.touched(lay, mask)].any(), (fam, mname, kind, a, b)      # exact zeros off the subset
    finally:
        ctx.tune(20, 1)
        ctx.vec_free(wv)
        ctx.mesh_free(h)


def test_invalid_masks_leave_no_atom(ctx):
    lay = exact_layout("p1_tri_crossed")
    h = ctx.mesh_upload(lay.coords, lay.cells.astype(np.int32))
    nc = lay.cells.shape[0]
    blk = ctx.mesh_blocked(h, 2)
    try:
        a0 = ctx.atom_assemble(h, X.MASS)
        ctx.atom_free(a0)
        for call in (lambda: ctx.atom_assemble_cells(h, X.MASS, 0, 0, 0, np.ones(nc - 1, np.uint8)),
                     lambda: ctx.atom_assemble_cells(h, X.MASS, 0, 0, 0, np.ones(nc + 1, np.uint8)),
                     lambda: ctx.atom_assemble_cells(blk, X.MASS, 0, 0, 0, np.ones(nc, np.uint8)),
                     lambda: ctx.atom_assemble_cells(h, 42, 0, 0, 0, np.ones(nc, np.uint8)),
                     lambda: ctx.atom_assemble_cells(h, X.WMASS, 0, 0, 0, np.ones(nc, np.uint8)),
                     lambda: ctx.atom_assemble_cells(h, X.DUDV, 2, 0, 0, np.ones(nc, np.uint8))):
            with pytest.raises(PgdError):
                call()
        out = ct.c_int64(0)                                  # no mask with nc > 0
        assert ctx.lib.pgd_atom_assemble_cells(ctx.h, h, X.MASS, 0, 0, 0, None, nc, ct.byref(out)) == -1 and out.value == 0
        # no atom behind: the next atom takes the handle the first one had
        a1 = ctx.atom_assemble(h, X.MASS)
        assert a1 == a0
        ctx.atom_free(a1)
    finally:
        ctx.mesh_free(blk)
        ctx.mesh_free(h)


# ------------------------------------------------------------------------------------------ frontend on the device
@pytest.fixture(scope="module")
def hip_backend():
    from pgdrome_amd.hip_backend import HipBackend
    old = fem._backend
    be = fem.set_backend(HipBackend(0))
    fem.clear_caches()
    yield be
    fem.set_backend(old)
    fem.clear_caches()


def _exact_dot(p, vals, lay, q):
    y = lay.matvec(vals, q)
    return sum((Fraction(float(a)) * b for a, b in zip(p, y)), Fraction(0))


@pytest.mark.parametrize("mk", [lambda: fem.RectangleMesh(P(0, 0), P(1, 1), 5, 4, "crossed"),
                                lambda: fem.BoxMesh(P(0, 0, 0), P(1, 1, 1), 3, 2, 3)])
def test_frontend_is_exact_on_the_device(hip_backend, mk):
    m = mk()
    cf = C._two_materials(m)
    dxs = fem.Measure("dx", domain=m, subdomain_data=cf)
    V = fem.FunctionSpace(m, "CG", 1)
    F = fem.interpolate(fem.Expression("1.0 + x[0]*x[0]/4", degree=2), V)
    G = fem.interpolate(fem.Expression("2.0 - x[0]/8", degree=1), V)
    u, v = fem.TrialFunction(V), fem.TestFunction(V)
    lay = W.WeightedExactLayout(m.coordinates(), m.cells())
    p = fem.vertex_to_dof_map(V)
    f, g = F.compute_vertex_values(), G.compute_vertex_values()
    for sid in (1, 2):
        mask = (cf.array() == sid).view(np.uint8)
        for form, kind, a, b in [(lambda d: F * G * d, X.MASS, 0, 0),
                                 (lambda d: fem.inner(fem.grad(F), fem.grad(G)) * d, X.STIFF, 0, 0),
                                 (lambda d: F.dx(0) * G * d, X.CONV, 0, 0)]:
            vals, S = SR.subset_atom(lay, kind, a, b, None, mask)
            ex = _exact_dot(g if kind == X.CONV else f, vals, lay, f if kind == X.CONV else g)
            got = fem.assemble(form(dxs(sid)))
            scale = float(np.abs(f) @ (sps.csr_matrix((S, lay.cols, lay.rp), shape=(lay.n, lay.n)) @ np.abs(g)))
            assert abs(Fraction(got) - ex) <= 1e-13 * scale, (sid, kind)
        # load vector and matrix
        vals, S = SR.subset_atom(lay, X.MASS, 0, 0, None, mask)
        b_ex = np.array([float(t) for t in lay.matvec(vals, g)])
        b = fem.assemble(G * v * dxs(sid)).get_local()[p]
        assert np.all(np.abs(b - b_ex) <= 1e-13 * (sps.csr_matrix((S, lay.cols, lay.rp), shape=(lay.n, lay.n)) @ np.abs(g))
                      + 1e-300)
        vals, S = SR.subset_atom(lay, X.STIFF, 0, 0, None, mask)
        A = fem.assemble(3.0 * fem.inner(fem.grad(u), fem.grad(v)) * dxs(sid)).array()
        Ad = np.array([[float(t) for t in r] for r in lay.dense(vals)]) * 3.0
        Sd = lay.dense(S.astype(object))
        bound = 3e-14 * np.array([[float(t) for t in r] for r in Sd]).max(axis=1, keepdims=True)
        assert np.all(np.abs(A - Ad) <= bound + 1e-300)


@pytest.mark.parametrize("mk", [lambda: fem.RectangleMesh(P(0, 0), P(1, 1), 5, 4, "crossed"),
                                lambda: fem.BoxMesh(P(0, 0, 0), P(1, 1, 1), 3, 2, 3)])
def test_two_material_elasticity(hip_backend, mk):
    """E_1 inner(C eps(u), eps(v)) dx(1) + E_2 ... dx(2) on the device against the oracle's masked atoms."""
    m = mk()
    D = m.geometry().dim()
    cf = C._two_materials(m)
    dxs = fem.Measure("dx", domain=m, subdomain_data=cf)
    V = fem.VectorFunctionSpace(m, "CG", 1)
    u, v = fem.TrialFunction(V), fem.TestFunction(V)
    if D == 3:
        energy = fem.inner(problems._voigt_C(0.3) * problems._strain(u), problems._strain(v))
    else:
        lam, mu = 0.6, 0.4
        energy = (2 * mu * (u[0].dx(0) * v[0].dx(0) + u[1].dx(1) * v[1].dx(1))
                  + mu * (u[0].dx(1) + u[1].dx(0)) * (v[0].dx(1) + v[1].dx(0))
                  + lam * (u[0].dx(0) + u[1].dx(1)) * (v[0].dx(0) + v[1].dx(1)))
    A = fem.assemble(1.0 * energy * dxs(1) + 20.0 * energy * dxs(2))
    assert A.is_symmetric()
    got = A.array()
    old = fem._backend
    fem.set_backend(SR.CellNumpyBackend())
    try:
        ref = fem.assemble(1.0 * energy * dxs(1) + 20.0 * energy * dxs(2)).array()
    finally:
        fem.set_backend(old)
    assert np.abs(got - ref).max() <= 1e-13 * np.abs(ref).max()


def test_two_material_box_operator(ctx):
    """K_1 + 100 K_2 + M with Dirichlet rows on a box: the device product against the CSR product of the oracle's masked
    atoms, and a PCG solve against spsolve."""
    c, e = FN.box_mesh((0, 0, 0), (1, 1, 1), 10, 10, 10)
    mid = c[e].mean(axis=1)
    ball = ((mid - 0.5) ** 2).sum(axis=1) < 0.3 ** 2
    m1, m2 = (~ball).astype(np.uint8), ball.astype(np.uint8)
    h = ctx.mesh_upload(c, e)
    K1, K2 = ctx.atom_assemble_cells(h, FN.STIFF, 0, 0, 0, m1), ctx.atom_assemble_cells(h, FN.STIFF, 0, 0, 0, m2)
    M = ctx.atom_assemble(h, FN.MASS)
    bc = np.where(np.any((c <= 1e-12) | (c >= 1 - 1e-12), axis=1))[0].astype(np.int32)
    op = ctx.op_combine(h, [K1, K2, M], [1.0, 100.0, 0.5], bc)
    A = (FN.assemble_atom(c, e[~ball], FN.STIFF) + 100.0 * FN.assemble_atom(c, e[ball], FN.STIFF)
         + 0.5 * FN.assemble_atom(c, e, FN.MASS)).tocsr()
    A, _ = FN.apply_dirichlet(A, np.zeros(c.shape[0]), bc)
    x = np.random.default_rng(5).uniform(-1, 1, c.shape[0])
    xv, yv = ctx.vec_from(x), ctx.vec_alloc(c.shape[0])
    ctx.spmv(op, xv, yv)
    y = ctx.vec_download(yv)
    assert np.all(np.abs(y - A @ x) <= 1e-13 * (abs(A) @ np.abs(x)) + 1e-300)
    print("two-material box operator: product form %d" % ctx.atom_product_form(op))
    b = A @ np.ones(c.shape[0])
    bv, sv = ctx.vec_from(b), ctx.vec_alloc(c.shape[0])
    it, rel = ctx.pcg_solve(op, bv, sv, 1e-12, 0.0, 20000)
    ref = spla.spsolve(A.tocsc(), b)
    assert np.linalg.norm(ctx.vec_download(sv) - ref) <= 1e-8 * np.linalg.norm(ref), (it, rel)
    for a in (op, K1, K2, M):
        ctx.atom_free(a)
    for vv in (xv, yv, bv, sv):
        ctx.vec_free(vv)
    ctx.mesh_free(h)


@pytest.mark.parametrize("mk", [lambda: fem.RectangleMesh(P(0, 0), P(1, 1), 16, 16, "crossed"),
                                lambda: fem.BoxMesh(P(0, 0, 0), P(1, 1, 1), 7, 7, 7)])
def test_inclusion_heat_against_direct_solves(hip_backend, mk):
    from pgdrome_amd.solver import PGDProblem
    spec = problems.inclusion_heat(mk(), n_k=9, k_range=(0.1, 10.0), PGD_nmax=15, PGD_tol=1e-9)
    p = PGDProblem(**spec)
    p.solve_PGD(_problem="linear")
    C.check_inclusion_heat(spec, p, [0, 2, 4, 6, 8])
