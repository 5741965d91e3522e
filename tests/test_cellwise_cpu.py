"""Cell-wise constant (DG0) coefficients on a CPU: the DG0 space and its refusals, the grammar on CellwiseNumpyBackend (the numpy
oracle plus cell-weighted atoms, tests/cellwise_reference.py) - which atom every form shape asks for, and its value against the
exact rational reference -, the atom cache, the functional paths and cellwise_heat against direct solves and inclusion_heat."""
from fractions import Fraction

import numpy as np
import pytest
import scipy.sparse as sps
import scipy.sparse.linalg as spla

from oracle import fem_numpy as FN
from oracle.backend_numpy import NumpyBackend
from pgdrome_amd import fem, problems
from tests import cellwise_reference as CR
from tests import exact_reference as X
from tests import subdomain_reference as SR
from tests import test_subdomain_cpu as SC
from tests import weighted_reference as W

P = fem.Point


@pytest.fixture(autouse=True)
def cw_backend():
    old = fem._backend
    be = fem.set_backend(CR.CellwiseNumpyBackend())
    fem.clear_caches()
    yield be
    fem.set_backend(old)
    fem.clear_caches()


def _square():
    return fem.RectangleMesh(P(0, 0), P(1, 1), 5, 4, "crossed")


def _box():
    return fem.BoxMesh(P(0, 0, 0), P(1, 1, 1), 3, 2, 3)


def _field(mesh, values=None):
    k = fem.Function(fem.FunctionSpace(mesh, "DG", 0))
    k.vector()[:] = CR.dyadic_field(mesh.num_cells()) if values is None else values
    return k


# ------------------------------------------------------------------------------------------------- the DG0 space
@pytest.mark.parametrize("mk", [lambda: fem.IntervalMesh(7, 0.0, 2.0), _square, _box])
def test_dg0_space_surface(mk):
    m = mk()
    for family in ("DG", "Discontinuous Lagrange"):
        V0 = fem.FunctionSpace(m, family, 0)
        assert V0.dim() == m.num_cells() and V0.mesh() is m
        assert V0.ufl_element().degree() == 0 and V0.ufl_element().family() == "Discontinuous Lagrange"
    mid = m.coordinates()[m.cells()].mean(axis=1)
    assert np.array_equal(V0.tabulate_dof_coordinates(), mid)              # dof i = cell i, on intervals too
    assert np.array_equal(V0.dofmap().dofs(), np.arange(m.num_cells()))
    # the dolfin idiom: one value per marker
    markers = fem.MeshFunction("size_t", m, m.topology().dim(), 0)
    markers.array()[::3] = 1
    markers.array()[1::3] = 2
    k_values = [1.0, 10.0, 0.25]
    kappa = fem.Function(V0)
    v0 = kappa.vector().version
    kappa.vector()[:] = np.choose(np.asarray(markers.array(), dtype=np.int32), k_values)
    assert kappa.vector().version > v0
    assert np.array_equal(kappa.vector().get_local(), np.array(k_values)[markers.array()])
    assert np.array_equal(kappa.vector()[:], kappa.vector().get_local()) and len(kappa.vector()) == m.num_cells()
    # set_local / assign / copy
    other = fem.Function(V0)
    v1 = other.vector().version
    other.vector().set_local(np.arange(m.num_cells(), dtype=float))
    assert other.vector().version > v1 and other.vector()[2] == 2.0
    v2 = kappa.vector().version
    kappa.assign(other)
    assert kappa.vector().version > v2 and np.array_equal(kappa.vector().get_local(), np.arange(m.num_cells()))
    dup = kappa.copy(deepcopy=True)
    assert dup is not kappa and dup.function_space() is V0
    dup.vector()[0] = -5.0
    assert kappa.vector()[0] == 0.0 and dup.vector()[0] == -5.0
    # interpolation: the value at the cell midpoint
    e = fem.Expression("1.0 + 2.0*x[0]*x[0]", degree=2)
    f = fem.interpolate(e, V0)
    assert np.array_equal(f.vector().get_local(), 1.0 + 2.0 * mid[:, 0] ** 2)
    assert np.array_equal(fem.interpolate(fem.Constant(3.0), V0).vector().get_local(), np.full(m.num_cells(), 3.0))
    g = fem.Function(V0)
    g.interpolate(e)
    assert np.array_equal(g.vector().get_local(), f.vector().get_local())


def test_dg_refusals():
    m = _square()
    V0 = fem.FunctionSpace(m, "DG", 0)
    V = fem.FunctionSpace(m, "CG", 1)
    kappa = _field(m)
    for call in (lambda: fem.FunctionSpace(m, "DG", 1), lambda: fem.FunctionSpace(m, "Discontinuous Lagrange", 2),
                 lambda: fem.VectorFunctionSpace(m, "DG", 0), lambda: fem.TrialFunction(V0), lambda: fem.TestFunction(V0),
                 lambda: fem.DirichletBC(V0, 0.0, lambda x, on: on), lambda: fem.project(fem.Constant(1.0), V0),
                 lambda: fem.project(fem.interpolate(fem.Constant(1.0), V), V0), lambda: kappa.compute_vertex_values()):
        with pytest.raises(NotImplementedError):
            call()
    # ... and what a nodal Function offers beyond being a coefficient says that a DG0 one does not, by name
    F = fem.interpolate(fem.Expression("1.0 + x[0]", degree=1), V)
    for call in (lambda: fem.norm(kappa), lambda: fem.norm(kappa, "H1"), lambda: fem.errornorm(kappa, F),
                 lambda: fem.errornorm(F, kappa), lambda: kappa(0.5, 0.5), lambda: kappa((0.5, 0.5)),
                 lambda: fem.interpolate(kappa, V), lambda: fem.point_gradient(kappa, np.array([0.5, 0.5])),
                 lambda: fem.grad(kappa), lambda: kappa.dx(0), lambda: fem.inner(fem.grad(kappa), fem.grad(F))):
        with pytest.raises(NotImplementedError, match="DG0"):
            call()


def test_integrand_refusals():
    m, other = _square(), _square()
    V = fem.FunctionSpace(m, "CG", 1)
    u, v = fem.TrialFunction(V), fem.TestFunction(V)
    F = fem.interpolate(fem.Expression("1.0 + x[0]", degree=1), V)
    kappa, kappa2 = _field(m), _field(m)
    with pytest.raises(NotImplementedError):                               # two DG0 factors
        fem.assemble(kappa * kappa2 * u * v * fem.dx).array()
    with pytest.raises(NotImplementedError):
        fem.assemble(kappa * kappa * F * fem.dx(m))
    with pytest.raises(NotImplementedError):                               # a differentiated DG0 factor
        fem.assemble(kappa.dx(0) * v * fem.dx)
    with pytest.raises(NotImplementedError):
        fem.assemble(fem.inner(fem.grad(kappa), fem.grad(v)) * fem.dx)
    with pytest.raises(NotImplementedError):                               # DG0 on ds
        fem.assemble(kappa * u * v * fem.ds).array()
    with pytest.raises(NotImplementedError):
        fem.assemble(kappa * v * fem.ds)
    with pytest.raises(NotImplementedError):
        fem.assemble(kappa * F * fem.ds(m))
    with pytest.raises(ValueError):                                        # a field of another mesh
        fem.assemble(_field(other) * u * v * fem.dx).array()
    with pytest.raises(ValueError):
        fem.assemble(_field(other) * F * F * fem.dx(m))


def test_backend_without_atom_cellwise_refuses():
    fem.set_backend(NumpyBackend())
    m = _square()
    V = fem.FunctionSpace(m, "CG", 1)
    u, v = fem.TrialFunction(V), fem.TestFunction(V)
    F = fem.interpolate(fem.Expression("1.0", degree=1), V)
    kappa = _field(m)
    with pytest.raises(NotImplementedError, match="atom_cellwise"):
        fem.assemble(kappa * F * F * fem.dx(m))
    with pytest.raises(NotImplementedError, match="atom_cellwise"):
        fem.assemble(kappa * u * v * fem.dx).array()


def test_sharded_layout_refuses():
    c, e = FN.box_mesh((0, 0, 0), (1, 1, 1), 2, 2, 3)
    n = c.shape[0]
    mesh = fem.Mesh(c, e, part=fem.Partition(None, 0, n, n, 0, 0, 0))
    with pytest.raises(NotImplementedError, match="sharded"):
        fem.FunctionSpace(mesh, "DG", 0)
    plain = fem.Mesh(c, e)
    kv = _field(plain).vector()
    with pytest.raises(NotImplementedError, match="sharded"):
        mesh.layout(1).atom(FN.MASS, cw=kv)
    with pytest.raises(NotImplementedError, match="sharded"):
        fem._block_layout(mesh, 1, 3).atom(FN.MASS, cw=kv, cv=0, cu=0)


# ------------------------------------------------------------------------------- which atom every form shape asks for
def _two_materials(mesh):
    return SC._two_materials(mesh)


def _shapes(m, V, kappa, E, d):
    """(name, rank, form, (kind, da, db), nodal weight?) for every shape of the grammar, over the measure d."""
    ax = m.geometry().dim() - 1
    u, v = fem.TrialFunction(V), fem.TestFunction(V)
    F = fem.interpolate(fem.Expression("1.0 + x[0]*x[0]/4", degree=2), V)
    G = fem.interpolate(fem.Expression("2.0 - x[0]/8", degree=1), V)
    gd = fem.inner(fem.grad(u), fem.grad(v))
    one_d = m.geometry().dim() == 1
    dudv = (FN.STIFF, 0, 0) if one_d else (FN.DUDV, 0, ax)
    wdudv = (X.WSTIFF, 0, 0) if one_d else (W.WDUDV, 0, ax)
    return F, G, [
        # matrices: the five bilinear shapes, without and with the one nodal weight
        ("mass", 2, kappa * u * v * d, (FN.MASS, 0, 0), False),
        ("stiff", 2, kappa * gd * d, (FN.STIFF, 0, 0), False),
        ("dudv", 2, kappa * u.dx(0) * v.dx(ax) * d, dudv, False),
        ("conv", 2, kappa * u.dx(ax) * v * d, (FN.CONV, ax, 0), False),
        ("convt", 2, u * kappa * v.dx(ax) * d, (FN.CONVT, 0, ax), False),
        ("wmass", 2, kappa * E * u * v * d, (FN.WMASS, 0, 0), True),
        ("wstiff", 2, kappa * E * gd * d, (X.WSTIFF, 0, 0), True),
        ("wdudv", 2, E * kappa * u.dx(0) * v.dx(ax) * d, wdudv, True),
        ("wconv", 2, E * u.dx(ax) * v * kappa * d, (W.WCONV, ax, 0), True),
        ("wconvt", 2, kappa * E * u * v.dx(ax) * d, (W.WCONVT, 0, ax), True),
        # load vectors
        ("load", 1, kappa * v * d, (FN.MASS, 0, 0), False),
        ("load_f", 1, kappa * G * v * d, (FN.MASS, 0, 0), False),
        ("load_grad", 1, kappa * fem.inner(fem.grad(F), fem.grad(v)) * d, (FN.STIFF, 0, 0), False),
        ("load_dx", 1, kappa * F.dx(ax) * v * d, (FN.CONV, ax, 0), False),
        ("load_w", 1, kappa * E * G * v * d, (FN.WMASS, 0, 0), True),
        # functionals
        ("area", 0, kappa * fem.Constant(2.0) * d, (FN.MASS, 0, 0), False),
        ("fg", 0, kappa * F * G * d, (FN.MASS, 0, 0), False),
        ("grad", 0, kappa * fem.inner(fem.grad(F), fem.grad(G)) * d, (FN.STIFF, 0, 0), False),
        ("dx", 0, F.dx(ax) * kappa * G * d, (FN.CONVT, 0, ax), False),        # (the differentiated factor stands on the test side)
        ("wgrad", 0, kappa * E * fem.inner(fem.grad(F), fem.grad(G)) * d, (X.WSTIFF, 0, 0), True),
    ]


def _run(form, rank):
    out = fem.assemble(form)
    if rank == 2:
        return out.array()
    return out.get_local() if rank == 1 else out


@pytest.mark.parametrize("mk", [lambda: fem.IntervalMesh(9, 0.0, 1.0), _square, _box])
@pytest.mark.parametrize("subdomain", [False, True])
def test_form_mapping_and_exactness(cw_backend, mk, subdomain):
    """Every shape asks the backend for ONE cell-weighted atom of the expected kind, axes, nodal weight, field and cell set, and
    the assembled result agrees with the exact reference sum_c kappa_c K_c.  (Kinds 7-9 - WDUDV, WCONV, WCONVT - are answered by
    CellwiseNumpyBackend FROM that reference: for them this checks the mapping and the frontend's arithmetic around the atom, not
    the atom's values.  Those are checked independently on the device, tests/test_cellwise_gpu.py.)"""
    m = mk()
    V = fem.FunctionSpace(m, "CG", 1)
    kappa = _field(m)
    kv = kappa.vector().get_local()
    E = fem.interpolate(fem.Expression("1.0 + x[0]/2", degree=1), V)
    cf = _two_materials(m)
    d = fem.Measure("dx", domain=m, subdomain_data=cf)(2) if subdomain else fem.dx(m)
    mask = (cf.array() == 2).view(np.uint8) if subdomain else None
    F, G, shapes = _shapes(m, V, kappa, E, d)
    lay = W.WeightedExactLayout(m.coordinates(), m.cells())
    p = fem.vertex_to_dof_map(V)
    f, g, e = F.compute_vertex_values(), G.compute_vertex_values(), E.compute_vertex_values()
    one = np.ones(lay.n)
    for name, rank, form, (kind, da, db), weighted in shapes:
        kappa.vector()[:] = kv                                              # a new version: the atom is assembled afresh
        n0 = len(cw_backend.cellwise_atoms)
        got = _run(form, rank)
        new = cw_backend.cellwise_atoms[n0:]
        assert len(new) == 1, name
        k_, da_, db_, w_, c_, m_ = new[0]
        assert (k_, da_, db_) == (kind, da, db), name
        wn = e
        if name == "load_w" and w_ == g.tobytes():                          # (E * G * v: either nodal factor may be the weight)
            wn, g_w = g, e
        else:
            g_w = g
        assert (w_ == wn.tobytes()) if weighted else (w_ is None), name
        assert c_ == kv.tobytes(), name
        assert m_ == (mask.tobytes() if subdomain else None), name
        # the value
        vals, S = CR.cellwise_atom(lay, kind, da, db, wn if weighted else None, kv, mask)
        Sm = sps.csr_matrix((S, lay.cols, lay.rp), shape=(lay.n, lay.n))
        if rank == 2:
            Ad = np.array([[float(t) for t in r] for r in lay.dense(vals)])
            Sd = np.array([[float(t) for t in r] for r in lay.dense(S.astype(object))])
            assert np.all(np.abs(got[np.ix_(np.argsort(p), np.argsort(p))] - Ad) <= 1e-14 * Sd.max(axis=1, keepdims=True) + 1e-300), name
        elif rank == 1:
            x = {"load": one, "load_f": g, "load_grad": f, "load_dx": f, "load_w": g_w}[name]
            ex = np.array([float(t) for t in lay.matvec(vals, x)])
            assert np.all(np.abs(got[p] - ex) <= 1e-13 * (Sm @ np.abs(x)) + 1e-300), name
        else:
            l, r = {"area": (one, one), "fg": (f, g), "grad": (f, g), "dx": (f, g), "wgrad": (f, g)}[name]
            scale = {"area": 2.0}.get(name, 1.0)
            ex = scale * sum((Fraction(float(a)) * b for a, b in zip(l, lay.matvec(vals, r))), Fraction(0))
            assert abs(Fraction(got) - ex) <= 1e-13 * scale * float(np.abs(l) @ (Sm @ np.abs(r))), name


def test_backend_atoms_against_the_exact_reference(cw_backend):
    """CellwiseNumpyBackend itself (both of its routes) against the exact sums, with the bound of the subdomain atoms.  Only the
    oracle route (kinds 1-6 of a field with few levels) is an independent computation; the other route IS the exact sum rounded
    once, so for kinds 7-9 and many-valued fields this pins the plumbing (mask, weight, pattern order), not the values."""
    m = fem.RectangleMesh(P(0, 0), P(1, 1), 3, 2, "crossed")
    lay = W.WeightedExactLayout(m.coordinates(), m.cells())
    mh = cw_backend.mesh(m.coordinates(), m.cells())
    rp, cols = cw_backend.mesh_pattern(mh)
    nc = m.num_cells()
    w = X.weight_of(lay.coords)
    wv = cw_backend.vec_zeros(lay.n)
    cw_backend.vec_upload(wv, w)
    for kappa in (CR.dyadic_field(nc), CR.level_field(nc, 2), np.random.default_rng(3).uniform(0.5, 2.0, nc) * np.arange(1, nc + 1)):
        cv = cw_backend.vec_zeros(nc)
        cw_backend.vec_upload(cv, kappa)
        for mname, mask in list(SR.masks(nc, seed=3).items()) + [("unmasked", None)]:
            for kind, a, b in X.kinds_and_pairs(2) + W.kinds_and_pairs(2):
                weighted = kind >= X.WMASS
                vals, S = CR.cellwise_atom(lay, kind, a, b, w if weighted else None, kappa, mask)
                got = SR.on_pattern(cw_backend._obj[cw_backend.atom_cellwise(mh, kind, a, b, wv if weighted else 0, cv, mask)][1],
                                    rp, cols)
                ex = np.array([float(x) for x in vals])
                assert np.all(np.abs(got - ex) <= 1e-14 * lay.row_max(S) + 1e-300), (mname, kind, a, b)
    # kappa = 1: the unweighted exact atom; kappa = the indicator of a mask: the subset atom
    half = SR.masks(nc, seed=3)["half"]
    for kind, a, b in X.kinds_and_pairs(2) + W.kinds_and_pairs(2):
        wk = w if kind >= X.WMASS else None
        assert all(x == y for x, y in zip(CR.cellwise_atom(lay, kind, a, b, wk, np.ones(nc))[0], lay.atom(kind, a, b, wk)[0]))
        assert all(x == y for x, y in zip(CR.cellwise_atom(lay, kind, a, b, wk, half.astype(float))[0],
                                          SR.subset_atom(lay, kind, a, b, wk, half)[0]))


@pytest.mark.parametrize("mk", [_square, _box])
def test_vector_valued_spaces_embed_the_cell_weighted_atom(cw_backend, mk):
    m = mk()
    D = m.geometry().dim()
    kappa = _field(m, CR.level_field(m.num_cells(), 4))
    V = fem.VectorFunctionSpace(m, "CG", 1)
    Vs = fem.FunctionSpace(m, "CG", 1)
    u, v = fem.TrialFunction(V), fem.TestFunction(V)
    us, vs = fem.TrialFunction(Vs), fem.TestFunction(Vs)
    E = fem.interpolate(fem.Expression("1.0 + x[0]/2", degree=1), Vs)
    n0 = len(cw_backend.cellwise_atoms)
    A = fem.assemble(kappa * u[1].dx(0) * v[0].dx(D - 1) * fem.dx).array()
    assert [a[:3] for a in cw_backend.cellwise_atoms[n0:]] == [(FN.DUDV, 0, D - 1)]
    ref = fem.assemble(kappa * us.dx(0) * vs.dx(D - 1) * fem.dx).array()
    assert len(cw_backend.cellwise_atoms) == n0 + 1                      # the scalar atom is shared
    assert np.array_equal(A[0::D, 1::D], ref) and not A[1::D].any() and not A[0::D, 0::D].any()
    # components with a nodal weight, a load vector and a functional
    B = fem.assemble(kappa * E * u[0] * v[1] * fem.dx).array()
    assert np.array_equal(B[1::D, 0::D], fem.assemble(kappa * E * us * vs * fem.dx).array())
    b = fem.assemble(kappa * fem.Constant(2.0) * v[1] * fem.dx).get_local()
    assert np.array_equal(b[1::D], fem.assemble(kappa * fem.Constant(2.0) * vs * fem.dx).get_local()) and not b[0::D].any()
    U = fem.interpolate(fem.Expression(("x[0]", "1.0 + x[1]") if D == 2 else ("x[0]", "1.0 + x[1]", "x[2]"), degree=1), V)
    U1 = fem.interpolate(fem.Expression("1.0 + x[1]", degree=1), Vs)
    assert fem.assemble(kappa * U[1] * U[1] * fem.dx(m)) == pytest.approx(fem.assemble(kappa * U1 * U1 * fem.dx(m)), rel=1e-13)
    # with dx(id)
    cf = _two_materials(m)
    dxs = fem.Measure("dx", domain=m, subdomain_data=cf)
    whole = fem.assemble(kappa * fem.inner(u, v) * fem.dx(m)).array()
    parts = fem.assemble(kappa * fem.inner(u, v) * dxs(1) + kappa * fem.inner(u, v) * dxs(2)).array()
    assert np.abs(whole - parts).max() <= 1e-13 * np.abs(whole).max()


# ---------------------------------------------------------------------------------------------------------- cache
def test_atom_cache(cw_backend):
    import gc
    m = _box()
    V = fem.FunctionSpace(m, "CG", 1)
    u, v = fem.TrialFunction(V), fem.TestFunction(V)
    F = fem.interpolate(fem.Expression("1.0 + x[0]", degree=1), V)
    kappa = _field(m)
    lay = V._lay
    gd = fem.inner(fem.grad(u), fem.grad(v))
    freed = []
    real_free = cw_backend.atom_free
    cw_backend.atom_free = lambda a: (freed.append(a), real_free(a))[1]
    try:
        # the same field: the same atom, from a matrix, a load vector and a functional
        A = fem.assemble(kappa * gd * fem.dx)
        A.array()
        n1 = len(cw_backend.cellwise_atoms)
        A.array()
        fem.assemble(kappa * gd * fem.dx).array()
        fem.assemble(kappa * fem.inner(fem.grad(F), fem.grad(v)) * fem.dx)
        s0 = fem.assemble(kappa * fem.inner(fem.grad(F), fem.grad(F)) * fem.dx(m))
        assert len(cw_backend.cellwise_atoms) == n1 and len(lay._cw_atoms) == 1
        (a0,) = [e[0] for e in lay._cw_atoms.values()]
        # a changed value: a new atom, the old one freed
        kappa.vector()[0] = 100.0
        s1 = fem.assemble(kappa * fem.inner(fem.grad(F), fem.grad(F)) * fem.dx(m))
        assert s1 != s0 and len(cw_backend.cellwise_atoms) == n1 + 1 and len(lay._cw_atoms) == 1 and a0 in freed
        ref = F.vector().get_local() @ (CR.stiffness(m.coordinates(), m.cells(), kappa.vector().get_local()) @ F.vector().get_local())
        assert s1 == pytest.approx(ref, rel=1e-12)
        # a dead field: its atom is freed by the next request
        (a1,) = [e[0] for e in lay._cw_atoms.values()]
        other = _field(m, CR.level_field(m.num_cells(), 7))
        del kappa, A
        gc.collect()
        fem.assemble(other * F * F * fem.dx(m))
        assert a1 in freed and len(lay._cw_atoms) == 1
    finally:
        cw_backend.atom_free = real_free


def test_nine_elasticity_atoms_of_one_field_live_side_by_side(cw_backend):
    m = fem.BoxMesh(P(0, 0, 0), P(1, 1, 1), 2, 3, 2)
    kappa = _field(m, CR.level_field(m.num_cells(), 5))
    V = fem.VectorFunctionSpace(m, "CG", 1)
    u, v = fem.TrialFunction(V), fem.TestFunction(V)
    e = fem.inner(problems._voigt_C(0.3) * problems._strain(u), problems._strain(v))
    A = fem.assemble(kappa * e * fem.dx)
    assert A.is_symmetric()
    got = A.array()
    base = V._lay.base
    assert sorted(k[1:4] for k in base._cw_atoms) == sorted((FN.DUDV, a, b) for a in range(3) for b in range(3))
    n = len(cw_backend.cellwise_atoms)
    A.array()
    assert len(cw_backend.cellwise_atoms) == n == 9                      # none evicted another
    # against one dx(id) form per level
    cf = fem.MeshFunction("size_t", m, 3, 0)
    levels = np.unique(kappa.vector().get_local())
    cf.array()[:] = np.searchsorted(levels, kappa.vector().get_local())
    dxs = fem.Measure("dx", domain=m, subdomain_data=cf)
    ref = fem.assemble(sum((float(l) * e * dxs(i) for i, l in enumerate(levels)), 0)).array()
    assert np.abs(got - ref).max() <= 1e-13 * np.abs(ref).max()
    # a new version of the field frees all nine and their embeddings
    old = {a[0] for a in base._cw_atoms.values()}
    assert old <= {k[1] for k in V._lay._catoms}
    kappa.vector()[:] = 2.0 * kappa.vector().get_local()
    got2 = fem.assemble(kappa * e * fem.dx).array()
    new = {a[0] for a in base._cw_atoms.values()}
    assert len(new) == 9 and new <= {k[1] for k in V._lay._catoms}
    assert not (old - new) & {k[1] for k in V._lay._catoms}             # (handle numbers are reused)
    assert np.abs(got2 - 2.0 * got).max() <= 1e-13 * np.abs(got).max()


# ----------------------------------------------------------------------------------------------------- functionals
def test_functionals_take_the_general_path(cw_backend):
    m = _square()
    V = fem.FunctionSpace(m, "CG", 1)
    F = fem.interpolate(fem.Expression("1.0 + x[0]*x[0]/4", degree=2), V)
    G = fem.interpolate(fem.Expression("2.0 - x[0]/8", degree=1), V)
    kappa = _field(m)
    kv = kappa.vector().get_local()
    lay = W.WeightedExactLayout(m.coordinates(), m.cells())
    f, g = F.compute_vertex_values(), G.compute_vertex_values()
    for forms, kind in (((kappa * F * G, F * kappa * G, F * G * kappa, kappa * (F * G)), X.MASS),
                        ((kappa * fem.inner(fem.grad(F), fem.grad(G)), fem.inner(fem.grad(F), fem.grad(G)) * kappa), X.STIFF)):
        vals, S = CR.cellwise_atom(lay, kind, 0, 0, None, kv)
        ex = sum((Fraction(float(a)) * b for a, b in zip(f, lay.matvec(vals, g))), Fraction(0))
        scale = float(np.abs(f) @ (sps.csr_matrix((S, lay.cols, lay.rp), shape=(lay.n, lay.n)) @ np.abs(g)))
        for integrand in forms:
            assert not isinstance(integrand, fem._FastProd)
            form = integrand * fem.dx(m)
            assert type(form) is not fem._FastForm
            n0 = fem.STATS_FAST["requests"]
            got = fem.assemble(form)
            assert fem.STATS_FAST["requests"] == n0
            assert abs(Fraction(got) - ex) <= 1e-13 * scale
    # ... also inside a functional_scope, and never the unweighted value
    plain = fem.assemble(F * G * fem.dx(m))
    for _ in range(3):
        with fem.functional_scope(("cellwise-test", 0), [F.vector()]):
            got = fem.assemble(kappa * F * G * fem.dx(m))
        vals, S = CR.cellwise_atom(lay, X.MASS, 0, 0, None, kv)
        ex = sum((Fraction(float(a)) * b for a, b in zip(f, lay.matvec(vals, g))), Fraction(0))
        assert abs(Fraction(got) - ex) <= 1e-13 * float(np.abs(f) @ (sps.csr_matrix((S, lay.cols, lay.rp), shape=(lay.n, lay.n)) @ np.abs(g)))
        assert abs(got - plain) > 1e-3 * abs(plain)


# --------------------------------------------------------------------------------------------------- cellwise_heat
def ball_indicator(mesh):
    """The indicator (per cell) of inclusion_heat's ball."""
    mk = problems.inclusion_heat(mesh, n_k=3)["param"]["markers"].array()
    return (mk == problems.INCLUSION).astype(np.float64)


def direct_cellwise(spec):
    """The separated problem as ONE linear system over space x theta built from the oracle's atoms, solved directly: U[:, j] is
    the discrete solution at the theta node j that the PGD expansion converges to."""
    mesh, tmesh = spec["Vs"][0].mesh(), spec["Vs"][1].mesh()
    Xc, C = mesh.coordinates(), mesh.cells()
    tx, tc = tmesh.coordinates(), tmesh.cells()
    K0 = CR.stiffness(Xc, C, spec["param"]["kappa0"].vector().get_local())
    K1 = CR.stiffness(Xc, C, spec["param"]["kappa1"].vector().get_local())
    M = FN.assemble_atom(Xc, C, FN.MASS)
    Mt, Wt = FN.assemble_atom(tx, tc, FN.MASS), FN.assemble_atom(tx, tc, FN.WMASS, 0, 0, tx[:, 0].copy())
    nx, nt = Xc.shape[0], tx.shape[0]
    A = (sps.kron(K0, Mt) + sps.kron(K1, Wt)).tocsr()
    b = spec["param"]["f"] * np.kron(M @ np.ones(nx), Mt @ np.ones(nt))
    free = np.where(~np.repeat(mesh.vertex_on_boundary(), nt))[0]
    U = np.zeros(nx * nt)
    U[free] = spla.spsolve(A[free][:, free].tocsc(), b[free])
    return U.reshape(nx, nt)


def check_cellwise_heat(spec, p, js):
    sol = p.return_PGD()
    U = direct_cellwise(spec)
    tnodes = spec["Vs"][1].mesh().coordinates()[:, 0]
    errs = []
    for j in js:
        u = sol.evaluate(0, [1], [tnodes[j]], 0).compute_vertex_values()
        errs.append(float(np.linalg.norm(u - U[:, j]) / np.linalg.norm(U[:, j])))
    print("cellwise_heat: modes %d, relative L2 errors at theta = %s: %s" % (p.PGD_modes, list(tnodes[list(js)]), errs))
    assert max(errs) <= SC.INCLUSION_TOL
    return errs


def heat_spec(mesh, **kw):
    """kappa0 a seeded 8-level field (2^(l - 1), l = 0 ... 7), kappa1 the indicator of inclusion_heat's ball."""
    args = dict(n_t=9, t_range=(0.1, 10.0), PGD_nmax=15, PGD_tol=1e-9)
    args.update(kw)
    return problems.cellwise_heat(mesh, CR.level_field(mesh.num_cells(), 11), ball_indicator(mesh), **args)


@pytest.mark.parametrize("mk", [lambda: fem.RectangleMesh(P(0, 0), P(1, 1), 16, 16, "crossed"),
                                lambda: fem.BoxMesh(P(0, 0, 0), P(1, 1, 1), 7, 7, 7)])
def test_cellwise_heat_against_direct_solves(cw_backend, mk):
    from pgdrome_amd.solver import PGDProblem
    spec = heat_spec(mk())
    assert spec["param"]["kappa1"].vector().get_local().sum() > 0
    p = PGDProblem(**spec)
    p.solve_PGD(_problem="linear")
    check_cellwise_heat(spec, p, [0, 2, 4, 6, 8])


def check_reproduces_inclusion_heat(mesh):
    """kappa0 = 1 outside the ball and 0 inside, kappa1 the ball's indicator, the same ranges: inclusion_heat, at the project's
    PGD bars - the same pass counts, amplitudes to 1e-7, modes to 1e-6 relative L2."""
    from pgdrome_amd.solver import PGDProblem
    ref = PGDProblem(**problems.inclusion_heat(mesh, n_k=9, k_range=(0.1, 10.0), PGD_nmax=15, PGD_tol=1e-9))
    ref.solve_PGD(_problem="linear")
    ind = ball_indicator(mesh)
    p = PGDProblem(**problems.cellwise_heat(mesh, 1.0 - ind, ind, n_t=9, t_range=(0.1, 10.0), PGD_nmax=15, PGD_tol=1e-9))
    p.solve_PGD(_problem="linear")
    assert p.PGD_modes == ref.PGD_modes
    assert [int(v) for v in p.num_fp_it] == [int(v) for v in ref.num_fp_it]
    np.testing.assert_allclose(p.amplitude, ref.amplitude, rtol=1e-7)
    for d in range(2):
        for k in range(p.PGD_modes):
            a, b = p.PGD_func[d][k].compute_vertex_values(), ref.PGD_func[d][k].compute_vertex_values()
            assert np.linalg.norm(a - b) <= 1e-6 * np.linalg.norm(b), (d, k)
    return p


def test_cellwise_heat_reproduces_inclusion_heat(cw_backend):
    check_reproduces_inclusion_heat(fem.RectangleMesh(P(0, 0), P(1, 1), 12, 12, "crossed"))
