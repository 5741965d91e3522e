"""The row-class form of P2 operators on box lattices (pgdrome_amd/csrc/pgd_p2lat.hip, PGD_TUNE_SPMV_P2_LATTICE,
settings["p2_product"] = "lattice") checked without a GPU, on its numpy restatement tests/p2_lattice_reference.py and on the
patterns the frontend builds on the numpy oracle backend; tests/test_p2_lattice_gpu.py compares the HIP product with the CSR
product bit by bit."""
import functools

import numpy as np
import pytest
import scipy.sparse as sps

from tests import p2_lattice_reference as PL
from tests import pmg_reference as PM

SHAPES = [(3, 3, 3), (5, 4, 4), (4, 5, 6)]


@pytest.fixture(scope="module")
def oracle_backend():
    from oracle.backend_numpy import NumpyBackend
    from pgdrome_amd import fem
    old = fem._backend
    be = fem.set_backend(NumpyBackend())
    fem.clear_caches()
    yield be
    _pattern.cache_clear()
    if old is not None:
        fem.set_backend(old)
    else:
        fem._backend = None
    fem.clear_caches()


@functools.lru_cache(maxsize=None)
def _pattern(shape, ncomp):
    """(the frontend's pattern of a P2 space as a CSR matrix of ones, the lattice of its nodes, its edge list)."""
    from pgdrome_amd import fem
    Vh = PM.space(shape, ncomp)
    rp, cols = fem.get_backend().mesh_pattern(Vh._lay.handle())
    rp, cols = np.asarray(rp), np.asarray(cols)
    ev = np.asarray(PM.base_layout(Vh).edge_vertices)
    M = sps.csr_matrix((np.ones(cols.size), cols, rp), shape=(rp.size - 1, rp.size - 1))
    assert M.has_sorted_indices or np.all([np.all(np.diff(cols[rp[r]:rp[r + 1]]) > 0) for r in range(rp.size - 1)])
    return M, PL.Lattice(shape, ev), ev


def test_tables_from_the_six_tetrahedra():
    """The widths 65, 27, 27, 19, 27, 19, 19, 27 (230 in all); every table holds its own node; the vertex columns come first; the
    seven positive pattern vectors are the seven non-zero parities."""
    tabs = PL.tables()
    assert len(PL.tetrahedra()) == 6 and len({tuple(t) for t in PL.tetrahedra()}) == 6
    assert tuple(len(t) for t in tabs) == PL.WIDTHS and sum(PL.WIDTHS) == 230
    for g, t in enumerate(tabs):
        assert (0, 0, 0, g) in t and len(set(t)) == len(t)
        assert all(-1 <= c <= 1 for e in t for c in e[:3]) and all(0 <= e[3] <= 7 for e in t)
        nvc = sum(e[3] == 0 for e in t)
        assert all(e[3] == 0 for e in t[:nvc]) and all(e[3] != 0 for e in t[nvc:])
    assert sorted(e[3] for e in tabs[0] if e[:3] == (0, 0, 0)) == list(range(8))


@pytest.mark.parametrize("ncomp", [1, 3])
@pytest.mark.parametrize("shape", SHAPES)
def test_every_row_is_an_ordered_subset_of_its_class_table(oracle_backend, shape, ncomp):
    """Node = (anchor, class) with the edge nodes ascending in the anchor first and the class second; the walk of the table in slot
    order - neighbours that do not exist left out - IS the frontend's sorted row, hull rows included."""
    M, lat, ev = _pattern(shape, ncomp)
    assert PL.bindable(shape, ev)
    key = lat.anchor[lat.nvert:] * 8 + lat.cls[lat.nvert:]
    assert np.all(key[1:] > key[:-1]) and set(lat.cls[lat.nvert:]) == set(range(1, 8))
    tabs = PL.tables()
    lengths = set()
    for r in range(M.shape[0]):
        w = PL.walk(lat, r, ncomp, tabs)
        assert all(a < b for a, b in zip(w, w[1:]))
        assert np.array_equal(w, M.indices[M.indptr[r]:M.indptr[r + 1]])
        lengths.add(len(w))
    assert max(lengths) <= 65 * ncomp and min(lengths) < 19 * ncomp
    if min(shape) >= 4:
        assert max(lengths) == 65 * ncomp      # an interior vertex


@pytest.mark.parametrize("ncomp", [1, 3])
@pytest.mark.parametrize("shape", SHAPES[:2])
def test_round_trip_and_exact_product(oracle_backend, shape, ncomp):
    """to_form / from_form round-trips; on integer data the form's product equals the sequential ascending-column chain of the CSR
    rows bit for bit (every sum is exact)."""
    M, lat, ev = _pattern(shape, ncomp)
    rng = np.random.default_rng(5)
    M = M.copy()
    M.data[:] = rng.integers(1, 10, M.nnz) * rng.choice([-1, 1], M.nnz)
    x = rng.integers(-9, 10, M.shape[0]).astype(np.float64)
    form = PL.to_form(M, lat, ncomp)
    assert form[0].shape == (65 * ncomp, ncomp * lat.nvert) and form[1].shape == (27 * ncomp, M.shape[0] - ncomp * lat.nvert)
    assert np.count_nonzero(form[0]) + np.count_nonzero(form[1]) == M.nnz
    back = PL.from_form(form, lat, ncomp, M)
    assert np.array_equal(back.indptr, M.indptr) and np.array_equal(back.indices, M.indices) and np.array_equal(back.data, M.data)
    y = PL.product(form, lat, ncomp, x)
    assert np.array_equal(y, PL.chain(M, x)) and np.array_equal(y, M @ x)


def _count(n, g, entry):
    """Rows of class g on an n^3-vertex box that store the column at `entry`: the row's node and the column's node both exist."""
    total = 1
    for k in range(3):
        bg, o, bc = (g >> k) & 1, entry[k], (entry[3] >> k) & 1
        total *= sum(1 for i in range(n) if i + bg < n and 0 <= i + o and i + o + bc < n)
    return total


@pytest.mark.parametrize("n", [33, 65])
def test_the_form_costs_less_than_a_quarter_more_than_the_values(n):
    """65 arrays over the vertex rows and 27 over the edge rows against the stored entries of an n^3-vertex box, both counted from
    the tables: below 1.25 times the CSR value array (about 1.12 at these sizes)."""
    tabs = PL.tables()
    nnz = sum(_count(n, g, e) for g in range(8) for e in tabs[g])
    rows = [_count(n, g, (0, 0, 0, g)) for g in range(8)]
    form = 65 * rows[0] + 27 * sum(rows[1:])
    print("%d^3 vertices: %d slots for %d entries, %.3f" % (n, form, nnz, form / nnz))
    assert nnz < form < 1.25 * nnz


def test_refusals(oracle_backend):
    """An entry off the table, an axis with 2 vertices and a permuted edge list are refused."""
    shape = (3, 3, 3)
    M, lat, ev = _pattern(shape, 1)
    L = M.tolil()
    L[0, 2] = 1.0                   # vertex 0 -> vertex 2: two steps along x
    with pytest.raises(ValueError):
        PL.to_form(L.tocsr(), lat, 1)
    L = M.tolil()
    far = int(lat.node_of[(lat.nvert - 2, 1)])      # an edge at the far corner, seen from vertex 0
    L[0, far] = 1.0
    with pytest.raises(ValueError):
        PL.to_form(L.tocsr(), lat, 1)
    assert PL.bindable(shape, ev)
    assert not PL.bindable((2, 3, 3), ev) and not PL.bindable((3, 3, 2), ev)
    swapped = ev.copy()
    swapped[[0, 1]] = ev[[1, 0]]
    assert not PL.bindable(shape, swapped)
    flipped = ev.copy()
    flipped[0] = ev[0, ::-1]
    assert not PL.bindable(shape, flipped)
    ev2 = np.asarray(PM.base_layout(PM.space((2, 3, 3), 1)).edge_vertices)
    assert not PL.bindable((2, 3, 3), ev2)


@pytest.mark.parametrize("value", ["lattice", "csr"])
def test_a_backend_without_the_form_ignores_the_key(oracle_backend, value):
    """The numpy oracle backend has no p2_product: the key is accepted, the solve is the Jacobi-PCG on its own product, and no
    binding is asked for."""
    from pgdrome_amd import fem
    assert value in fem.P2_PRODUCT_NAMES and not hasattr(oracle_backend, "p2_product")
    mesh = fem.BoxMesh(fem.Point(0, 0, 0), fem.Point(1, 1, 1), 3, 3, 3)
    Vh = fem.FunctionSpace(mesh, "P", 2)
    u, v = fem.TrialFunction(Vh), fem.TestFunction(Vh)
    st0 = dict(fem.STATS)
    info = fem.solve((fem.inner(fem.grad(u), fem.grad(v)) + u * v) * fem.dx == fem.Constant(1.0) * v * fem.dx, fem.Function(Vh),
                     fem.DirichletBC(Vh, 0.0, lambda x, on_boundary: on_boundary),
                     solver_parameters={"p2_product": value, "relative_tolerance": 1e-10})
    assert info["method"] == "jacobi_pcg" and info["product"] == "csr" and info["relres"] <= 1e-10
    assert fem.STATS.get("p2_lattice_solves", 0) == st0.get("p2_lattice_solves", 0)
    assert len(Vh._lay._p2_bound) == 0


def test_an_unknown_value_is_an_error(oracle_backend):
    from pgdrome_amd import fem
    mesh = fem.BoxMesh(fem.Point(0, 0, 0), fem.Point(1, 1, 1), 3, 3, 3)
    Vh = fem.FunctionSpace(mesh, "P", 2)
    u, v = fem.TrialFunction(Vh), fem.TestFunction(Vh)
    with pytest.raises(ValueError):
        fem.solve((fem.inner(fem.grad(u), fem.grad(v)) + u * v) * fem.dx == fem.Constant(1.0) * v * fem.dx, fem.Function(Vh),
                  solver_parameters={"p2_product": "ell"})
