"""The row-diagonal form of vector-valued P1 operators on box lattices (pgdrome_amd/csrc/pgd_bdia.hip, PGD_TUNE_SPMV_BLOCK_DIA,
settings["block_product"] = "diagonal") checked without a GPU, on its numpy restatement tests/block_dia_reference.py;
tests/test_block_dia_gpu.py compares the HIP product with the CSR product bit by bit."""
import numpy as np
import pytest
import scipy.sparse as sps

from tests import block_dia_reference as BD

SHAPES = [(5, 4, 3), (9, 7, 6)]


@pytest.fixture(scope="module")
def oracle_backend():
    from oracle.backend_numpy import NumpyBackend
    from pgdrome_amd import fem
    old = fem._backend
    be = fem.set_backend(NumpyBackend())
    fem.clear_caches()
    yield be
    if old is not None:
        fem.set_backend(old)
    else:
        fem._backend = None
    fem.clear_caches()


def test_slot_numbering_round_trip():
    """t -> step -> t for the 15 slots; the 12 steps of {-1, 0, 1}^3 with mixed signs have no slot; the centre is slot 7."""
    steps = [BD.step_of(t) for t in range(BD.NT)]
    assert len(set(steps)) == BD.NT and steps[7] == (0, 0, 0)
    assert [BD.slot_of(s) for s in steps] == list(range(BD.NT))
    every = [(dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]
    assert sum(BD.slot_of(s) is None for s in every) == 27 - BD.NT
    assert BD.slot_of((2, 0, 0)) is None and BD.slot_of((0, -2, 0)) is None


@pytest.mark.parametrize("shape", SHAPES + [(2, 2, 2), (2, 3, 2)])
def test_slots_ascend_with_the_node_offset(shape):
    """-P-nx-1, -P-nx, -P-1, -P, -nx-1, -nx, -1, 0, +1, +nx, +nx+1, +P, +P+1, +P+nx, +P+nx+1: strictly ascending from nx, ny >= 2 on."""
    nx, ny, _ = shape
    P = nx * ny
    offs = [BD.node_offset(t, shape) for t in range(BD.NT)]
    assert offs == [-P - nx - 1, -P - nx, -P - 1, -P, -nx - 1, -nx, -1, 0, 1, nx, nx + 1, P, P + 1, P + nx, P + nx + 1]
    assert all(a < b for a, b in zip(offs, offs[1:]))


@pytest.mark.parametrize("ncomp", [2, 3])
@pytest.mark.parametrize("shape", SHAPES)
def test_the_walk_is_the_sorted_row(shape, ncomp):
    """t ascending, d ascending inside t visits the stored columns of every row - rim rows included - in ascending order, and
    they are the columns of the blocked 15-point pattern (Kronecker product of the scalar pattern with a full block)."""
    M = BD.pattern(shape, ncomp)
    n = M.shape[0]
    lengths = set()
    for r in range(n):
        w = BD.walk(r, shape, ncomp)
        assert all(a < b for a, b in zip(w, w[1:]))
        assert np.array_equal(w, M.indices[M.indptr[r]:M.indptr[r + 1]])
        lengths.add(len(w))
    assert max(lengths) == 15 * ncomp and min(lengths) < 15 * ncomp       # interior rows and rim rows
    scalar = BD.pattern(shape, 1)
    K = sps.kron(scalar, np.ones((ncomp, ncomp))).tocsr()
    K.sort_indices()
    assert np.array_equal(K.indptr, M.indptr) and np.array_equal(K.indices, M.indices)


@pytest.mark.parametrize("ncomp", [2, 3])
@pytest.mark.parametrize("shape", SHAPES)
def test_integer_product_is_exact(shape, ncomp):
    """On integer-valued matrices with the pattern and integer x every sum is exact: the form's product equals M @ x."""
    rng = np.random.default_rng(5)
    M = BD.pattern(shape, ncomp)
    M.data[:] = rng.integers(-9, 10, M.nnz)
    x = rng.integers(-9, 10, M.shape[0]).astype(np.float64)
    form = BD.to_form(M, shape, ncomp)
    assert form.shape == (15 * ncomp, M.shape[0])
    assert np.count_nonzero(form) == np.count_nonzero(M.data)
    assert np.array_equal(BD.product(form, shape, ncomp, x), M @ x)


def test_an_entry_off_the_pattern_is_refused():
    shape, ncomp = (5, 4, 3), 3
    M = BD.pattern(shape, ncomp).tolil()
    M[0, ncomp * 2] = 1.0           # node 0 -> node 2: two steps along x
    with pytest.raises(ValueError):
        BD.to_form(M.tocsr(), shape, ncomp)


@pytest.mark.parametrize("value", ["diagonal", "csr"])
def test_a_backend_without_the_form_ignores_the_key(oracle_backend, value):
    """The numpy oracle backend has no block_product: the key is accepted, the solve is the Jacobi-PCG on its own product."""
    from pgdrome_amd import fem
    assert value in fem.BLOCK_PRODUCT_NAMES and not hasattr(oracle_backend, "block_product")
    mesh = fem.BoxMesh(fem.Point(0, 0, 0), fem.Point(1, 1, 1), 4, 4, 4)
    Vh = fem.VectorFunctionSpace(mesh, "P", 1)
    u, v = fem.TrialFunction(Vh), fem.TestFunction(Vh)
    a = sum(u[i].dx(k) * v[i].dx(k) * fem.dx for i in range(3) for k in range(3)) + fem.dot(u, v) * fem.dx
    sol = fem.Function(Vh)
    st0 = dict(fem.STATS)
    info = fem.solve(a == fem.Constant(-1.0) * v[2] * fem.dx, sol,
                     fem.DirichletBC(Vh, fem.Constant((0.0, 0.0, 0.0)), lambda x, on_boundary: on_boundary),
                     solver_parameters={"block_product": value, "relative_tolerance": 1e-10})
    assert info["method"] == "jacobi_pcg" and info["product"] == "csr" and info["relres"] <= 1e-10
    assert fem.STATS.get("block_dia_solves", 0) == st0.get("block_dia_solves", 0)


def test_an_unknown_value_is_an_error(oracle_backend):
    from pgdrome_amd import fem
    mesh = fem.BoxMesh(fem.Point(0, 0, 0), fem.Point(1, 1, 1), 3, 3, 3)
    Vh = fem.FunctionSpace(mesh, "P", 1)
    u, v = fem.TrialFunction(Vh), fem.TestFunction(Vh)
    with pytest.raises(ValueError):
        fem.solve((fem.inner(fem.grad(u), fem.grad(v)) + u * v) * fem.dx == fem.Constant(1.0) * v * fem.dx, fem.Function(Vh),
                  solver_parameters={"block_product": "ell"})
