"""The variable-coefficient multigrid preconditioner (pgdrome_amd/csrc/pgd_vmg.hip) checked without a GPU, on its numpy restatement
tests/vmg_reference.py; tests/test_vmg_gpu.py compares the HIP path with it.

1a  the claim the design rests on: the Galerkin operator P^T A P of a 15-point operator is a 15-point operator, on every level,
    for weighted, two-material and Robin operators and for hull, one-face and empty Dirichlet sets - exactly, in integer
    arithmetic, where the reference is rational;
1b  the cycle is a symmetric operator and PCG with it converges;
1c  iteration counts of the restatement against the Jacobi-PCG on the operator of problems.inclusion_heat.
"""
from fractions import Fraction

import numpy as np
import pytest
import scipy.sparse as sps

from tests import exact_reference as X
from tests import robin_reference as R
from tests import subdomain_reference as SD
from tests import vmg_reference as V
from tests import weighted_reference as W

FAMILIES = ("weighted", "two_material", "robin")
_LAYS = {}


def _layout(nn):
    if nn not in _LAYS:
        coords, cells = V.box((nn, nn, nn))
        _LAYS[nn] = W.WeightedExactLayout(coords, cells)
    return _LAYS[nn]


def _far_face_facets(lay, nn):
    """The boundary triangles of the face x_0 = max: the faces of the cells that lie in it."""
    hi = lay.coords[:, 0].max()
    on = lay.coords[:, 0] >= hi
    out = []
    for c in lay.cells[on[lay.cells].sum(axis=1) == 3]:
        out.append(c[on[c]])
    return np.array(out, dtype=np.int64)


def family_operator(family, nn):
    """(operator on the 6-tets-per-cube box of nn^3 nodes, exact: bool): an int64 CSR matrix - a positive multiple of the exact
    rational operator - for the rational families, float64 for the Robin one (a facet's measure is irrational in 3-D)."""
    lay = _layout(nn)
    if family == "weighted":
        w = X.weight_of(lay.coords)
        vals, _ = lay.atom(X.WSTIFF, 0, 0, w)
        return V.exact_integer_form(vals, lay.rp, lay.cols, lay.n)[0], True
    if family == "two_material":
        mask = V.inclusion_mask(lay.coords, lay.cells)
        assert 0 < mask.sum() < mask.size
        out_v, _ = SD.subset_atom(lay, X.STIFF, mask=1 - mask)
        in_v, _ = SD.subset_atom(lay, X.STIFF, mask=mask)
        vals = out_v + Fraction(1, 10) * in_v                     # kappa = 0.1 inside the inclusion
        return V.exact_integer_form(vals, lay.rp, lay.cols, lay.n)[0], True
    vals, _ = lay.atom(X.STIFF)
    K = V.float_csr(vals, lay)
    Rm = R.facet_mass_matrix(lay.coords, _far_face_facets(lay, nn), lay.n)
    return (2.0 * K + 3.0 * sps.csr_matrix(Rm)).tocsr(), False


@pytest.mark.parametrize("bc_name", ["hull", "face", "none"])
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("nn", [9, 17])
def test_galerkin_operator_stays_on_the_15_point_pattern(nn, family, bc_name):
    """Every entry of P^T A P off the 15-point pattern is zero on every coarse level: exactly (integer arithmetic on a multiple of
    the exact rational operator) for the weighted and the two-material stiffness, to n eps max|entry| for stiffness + Robin mass."""
    A, exact = family_operator(family, nn)
    lay = _layout(nn)
    bc = V.dirichlet_sets(lay.coords)[bc_name]
    A = V.apply_dirichlet_exact(A, bc)
    shape = (nn, nn, nn)
    on_fine = V.off_pattern_max(A, shape)
    assert on_fine[0] == 0 and on_fine[1] > 0                  # (the fine operator itself is a 15-point operator)
    el = V.eliminated_rows(A)
    assert el.sum() == bc.size
    if exact:
        levels = V.integer_hierarchy(A, shape, el)
    else:
        levels, sh, e = [], shape, el
        Af = A
        for _ in range(2):
            P, sh, e = V.interpolation(sh, e)
            Af = V.galerkin(Af, P, e)
            levels.append((Af, sh))
    assert len(levels) == 2
    for Ac, cs in levels:
        assert Ac.shape[0] == cs[0] * cs[1] * cs[2]
        off, big = V.off_pattern_max(Ac, cs)
        assert big > 0
        if exact:
            assert Ac.dtype == np.int64 and off == 0
        else:
            assert off <= Ac.shape[0] * np.finfo(np.float64).eps * big
        assert abs(Ac - Ac.T).max() <= (0 if exact else 1e-14 * big)


def _spd_case(family, nn=17):
    A, exact = family_operator(family, nn)
    lay = _layout(nn)
    sets = V.dirichlet_sets(lay.coords)
    bc = {"weighted": sets["hull"], "two_material": sets["face"], "robin": sets["none"]}[family]
    A = V.apply_dirichlet_exact(sps.csr_matrix(A, dtype=np.float64), bc)
    return A, bc, (nn, nn, nn)


@pytest.mark.parametrize("family", FAMILIES)
def test_cycle_is_symmetric_and_pcg_converges(family):
    """17^3 nodes = two levels.  <M x, y> = <x, M y> to rounding for seeded random vectors (zero on the eliminated nodes, where the
    cycle's vectors live); PCG with the cycle reaches rtol 1e-10 and the direct solution."""
    import scipy.sparse.linalg as spla
    A, bc, shape = _spd_case(family)
    M, levels = V.apply_preconditioner(A, shape)
    assert len(levels) == 2 and levels[1].A.shape[0] == 9 ** 3
    rng = np.random.default_rng(5)
    free = ~levels[0].el
    for _ in range(3):
        x, y = rng.uniform(-1, 1, A.shape[0]) * free, rng.uniform(-1, 1, A.shape[0]) * free
        Mx, My = M(x), M(y)
        assert abs(Mx @ y - x @ My) <= 1e-13 * np.linalg.norm(Mx) * np.linalg.norm(y)
        assert Mx @ x > 0.0
        assert np.all(Mx[~free] == 0.0)
    b = rng.uniform(-1, 1, A.shape[0])
    xs, it, rel = V.pcg(A, b, shape, rtol=1e-10)
    _, itj, _ = V.pcg(A, b, shape, rtol=1e-10, precond="jacobi")
    print("%s 17^3: V-cycle PCG %d iterations, Jacobi-PCG %d" % (family, it, itj))
    assert rel <= 1e-10 and it < itj
    assert np.linalg.norm(b - A @ xs) <= 1.0001e-10 * np.linalg.norm(b)
    ref = spla.spsolve(A.tocsc(), b)
    assert np.linalg.norm(xs - ref) <= 1e-8 * np.linalg.norm(ref)


def test_iteration_counts_on_the_inclusion_operator():
    """PCG iterations of the restatement / of the Jacobi-PCG on the scaled operator of problems.inclusion_heat (hull eliminated,
    right-hand side 1 on the free nodes, zero start, rtol 1e-10), recorded on the numpy restatement:

        kappa   17^3      33^3      65^3
        0.1     20 / 55   24 / 113  28 / 227
        10      22 / 56   27 / 117  31 / 235

    (l1-Jacobi, V(1,1), 24 sweeps on the 9^3 coarsest level.  The V-cycle count creeps by about 4 per doubling with this weak
    smoother and inexact coarsest solve, the Jacobi count doubles.)  Asserted at 65^3: at most a quarter of the Jacobi-PCG's
    iterations, and growth by less than a factor 1.5 from 33^3."""
    for kappa in (0.1, 10.0):
        counts = {}
        for nc in (16, 32, 64):
            A, b, shape = V.inclusion_operator(nc, kappa)
            x, it, rel = V.pcg(A, b, shape)
            xj, itj, relj = V.pcg(A, b, shape, precond="jacobi")
            print("kappa %g, %d^3 nodes: V-cycle PCG %d iterations, Jacobi-PCG %d" % (kappa, nc + 1, it, itj))
            assert rel <= 1e-10 and relj <= 1e-10
            assert np.abs(x - xj).max() <= 1e-9 * np.abs(xj).max()
            counts[nc] = (it, itj)
        assert 4 * counts[64][0] <= counts[64][1]
        assert counts[64][0] < 1.5 * counts[32][0]


def test_small_lattices_have_no_hierarchy():
    """At most 4096 nodes: the coarsest level alone is no multigrid - the library answers with the Jacobi-PCG."""
    A, b, shape = V.inclusion_operator(8, 10.0)
    assert V.build(V.scale_unit(A)[0], shape) is None


@pytest.mark.parametrize("prec", ["vmg", "variable_multigrid"])
def test_backend_without_the_cycle_answers_with_jacobi_pcg(prec):
    """The numpy oracle backend has no precondition_variable: the new names neither raise nor reach it as an unknown value."""
    from oracle.backend_numpy import NumpyBackend
    from pgdrome_amd import fem
    assert prec in fem.VARIABLE_MULTIGRID_NAMES and not set(fem.VARIABLE_MULTIGRID_NAMES) & set(fem.MULTIGRID_NAMES)
    old = fem._backend
    try:
        be = fem.set_backend(NumpyBackend())
        fem.clear_caches()
        assert not hasattr(be, "precondition_variable")
        mesh = fem.BoxMesh(fem.Point(0, 0, 0), fem.Point(1, 1, 1), 6, 6, 6)
        Vh = fem.FunctionSpace(mesh, "P", 1)
        u, v = fem.TrialFunction(Vh), fem.TestFunction(Vh)
        sol = fem.Function(Vh)
        st0 = dict(fem.STATS)
        info = fem.solve(fem.inner(fem.grad(u), fem.grad(v)) * fem.dx == fem.Constant(1.0) * v * fem.dx, sol,
                         fem.DirichletBC(Vh, 0.0, lambda x, on_boundary: on_boundary),
                         solver_parameters={"preconditioner": prec, "relative_tolerance": 1e-10})
        assert info["method"] == "jacobi_pcg" and info["relres"] <= 1e-10
        assert fem.STATS.get("vmg_solves", 0) == st0.get("vmg_solves", 0)
    finally:
        if old is not None:
            fem.set_backend(old)
        else:
            fem._backend = None
        fem.clear_caches()
