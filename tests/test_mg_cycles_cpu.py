"""What tests/test_mg_cycles_gpu.py rests on, checked without a GPU on the numpy restatements of the three multigrid cycles
(oracle/mg_numpy.py, tests/vmg_reference.py, tests/cmg_reference.py) over the case table tests/mg_cycle_cases.py:

  * the rounding noise N_k of the first three iterates under 1-ulp perturbations of the operator lies a factor 32 under the tolerance
    table TAU the device is held to;
  * every mutant of a cycle - one sweep less at the bottom, one wrong smoothing weight, one wrong row of the restriction or the
    interpolation, another damping on the coarse levels, one component left unscaled - moves the FIRST iterate by at least 1000 TAU,
    while the assertions on the converged solve (iteration count, solution to 1e-9) let most of them pass: recorded beside each;
  * MG.Slab over the whole lattice is MG.vcycle bit for bit.
"""
import contextlib

import numpy as np
import pytest
import scipy.sparse as sps

from oracle import mg_numpy as MG
from tests import cmg_reference as CM
from tests import mg_cycle_cases as T
from tests import vmg_reference as V

SEEDS = (1, 2, 3)
_CMG = {}


@pytest.fixture(scope="module")
def oracle_backend():
    from oracle.backend_numpy import NumpyBackend
    from pgdrome_amd import fem
    old = fem._backend
    be = fem.set_backend(NumpyBackend())
    fem.clear_caches()
    yield be
    _CMG.clear()
    if old is not None:
        fem.set_backend(old)
    else:
        fem._backend = None
    fem.clear_caches()


def _cmg(name):
    """(operator, right-hand sides, iterates) of a cmg case on the backend in use (the oracle's), built once."""
    if name not in _CMG:
        case = T.CMG_CASES[name]
        _, M, bc = T.cmg_operator(case, T.cmg_space(case))
        assert abs(M - M.T).max() <= 1e-14 * abs(M).max()
        _CMG[name] = (M,) + T.cmg_reference(case, M)
    return _CMG[name]


def _noise(base, runs):
    """{k: largest max-norm change of x_k relative to max |x_k|} over the perturbed runs and the kinds of right-hand side."""
    return {k: max(T.deviation(run[kind][k - 1], base[kind][k - 1]) for run in runs for kind in base) for k in T.KS}


def _report(cycle, name, N):
    print("noise %s %s: " % (cycle, name) + ", ".join("N_%d = %.1e (tau %.1e)" % (k, N[k], T.TAU[cycle][k]) for k in T.KS))
    for k in T.KS:
        assert T.TAU[cycle][k] <= T.TAU_CAP
        assert N[k] <= T.TAU[cycle][k] / 32, (cycle, name, k, N[k])


@pytest.mark.parametrize("name", sorted(T.VMG_CASES))
def test_noise_of_the_vmg_iterates_lies_under_the_tolerance(name):
    A, _ = T.vmg_operator(name)
    rhs, base = T.vmg_reference(name)
    assert len(V.build(V.scale_unit(A)[0], T.VMG_CASES[name]["shape"])) == T.VMG_CASES[name]["levels"]
    _report("vmg", name, _noise(base, [T.vmg_iterates(T.ulp_perturbed(A, s), T.VMG_CASES[name]["shape"], rhs) for s in SEEDS]))


@pytest.mark.parametrize("name", sorted(T.CMG_CASES))
def test_noise_of_the_cmg_iterates_lies_under_the_tolerance(oracle_backend, name):
    case = T.CMG_CASES[name]
    M, rhs, base = _cmg(name)
    assert [len(l) for l in CM.build(M, case["shape"], case["ncomp"])] == [case["levels"]] * case["ncomp"]
    _report("cmg", name, _noise(base, [T.cmg_iterates(T.ulp_perturbed(M, s), case["shape"], case["ncomp"], rhs) for s in SEEDS]))


@pytest.mark.parametrize("name", sorted(T.MG_CASES))
def test_noise_of_the_mg_iterates_lies_under_the_tolerance(name):
    case = T.MG_CASES[name]
    c, _ = T.mg_stencil(name)
    rhs, base = T.mg_reference(name)
    assert len(MG.build_levels(case["shape"][::-1], c)) == case["levels"]
    _report("mg", name, _noise(base, [T.mg_iterates(case["shape"], T.ulp_perturbed_stencil(c, s), rhs) for s in SEEDS]))


def _slab_stages(c, r):
    """The four stages on the whole lattice of T.SLAB_SHAPE: (t, b1, x1, z), each from the stage before."""
    zyx = T.SLAB_SHAPE[::-1]
    sl = MG.Slab(zyx, c, 0, zyx[0], 0, zyx[0])
    t = sl.down(r)
    b1 = sl.restrict(t)
    x1 = sl.coarse(b1)
    return sl, (t, b1, x1, sl.up(r, x1)[0])


def _slab_r():
    zyx = T.SLAB_SHAPE[::-1]
    c, _ = T.mg_stencil("slab")
    return c, np.random.default_rng(17).uniform(-1, 1, zyx) * MG.build_levels(zyx, c)[0].mask


def test_noise_of_the_slab_stages_lies_under_the_tolerance():
    c, r = _slab_r()
    _, base = _slab_stages(c, r)
    N = max(T.deviation(got, ref) for s in SEEDS for got, ref in zip(_slab_stages(T.ulp_perturbed_stencil(c, s), r)[1], base))
    print("noise slab stages: N = %.1e (tau %.1e)" % (N, T.TAU["slab"]))
    assert T.TAU["slab"] <= T.TAU_CAP and N <= T.TAU["slab"] / 32


def test_slab_over_the_whole_lattice_is_the_v_cycle_bit_for_bit():
    c, r = _slab_r()
    sl, (t, b1, x1, z) = _slab_stages(c, r)
    assert len(sl.levels) == 3
    assert np.array_equal(z, MG.vcycle(sl.levels, 0, r))
    assert sl.up(r, x1)[1] == float((r * z).sum())
    # ... and the partition of the GPU test sums to the whole right-hand side of level 1, with one contribution per entry
    parts = []
    for name in T.SLAB_PARTITION:
        zoff, nzloc, lz0, lz1 = T.SLABS[name]
        p = MG.Slab(sl.levels[0].shape, c, zoff, nzloc, lz0, lz1)
        tl = t[zoff:zoff + nzloc]
        assert np.array_equal(p.down(r[zoff:zoff + nzloc])[lz0:lz1], tl[lz0:lz1])
        parts.append(p.restrict(tl))
    assert np.array_equal(sum(parts), b1) and np.all(sum((p != 0.0).astype(int) for p in parts) <= 1)


# ---- mutants ---------------------------------------------------------------------------------------------------------------------

class _Transfer:
    """Stands in for a level's P where restriction and interpolation are mutated apart: `.T @ t` restricts, `@ e` interpolates."""

    def __init__(self, P, Rm):
        self.P, self.T = P, Rm

    def __matmul__(self, e):
        return self.P @ e


@contextlib.contextmanager
def _patched(module, attr, value):
    real = getattr(module, attr)
    setattr(module, attr, value)
    try:
        yield real
    finally:
        setattr(module, attr, real)


def _free_middle(L):
    free = np.where(~L.el)[0]
    return int(free[free.size // 2])


@contextlib.contextmanager
def _vmg_build_mutant(change):
    """V.build with `change(levels)` applied to every hierarchy it returns (the component cycle builds through it as well)."""
    real = V.build

    def build(A, shape):
        levels = real(A, shape)
        change(levels)
        return levels
    with _patched(V, "build", build):
        yield


def _coarse_weight(levels):
    w = levels[1].w.copy()
    w[_free_middle(levels[1])] *= 1.05
    levels[1].w = w


def _restriction_row(levels):
    P = levels[0].P
    Rm = sps.lil_matrix(P.T)
    i = _free_middle(levels[1])
    Rm[i, :] = Rm[i, :] * 0.5
    levels[0].P = _Transfer(P, Rm.tocsr())


def _far_face_weight(levels):
    """One weight 1/2 of a free fine node on the far z face dropped from the interpolation (the restriction keeps it)."""
    P = levels[0].P
    nx, ny, nz = levels[0].shape
    i = T.node_index((nx, ny, nz), (nx // 2, ny // 2, nz - 1))
    assert not levels[0].el[i]
    Pm = sps.lil_matrix(P)
    j = Pm.rows[i][0]
    assert Pm[i, j] == 0.5
    Pm[i, j] = 0.0
    levels[0].P = _Transfer(Pm.tocsr(), P.T)


@contextlib.contextmanager
def _mg_coarse_omega():
    real = MG.build_levels

    def build_levels(shape, c):
        levels = real(shape, c)
        for L in levels[1:]:
            L.w = 0.9 / L.S[1, 1, 1]
        return levels
    with _patched(MG, "build_levels", build_levels):
        yield


@contextlib.contextmanager
def _mg_restriction_row(fine):
    real = MG.restrict

    def restrict(r, cshape):
        out = real(r, cshape)
        if r.shape == fine:                                         # (the restriction from level 0, not mg_numpy.galerkin's)
            out[cshape[0] // 2, cshape[1] // 2, cshape[2] // 2] *= 0.5
        return out
    with _patched(MG, "restrict", restrict):
        yield


@contextlib.contextmanager
def _cmg_unscaled_component():
    def apply(levels, s, r):
        z = np.empty_like(r)
        n = len(levels)
        for c in range(n):
            z[c::n] = V.vcycle(levels[c], s[c::n] * r[c::n]) * (1.0 if c == 1 else s[c::n])
        return z
    with _patched(CM, "apply", apply):
        yield


# mutant -> (context manager, cases (cycle, name) it is tried on, whether the converged-solve assertions of tests/test_vmg_gpu.py,
# test_cmg_gpu.py and test_kernels_gpu.py - the same iteration count (vmg) or +-1 (mg, cmg), the solution to 1e-9 - would have
# noticed it on those cases: measured by this test, printed by it, recorded here as data)
MUTANTS = {
    "vmg_23_bottom_sweeps": (lambda: _patched(V, "BOTTOM_SWEEPS", 23), [("vmg", "17x17x17-weighted")], False),
    "vmg_coarse_l1_weight_5_percent": (lambda: _vmg_build_mutant(_coarse_weight), [("vmg", "17x17x17-weighted"), ("vmg", "33x25x20-mixed")], False),
    "vmg_restriction_halves_a_row": (lambda: _vmg_build_mutant(_restriction_row), [("vmg", "17x17x17-weighted")], False),
    "vmg_far_face_weight_dropped": (lambda: _vmg_build_mutant(_far_face_weight), [("vmg", "33x25x20-robin")], True),
    "mg_23_bottom_sweeps": (lambda: _patched(MG, "BOTTOM_SWEEPS", 23), [("mg", "20x17x12")], False),
    "mg_restriction_halves_a_row": (lambda: _mg_restriction_row((16, 18, 33)), [("mg", "33x18x16")], False),
    "mg_coarse_omega_0.9": (_mg_coarse_omega, [("mg", "33x18x16"), ("mg", "20x17x12")], False),
    "cmg_component_left_unscaled": (_cmg_unscaled_component, [("cmg", "17x17x17-roller")], True),
    "cmg_coarse_l1_weight_5_percent": (lambda: _vmg_build_mutant(_coarse_weight), [("cmg", "17x17x17-clamped")], False),
}


def _solve(cycle, name, b, rtol, maxit):
    if cycle == "vmg":
        A, _ = T.vmg_operator(name)
        return V.pcg(A, b, T.VMG_CASES[name]["shape"], rtol=rtol, maxit=maxit)[:2]
    if cycle == "cmg":
        case = T.CMG_CASES[name]
        return CM.pcg(_cmg(name)[0], b, case["shape"], case["ncomp"], rtol=rtol, maxit=maxit)[:2]
    zyx = T.MG_CASES[name]["shape"][::-1]
    x, it, _ = MG.pcg(zyx, T.mg_stencil(name)[0], b.reshape(zyx), rtol=rtol, maxit=maxit)
    return x.ravel(), it


def _base_x1(cycle, name):
    ref = T.vmg_reference(name) if cycle == "vmg" else T.mg_reference(name) if cycle == "mg" else _cmg(name)[1:]
    return ref[0]["zero"][0], ref[1]["zero"][0]


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_a_mutant_moves_the_first_iterate_far_beyond_the_tolerance(oracle_backend, mutant):
    make, cases, recorded = MUTANTS[mutant]
    moves, noticed = [], []
    for cycle, name in cases:
        b, x1 = _base_x1(cycle, name)
        rtol = 1e-10 if cycle == "mg" else 1e-12                    # (the tolerances of today's converged-solve tests)
        xc, itc = _solve(cycle, name, b, rtol, 5000)
        with make():
            m1, it1 = _solve(cycle, name, b, T.RTOL, 1)
            mc, itm = _solve(cycle, name, b, rtol, 4 * itc + 10)         # (a broken symmetry may never converge: four times the count says so)
        assert it1 == 1
        moves.append(T.deviation(m1, x1))
        final = float(np.linalg.norm(mc - xc) / np.linalg.norm(xc))
        seen = abs(itm - itc) > (0 if cycle == "vmg" else 1) or final > 1e-9
        noticed.append(seen)
        print("mutant %s on %s %s: x_1 moves %.1e (1000 tau_1 = %.1e); converged solve: %d iterations (base %d), solution moves %.1e: %s today"
              % (mutant, cycle, name, moves[-1], 1000 * T.TAU[cycle][1], itm, itc, final, "NOTICED" if seen else "not noticed"))
    assert max(m / T.TAU[c][1] for m, (c, _) in zip(moves, cases)) >= 1000.0
    if recorded is not None and recorded != any(noticed):
        print("mutant %s: recorded as %snoticed by the converged-solve assertions, measured otherwise" % (mutant, "" if recorded else "not "))
