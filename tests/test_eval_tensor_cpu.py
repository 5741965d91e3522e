"""fem.stress_quantity, the eigenvalue algorithm of the device routine restated in numpy, and the host path of
PGD.evaluate_gradient_many for "max_principal", "min_principal", "tresca" and "stress_component" (oracle backend, no GPU)
against tests/eval_tensor_reference.py."""
import numpy as np
import pytest

from oracle.backend_numpy import NumpyBackend
from pgdrome_amd import fem, problems
from pgdrome_amd.solver import PGDProblem
from tests.eval_gradient_reference import samples_of, two_valued
from tests.eval_many_reference import U53
from tests.eval_tensor_reference import (EIG_MAX, EIG_MIN, EIG_SPREAD, VALUE, deflating_eigenvalues, families, frobenius, jacobi_eigenvalues,
                                         planes_of, run_and_check_tensor, stress_matrix, tensor_bound, trigonometric_eigenvalues,
                                         value_reference)
from tests.test_eval_gradient_cpu import one_mode_solution

P = fem.Point
E_MOD, NU, EPS = 210.0, 0.3, 1e-3
MU, LAME = E_MOD / (2 * (1 + NU)), E_MOD * NU / ((1 + NU) * (1 - 2 * NU))
QUANTITIES = ["max_principal", "min_principal", "tresca", "stress_component"]


@pytest.fixture(scope="module")
def oracle():
    old = fem._backend
    fem.set_backend(NumpyBackend())
    fem.clear_caches()
    yield
    fem.set_backend(old)
    fem.clear_caches()


# ------------------------------------------------------------------------------------------------ fem.stress_quantity
# the gradient g[c G + d] = d u_c / d x_d of a strain state and the stress tensor sigma = 2 mu eps + lambda tr(eps) I computed by hand
def _states(G):
    z = np.zeros((G, G))
    uni, shear, vol = z.copy(), z.copy(), EPS * np.eye(G)
    uni[0, 0] = EPS                                      # uniaxial STRAIN eps_xx: sigma_xx = (lambda + 2 mu) eps, the others lambda eps
    shear[0, 1] = EPS                                    # u_x = eps y: eps_xy = eps / 2, sigma_xy = mu eps
    sig_uni = np.diag([LAME * EPS + 2 * MU * EPS, LAME * EPS, LAME * EPS])
    sig_shear = np.zeros((3, 3))
    sig_shear[0, 1] = sig_shear[1, 0] = MU * EPS
    sig_vol = np.diag([G * LAME * EPS + 2 * MU * EPS] * G + [G * LAME * EPS] * (3 - G))      # (2-D: sigma_zz = lambda tr eps)
    return {"uniaxial": (uni, sig_uni), "shear": (shear, sig_shear), "volumetric": (vol, sig_vol)}


@pytest.mark.parametrize("state", ["uniaxial", "shear", "volumetric"])
@pytest.mark.parametrize("G", [3, 2])
def test_stress_quantity_on_hand_computed_stresses(G, state):
    grad, sigma = _states(G)[state]
    g = grad.reshape(-1)
    L, kind = fem.stress_quantity("max_principal", G, NU)
    assert kind == EIG_MAX and L.shape == (4 if G == 2 else 6, G * G)
    planes = E_MOD * (L @ g)
    want = [sigma[0, 0], sigma[1, 1], sigma[2, 2], sigma[0, 1], sigma[1, 2], sigma[0, 2]][:L.shape[0]]
    assert np.allclose(planes, want, rtol=1e-13, atol=1e-13 * E_MOD * EPS)
    if G == 2:
        assert abs(planes[2] - NU * (planes[0] + planes[1])) <= 1e-13 * E_MOD * EPS          # plane strain
    assert np.array_equal(fem.stress_quantity("min_principal", G, NU)[0], L) and fem.stress_quantity("min_principal", G, NU)[1] == EIG_MIN
    assert np.array_equal(fem.stress_quantity("tresca", G, NU)[0], L) and fem.stress_quantity("tresca", G, NU)[1] == EIG_SPREAD
    assert np.allclose(L, stress_matrix(G, NU), rtol=1e-14, atol=1e-16)                      # the independent restatement
    comps = [(a, b) for a in range(G) for b in range(G)] + ([(2, 2)] if G == 2 else [])
    for a, b in comps:
        row, kind = fem.stress_quantity("stress_component", G, NU, component=(a, b))
        assert kind == VALUE and row.shape == (1, G * G)
        assert abs(E_MOD * (row @ g)[0] - sigma[a, b]) <= 1e-13 * E_MOD * EPS
    w = np.linalg.eigvalsh(sigma)
    U = planes[:, None]
    assert abs(value_reference(U, EIG_MAX)[0] - w[2]) <= 1e-12 * E_MOD * EPS
    assert abs(value_reference(U, EIG_SPREAD)[0] - (w[2] - w[0])) <= 1e-12 * E_MOD * EPS


def test_the_kinds_are_one_set_of_numbers():
    """pgd_eval_quantity of the header, the binding's EVAL_Q_*, the frontend's and the restatement's are the same integers."""
    import re
    from pathlib import Path
    from pgdrome_amd import _lib
    from tests import eval_tensor_reference as R
    text = (Path(__file__).resolve().parent.parent / "include" / "pgd_amd.h").read_text()
    body = re.search(r"enum pgd_eval_quantity \{(.*?)\}", text, flags=re.S).group(1)
    header = {k: int(v) for k, v in re.findall(r"PGD_(EVAL_Q_[A-Z_]+) = (\d+)", body)}
    assert header == {"EVAL_Q_NORM": 0, "EVAL_Q_VALUE": 1, "EVAL_Q_EIG_MAX": 2, "EVAL_Q_EIG_MIN": 3, "EVAL_Q_EIG_SPREAD": 4}
    for name, value in header.items():
        assert getattr(_lib, name) == value and getattr(fem, name) == value and getattr(R, name[len("EVAL_Q_"):]) == value


def test_stress_quantity_refusals():
    for bad in [("max_principal", 3, None), ("max_principal", 3, 0.5), ("tresca", 2, -1.0), ("min_principal", 3, 0.7),
                ("max_principal", 1, 0.3), ("von_mises", 3, 0.3), ("stress_component", 3, 0.3), ("stress_component", 2, 0.3, (0, 2)),
                ("stress_component", 3, 0.3, (0, 3)), ("stress_component", 3, 0.3, "xy"), ("tresca", 3, 0.3, (0, 1))]:
        with pytest.raises(ValueError):
            fem.stress_quantity(*bad)
    fem.stress_quantity("tresca", 3, -0.99)
    fem.stress_quantity("tresca", 3, 0.499)


# ------------------------------------------------------------------------------------------------ the algorithm
@pytest.fixture(scope="module")
def family_cases():
    """400 tensors of every family, full and plane (yz = xz = 0), with their eigenvalues from long double Jacobi rotations."""
    out = {}
    for plane in (False, True):
        for name, T in families(np.random.default_rng(20261020 + plane), 400, plane).items():
            out[(name, plane)] = (T, jacobi_eigenvalues(T).astype(np.float64))
    return out


def _units(got, want, T):
    nf = frobenius(planes_of(T, 6))
    return np.abs(got - want) / (U53 * np.where(nf > 0, nf, 1.0))


def test_the_arbiter_agrees_with_eigvalsh(family_cases):
    """The long double Jacobi eigenvalues and eigvalsh agree within the 16 u |sigma|_F the bound reserves for eigvalsh."""
    for (name, plane), (T, w) in family_cases.items():
        ev = np.linalg.eigvalsh(T)
        assert max(_units(ev[:, k], w[:, k], T).max() for k in range(3)) <= 16.0, (name, plane)


def test_deflating_form_stays_within_32_units(family_cases):
    """The algorithm of the device routine, operation by operation in numpy: within 32 u |sigma|_F of the exact eigenvalues on every
    family, the close pairs and the uniaxial states included - the allowance the device bound gives the routine."""
    worst = {}
    for (name, plane), (T, w) in family_cases.items():
        lo, hi = deflating_eigenvalues(T)
        worst[(name, plane)] = max(_units(lo, w[:, 0], T).max(), _units(hi, w[:, 2], T).max())
        assert np.all(hi >= lo)
    print("deflating form, largest error in u |sigma|_F:", {k: round(v, 2) for k, v in worst.items()})
    assert max(worst.values()) <= 32.0, worst


def test_trigonometric_formula_is_why_it_is_not_used(family_cases):
    """All three roots from the angle: on uniaxial stress in a rotated frame (a double eigenvalue, h = +-1) the error exceeds
    10^6 u |sigma|_F - the sqrt(u) of acos at the ends of its range."""
    T, w = family_cases[("rotated uniaxial", False)]
    lo, hi = trigonometric_eigenvalues(T)
    assert max(_units(lo, w[:, 0], T).max(), _units(hi, w[:, 2], T).max()) > 1e6
    lo, hi = deflating_eigenvalues(T)
    assert max(_units(lo, w[:, 0], T).max(), _units(hi, w[:, 2], T).max()) <= 32.0


def test_tensor_bound_is_the_stated_one():
    U = np.array([[3.0], [0.0], [0.0], [4.0], [0.0], [0.0]])                  # |sigma|_F = sqrt(9 + 2 * 16)
    e = np.full((6, 1), 1e-3)
    ne = 1e-3 * np.sqrt(3 + 2 * 3)
    want = ne + 48 * U53 * (np.sqrt(41.0) + ne)
    assert abs(tensor_bound(e, U, EIG_MAX)[0] - want) <= 1e-14 * want and abs(tensor_bound(e, U, EIG_SPREAD)[0] - 2 * want) <= 2e-14 * want
    assert tensor_bound(e[:1], U[:1], VALUE)[0] == 1e-3


# ------------------------------------------------------------------------------------------------ the frontend's host path
@pytest.fixture(scope="module")
def elastic_p1(oracle):
    mesh = fem.BoxMesh(P(0, 0, 0), P(2, 1, 1), 3, 2, 2)
    p = PGDProblem(**problems.elastic_block(mesh, 5, PGD_nmax=2))
    p.solve_PGD(_problem="linear", settings={"relative_tolerance": 1e-11})
    return mesh, p.return_PGD()


@pytest.fixture(scope="module")
def elastic_p2(oracle):
    mesh = fem.BoxMesh(P(0, 0, 0), P(2, 1, 1), 2, 2, 2)
    p = PGDProblem(**problems.elastic_block(mesh, 5, PGD_nmax=2, degree=2))
    p.solve_PGD(_problem="linear", settings={"relative_tolerance": 1e-11})
    return mesh, p.return_PGD()


def _component(quantity):
    return (0, 1) if quantity == "stress_component" else None


@pytest.mark.parametrize("planes", ["stored", "fused"])
@pytest.mark.parametrize("quantity", QUANTITIES)
def test_host_path_p1(elastic_p1, quantity, planes):
    """Against the loop evaluate -> gradient -> eigvalsh, with a float E and with a DG0 E."""
    mesh, sol = elastic_p1
    res, ref = run_and_check_tensor(sol, [1], samples_of(sol, (1,), 7, 5), quantity, NU, E_MOD, _component(quantity), planes=planes,
                                    sample_chunk=4)
    if quantity == "tresca":
        assert np.array_equal(res.max_abs, res.max) and np.all(res.min >= 0.0)
    run_and_check_tensor(sol, [1], samples_of(sol, (1,), 5, 6), quantity, NU, two_valued(mesh, 70.0, 210.0), _component(quantity),
                         planes=planes)


@pytest.mark.parametrize("planes", ["stored", "fused"])
@pytest.mark.parametrize("at", ["midpoint", "vertices"])
@pytest.mark.parametrize("quantity", QUANTITIES)
def test_host_path_p2(elastic_p2, quantity, at, planes):
    mesh, sol = elastic_p2
    run_and_check_tensor(sol, [1], samples_of(sol, (1,), 5, 5), quantity, NU, E_MOD, _component(quantity), at=at, planes=planes,
                         sample_chunk=3)
    run_and_check_tensor(sol, [1], samples_of(sol, (1,), 4, 6), quantity, NU, two_valued(mesh, 70.0, 210.0), _component(quantity), at=at,
                         planes=planes)


def test_signed_statistics_on_a_compressed_block(oracle):
    """u = -eps x: every principal stress is negative, so max |v| is |min|, not max."""
    mesh = fem.BoxMesh(P(0, 0, 0), P(1, 1, 1), 2, 2, 2)
    V = fem.VectorFunctionSpace(mesh, "CG", 1)
    X = mesh.coordinates()
    sol = one_mode_solution(mesh, V, np.stack([-EPS * X[:, 0], 0 * X[:, 0], 0 * X[:, 0]], axis=1))
    res = sol.evaluate_gradient_many(0, [1], [[0.5]], 0, quantity="max_principal", nu=NU, scale=E_MOD, envelope=True)
    tol = 1e-12 * E_MOD * EPS
    assert abs(res.max[0] + LAME * EPS) <= tol and abs(res.max_abs[0] - LAME * EPS) <= tol
    res = sol.evaluate_gradient_many(0, [1], [[0.5]], 0, quantity="min_principal", nu=NU, scale=E_MOD)
    assert abs(res.min[0] + (LAME + 2 * MU) * EPS) <= tol and abs(res.max_abs[0] - (LAME + 2 * MU) * EPS) <= tol
    res = sol.evaluate_gradient_many(0, [1], [[0.5]], 0, quantity="tresca", nu=NU, scale=E_MOD)
    assert abs(res.max[0] - 2 * MU * EPS) <= tol and np.array_equal(res.max_abs, res.max)
    res = sol.evaluate_gradient_many(0, [1], [[0.5]], 0, quantity="stress_component", nu=NU, scale=E_MOD, component=(0, 0))
    assert abs(res.max[0] + (LAME + 2 * MU) * EPS) <= tol


def test_refusals_and_the_cache(elastic_p1, oracle):
    mesh, sol = elastic_p1
    coords = samples_of(sol, (1,), 3, 1)
    for kw in [dict(quantity="max_principal"), dict(quantity="tresca", nu=0.5), dict(quantity="min_principal", nu=-1.5),
               dict(quantity="stress_component", nu=NU), dict(quantity="stress_component", nu=NU, component=(0, 3)),
               dict(quantity="von_mises", nu=NU), dict(quantity="gradient_norm", component=(0, 1)), dict(quantity="principal", nu=NU)]:
        with pytest.raises(ValueError):
            sol.evaluate_gradient_many(0, [1], coords, 0, **kw)
    # a scalar space has no stress
    ms = fem.BoxMesh(P(0, 0, 0), P(1, 1, 1), 2, 2, 2)
    Vs = fem.FunctionSpace(ms, "CG", 1)
    scalar = one_mode_solution(ms, Vs, np.arange(Vs.dim(), dtype=np.float64))
    with pytest.raises(ValueError, match="displacement"):
        scalar.evaluate_gradient_many(0, [1], [[0.5]], 0, quantity="max_principal", nu=NU)
    # nu and the component are part of what the cached planes were built from
    builds = lambda: fem.STATS.get("gradient_mode_builds", 0)
    a = sol.evaluate_gradient_many(0, [1], coords, 0, quantity="max_principal", nu=NU)
    n0 = builds()
    sol.evaluate_gradient_many(0, [1], coords, 0, quantity="max_principal", nu=NU)
    assert builds() == n0
    b = sol.evaluate_gradient_many(0, [1], coords, 0, quantity="max_principal", nu=0.2)
    assert builds() == n0 + 1 and not np.array_equal(a.max, b.max)
    sol.evaluate_gradient_many(0, [1], coords, 0, quantity="stress_component", nu=0.2, component=(0, 0))
    sol.evaluate_gradient_many(0, [1], coords, 0, quantity="stress_component", nu=0.2, component=(1, 1))
    assert builds() == n0 + 3
    # the old refusals at the vertices stay (P2 only: here the P1 one)
    with pytest.raises(ValueError, match="P1"):
        sol.evaluate_gradient_many(0, [1], coords, 0, quantity="tresca", nu=NU, at="vertices")


def test_vertices_refuse_threshold_and_fields(elastic_p2):
    mesh, sol = elastic_p2
    coords = samples_of(sol, (1,), 3, 1)
    for kw in (dict(threshold=0.0), dict(fields=True)):
        with pytest.raises(ValueError, match="vertices"):
            sol.evaluate_gradient_many(0, [1], coords, 0, quantity="max_principal", nu=NU, at="vertices", **kw)
