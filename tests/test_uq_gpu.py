"""PGD.variance_decomposition through the frontend on the MI355X: the fixed dimension just above DEVICE_EVAL_MIN_DOFS, so the
forms run in pgd_quad_forms, the ratio fields in pgd_vec_ratio and the mean in pgd_eval_batch; the same call through the numpy
route (DEVICE_EVAL_MIN_DOFS raised out of reach) beside it.  The Q matrices of both routes are the same K x K host arithmetic
on the same moments (the parameter dimensions have 33 and 17 nodes: numpy either way), so both routes are held to the derived
bound of tests/uq_reference.py around the longdouble values of those forms."""
import numpy as np
import pytest

from pgdrome_amd import fem, model
from pgdrome_amd.model import PGD
from tests import uq_reference as R

pytestmark = pytest.mark.gpu

U53 = 2.0 ** -53


@pytest.fixture(scope="module")
def hip():
    from pgdrome_amd.hip_backend import HipBackend
    old = fem._backend
    fem.set_backend(HipBackend(0))
    fem.clear_caches()
    yield
    fem.set_backend(old)
    fem.clear_caches()


def synthetic(V, Vps, seed):
    """12 seeded modes on the fixed space and on the two parameter spaces; every fixed mode vanishes at the first 100 dofs."""
    rng = np.random.default_rng(seed)
    K = 12
    modes, mats = [], []
    for i, W in enumerate([V] + list(Vps)):
        F = rng.standard_normal((W.dim(), K)) * (1.0 if i == 0 else 0.5) + (0.0 if i == 0 else 1.0)
        if i == 0:
            F[:100] = 0.0
        fs = []
        for k in range(K):
            f = fem.Function(W)
            f.vector()._host = np.ascontiguousarray(F[:, k])
            f.vector().touched_host()
            fs.append(f)
        modes.append(fs)
        mats.append(F)
    sol = PGD(name="synthetic", n_modes=K, fmeshes=[W.mesh() for W in [V] + list(Vps)], pgd_modes=modes, name_coord=["x", "p", "q"],
              modes_info=["U", "Node", "Vector" if V._ncomp > 1 else "Scalar"])
    return sol, mats


def host(f):
    return f.vector().host()


@pytest.mark.parametrize("space", ["scalar-41", "vector-29"])
def test_variance_decomposition_on_the_device_and_in_numpy(hip, monkeypatch, space):
    if space == "scalar-41":
        V = fem.FunctionSpace(fem.BoxMesh(fem.Point(0, 0, 0), fem.Point(1, 1, 1), 40, 40, 40), "CG", 1)
        assert V.dim() == 68921
    else:
        V = fem.VectorFunctionSpace(fem.BoxMesh(fem.Point(0, 0, 0), fem.Point(1, 1, 1), 28, 28, 28), "CG", 1)
        assert V.dim() == 3 * 24389
    assert V.dim() >= model.DEVICE_EVAL_MIN_DOFS
    Vps = [fem.FunctionSpace(fem.IntervalMesh(32, 0.0, 1.0), "CG", 1), fem.FunctionSpace(fem.IntervalMesh(16, -1.0, 1.0), "CG", 1)]
    sol, mats = synthetic(V, Vps, 41 if space == "scalar-41" else 29)
    rho = lambda x: 1.0 + 0.5 * x

    calls, batches = fem.STATS.get("quad_forms_calls", 0), fem.STATS.get("compress_eval_batch_calls", 0)
    dev = sol.variance_decomposition(0, densities={1: rho}, order=2)
    assert fem.STATS.get("quad_forms_calls", 0) == calls + 1                    # all seven forms in one call
    assert fem.STATS.get("compress_eval_batch_calls", 0) == batches + 1         # the mean
    lean = sol.variance_decomposition(0, densities={1: rho}, order=2, fields=False)
    assert fem.STATS.get("quad_forms_calls", 0) == calls + 2
    with monkeypatch.context() as m:
        m.setattr(model, "DEVICE_EVAL_MIN_DOFS", 1 << 40)
        calls = fem.STATS.get("quad_forms_calls", 0)
        ref = sol.variance_decomposition(0, densities={1: rho}, order=2)
        assert fem.STATS.get("quad_forms_calls", 0) == calls

    keys = list(dev.forms)
    assert keys == list(ref.forms) == ["total", (1,), (2,), (1, 2), ("T", 1), ("T", 2)]
    assert all(np.array_equal(dev.forms[k], ref.forms[k]) for k in keys)         # the same host arithmetic
    Q = np.stack([dev.forms[k] for k in keys])
    F = mats[0]
    exact = np.maximum(R.quad_exact(F, Q), 0.0)                                   # (every form is PSD; the routes clamp)
    tol = R.bound(F.shape[1], R.scale(F, Q))
    field = lambda res, k: res.variance if k == "total" else res.partial_total[k[1]] if k[0] == "T" else res.partial[k]
    for name, res in (("device", dev), ("numpy", ref)):
        worst = {}
        for i, k in enumerate(keys):
            got = host(field(res, k))
            worst[k] = float((np.abs(got - exact[i])[100:] / tol[i][100:]).max())
            assert np.all(got[:100] == 0.0) and np.all(got >= 0.0)
            assert res.extrema[k] == (got.min(), got.max())
        print(name, "max error / bound:", worst)
        assert max(worst.values()) <= 1.0
        assert res.variance_min == 0.0 and res.variance_max == host(res.variance).max()
    assert lean.extrema == dev.extrema and lean.variance is None and not lean.sobol
    assert abs(dev.floor - ref.floor) <= tol[0].max() * 1e-12

    # ratio fields: S = A / V with |dA| <= tA, |dV| <= tV gives |dS| <= (tA + S tV) / (V - tV) and one rounding of the quotient;
    # zero at the dofs where every mode vanishes
    Vx, tV = exact[0].astype(np.float64), tol[0]
    above = Vx > 2.0 * max(dev.floor, ref.floor)
    assert above[100:].all() and not above[:100].any()
    for i, k in enumerate(keys[1:], start=1):
        S = (exact[i] / np.where(above, exact[0], 1.0)).astype(np.float64)
        tS = (tol[i] + S * tV) / np.where(above, Vx - tV, 1.0) + 2 * U53 * S
        for name, res in (("device", dev), ("numpy", ref)):
            got = host(res.total[k[1]] if k[0] == "T" else res.sobol[k])
            ratio = (np.abs(got - S)[above] / tS[above]).max()
            print(name, k, "ratio field: max error / bound", float(ratio))
            assert ratio <= 1.0 and np.all(got[~above] == 0.0)
        # the device's quotient is the correctly rounded one of its own two fields
        a, v = host(field(dev, k)), host(dev.variance)
        ok = v > dev.floor
        assert np.array_equal(host(dev.total[k[1]] if k[0] == "T" else dev.sobol[k])[ok], a[ok] / v[ok])

    # the mean, and the global numbers (mass Gram from pgd_vec_gram on one side, numpy on the other)
    mtol = (F.shape[1] + 2) * U53 * (np.abs(F) @ np.abs(dev.mean_coefficients))
    assert np.all(np.abs(host(dev.mean) - host(ref.mean)) <= 2 * mtol)
    assert abs(dev.global_variance - ref.global_variance) <= 1e-12 * ref.global_variance
    for k in ref.global_sobol:
        assert abs(dev.global_sobol[k] - ref.global_sobol[k]) <= 1e-12
    for i in ref.global_total:
        assert abs(dev.global_total[i] - ref.global_total[i]) <= 1e-12
