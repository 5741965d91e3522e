"""PGD.parameter_moments / quadratic_forms / variance_decomposition on the host route (oracle backend, no GPU) against the
tensor quadrature of tests/uq_reference.py, closed forms and the identities of the decomposition.  Every input is seeded.

Every tolerance against the quadrature is ``uq_reference.decomposition_bound`` (derived there), printed as max error / bound."""
import itertools

import numpy as np
import pytest

from oracle.backend_numpy import NumpyBackend
from pgdrome_amd import fem
from pgdrome_amd.model import PGD, variance_forms
from tests import uq_reference as R

U53 = 2.0 ** -53


@pytest.fixture(scope="module")
def oracle():
    old = fem._backend
    fem.set_backend(NumpyBackend())
    fem.clear_caches()
    yield
    fem.set_backend(old)
    fem.clear_caches()


def model(spaces, mats):
    """PGD whose dimension d has the columns of mats[d] (the order of Vector.host()) as modes on spaces[d]."""
    modes = []
    for V, F in zip(spaces, mats):
        modes.append([function(V, F[:, k]) for k in range(F.shape[1])])
    return PGD(name="synthetic", n_modes=mats[0].shape[1], fmeshes=[V.mesh() for V in spaces], pgd_modes=modes,
               name_coord=["x%d" % d for d in range(len(spaces))], modes_info=["U", "Node", "Scalar"])


def function(V, a):
    f = fem.Function(V)
    f.vector()._host = np.array(a, dtype=np.float64)
    f.vector().touched_host()
    return f


def interval_space(rng, cells, a, b, degree, uniform=False):
    x = np.linspace(a, b, cells + 1) if uniform else np.sort(np.concatenate([[a, b], rng.uniform(a, b, cells - 1)]))
    return fem.FunctionSpace(fem.Mesh(x.reshape(-1, 1), np.stack([np.arange(cells), np.arange(1, cells + 1)], axis=1)), "CG", degree)


def host(f):
    return f.vector().host()


def reference_moments(V, G, rho=None):
    w, Gq = R.dim_quadrature(V, G, rho)
    m = (Gq * w).sum(axis=1)
    A = Gq - m[:, None]
    mh, Aa = (np.abs(Gq) * w).sum(axis=1), np.abs(A)
    return m, (A * w) @ A.T, mh, (Aa * w) @ Aa.T


@pytest.mark.parametrize("degree", [1, 2])
@pytest.mark.parametrize("weighted", [False, True])
def test_parameter_moments_against_quadrature(oracle, degree, weighted):
    rng = np.random.default_rng(10 * degree + weighted)
    V = interval_space(rng, 9, -0.5, 2.0, degree)
    Vx = interval_space(rng, 4, 0.0, 1.0, 1)
    K, n = 5, V.dim()
    G = rng.standard_normal((n, K))
    sol = model([Vx, V], [rng.standard_normal((Vx.dim(), K)), G])
    rho = function(V, rng.uniform(0.1, 3.0, n)) if weighted else None
    m, C = sol.parameter_moments(1, density=rho)
    mr, Cr, mh, Ch = reference_moments(V, G, None if rho is None else host(rho))
    c = (n + 10) * U53
    em, eC = np.abs(m - mr) / (c * mh), np.abs(C - Cr) / (c * Ch)
    print("m: max error / bound", em.max(), " C:", eC.max())
    assert em.max() <= 1.0 and eC.max() <= 1.0 and np.array_equal(C, C.T)
    # a density given as an Expression or as a callable is interpolated to the same Function
    if weighted and degree == 1:
        e = fem.Expression("1.0 + x[0]*x[0]", degree=2)
        m1, C1 = sol.parameter_moments(1, density=e)
        m2, C2 = sol.parameter_moments(1, density=lambda x: 1.0 + x * x)
        m3, C3 = sol.parameter_moments(1, density=function(V, 1.0 + V._lay.coords[:, 0] ** 2))
        assert np.array_equal(m1, m3) and np.array_equal(C1, C3) and np.array_equal(m2, m3) and np.array_equal(C2, C3)
        # the normalisation: a multiple of the density changes nothing beyond rounding
        m4, C4 = sol.parameter_moments(1, density=function(V, 7.0 * (1.0 + V._lay.coords[:, 0] ** 2)))
        assert np.abs(m4 - m3).max() <= 4 * c * mh.max() and np.abs(C4 - C3).max() <= 4 * c * Ch.max()


def test_nearly_constant_modes_keep_their_variance(oracle):
    """Modes 1 + 1e-6 h: C holds a relative 1e-9 (the difference S - m m^T loses six digits more)."""
    rng = np.random.default_rng(3)
    V = interval_space(rng, 12, 0.0, 1.0, 2)
    Vx = interval_space(rng, 3, 0.0, 1.0, 1)
    K = 4
    G = 1.0 + 1e-6 * rng.standard_normal((V.dim(), K))
    sol = model([Vx, V], [np.ones((Vx.dim(), K)), G])
    m, C = sol.parameter_moments(1)
    mr, Cr, _, _ = reference_moments(V, G)
    scale = np.sqrt(np.outer(np.diag(Cr), np.diag(Cr)))
    rel = np.abs(C - Cr) / scale
    w, Gq = R.dim_quadrature(V, G)
    S = (Gq * w) @ Gq.T
    naive = np.abs((S.astype(np.float64) - np.outer(m, m)) - Cr) / scale
    print("centred: relative error", float(rel.max()), " uncentred S - m m^T in double:", float(naive.max()))
    assert rel.max() <= 1e-9
    assert naive.max() > 1e-6                     # what the requirement is about: this data separates the two formulas


@pytest.fixture(scope="module")
def three_parameters(oracle):
    rng = np.random.default_rng(1)
    K = 4
    Vx = interval_space(rng, 20, 0.0, 1.0, 1, uniform=True)
    Vs = [interval_space(rng, 6, 0.0, 1.0, 2), interval_space(rng, 5, -1.0, 2.0, 1), interval_space(rng, 4, 0.0, 3.0, 2)]
    mats = [rng.standard_normal((V.dim(), K)) for V in [Vx] + Vs]
    mats[0][[0, -1]] = 0.0                        # "Dirichlet nodes": every mode vanishes there
    rho = function(Vs[0], rng.uniform(0.2, 2.0, Vs[0].dim()))
    return model([Vx] + Vs, mats), Vx, Vs, mats, rho


def test_identities_of_the_forms(three_parameters):
    sol, Vx, Vs, mats, rho = three_parameters
    moments = {1: sol.parameter_moments(1, density=rho), 2: sol.parameter_moments(2), 3: sol.parameter_moments(3)}
    forms = variance_forms(moments, [1, 2, 3], order=2)
    C = {d: moments[d][1] for d in moments}
    M = {d: np.outer(moments[d][0], moments[d][0]) for d in moments}
    m = moments[1][0] * moments[2][0] * moments[3][0]
    full = (C[1] + M[1]) * (C[2] + M[2]) * (C[3] + M[3])
    size = np.abs(full).max()
    # all subsets: the third-order term is formed here
    subsets = dict(forms)
    subsets[(1, 2, 3)] = C[1] * C[2] * C[3]
    total = sum(subsets[B] for B in subsets if isinstance(B, tuple) and B[0] != "T")
    assert np.abs(total - forms["total"]).max() <= 16 * U53 * size
    assert np.abs(full - np.outer(m, m) - forms["total"]).max() <= 16 * U53 * size
    for i in (1, 2, 3):
        Ti = sum(subsets[B] for B in subsets if isinstance(B, tuple) and B[0] != "T" and i in B)
        assert np.abs(Ti - forms[("T", i)]).max() <= 16 * U53 * size
    for key, Q in subsets.items():
        assert np.array_equal(Q, Q.T), key
        lam = np.linalg.eigvalsh(Q)
        assert lam.min() >= -64 * U53 * max(lam.max(), 0.0) - 1e-300, (key, lam)


@pytest.mark.parametrize("case", ["all-random", "given-2", "given-1-and-3"])
def test_variance_decomposition_against_tensor_quadrature(three_parameters, case):
    sol, Vx, Vs, mats, rho = three_parameters
    given = {"all-random": {}, "given-2": {2: 0.37}, "given-1-and-3": {1: 0.61, 3: 2.2}}[case]
    densities = {} if 1 in given else {1: rho}
    res = sol.variance_decomposition(0, densities=densities, given=given, order=2)
    dims, ndofs = [], []
    for d in (1, 2, 3):
        if d in given:
            g = sol._free_modes_at(d, np.array([given[d]]), 0)[:, 0]
            dims.append(R.point_dimension(g))
            ndofs.append(0)
        else:
            dims.append(R.dim_quadrature(Vs[d - 1], mats[d], host(rho) if d == 1 else None))
            ndofs.append(Vs[d - 1].dim())
    ref = R.brute_force(mats[0], dims, order=2)
    bv, bm = R.decomposition_bound(mats[0], dims, ndofs)
    random = [d for d in (1, 2, 3) if d not in given]
    assert res.random == random and sorted(res.sobol) == sorted(
        [(i,) for i in random] + list(itertools.combinations(random, 2))) and sorted(res.total) == random
    worst = {"mean": (np.abs(host(res.mean) - ref["mean"])[1:-1] / bm[1:-1]).max(),
             "total": (np.abs(host(res.variance) - ref["total"])[1:-1] / bv[1:-1]).max()}
    for k, f in res.partial.items():
        worst[k] = (np.abs(host(f) - ref[tuple(i - 1 for i in k)])[1:-1] / bv[1:-1]).max()
    for i, f in res.partial_total.items():
        worst[("T", i)] = (np.abs(host(f) - ref[("T", i - 1)])[1:-1] / bv[1:-1]).max()
    print(case, "max error / bound:", {k: float(v) for k, v in worst.items()})
    assert max(worst.values()) <= 1.0
    V = host(res.variance)
    assert res.variance_min == V.min() == 0.0 and res.variance_max == V.max() and np.all(V >= 0.0)
    assert np.array_equal(host(res.std), np.sqrt(V))
    # ratio fields: the quotient of the two fields above the floor, exactly 0 at and below it (the two end nodes)
    assert res.floor == 1e-12 * res.variance_max
    for k, f in list(res.sobol.items()) + [(("T", i), f) for i, f in res.total.items()]:
        num = host(res.partial_total[k[1]] if k[0] == "T" else res.partial[k])
        above = V > res.floor
        assert above[1:-1].all() and not above[0] and not above[-1]
        assert np.array_equal(host(f)[above], num[above] / V[above]) and host(f)[0] == 0.0 == host(f)[-1]
    # the global indices: ratios of the integrals over the body (P1 on a uniform mesh: the integrand is piecewise of degree 2 in F)
    wq, Fq = R.dim_quadrature(Vx, mats[0])
    refq = R.brute_force(Fq.T, dims, order=2)
    bq, _ = R.decomposition_bound(Fq.T.astype(np.float64), dims, ndofs)
    tot = float((wq * refq["total"]).sum())
    slack = float((wq * bq).sum()) * (1.0 + (Vx.dim() + 10))       # the mass Gram of the fixed modes: n + 10 roundings more
    assert abs(res.global_variance - tot * 1.0) <= slack            # |body| = 1
    for k, s in res.global_sobol.items():
        want = float((wq * refq[tuple(i - 1 for i in k)]).sum()) / tot
        assert abs(s - want) <= 2 * slack / tot, (k, s, want)
    for i, s in res.global_total.items():
        want = float((wq * refq[("T", i - 1)]).sum()) / tot
        assert abs(s - want) <= 2 * slack / tot, (i, s, want)
    # fields=False: the same numbers, no field
    lean = sol.variance_decomposition(0, densities=densities, given=given, order=2, fields=False)
    assert lean.mean is None and lean.variance is None and lean.std is None and not lean.sobol and not lean.total
    assert (lean.variance_min, lean.variance_max) == (res.variance_min, res.variance_max)
    assert lean.global_sobol == res.global_sobol and lean.global_total == res.global_total and lean.extrema == res.extrema


def product_model(rng, a, split=True):
    """u = f(x) prod_d (1 + a_d mu_d) on [-1, 1]^P, written with two modes f = f' + f''."""
    Vx = interval_space(rng, 15, 0.0, 1.0, 1)
    Vs = [interval_space(rng, 4 + d, -1.0, 1.0, 1 + d % 2) for d in range(len(a))]
    f = rng.standard_normal(Vx.dim())
    f1 = rng.standard_normal(Vx.dim())
    mats = [np.stack([f1, f - f1], axis=1)] + [np.stack([1.0 + ad * V._lay.coords[:, 0]] * 2, axis=1) for ad, V in zip(a, Vs)]
    return model([Vx] + Vs, mats), f, mats, Vs


def test_product_function_has_its_closed_form_indices(oracle):
    rng = np.random.default_rng(5)
    a = [0.9, -0.4, 0.25]
    sol, f, mats, Vs = product_model(rng, a)
    res = sol.variance_decomposition(0, order=2)
    v = [ad * ad / 3.0 for ad in a]
    dims = [R.dim_quadrature(V, G) for V, G in zip(Vs, mats[1:])]
    bv, bm = R.decomposition_bound(mats[0], dims, [V.dim() for V in Vs])
    worst = {"mean": (np.abs(host(res.mean) - f) / bm).max(),
             "total": (np.abs(host(res.variance) - f * f * (np.prod([1.0 + vd for vd in v]) - 1.0)) / bv).max()}
    for B, field in res.partial.items():
        worst[B] = (np.abs(host(field) - f * f * np.prod([v[d - 1] for d in B])) / bv).max()
    for i, field in res.partial_total.items():
        worst[("T", i)] = (np.abs(host(field) - f * f * v[i - 1] * np.prod([1.0 + v[d] for d in range(3) if d != i - 1])) / bv).max()
    print("max error / bound:", {k: float(x) for k, x in worst.items()})
    assert max(worst.values()) <= 1.0
    # the index fields do not depend on x; the global ones are the same numbers
    tot = np.prod([1.0 + vd for vd in v]) - 1.0
    for B, s in res.global_sobol.items():
        assert abs(s - np.prod([v[d - 1] for d in B]) / tot) <= 1e-13


def test_additive_model_has_no_interactions(oracle):
    rng = np.random.default_rng(6)
    Vx = interval_space(rng, 15, 0.0, 1.0, 2)
    Vs = [interval_space(rng, 5, 0.0, 1.0, 1), interval_space(rng, 6, -1.0, 1.0, 2), interval_space(rng, 4, 0.0, 2.0, 1)]
    F = rng.standard_normal((Vx.dim(), 4))                       # u = f_0 + sum_d f_d g_d(mu_d)
    mats = [F]
    for d, V in enumerate(Vs):
        G = np.ones((V.dim(), 4))
        G[:, d + 1] = rng.standard_normal(V.dim())
        mats.append(G)
    sol = model([Vx] + Vs, mats)
    res = sol.variance_decomposition(0, order=2)
    dims = [R.dim_quadrature(V, G) for V, G in zip(Vs, mats[1:])]
    bv, _ = R.decomposition_bound(F, dims, [V.dim() for V in Vs])
    V = host(res.variance)
    for B in itertools.combinations((1, 2, 3), 2):
        print(B, "max interaction / bound", (np.abs(host(res.partial[B])) / bv).max())
        assert np.all(np.abs(host(res.partial[B])) <= bv)
    first = sum(host(res.partial[(i,)]) for i in (1, 2, 3))
    assert np.all(np.abs(first - V) <= 4 * bv)
    above = V > res.floor
    assert above.all()
    s = sum(host(res.sobol[(i,)]) for i in (1, 2, 3))
    print("max |sum S_i - 1| V / bound", (np.abs(s - 1.0) * V / (4 * bv + 4 * U53 * V)).max())
    assert np.all(np.abs(s - 1.0) * V <= 4 * bv + 4 * U53 * V)   # three quotients, one rounding each, and their sum
    for i in (1, 2, 3):                                          # total effect = first order
        assert np.all(np.abs(host(res.partial_total[i]) - host(res.partial[(i,)])) <= 2 * bv)
    assert abs(sum(res.global_sobol[(i,)] for i in (1, 2, 3)) - 1.0) <= 1e-12


def test_one_parameter_has_index_one(oracle):
    rng = np.random.default_rng(8)
    Vx, Vp = interval_space(rng, 30, 0.0, 1.0, 1), interval_space(rng, 7, 0.0, 1.0, 2)
    F = rng.standard_normal((Vx.dim(), 3))
    F[:5] = 0.0
    sol = model([Vx, Vp], [F, rng.standard_normal((Vp.dim(), 3))])
    res = sol.variance_decomposition(0)
    V = host(res.variance)
    above = V > res.floor
    assert above[5:].all() and not above[:5].any()
    for f in (res.sobol[(1,)], res.total[1]):
        assert np.array_equal(host(f)[above], np.ones(above.sum())) and np.all(host(f)[~above] == 0.0)
    assert res.global_sobol == {(1,): 1.0} and res.global_total == {1: 1.0}


def test_quadratic_forms_on_the_host(oracle):
    rng = np.random.default_rng(9)
    Vx, Vp = interval_space(rng, 40, 0.0, 1.0, 1), interval_space(rng, 3, 0.0, 1.0, 1)
    K = 5
    F = rng.standard_normal((Vx.dim(), K))
    sol = model([Vx, Vp], [F, rng.standard_normal((Vp.dim(), K))])
    Q = rng.standard_normal((70, K, K))                          # not symmetric, more than 64
    fs, mn, mx = sol.quadratic_forms(0, Q, row_chunk=7)
    exact, B = R.quad_exact(F, Q), R.scale(F, Q)
    got = np.stack([host(f) for f in fs])
    ratio = np.abs(got - exact) / R.bound(K, B)
    print("max error / bound", float(ratio.max()))
    assert ratio.max() <= 1.0
    assert np.array_equal(mn, got.min(axis=1)) and np.array_equal(mx, got.max(axis=1))
    fs1, mn1, mx1 = sol.quadratic_forms(0, Q[3], clamp=True)
    assert len(fs1) == 1 and np.array_equal(host(fs1[0]), np.maximum(got[3], 0.0)) and mn1[0] == max(mn[3], 0.0)
    none, mn2, mx2 = sol.quadratic_forms(0, Q, fields=False)
    assert none is None and np.array_equal(mn2, mn) and np.array_equal(mx2, mx)


def test_refusals(oracle):
    rng = np.random.default_rng(11)
    Vx, Vp, Vq = interval_space(rng, 8, 0.0, 1.0, 1), interval_space(rng, 5, 0.0, 1.0, 1), interval_space(rng, 4, 0.0, 1.0, 2)
    K = 3
    sol = model([Vx, Vp, Vq], [rng.standard_normal((V.dim(), K)) for V in (Vx, Vp, Vq)])
    with pytest.raises(ValueError, match="negative"):
        sol.parameter_moments(1, density=function(Vp, np.array([1.0, 1.0, -1e-3, 1.0, 1.0, 1.0])))
    with pytest.raises(ValueError, match="positive integral"):
        sol.parameter_moments(1, density=function(Vp, np.zeros(Vp.dim())))
    with pytest.raises(ValueError, match="another space"):
        sol.parameter_moments(1, density=function(Vq, np.ones(Vq.dim())))
    with pytest.raises(ValueError, match="density must be"):
        sol.parameter_moments(1, density=3.0)
    with pytest.raises(ValueError, match="a value and a density"):
        sol.parameter_moments(1, density=lambda x: 1.0, given=0.5)
    with pytest.raises(ValueError, match="outside the mesh"):
        sol.parameter_moments(1, given=1.5)
    with pytest.raises(ValueError):
        sol.parameter_moments(7)
    m, C = sol.parameter_moments(2, given=0.3)
    assert np.array_equal(C, np.zeros((K, K))) and np.array_equal(m, sol._free_modes_at(2, np.array([0.3]), 0)[:, 0])
    with pytest.raises(ValueError, match="no random dimension"):
        sol.variance_decomposition(0, given={1: 0.5, 2: 0.5})
    with pytest.raises(ValueError, match="order"):
        sol.variance_decomposition(0, order=3)
    with pytest.raises(ValueError, match="names dimension"):
        sol.variance_decomposition(0, given={0: 0.5})
    with pytest.raises(ValueError, match="names dimension"):
        sol.variance_decomposition(0, densities={5: None})
    with pytest.raises(ValueError, match="a value and a density"):
        sol.variance_decomposition(0, densities={1: lambda x: 1.0}, given={1: 0.5})
    with pytest.raises(ValueError, match="not possible"):
        sol.variance_decomposition(3)
    with pytest.raises(ValueError, match="variance_floor"):
        sol.variance_decomposition(0, variance_floor=-1.0)
    with pytest.raises(ValueError, match="shape"):
        sol.quadratic_forms(0, np.zeros((2, K, K + 1)))
    with pytest.raises(ValueError, match="not finite"):
        sol.quadratic_forms(0, np.full((K, K), np.nan))
    # interp1d modes, a vector-valued parameter space, a row-sharded dimension
    att = sol.mesh[1].attributes[0]
    sol._gram_family(1, 0)
    att.interpolationInfo["name"] = 0
    try:
        with pytest.raises(NotImplementedError, match="interp1d"):
            sol.parameter_moments(1)
        with pytest.raises(NotImplementedError, match="interp1d"):
            sol.variance_decomposition(0)
    finally:
        att.interpolationInfo["name"] = 1
    Vp.mesh().part = object()
    try:
        with pytest.raises(NotImplementedError, match="row-sharded"):
            sol.parameter_moments(1)
    finally:
        Vp.mesh().part = None
    Vv = fem.VectorFunctionSpace(fem.UnitSquareMesh(2, 2), "CG", 1)
    vec = model([Vx, Vv], [rng.standard_normal((Vx.dim(), 2)), rng.standard_normal((Vv.dim(), 2))])
    with pytest.raises(NotImplementedError, match="vector-valued"):
        vec.parameter_moments(1)
    with pytest.raises(NotImplementedError, match="vector-valued"):
        vec.variance_decomposition(0)
