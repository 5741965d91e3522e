"""PGD.mode_gram / separated_norm / distance / evaluate_norm_many / compress on the host route (oracle backend, no GPU): against
dense reconstructions, np.linalg.svd and the restatement of tests/gram_reference.py.  Every input is seeded.

Tolerances: the Gram route resolves a component to sqrt(2^-53) |u| = 1.05e-8 |u| (the squares carry 2^-53), so errors and
distances are compared to 1e-8 |u| where both sides come from Grams, and to the 1e-7 |u| the interface documents where one
side is dense."""
import os

import numpy as np
import pytest

from oracle.backend_numpy import NumpyBackend
from pgdrome_amd import fem
from pgdrome_amd.model import PGD, compress_grams
from tests.gram_reference import compress_reference, dense_field


@pytest.fixture(scope="module")
def oracle():
    old = fem._backend
    fem.set_backend(NumpyBackend())
    fem.clear_caches()
    yield
    fem.set_backend(old)
    fem.clear_caches()


def model(spaces, mats, name="synthetic"):
    """PGD whose dimension d has the columns of mats[d] (vertex order, as Vector.host()) as modes on spaces[d]."""
    modes = []
    for V, F in zip(spaces, mats):
        fs = []
        for k in range(F.shape[1]):
            f = fem.Function(V)
            f.vector()._host = np.array(F[:, k], dtype=np.float64)
            f.vector().touched_host()
            fs.append(f)
        modes.append(fs)
    return PGD(name=name, n_modes=mats[0].shape[1], fmeshes=[V.mesh() for V in spaces], pgd_modes=modes,
               name_coord=["x%d" % d for d in range(len(spaces))], modes_info=["U", "Node", "Scalar"])


def host_modes(sol, attri=0):
    return [np.stack([f.vector().host() for f in pm.attributes[attri].interpolationfct[:sol.used_numModes]], axis=1) for pm in sol.mesh]


def interval_spaces(sizes, degree=1):
    return [fem.FunctionSpace(fem.IntervalMesh(n - 1, 0.0, 1.0 + d), "CG", degree) for d, n in enumerate(sizes)]


@pytest.fixture(scope="module")
def two_dims(oracle):
    """u = Q1 diag(w) Q2^T with w_k = 10^(-0.7 k), written with 10 non-orthogonal modes per dimension (F1 = Q1 A, F2 = Q2 diag(w) A^-T)."""
    rng = np.random.default_rng(7)
    K = 10
    Q1, Q2 = np.linalg.qr(rng.standard_normal((200, K)))[0], np.linalg.qr(rng.standard_normal((60, K)))[0]
    w = 10.0 ** (-0.7 * np.arange(K))
    A = np.eye(K) + 0.3 * rng.standard_normal((K, K))
    F1, F2 = Q1 @ A, (Q2 * w) @ np.linalg.inv(A).T
    spaces = interval_spaces([200, 60])
    return model(spaces, [F1, F2]), F1 @ F2.T, spaces


def test_two_dimensions_are_the_optimal_truncation(two_dims):
    sol, U, _ = two_dims
    sv = np.linalg.svd(U, compute_uv=False)
    tails = np.sqrt(np.concatenate([np.cumsum((sv ** 2)[::-1])[::-1], [0.0]])) / np.linalg.norm(sv)
    tol = 1e-4
    R = int(np.argmax(tails <= tol))
    assert 1 < R < 10 and tails[R] < 0.7 * tol < 0.7 * tails[R - 1]          # the data decides, not the rounding
    res = sol.compress(tol=tol)
    info = res.compression
    print("R", R, "rel_error", info["rel_error"], "svd tail", tails[R], "ranks", info["ranks"])
    assert info["modes_in"] == 10 and info["modes_out"] == R == res.numModes == res.used_numModes
    assert info["converged"] and info["metric"] == "l2" and info["tol"] == tol and info["ranks"] == [10, 10]
    assert abs(info["rel_error"] - tails[R]) <= 1e-8
    F1, F2 = host_modes(res)
    assert F1.shape == (200, R) and F2.shape == (60, R)
    assert np.linalg.norm(F1 @ F2.T - U) <= (tol + 1e-7) * np.linalg.norm(U)
    # balanced, ordered, signed
    n1, n2 = np.linalg.norm(F1, axis=0), np.linalg.norm(F2, axis=0)
    assert np.allclose(n1, n2, rtol=1e-6) and np.all(np.diff(n1 * n2) <= 0)
    assert all(F2[np.argmax(np.abs(F2[:, i])), i] > 0 for i in range(R))
    # the original is untouched, the result owns its modes
    assert sol.numModes == 10 and np.array_equal(host_modes(sol)[0] @ host_modes(sol)[1].T, U)
    # minimal: one mode fewer misses tol by exactly the Eckart-Young tail
    less = sol.compress(tol=tol, max_modes=R - 1)
    assert less.compression["modes_out"] == R - 1 and not less.compression["converged"]
    assert abs(less.compression["rel_error"] - tails[R - 1]) <= 1e-8
    G1, G2 = host_modes(less)
    assert abs(np.linalg.norm(G1 @ G2.T - U) / np.linalg.norm(U) - tails[R - 1]) <= 1e-7
    # the restatement on the same Grams agrees
    ref = compress_reference([sol.mode_gram(0), sol.mode_gram(1)], tol)
    assert ref["R"] == R and abs(ref["rel_error"] - info["rel_error"]) <= 1e-8
    W1, W2 = ref["W"]
    assert np.linalg.norm((host_modes(sol)[0] @ W1) @ (host_modes(sol)[1] @ W2).T - F1 @ F2.T) <= 1e-7 * np.linalg.norm(U)


def split_terms(rng, sizes):
    """8 terms in three dimensions from 3 rank-one terms: a factor of each is split as f = f' + f'' (+ f''')."""
    base = [[rng.standard_normal(n) for n in sizes] for _ in range(3)]
    terms = []
    for t, (vecs, parts) in enumerate(zip(base, (3, 3, 2))):
        cuts = rng.standard_normal((parts - 1, sizes[t]))
        pieces = list(cuts) + [vecs[t] - cuts.sum(axis=0)]
        for p in pieces:
            terms.append([p if d == t else vecs[d] for d in range(3)])
    return [np.stack([term[d] for term in terms], axis=1) for d in range(3)], base


def test_three_dimensions_recover_the_split_terms(oracle):
    rng = np.random.default_rng(3)
    sizes = [30, 20, 15]
    mats, _ = split_terms(rng, sizes)
    assert mats[0].shape == (30, 8)
    U = dense_field(mats)
    sol = model(interval_spaces(sizes), mats)
    Gs = [sol.mode_gram(d) for d in range(3)]
    ref = compress_reference(Gs, 1e-6)                       # the seed is one at which the restatement itself gets there
    Uref = dense_field([F @ W for F, W in zip(mats, ref["W"])])
    print("reference: R", ref["R"], "rel_error", ref["rel_error"], "dense", np.linalg.norm(Uref - U) / np.linalg.norm(U))
    assert ref["R"] <= 3 and np.linalg.norm(Uref - U) <= 2e-6 * np.linalg.norm(U)
    res = sol.compress(tol=1e-6)
    info = res.compression
    dense = np.linalg.norm(dense_field(host_modes(res)) - U) / np.linalg.norm(U)
    print("compress: R", info["modes_out"], "rel_error", info["rel_error"], "dense", dense, "sweeps", info["sweeps"])
    assert info["modes_out"] <= 3 and info["converged"] and info["modes_in"] == 8
    assert dense <= 2e-6
    assert info["ranks"] == [5, 5, 4]                        # the spans: 3 + 2 split pieces, 3 + 2, 3 + 1
    assert sol.distance(res) <= 1e-6 + 1e-7
    plan = compress_grams(Gs, 1e-6)                          # the host half alone: the same plan
    assert plan["R"] == info["modes_out"] and plan["rel_error"] == info["rel_error"]


def test_incompressible_input_comes_back_unchanged(oracle):
    rng = np.random.default_rng(3)
    K = 6
    mats = [np.linalg.qr(rng.standard_normal((n, K)))[0] for n in (40, 30)]
    sol = model(interval_spaces([40, 30]), mats)
    res = sol.compress(tol=1e-3)
    assert res.compression["modes_out"] == K == res.numModes and res.compression["rel_error"] == 0.0 and res.compression["converged"]
    for a, b in zip(host_modes(res), mats):
        assert np.array_equal(a, b)
    assert res.mesh[0].attributes[0].interpolationfct[0] is not sol.mesh[0].attributes[0].interpolationfct[0]
    # asked for fewer modes anyway: the best of that rank, and it says that tol was missed
    forced = sol.compress(tol=1e-3, max_modes=4)
    assert forced.compression["modes_out"] == 4 and not forced.compression["converged"]
    assert abs(forced.compression["rel_error"] - np.sqrt(2.0 / 6.0)) <= 1e-8


def test_norms_and_distances_equal_the_dense_values(two_dims):
    sol, U, spaces = two_dims
    rng = np.random.default_rng(17)
    other = model(spaces, [rng.standard_normal((200, 4)), rng.standard_normal((60, 4))], name="other")
    V = dense_field(host_modes(other))
    assert abs(sol.separated_norm() - np.linalg.norm(U)) <= 1e-12 * np.linalg.norm(U)
    assert sol.distance(sol) <= 1e-7
    same = model(spaces, host_modes(sol))
    assert sol.distance(same) <= 1e-7
    dense = np.linalg.norm(U - V)
    assert abs(sol.distance(other, relative=False) - dense) <= 1e-7 * np.linalg.norm(U)
    assert abs(sol.distance(other) - dense / np.linalg.norm(U)) <= 1e-7
    # a small known difference: one mode perturbed by 1e-4 of the field
    mats = host_modes(sol)
    mats[0] = mats[0].copy()
    mats[0][:, 0] += 1e-4 * np.linalg.norm(U) * rng.standard_normal(200) / np.linalg.norm(mats[1][:, 0])
    near = model(spaces, mats)
    assert abs(sol.distance(near) - np.linalg.norm(dense_field(mats) - U) / np.linalg.norm(U)) <= 1e-7
    G = sol.mode_gram(0, other=other)
    assert G.shape == (10, 4) and np.allclose(G, host_modes(sol)[0].T @ host_modes(other)[0], rtol=0, atol=1e-13 * np.abs(G).max())


def test_evaluate_norm_many_equals_the_norms_of_the_fields(two_dims):
    sol, _, _ = two_dims
    coords = np.random.default_rng(2).uniform(0.0, 2.0, size=(23, 1))
    res = sol.evaluate_many(0, [1], coords, 0, fields=True)
    want = np.array([np.linalg.norm(f.vector().host()) for f in res.fields])
    got = sol.evaluate_norm_many(0, [1], coords, 0)
    assert got.shape == (23,) and np.all(np.abs(got - want) <= 1e-12 * want.max())


@pytest.mark.parametrize("degree", [1, 2])
def test_mass_metric_on_an_interval(oracle, degree):
    rng = np.random.default_rng(degree)
    spaces = [fem.FunctionSpace(fem.IntervalMesh(24, 0.0, 3.0), "CG", degree), fem.FunctionSpace(fem.IntervalMesh(11, -1.0, 1.0), "CG", 1)]
    sol = model(spaces, [rng.standard_normal((V.dim(), 5)) for V in spaces])
    for d, V in enumerate(spaces):
        u, v = fem.TrialFunction(V), fem.TestFunction(V)
        M = fem.assemble(u * v * fem.dx).array()
        F = np.stack([f.vector().get_local() for f in sol.mesh[d].attributes[0].interpolationfct], axis=1)       # dof order, as M
        G = sol.mode_gram(d, metric="mass")
        assert np.array_equal(G, G.T) and np.all(np.abs(G - F.T @ M @ F) <= 1e-12 * np.abs(G).max())
    # the L2 norm of the separated function is the product structure's: prod_d of 1-D integrals, term by term
    assert sol.separated_norm(metric="mass") > 0.0
    res = sol.compress(tol=1e-6, metric="mass")
    assert res.compression["metric"] == "mass" and sol.distance(res, metric="mass") <= 1e-6 + 1e-7


def test_refusals(two_dims, monkeypatch):
    sol, _, spaces = two_dims
    with pytest.raises(ValueError, match="half the digits"):
        sol.compress(tol=1e-8)
    with pytest.raises(ValueError):
        sol.compress(max_modes=0)
    for call in (lambda: sol.compress(metric="h1"), lambda: sol.mode_gram(0, metric="h1"), lambda: sol.distance(sol, metric="h1"),
                 lambda: sol.separated_norm(metric="h1"), lambda: sol.evaluate_norm_many(0, [1], [[0.5]], 0, metric="h1")):
        with pytest.raises(ValueError):
            call()
    rng = np.random.default_rng(1)
    elsewhere = model(interval_spaces([200, 61]), [rng.standard_normal((200, 3)), rng.standard_normal((61, 3))])
    with pytest.raises(ValueError, match="different spaces"):
        sol.mode_gram(1, other=elsewhere)
    with pytest.raises(ValueError, match="different spaces"):
        sol.distance(elsewhere)
    # interp1d modes
    arrays = model(spaces, host_modes(sol))
    arrays.mesh[1].attributes[0].interpolationInfo = {"name": 0, "kind": "linear"}
    for call in (lambda: arrays.compress(), lambda: arrays.mode_gram(1), lambda: arrays.separated_norm(), lambda: sol.distance(arrays)):
        with pytest.raises(NotImplementedError):
            call()
    # a row-sharded dimension
    monkeypatch.setattr(spaces[0].mesh(), "part", fem.Partition(None, 0, 8, 16, 0, 1, 0), raising=False)
    for call in (lambda: sol.compress(), lambda: sol.mode_gram(0), lambda: sol.separated_norm(), lambda: sol.distance(sol),
                 lambda: sol.evaluate_norm_many(0, [1], [[0.5]], 0)):
        with pytest.raises(NotImplementedError, match="row-sharded"):
            call()


def test_compressed_model_survives_its_result_files(two_dims, tmp_path):
    sol, _, _ = two_dims
    res = sol.compress(tol=1e-5)
    folder = str(tmp_path)
    res.write_pxdmf(folder)
    res.write_hdf5(folder)
    back = PGD().load_pxdmf(os.path.join(folder, "synthetic.pxdmf"))
    assert back.numModes == res.numModes
    for d in (0, 1):
        back.mesh[d].attributes[0].interpolationInfo = {"name": 1, "family": "CG", "degree": 1, "_type": "scalar"}
    u, v, w = (m.evaluate(0, [1], [0.6], 0) for m in (back, res, sol))
    scale = np.abs(w.vector().host()).max()
    assert np.abs(u.vector().get_local() - v.vector().get_local()).max() <= 1e-12 * scale
    assert np.abs(v.vector().host() - w.vector().host()).max() <= 1e-4 * scale
    # and the other online calls take it as any model
    many = res.evaluate_many(0, [1], [[0.6], [1.2]], 0, fields=True)
    assert np.array_equal(many.fields[0].vector().host(), v.vector().host()) or \
        np.abs(many.fields[0].vector().host() - v.vector().host()).max() <= 1e-13 * scale
