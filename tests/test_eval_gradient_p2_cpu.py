"""PGD.evaluate_gradient_many on P2 modes, host path (oracle backend, no GPU): the restatement of
tests/eval_gradient_p2_reference.py against analytic gradients and fem.point_gradient, then the frontend with at="midpoint" and
at="vertices" inside the derived bounds around a loop over PGD.evaluate, the peak property of the vertex values, the refusals and
the cache."""
import math

import numpy as np
import pytest

from pgdrome_amd import fem, problems
from pgdrome_amd.solver import PGDProblem
from tests.eval_gradient_p2_reference import planes_p2, point_gradients, run_and_check_p2, shape_values
from tests.eval_gradient_reference import LD, samples_of, two_valued
from tests.test_eval_gradient_cpu import E_MOD, MU, NU, one_mode_solution, oracle  # noqa: F401  (oracle: the fixture)

P = fem.Point


def _meshes():
    return {
        "rect-crossed": fem.RectangleMesh(P(0, 0), P(3, 2), 3, 2, "crossed"),
        "box": fem.BoxMesh(P(0, 0, 0), P(2, 3, 2), 2, 3, 2),
        "rect-stretched": fem.RectangleMesh(P(0, 0), P(0.3, 0.74), 3, 2, "crossed"),
        "box-stretched": fem.BoxMesh(P(0, 0, 0), P(0.2, 1.11, 2.0 / 3.0), 2, 3, 2),
    }


def random_barycentric(rng, n, G):
    lam = rng.uniform(0.05, 1.0, size=(n, G + 1))
    return lam / lam.sum(axis=1, keepdims=True)


@pytest.mark.parametrize("name", list(_meshes()))
def test_restatement_on_quadratic_polynomials(oracle, name):
    """P2 holds a quadratic polynomial exactly, so the restatement must give its gradient 2 Q x + b at any point of any cell."""
    mesh = _meshes()[name]
    lay = fem.FunctionSpace(mesh, "CG", 2)._lay
    X, rec = lay.coords, lay.cells
    G = X.shape[1]
    rng = np.random.default_rng(G)
    Q = rng.standard_normal((2, G, G))
    Q = Q + np.transpose(Q, (0, 2, 1))
    b = rng.standard_normal((2, G))
    U = np.einsum("nd,cde,ne->nc", X, Q, X) + X @ b.T + 0.7                      # two components
    lam = random_barycentric(rng, 4, G)
    g = point_gradients(X, rec, U, lam)
    assert g.dtype == LD and g.shape == (4, rec.shape[0], 2 * G)
    for a in range(4):
        x = np.einsum("i,eid->ed", lam[a], X[rec[:, :G + 1]])
        exact = 2.0 * np.einsum("cde,ne->ncd", Q, x) + b[None]
        scale = np.abs(exact).max()
        assert np.abs(g[a].astype(np.float64).reshape(-1, 2, G) - exact).max() <= 1e-13 * max(scale, 1.0), name
    # and the shape functions sum to one and reproduce the field
    N = shape_values(lam[0], G)
    assert abs(N.sum() - 1.0) < 1e-15
    x0 = np.einsum("i,eid->ed", lam[0], X[rec[:, :G + 1]])
    assert np.allclose(np.einsum("j,ejc->ec", N, U[rec]), np.einsum("nd,cde,ne->nc", x0, Q, x0) + x0 @ b.T + 0.7, rtol=0, atol=1e-12)


def test_restatement_on_integers():
    """Integer data on unit lattices with integer 4 lam: int64, and the planes of x^2 - 3 x y + 2 y at the vertices by hand."""
    mesh = fem.RectangleMesh(P(0, 0), P(3, 2), 3, 2)
    lay = fem.DofLayout(mesh, 2)
    X, rec = lay.coords, lay.cells
    U = np.rint(4 * (X[:, 0] ** 2 - 3 * X[:, 0] * X[:, 1] + 2 * X[:, 1])).astype(np.int64)       # (edge midpoints: quarters)
    g = point_gradients(X, rec, U, np.eye(3))
    assert g.dtype == np.int64
    xv = X[rec[:, :3]]                                                           # (cells, vertex, d)
    want = np.stack([4 * (2 * xv[..., 0] - 3 * xv[..., 1]), 4 * (-3 * xv[..., 0] + 2)], axis=-1)      # (cells, vertex, d)
    assert np.array_equal(g, np.transpose(np.rint(want).astype(np.int64), (1, 0, 2)))
    p = planes_p2(X, rec, U, np.array([[0.5, 0.5, 0.0]]), np.array([[1, 1]]), np.arange(1, len(rec) + 1))
    assert p.dtype == np.int64 and p.shape == (1, 1, len(rec))


@pytest.mark.parametrize("name", ["rect-crossed", "box"])
def test_restatement_equals_point_gradient(oracle, name):
    mesh = _meshes()[name]
    V = fem.FunctionSpace(mesh, "CG", 2)
    lay = V._lay
    X, rec = lay.coords, lay.cells
    G = X.shape[1]
    rng = np.random.default_rng(7 + G)
    f = fem.Function(V)
    f.vector()._host = rng.standard_normal(lay.n)
    f.vector().touched_host()
    lam = random_barycentric(rng, 3, G)
    g = point_gradients(X, rec, f.vector().host(), lam).astype(np.float64)
    for a in range(3):
        x = np.einsum("i,eid->ed", lam[a], X[rec[:, :G + 1]])
        for e in range(rec.shape[0]):
            pg = fem.point_gradient(f, x[e])
            assert np.abs(pg - g[a, e]).max() <= 1e-12 * max(1.0, np.abs(pg).max()), (name, a, e)


# ------------------------------------------------------------------------------------------ through the frontend
@pytest.fixture(scope="module")
def elastic_p2(oracle):
    mesh = fem.BoxMesh(P(0, 0, 0), P(2, 1, 1), 2, 2, 2)
    p = PGDProblem(**problems.elastic_block(mesh, 5, PGD_nmax=2, degree=2))
    p.solve_PGD(_problem="linear", settings={"relative_tolerance": 1e-11})
    return mesh, p.return_PGD()


@pytest.fixture(scope="module")
def reaction_p2(oracle):
    mesh = fem.RectangleMesh(P(0, 0), P(1.5, 1), 4, 3)
    p = PGDProblem(**problems.reaction_diffusion(mesh, 7, PGD_nmax=3, degree=2))
    p.solve_PGD(_problem="linear")
    return mesh, p.return_PGD()


@pytest.mark.parametrize("planes", ["stored", "fused"])
@pytest.mark.parametrize("at", ["midpoint", "vertices"])
def test_host_path_on_the_elastic_block(elastic_p2, at, planes):
    mesh, sol = elastic_p2
    run_and_check_p2(sol, [1], samples_of(sol, (1,), 9, 5), "von_mises", two_valued(mesh, 1.0 / (1.0 + NU), 3.0 / (1.0 + NU)), at,
                     planes=planes, sample_chunk=4)
    run_and_check_p2(sol, [1], samples_of(sol, (1,), 5, 6), "gradient_norm", None, at, planes=planes)


@pytest.mark.parametrize("planes", ["stored", "fused"])
@pytest.mark.parametrize("at", ["midpoint", "vertices"])
def test_host_path_on_reaction_diffusion(reaction_p2, at, planes):
    mesh, sol = reaction_p2
    run_and_check_p2(sol, [1], samples_of(sol, (1,), 11, 3), "gradient_norm", two_valued(mesh, 0.7, 2.5), at, planes=planes)
    run_and_check_p2(sol, [1], samples_of(sol, (1,), 4, 4), "gradient_norm", 0.5, at, planes=planes, sample_chunk=3)


@pytest.mark.parametrize("planes", ["stored", "fused"])
def test_host_path_on_one_mode_models(oracle, planes):
    """A random scalar P2 field on the crossed rectangle and a random displacement on a stretched box, one mode each."""
    rng = np.random.default_rng(12)
    for name, vector in (("rect-crossed", False), ("box-stretched", True)):
        mesh = _meshes()[name]
        V = fem.VectorFunctionSpace(mesh, "CG", 2) if vector else fem.FunctionSpace(mesh, "CG", 2)
        sol = one_mode_solution(mesh, V, rng.standard_normal(V.dim()))
        for at in ("midpoint", "vertices"):
            run_and_check_p2(sol, [1], [[0.25], [0.5], [1.0]], "von_mises" if vector else "gradient_norm", 1.5 if vector else None, at,
                             planes=planes)


@pytest.mark.parametrize("dim", [3, 2])
def test_von_mises_of_a_quadratic_displacement(oracle, dim):
    """u = EPS (x^2, -NU x y, ...): the strain is linear in x, the von Mises stress at a point follows from the analytic strain
    there (deviator, 2-D: plane strain), and P2 holds u exactly - at the barycentres and at the vertices of every cell."""
    EPS = 1e-3
    if dim == 3:
        mesh = fem.BoxMesh(P(0, 0, 0), P(1, 1, 1), 2, 2, 2)
        disp = lambda X: EPS * np.stack([X[:, 0] ** 2, -NU * X[:, 0] * X[:, 1], X[:, 1] * X[:, 2]], axis=1)
        grad = lambda x: EPS * np.array([[2 * x[0], 0, 0], [-NU * x[1], -NU * x[0], 0], [0, x[2], x[1]]])
    else:
        mesh = fem.RectangleMesh(P(0, 0), P(1, 1), 3, 2)
        disp = lambda X: EPS * np.stack([X[:, 0] ** 2, -NU * X[:, 0] * X[:, 1]], axis=1)
        grad = lambda x: EPS * np.array([[2 * x[0], 0], [-NU * x[1], -NU * x[0]]])

    def von_mises(x):
        eps = np.zeros((3, 3))
        H = grad(x)
        eps[:dim, :dim] = 0.5 * (H + H.T)
        s = 2.0 * MU * (eps - np.trace(eps) / 3.0 * np.eye(3))
        return math.sqrt(1.5 * (s * s).sum())

    V = fem.VectorFunctionSpace(mesh, "CG", 2)
    lay = V._lay.base
    sol = one_mode_solution(mesh, V, disp(lay.coords))
    Xv = lay.coords[lay.cells[:, :dim + 1]]                                      # (cells, vertex, d)
    tol = 1e-12 * E_MOD * EPS
    mid = sol.evaluate_gradient_many(0, [1], [[0.5]], 0, quantity="von_mises", scale=2.0 * MU, fields=True, at="midpoint")
    want = np.array([von_mises(x) for x in Xv.mean(axis=1)])
    assert np.abs(mid.fields[0].vector().host() - want).max() <= tol and abs(mid.max[0] - want.max()) <= tol
    ver = sol.evaluate_gradient_many(0, [1], [[0.5]], 0, quantity="von_mises", scale=2.0 * MU, envelope=True, at="vertices")
    corner = np.array([[von_mises(x) for x in cell] for cell in Xv])             # (cells, vertex)
    assert abs(ver.max[0] - corner.max()) <= tol and abs(ver.min[0] - corner.min()) <= tol
    assert np.abs(ver.envelope_max.vector().host() - corner.max(axis=1)).max() <= tol
    assert np.abs(ver.envelope_min.vector().host() - corner.min(axis=1)).max() <= tol


def test_the_vertex_maximum_is_the_maximum_over_the_mesh(elastic_p2):
    """|L grad u| is convex on a cell: ``max`` of at="vertices" equals the largest vertex value of the restatement, and no value
    at 50 random interior points of any cell exceeds its cell's ``envelope_max``."""
    mesh, sol = elastic_p2
    coords = samples_of(sol, (1,), 4, 21)
    scale = two_valued(mesh, 1.0, 2.5)
    res, ref, _ = run_and_check_p2(sol, [1], coords, "von_mises", scale, "vertices")
    assert np.all(np.abs(res.max - ref.astype(np.float64).max(axis=1)) <= 1e-12 * res.max)
    V = sol.mesh[0].attributes[0].interpolationfct[0].function_space()
    lay = V._lay.base
    L = fem.gradient_quantity("von_mises", 3, 3)
    lam = random_barycentric(np.random.default_rng(3), 50, 3)
    emx = res.envelope_max.vector().host()
    for j, c in enumerate(coords):
        u = sol.evaluate(0, [1], list(c), 0).vector().host().reshape(-1, 3)
        inner = np.empty((0, mesh.num_cells()))
        for l0 in range(0, 50, 4):                                               # (the restatement takes a few points at a time)
            p = planes_p2(lay.coords, lay.cells, u, lam[l0:l0 + 4], L, scale.vector().host())
            inner = np.concatenate([inner, np.sqrt((p * p).sum(axis=0)).astype(np.float64)])
        assert np.all(inner <= res.max[j] * (1.0 + 1e-12))
        assert np.all(inner.max(axis=0) <= emx * (1.0 + 1e-12))


@pytest.mark.parametrize("planes", ["stored", "fused"])
def test_interval_p2_on_the_host(oracle, planes):
    m1 = fem.IntervalMesh(5, 0.0, 2.0)
    V = fem.FunctionSpace(m1, "CG", 2)
    x = V._lay.coords[:, 0]
    sol = one_mode_solution(m1, V, 3.0 * x * x - x)                               # u' = 6 x - 1
    xv = m1.coordinates()[m1.cells()][:, :, 0]                                   # (cells, 2)
    mid = sol.evaluate_gradient_many(0, [1], [[0.5]], 0, fields=True, at="midpoint", planes=planes)
    assert np.abs(mid.fields[0].vector().host() - np.abs(6.0 * xv.mean(axis=1) - 1.0)).max() <= 1e-12
    ver = sol.evaluate_gradient_many(0, [1], [[0.5]], 0, envelope=True, at="vertices", planes=planes)
    assert abs(ver.max[0] - 11.0) <= 1e-12 and abs(ver.min[0] - np.abs(6.0 * xv - 1.0).min()) <= 1e-12
    assert np.abs(ver.envelope_max.vector().host() - np.abs(6.0 * xv - 1.0).max(axis=1)).max() <= 1e-12


def test_refusals(elastic_p2, oracle):
    mesh, sol = elastic_p2
    coords = samples_of(sol, (1,), 4, 8)
    with pytest.raises(ValueError, match="at="):
        sol.evaluate_gradient_many(0, [1], coords, 0, at="gauss")
    with pytest.raises(ValueError, match="vertices"):
        sol.evaluate_gradient_many(0, [1], coords, 0, at="vertices", fields=True)
    with pytest.raises(ValueError, match="vertices"):
        sol.evaluate_gradient_many(0, [1], coords, 0, at="vertices", threshold=0.5)
    with pytest.raises(NotImplementedError, match="midpoint.*vertices"):
        sol.evaluate_gradient_many(0, [1], coords, 0)                             # P2 with at=None: as before, the choices named
    # the byte count of the derived modes carries the points
    K, nc = sol.used_numModes, mesh.num_cells()
    nbytes = K * 6 * 4 * nc * 8
    with pytest.raises(ValueError, match=r"%d bytes .*4 points x %d cells" % (nbytes, nc)):
        sol.evaluate_gradient_many(0, [1], coords, 0, quantity="von_mises", at="vertices", modes_max_bytes=nbytes - 1)
    sol.evaluate_gradient_many(0, [1], coords, 0, quantity="von_mises", at="vertices", modes_max_bytes=nbytes)
    with pytest.raises(ValueError, match=str(K * 6 * nc * 8)):
        sol.evaluate_gradient_many(0, [1], coords, 0, quantity="von_mises", at="midpoint", modes_max_bytes=K * 6 * nc * 8 - 1)
    # "auto" falls to the fused path where the vertex planes do not fit, and gives the same numbers
    a = sol.evaluate_gradient_many(0, [1], coords, 0, quantity="von_mises", at="vertices", planes="auto", modes_max_bytes=nbytes - 1)
    b = sol.evaluate_gradient_many(0, [1], coords, 0, quantity="von_mises", at="vertices")
    assert np.allclose(a.max, b.max, rtol=1e-12, atol=0.0)
    # P1 modes: "midpoint" is today's path, "vertices" has nothing to choose
    m1 = fem.BoxMesh(P(0, 0, 0), P(1, 1, 1), 2, 2, 2)
    V1 = fem.FunctionSpace(m1, "CG", 1)
    p1 = one_mode_solution(m1, V1, np.arange(V1.dim(), dtype=np.float64) ** 2)
    with pytest.raises(ValueError, match="P1"):
        p1.evaluate_gradient_many(0, [1], [[0.5]], 0, at="vertices")
    x, y = p1.evaluate_gradient_many(0, [1], [[0.5]], 0, fields=True), p1.evaluate_gradient_many(0, [1], [[0.5]], 0, fields=True, at="midpoint")
    assert np.array_equal(x.fields[0].vector().host(), y.fields[0].vector().host()) and np.array_equal(x.max, y.max)


def test_cache_of_the_derived_modes(elastic_p2):
    mesh, sol = elastic_p2
    coords = samples_of(sol, (1,), 5, 7)
    builds = lambda: fem.STATS.get("gradient_mode_builds", 0)
    a = sol.evaluate_gradient_many(0, [1], coords, 0, quantity="von_mises", at="midpoint")
    n0 = builds()
    b = sol.evaluate_gradient_many(0, [1], coords, 0, quantity="von_mises", at="midpoint")
    assert builds() == n0 and np.array_equal(a.max, b.max)                       # reused
    c = sol.evaluate_gradient_many(0, [1], coords, 0, quantity="von_mises", at="vertices")
    assert builds() == n0 + 1 and sol.mesh[0].attributes[0]._gradient_modes.key[-1] == "vertices"      # another `at`: rebuilt
    assert np.all(c.max >= a.max * (1.0 - 1e-12))                                # the barycentre is a point of the cell
    sol.evaluate_gradient_many(0, [1], coords, 0, quantity="von_mises", at="vertices")
    assert builds() == n0 + 1
    sol.evaluate_gradient_many(0, [1], coords, 0, quantity="von_mises", at="vertices", planes="fused")
    assert builds() == n0 + 1                                                    # fused builds nothing
