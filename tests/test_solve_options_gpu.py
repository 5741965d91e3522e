"""Every opt-in cycle and product form of the linear solve through the frontend on the device, one row each: what info and fem.STATS
report equals what the library's own counters (pgd_*_counts) say, and behind the solve every knob is off again - the same system
under default settings is the Jacobi-PCG on the CSR product and moves none of the six counters.  The problems are the applying
frontend cases of tests/test_{vmg,cmg,pmg,block_dia,p2_lattice}_gpu.py on their 16^3-cell box (17^3 vertices, 33^3 P2 nodes);
tests/test_solve_options_cpu.py pins the call pattern itself without a GPU."""
import pytest

from pgdrome_amd import fem, problems

pytestmark = pytest.mark.gpu

P = fem.Point
STATS_METHODS = ("mg_stats", "vmg_stats", "cmg_stats", "pmg_stats", "bdia_stats", "p2lat_stats")


@pytest.fixture(scope="module")
def hip_backend():
    from pgdrome_amd.hip_backend import HipBackend
    old = fem._backend
    be = fem.set_backend(HipBackend(0))
    fem.clear_caches()
    yield be
    fem.set_backend(old)
    fem.clear_caches()


def _scalar(degree, weighted):
    Vh = fem.FunctionSpace(fem.BoxMesh(P(0, 0, 0), P(1, 1, 1), 16, 16, 16), "P", degree)
    u, v = fem.TrialFunction(Vh), fem.TestFunction(Vh)
    if weighted:       # SPD, not one stencil
        w = fem.interpolate(fem.Expression("1 + x[0] + x[1]*x[2]", degree=1), Vh)
        a = sum(w * u.dx(k) * v.dx(k) * fem.dx for k in range(3))
    else:
        a = fem.inner(fem.grad(u), fem.grad(v)) * fem.dx + fem.Constant(3.0) * u * v * fem.dx
    return a, fem.Constant(1.0) * v * fem.dx, fem.Function(Vh), fem.DirichletBC(Vh, 0.0, lambda x, on_boundary: on_boundary)


def _elasticity():
    Vh = fem.VectorFunctionSpace(fem.BoxMesh(P(0, 0, 0), P(1, 1, 1), 16, 16, 16), "P", 1)
    u, v = fem.TrialFunction(Vh), fem.TestFunction(Vh)
    a = (fem.inner(problems._voigt_C(0.3) * problems._strain(u), problems._strain(v)) + fem.Constant(2.0) * fem.inner(u, v)) * fem.dx
    return (a, fem.dot(fem.Constant((0.0, 0.0, -1.0)), v) * fem.dx, fem.Function(Vh),
            fem.DirichletBC(Vh, fem.Constant((0.0, 0.0, 0.0)), problems._clamped))


# settings key, value, the problem, the library's stats method and the counter in it, what info says (key, value), the fem.STATS
# key, the preconditioner pcg_last_form names
ROWS = [
    ("preconditioner", "amg", lambda: _scalar(1, False), "mg_stats", "solves", ("method", "mg_pcg"), "mg_solves", "MG"),
    ("preconditioner", "vmg", lambda: _scalar(1, True), "vmg_stats", "solves", ("method", "vmg_pcg"), "vmg_solves", "VMG"),
    ("preconditioner", "cmg", _elasticity, "cmg_stats", "solves", ("method", "cmg_pcg"), "cmg_solves", "CMG"),
    ("preconditioner", "pmg", lambda: _scalar(2, False), "pmg_stats", "solves", ("method", "pmg_pcg"), "pmg_solves", "PMG"),
    ("block_product", "diagonal", _elasticity, "bdia_stats", "products", ("product", "block_dia"), "block_dia_solves", "JACOBI"),
    ("p2_product", "lattice", lambda: _scalar(2, False), "p2lat_stats", "products", ("product", "p2_lattice"), "p2_lattice_solves", "JACOBI"),
]


@pytest.mark.parametrize("key,value,problem,stats,counter,says,stat,precond", ROWS, ids=[r[1] for r in ROWS])
def test_an_option_is_reported_as_the_library_counts_it_and_is_off_behind_the_solve(hip_backend, key, value, problem, stats, counter,
                                                                                   says, stat, precond):
    a, L, sol, bc = problem()
    read = getattr(hip_backend, stats)
    lib0, st0 = read(), dict(fem.STATS)
    info = fem.solve(a == L, sol, bc, solver_parameters={key: value, "relative_tolerance": 1e-10})
    lib1, st1 = read(), dict(fem.STATS)
    print("%s=%s: %s, library %s -> %s" % (key, value, info, lib0, lib1))
    advanced = lib1[counter] - lib0[counter]
    assert advanced == 1 if counter == "solves" else advanced > 0          # (one solve under the cycle; products from the form)
    assert lib1["fallbacks"] == lib0["fallbacks"]
    assert info[says[0]] == says[1] and st1.get(stat, 0) == st0.get(stat, 0) + 1
    assert {k for k in st1 if k.endswith("_solves") and k != "linear_solves" and st1[k] != st0.get(k, 0)} == {stat}
    assert hip_backend.pcg_last_form()[1] == precond
    # the same system under default settings: no knob was left on
    everything = {m: getattr(hip_backend, m)() for m in STATS_METHODS}
    plain = fem.solve(a == L, fem.Function(sol.function_space()), bc, solver_parameters={"relative_tolerance": 1e-10})
    assert (plain["method"], plain["product"]) == ("jacobi_pcg", "csr") and plain["relres"] <= 1e-10
    assert {m: getattr(hip_backend, m)() for m in STATS_METHODS} == everything
    assert hip_backend.pcg_last_form()[1] == "JACOBI"
    assert {k: v for k, v in fem.STATS.items() if k.endswith("_solves") and k != "linear_solves"} == \
        {k: v for k, v in st1.items() if k.endswith("_solves") and k != "linear_solves"}
