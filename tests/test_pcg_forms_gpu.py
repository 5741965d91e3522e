"""Which recurrence and which preconditioner pgd_pcg_solve picks (pgd_pcg_last_form), pinned case by case against the two decision
tables written out in tests/pcg_form_cases.py, and that every form it picks solves: the knob-flipping tests elsewhere compare one
form with another and would pass with the wrong form on both sides."""
import numpy as np
import pytest

from pgdrome_amd import fem
from tests import pcg_form_cases as PC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def systems():
    """The HIP backend's context (the frontend is set to it: one system assembles through the frontend) and the systems built on it so far."""
    from pgdrome_amd.hip_backend import HipBackend
    old = fem._backend
    be = fem.set_backend(HipBackend(0))
    fem.clear_caches()
    built = {}
    yield be.ctx, built
    for s in built.values():
        s["free"]()
    built.clear()
    fem.set_backend(old)
    fem.clear_caches()


@pytest.mark.parametrize("name,system,bc,knobs,form,precond,fallback", PC.CASES, ids=[c[0] for c in PC.CASES])
def test_the_form_is_the_tables_and_it_solves(systems, name, system, bc, knobs, form, precond, fallback):
    """(1) the reported (form, preconditioner) are the table's; a request that falls back moves its counter, and only then.
    (2) cut at 37 iterations (rtol 0: nothing can stop it earlier) the solve has counted 37.
    (3) at convergence (rtol 1e-10) the true residual through the plain CSR product is at most 1.05e-10 |b|, the bound of
        tests/test_pcg_recompute_gpu.py.
    (4) the same solve again returns the same bits, cut and converged."""
    ctx, built = systems
    if system not in built:
        built[system] = PC.build_system(ctx, system)
    s = built[system]
    stats = {"mg": ctx.mg_stats, "vmg": ctx.vmg_stats, "cmg": ctx.cmg_stats}
    try:
        PC.set_knobs(ctx, knobs)
        before = {k: f() for k, f in stats.items()}
        cut = PC.solve(ctx, s, bc, PC.CUT, 0.0)
        after = {k: f() for k, f in stats.items()}
        chosen = ctx.pcg_last_form()
        cut2 = PC.solve(ctx, s, bc, PC.CUT, 0.0)
        full = PC.solve(ctx, s, bc, 10000, 1e-10, residual=True)
        chosen_full = ctx.pcg_last_form()
        full2 = PC.solve(ctx, s, bc, 10000, 1e-10)
    finally:
        PC.set_knobs(ctx, {})
    print("%s: %s, cut %d iterations, converged in %d, reported %.3g, true residual %.3g" % (name, chosen, cut[0], full[0], full[1], full[3]))
    assert chosen == (form, precond) and chosen_full == (form, precond)
    for k in stats:
        moved = 1 if k == fallback else 0
        assert after[k]["fallbacks"] == before[k]["fallbacks"] + moved, k
        assert after[k]["solves"] == before[k]["solves"] + (1 if k.upper() == precond else 0), k
    assert cut[0] == PC.CUT
    assert full[0] < 10000 and full[1] <= 1e-10 and full[3] <= 1.05e-10
    assert cut2[0] == cut[0] and cut2[1] == cut[1] and np.array_equal(cut2[2], cut[2])
    assert full2[0] == full[0] and full2[1] == full[1] and np.array_equal(full2[2], full[2])
