"""The restatement of pgd_bicgstab_solve (tests/bicgstab_reference.py) checked by itself: it solves the systems of
tests/bicgstab_cases.py, its rounding noise per step is the stored table (tests/golden/bicgstab_noise.json) and stays under the cap
where the GPU test pins a step, three deliberately wrong recurrences are far outside that bound, and the breakdown table holds in
exact rationals."""
import json
import os
from fractions import Fraction

import numpy as np
import pytest

from tests import bicgstab_cases as C
from tests import bicgstab_reference as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bicgstab_noise.json")


def stored_noise():
    with open(GOLDEN) as f:
        return json.load(f)["noise"]


def _rel(a, b):
    return float(np.linalg.norm(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)) / np.linalg.norm(np.asarray(b, dtype=np.float64)))


@pytest.mark.parametrize("start", C.STARTS)
@pytest.mark.parametrize("name", C.NAMES)
def test_restatement_reaches_the_direct_solution(name, start):
    """Run to rtol = 1e-11 in both float64 orders: the SuperLU solution to 1e-8, the reported residual is met and honest."""
    cs = C.case(name)
    for arith in ("f64_asc", "f64_desc"):
        res = R.solve(cs.A, cs.b, cs.starts[start], rtol=1e-11, atol=0.0, maxit=20000, arith=arith)
        assert res.status == R.OK and 1 <= res.iters < 20000 and res.relres <= 1.0000001e-11, res
        assert _rel(res.x, cs.xstar) <= 1e-8, (name, start, arith, res)
        assert np.linalg.norm(cs.b - cs.A @ res.x) <= 1.01e-11 * np.linalg.norm(cs.b)
        assert len(res.steps) == res.iters and np.array_equal(res.steps[-1][0], res.x)


@pytest.mark.parametrize("name", C.NAMES)
def test_maxit_k_leaves_the_kth_iterate(name):
    """The observation the GPU test rests on, in the restatement: x after maxit = k is the k-th iterate of the longer run, bit for bit."""
    cs = C.case(name)
    traj, res = R.trajectory(cs.A, cs.b, cs.starts["warm"], 8)
    assert res.iters == 8 and len(traj) == 8
    for k in (1, 2, 5, 8):
        one = R.solve(cs.A, cs.b, cs.starts["warm"], rtol=1e-30, atol=0.0, maxit=k)
        assert one.iters == k and np.array_equal(one.x, traj[k - 1]) and one.events == ["confirm"]


@pytest.mark.skipif(not R.HAVE_EXTENDED, reason="np.longdouble is no extended type on this machine")
def test_the_stored_noise_table_is_reproduced():
    table = R.noise_table(C.table_cases())
    stored = stored_noise()
    assert sorted(table) == sorted(stored)
    for key, row in table.items():
        assert len(row) == R.NOISE_STEPS == len(stored[key])
        np.testing.assert_allclose(row, stored[key], rtol=1e-9, atol=0.0, err_msg=key)


def test_steps_one_to_six_are_pinned_everywhere():
    """The cap is a condition: a step is pinned only if 32 noise_k <= 1e-9, and the steps 1..6 of every system and start are."""
    stored = stored_noise()
    assert sorted(stored) == sorted("%s/%s" % (cs.name, s) for cs in C.table_cases() for s in C.STARTS)
    for key, row in stored.items():
        assert R.pinned_steps(row) >= 6, (key, row)
        assert all(np.isfinite(v) and v > 0 for v in row[:6])


@pytest.mark.parametrize("variant", [v for v in R.VARIANTS if v])
@pytest.mark.parametrize("name", C.NAMES)
def test_a_wrong_recurrence_is_far_outside_the_bound(name, variant):
    """beta without alpha / omega, p = r + beta (p + omega v), x without omega z: each moves some pinned iterate by more than 1e-3,
    from either start - six orders of magnitude above the largest bound the GPU test allows (1e-9)."""
    cs = C.case(name)
    stored = stored_noise()
    for start in C.STARTS:
        K = R.pinned_steps(stored["%s/%s" % (name, start)])
        right, _ = R.trajectory(cs.A, cs.b, cs.starts[start], K)
        wrong, _ = R.trajectory(cs.A, cs.b, cs.starts[start], K, variant=variant)
        assert len(right) == K
        worst = max([_rel(w, r) for w, r in zip(wrong, right)] + [np.inf] * (len(wrong) < K))
        assert worst > 1e-3, (name, start, variant, worst)


@pytest.mark.parametrize("name", C.RECOMBINED)
def test_a_diagonal_left_from_the_first_combine(name):
    """The recombined systems run with the Jacobi diagonal of the matrix they replace: far outside the bound on the graded mesh,
    nothing at all on the uniform ones (a constant diagonal inside the hull, and BiCGStab does not see the scale of its right
    preconditioner) - the graded mesh is what makes the GPU test of the recombined handle see a stale diagonal."""
    old, new = C.recombined(name)
    right, _ = R.trajectory(new.A, new.b, new.starts["warm"], 6)
    stale, _ = R.trajectory(new.A, new.b, new.starts["warm"], 6, diagonal=old.A.diagonal())
    worst = max(_rel(s, r) for s, r in zip(stale, right))
    if name == "rect9x7_graded":
        assert len(stale) == 6 and worst > 1e-3, worst
    else:
        assert worst <= 1e-12, worst
    # ... and the values of the matrix it replaces move every system
    assert _rel(R.trajectory(old.A, new.b, new.starts["warm"], 6)[0][5], right[5]) > 1e-3


def test_the_spd_lattice_is_the_smallest_pinned_one():
    cs = C.case("spd_lattice")
    assert abs(cs.A - cs.A.T).max() <= 4e-16 * abs(cs.A).max() and cs.n == int(np.prod(C.SPD_LATTICE_NODES))      # (symmetric to the rounding of the assembly)
    assert C.smallest_pinned_lattice(cs.n) == C.SPD_LATTICE_NODES


def test_the_convective_systems_are_not_symmetric_and_negdiag_is_negative():
    for name in ("rect9x7", "box6x5x4", "line41", "rect40x25", "p2line", "negdiag"):
        A = C.case(name).A
        assert abs(A - A.T).max() > 1e-3 * abs(A).max(), name
    assert np.all(C.case("negdiag").A.diagonal() < 0) and np.array_equal(C.case("negdiag").A.toarray(), -C.case("rect9x7").A.toarray())
    assert C.case("rect40x25").n == 1000 and C.case("rect9x7").n == 63 and C.case("box6x5x4").n == 120 and C.case("line41").n == 41


@pytest.mark.parametrize("row", C.table() + list(C.RECOVERABLE), ids=lambda t: t.name)
def test_breakdown_table_in_exact_rationals(row):
    """The event happens exactly, and the float64 runs in both orders take the same path to the same x."""
    ex = R.solve(row.A, row.b, np.zeros(row.n), rtol=1e-10, atol=0.0, maxit=100, arith="exact")
    assert ex.status == row.status and list(ex.events) == list(row.events), ex
    assert ex.iters == row.iters
    if row.exact:
        assert ex.arith.dyadic and ex.arith.bits <= 40
        assert [Fraction(v) for v in ex.x] == [Fraction(v) for v in row.x]
        if row.status == R.OK:
            assert ex.relres == 0.0
    else:
        # dyadic up to the event (the first iteration), not after the restart: the outcome to rounding
        first = R.solve(row.A, row.b, np.zeros(row.n), rtol=1e-10, atol=0.0, maxit=1, arith="exact")
        assert first.arith.dyadic and first.arith.bits <= 40 and row.events[0] in first.events
        assert np.abs(np.array([float(v) for v in ex.x]) - row.x).max() == 0.0 and ex.relres == 0.0
    for arith in ("f64_asc", "f64_desc"):
        fl = R.solve(row.A, row.b, np.zeros(row.n), rtol=1e-10, atol=0.0, maxit=100, arith=arith)
        assert fl.status == ex.status and fl.events == ex.events and fl.iters == ex.iters
        if row.exact:
            assert np.array_equal(fl.x, row.x)
        else:
            assert np.abs(fl.x - row.x).max() <= 1e-15 * np.abs(row.x).max()


def test_zero_diagonal_ends_singular_with_x_unchanged():
    """As pgd_krylov.hip reads: 1 / 0 makes y non-finite, rhat . v is NaN in every attempt, five breakdowns, x never written."""
    cs, vals = C.line41_zero_diagonal()
    import scipy.sparse as sps
    from oracle import fem_numpy as F
    rp, cols = F.csr_pattern(cs.n, cs.cells)
    A = sps.csr_matrix((vals, cols, rp), shape=(cs.n, cs.n))
    assert A.diagonal()[20] == 0.0 and np.count_nonzero(A.diagonal() == 0.0) == 1
    for start in C.STARTS:
        res = R.solve(A, cs.b, cs.starts[start], rtol=1e-10, atol=0.0, maxit=100)
        assert res.status == R.SINGULAR and res.events == list(C.FIVE) and np.array_equal(res.x, cs.starts[start])


def test_edges_of_the_restatement():
    cs = C.case("rect9x7")
    res = R.solve(cs.A, cs.b, cs.starts["warm"], rtol=1e-10, atol=0.0, maxit=0)
    assert res.iters == 0 and np.array_equal(res.x, cs.starts["warm"])
    assert abs(res.relres - np.linalg.norm(cs.b - cs.A @ cs.starts["warm"]) / np.linalg.norm(cs.b)) <= 1e-14 * res.relres
    done = R.solve(cs.A, cs.b, cs.xstar, rtol=1e-10, atol=0.0, maxit=100)
    assert done.iters == 0 and done.events == ["confirm"]
    loose = R.solve(cs.A, cs.b, cs.starts["zero"], rtol=1e-30, atol=0.05 * np.linalg.norm(cs.b), maxit=100)
    assert 1 <= loose.iters < 10 and loose.relres <= 0.05 * 1.0000001
    # a tolerance out of reach: three legs; the residual reported after the last one is the recurrence's, started from the true one
    far = R.solve(cs.A, cs.b, cs.starts["warm"], rtol=1e-16, atol=0.0, maxit=300)
    assert far.events.count("leg") == 3 and far.events[-1] == "leg" and far.iters <= 300
    true = np.linalg.norm(cs.b - cs.A @ far.x) / np.linalg.norm(cs.b)
    assert abs(far.relres - true) <= 4e-15 * np.linalg.norm(abs(cs.A) @ np.abs(far.x) + np.abs(cs.b)) / np.linalg.norm(cs.b)
    assert R.solve(cs.A, cs.b, cs.starts["zero"], maxit=-1).status == R.INVALID
    assert R.solve(cs.A, cs.b[:-1], cs.starts["zero"]).status == R.INVALID
