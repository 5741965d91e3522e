"""The host-driven PCG pieces without a GPU: the plain reference (tests/slot_reference.py) against its own definition, the numpy
oracle (oracle/backend_numpy.py) piece by piece against the reference, and both recurrences of the reference - in the call
order of pgdrome_amd/dist.py - against a direct solve."""
import numpy as np
import pytest

from oracle.backend_numpy import NumpyBackend
from tests import slot_reference as R

U = 2.0 ** -53
VEC_RTOL = 4 * U          # entries and scalars that one or two operations form: the oracle multiplies and adds separately (two
                          # roundings), the reference's fma has one - 3 U of difference at most.  Relative to the SUM OF THE |TERMS|
                          # (State.vmag): relative to the result no bar can hold for a product and a sum that cancel
# Entries at the end of a longer chain: roundings of the oracle's path + roundings of the reference's path, each relative to the
# same sum of |terms| (first order; a rounding of a value that is fed forward counts once more in every value formed from it)
CHAIN_ROUNDINGS = {
    ("pcg_xr_slot", "z"): 5,          # r: 2 + 1, then z = dinv r adds one rounding on either side
    ("cg_update_slot", "x"): 6,       # p: 2 (oracle) and 1 (reference); alpha * p, then + x: 2 and 1 more
    ("cg_update_slot", "r"): 6,       # the same through s
    ("cg_update_slot", "u"): 8,       # ... and u = dinv r adds one on either side
}
DOT_RTOL = 1e-13          # the bar the project's dots are held to, relative to sum |a_i b_i|
CASES = R.all_cases()


# ------------------------------------------------------------------ the reference's own arithmetic
def test_fma_and_exact_dot_match_their_definitions():
    rng = np.random.default_rng(11)
    a, b, c = (R.wide(rng, 4000) for _ in range(3))
    c[:1000] = -(a[:1000] * b[:1000]) * (1.0 + rng.uniform(-4e-16, 4e-16, 1000))      # heavy cancellation: the low product bits decide
    got = R.fma_vec(a, b, c)
    want = np.array([R.fma_fraction(float(x), float(y), float(z)) for x, y, z in zip(a, b, c)])
    assert R.same_bits(got, want)
    assert np.any(got != a * b + c)                       # (the cases do tell an fma from a product and a sum)
    from fractions import Fraction
    exact = sum((Fraction(float(x)) * Fraction(float(y)) for x, y in zip(a, b)), Fraction(0))
    assert R.exact_dot(a, b) == float(exact)
    assert R.exact_dot(a[:0], b[:0]) == 0.0


# ------------------------------------------------------------------ the oracle, piece by piece
class OracleRun:
    """A NumpyBackend loaded with a copy of a reference state."""

    def __init__(self, st):
        self.be = NumpyBackend()
        self.h = {k: self.be.vec_from(a) for k, a in st.v.items()}
        self.be.slots[:] = st.S
        self.be._flags = list(st.flags)

    def call(self, name, args):
        getattr(self.be, name)(*[self.h[a] if isinstance(a, str) else a for a in args])

    def compare(self, ref, sums=(), skip=(), what="", piece=None):
        for k, h in self.h.items():
            got, want = self.be.vec_to_host(h), ref.v[k]
            if k not in ref.vmag:
                assert R.same_bits(got, want), (what, k, "not written")
                continue
            bar = CHAIN_ROUNDINGS.get((piece, k), 4) * U * ref.vmag[k]          # (zero outside the range: untouched entries)
            assert np.all(np.abs(got - want) <= bar), (what, k, float(np.max(np.abs(got - want) / (ref.vmag[k] + 1e-300)) / U))
        for i in range(R.NSLOTS):
            got, want = self.be.slots[i], ref.S[i]
            if i in skip:
                continue
            if i in sums and i in ref.mag:          # (a piece the done flag turned into a no-op wrote no sum)
                assert abs(got - want) <= DOT_RTOL * ref.mag[i], (what, "slot", i, got, want)
            elif want != want:
                assert got != got, (what, "slot", i)
            else:
                assert abs(got - want) <= VEC_RTOL * abs(want), (what, "slot", i, got, want)
        assert tuple(self.be.flags()) == tuple(ref.flags), (what, "flags")


# (piece, reference function, arguments with vector names, slots that hold sums, slots left unspecified, pure outputs)
def _vector_pieces(lo, hi):
    return [
        ("pcg_init_slot", R.pcg_init, ("b", "q", "dinv", "r", "z", "p", lo, hi, 30), (30, 31, 32), (), ("r", "z", "p")),
        ("pcg_xr_slot", R.pcg_xr, ("x", "r", "p", "q", "dinv", "z", lo, hi, 9, 10, 33), (33, 34), (), ("z",)),
        ("pcg_p_slot", R.pcg_p, ("p", "z", lo, hi, 9, 10), (), (), ()),
        ("cg_init_slot", R.cg_init, ("b", "q", "dinv", "r", "u", "p", "s", lo, hi, 24), (24, 25, 32), R.CG_SCRATCH, ("r", "u", "p", "s")),
        ("cg_update_slot", R.cg_update, ("x", "r", "u", "w", "p", "s", "dinv", lo, hi, 24), (24, 25), (), ()),
    ]


def _prepare(n, seed, outputs):
    st = R.make_state(n, seed, outputs)
    st.S[9], st.S[10] = 0.8125, 1.75          # a quotient that is not a float: alpha (xr) / beta (p) need their one division
    st.S[29], st.S[30] = 0.6, -0.35           # alpha, beta of the single-reduction update (base 24)
    return st


@pytest.mark.parametrize("case", CASES, ids=R.case_id)
@pytest.mark.parametrize("done", [0, 1], ids=["live", "done"])
def test_oracle_vector_pieces(case, done):
    n, label, lo, hi = case
    for name, fn, args, sums, skip, outputs in _vector_pieces(lo, hi):
        st = _prepare(n, 100 + n, outputs)
        st.flags = [done, 3, 0]
        run = OracleRun(st)
        fn(st, *args)
        run.call(name, args)
        run.compare(st, sums, skip, (name, label, done), piece=name)
        if done and name not in ("pcg_init_slot", "cg_init_slot"):      # a no-op: the reference left everything as it was
            ref0 = _prepare(n, 100 + n, outputs)
            assert all(R.same_bits(st.v[k], ref0.v[k]) for k in st.v) and R.same_bits(st.S, ref0.S)
        if lo == (n if hi < 0 else hi) and not (done and name in ("pcg_xr_slot", "cg_update_slot")):
            assert all(st.S[i] == 0.0 for i in sums), (name, "an empty range writes zeros")


SCALAR_STARTS = [
    # (rr, bb, rtol, atol): live, met by rtol, met by atol, NaN residual, NaN right-hand side norm
    (3.0, 100.0, 1e-3, 0.0), (9e-5, 100.0, 1e-3, 0.0), (0.5, 100.0, 1e-9, 1.0), (float("nan"), 100.0, 1e-3, 0.0),
    (3.0, float("nan"), 1e-3, 0.25), (0.01, float("nan"), 1e-3, 0.25),
]


@pytest.mark.parametrize("done", [0, 1], ids=["live", "done"])
@pytest.mark.parametrize("start", SCALAR_STARTS)
def test_oracle_scalar_pieces(start, done):
    rr, bb, rtol, atol = start
    for name, fn, args in (("pcg_tol_slot", R.pcg_tol, (rtol, atol, 11, 12, 13)),
                           ("pcg_check_slot", R.pcg_check, (11, 13)),
                           ("cg_scalars_slot", R.cg_scalars, (24, 1, rtol, atol)),
                           ("cg_scalars_slot", R.cg_scalars, (24, 0, rtol, atol))):
        for nan_in_d in (False, True):
            st = R.make_state(4, 5)
            st.flags = [done, 7, 0]
            st.S[11], st.S[12], st.S[13] = rr, bb, max(rtol * rtol * 100.0, atol * atol)
            st.S[24:33] = [2.5, rr, 1.25, 0.5, float("nan") if nan_in_d else 0.125, 0.6, 0.3, 3.5, bb]
            st.S[5] = st.S[13]
            run = OracleRun(st)
            fn(st, *args)
            run.call(name, args)
            run.compare(st, what=(name, start, done, nan_in_d))
    # what the reference itself must do with a NaN (the oracle is compared with THIS)
    st = R.make_state(4, 5)
    st.S[11] = float("nan")
    R.pcg_check(st, 11, 13)
    assert st.flags == [1, 1, R.ERR_SINGULAR]
    R.pcg_check(st, 11, 13)
    assert st.flags == [1, 1, R.ERR_SINGULAR]


def test_oracle_spmv_dot_slot():
    P = R.hull_problem("box")
    n, A = P["n"], P["A"]
    for lo, hi in ((0, -1), (3, n - 4), (n // 2, n // 2), (n, n)):
        for done in (0, 1):
            st = R.make_state(n, 8, ("w",))
            st.flags = [done, 0, 0]
            run = OracleRun(st)
            op = run.be._put((None, A))
            R.spmv_dot_slot(st, A, "p", "w", "p", lo, hi, 31)
            run.be.spmv_dot_slot(op, run.h["p"], run.h["w"], run.h["p"], lo, hi, 31)
            run.compare(st, sums=(31,), what=("spmv_dot_slot", lo, hi, done))


# ------------------------------------------------------------------ whole recurrences of the reference against a direct solve
RTOL = 1e-10


def _names(st):
    return {k: k for k in st.v}


@pytest.fixture(scope="module", params=["box", "interval"])
def problem(request):
    return R.hull_problem(request.param)


def _start(P):
    n = P["n"]
    v = {k: np.zeros(n) for k in ("x", "r", "z", "u", "w", "p", "s", "q")}
    v["b"] = P["b"]
    v["dinv"] = 1.0 / P["A"].diagonal()
    return R.State(v)


@pytest.mark.parametrize("form", ["pcg", "cg"])
def test_reference_recurrences_solve_the_system(problem, form):
    """x agrees with the direct solve to 1e-8 (the bar of the sharded tests), flags[1] counts the live iterations, and one more
    round after the stop changes nothing."""
    P = problem
    st = _start(P)
    be = R.RefBackend(st)
    ranges = [(0, P["n"], 0)]
    if form == "pcg":
        rounds, rz = R.drive_pcg(be, P["A"], _names(st), ranges, RTOL, 0.0, 500)
    else:
        rounds = R.drive_cg(be, P["A"], _names(st), ranges, RTOL, 0.0, 500)
    assert st.flags[0] == 1 and st.flags[2] == 0 and 0 < rounds < 500
    assert st.flags[1] == rounds          # every live round counts once: in `check`, or in the scalar step that follows the update
    assert np.linalg.norm(st.v["x"] - P["sol"]) <= 1e-8 * np.linalg.norm(P["sol"])
    res = P["b"] - P["A"] @ st.v["x"]
    assert np.linalg.norm(res) <= 10 * RTOL * np.linalg.norm(P["b"])
    assert st.S[R.S_LAST_RR] == st.S[rz + 1 if form == "pcg" else R.CG_BASE + 1]      # S[6]: the r.r that met the bar
    assert st.S[R.S_LAST_RR] <= st.S[R.S_TOL2] == RTOL * RTOL * (P["b"] @ P["b"])
    frozen = st.copy()
    no = R.HostAllreduce(be, [0])
    if form == "pcg":
        R.pcg_round(be, P["A"], _names(st), ranges, no, rounds, rz)
    else:
        R.cg_round(be, P["A"], _names(st), ranges, no, RTOL, 0.0)
    assert all(R.same_bits(st.v[k], frozen.v[k]) for k in st.v) and R.same_bits(st.S, frozen.S) and st.flags == frozen.flags


@pytest.mark.parametrize("form", ["pcg", "cg"])
def test_oracle_recurrences_agree_with_the_reference(problem, form):
    """The same drivers on the oracle: the same stop iteration +-1 (its sums are numpy's) and the same solution."""
    P = problem
    st = _start(P)
    ref = R.RefBackend(st)
    run = OracleRun(_start(P))
    op = run.be._put((None, P["A"]))
    ranges = [(0, P["n"], 0)]
    if form == "pcg":
        k_ref, _ = R.drive_pcg(ref, P["A"], _names(st), ranges, RTOL, 0.0, 500)
        k_or, _ = R.drive_pcg(run.be, op, run.h, ranges, RTOL, 0.0, 500)
    else:
        k_ref = R.drive_cg(ref, P["A"], _names(st), ranges, RTOL, 0.0, 500)
        k_or = R.drive_cg(run.be, op, run.h, ranges, RTOL, 0.0, 500)
    assert abs(k_ref - k_or) <= 1 and run.be.flags()[1] == k_or and run.be.flags()[2] == 0
    x = run.be.vec_to_host(run.h["x"])
    assert np.linalg.norm(x - P["sol"]) <= 1e-8 * np.linalg.norm(P["sol"])


def test_two_ranges_in_one_bank_match_the_whole_range(problem):
    """The drivers over two row ranges split at an odd row, each with its own slot indices and the host sum in place of the
    all-reduce: what the GPU test runs on the device, here on the reference."""
    P = problem
    m = (P["n"] // 2) | 1
    ranges = [(0, m, 0), (m, P["n"], R.HALF)]
    for form in ("pcg", "cg"):
        whole, split = _start(P), _start(P)
        if form == "pcg":
            k1, _ = R.drive_pcg(R.RefBackend(whole), P["A"], _names(whole), [(0, P["n"], 0)], RTOL, 0.0, 500)
            k2, _ = R.drive_pcg(R.RefBackend(split), P["A"], _names(split), ranges, RTOL, 0.0, 500)
        else:
            k1 = R.drive_cg(R.RefBackend(whole), P["A"], _names(whole), [(0, P["n"], 0)], RTOL, 0.0, 500)
            k2 = R.drive_cg(R.RefBackend(split), P["A"], _names(split), ranges, RTOL, 0.0, 500)
        assert abs(k1 - k2) <= 2 and split.flags == [1, k2, 0]
        assert np.linalg.norm(split.v["x"] - P["sol"]) <= 1e-8 * np.linalg.norm(P["sol"])
