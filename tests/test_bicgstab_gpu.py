"""pgd_bicgstab_solve (csrc/pgd_krylov.hip) held to its restatement (tests/bicgstab_reference.py) iterate by iterate.

x after maxit = k is exactly the k-th iterate (the confirmation pass at it == maxit recomputes b - A x and leaves x alone), so
maxit = 1..K from the same start walks the trajectory.  Each x_k must lie within max(32 noise_k, 1e-14) of the float64 restatement,
noise_k being what rounding alone does to that iterate (tests/golden/bicgstab_noise.json, measured on the CPU; a step is pinned
only while 32 noise_k <= 1e-9, and a wrong coefficient moves a pinned iterate by more than 1e-3: tests/test_bicgstab_cpu.py).
The reported residual must be the true one; the breakdown and restart paths are met on 2- and 3-row systems whose arithmetic is
exact; the error returns leave x as the header says and the context usable.

Room the bound left on the MI355X - last pinned step K, largest deviation / bound over the steps 1..K from the zero / the warm
start (the test prints these lines, pytest -s):
    rect9x7     K = 12   0.117 / 0.073        p2line       K = 12   0.143 / 0.118
    box6x5x4    K = 12   0.054 / 0.112        negdiag      K =  8   0.037 / 0.032
    line41      K = 12   0.054 / 0.077        spd_lattice  K = 12   0.212 / 0.231
    rect40x25   K = 12   0.072 / 0.053        recombined handle (K = 6): rect9x7 0.051, rect9x7_graded 0.040, spd_lattice 0.118

Libraries made wrong on purpose, run under this file on the MI355X: p = r + beta (p + omega v) in k_bi_p fails 26 tests, x without
omega z in k_bi_x 30, beta without alpha / omega 21 (all 14 trajectories each time); pgd_op_combine leaving dinv_valid set fails
test_recombined_handle_uses_the_new_diagonal_and_values[rect9x7_graded] alone."""
import json
import os

import numpy as np
import pytest

from oracle import fem_numpy as F
from pgdrome_amd._lib import PgdError
from tests import bicgstab_cases as C
from tests import bicgstab_reference as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bicgstab_noise.json")
with open(GOLDEN) as _f:
    NOISE = json.load(_f)["noise"]


class Device:
    """The device objects of the cases, made on first use and freed with the module."""

    def __init__(self, ctx):
        self.ctx, self.made = ctx, {}

    def get(self, cs, vals=None, key=None):
        """(mesh, operator, atoms) of a Case / Tiny; vals: other values on the same pattern."""
        key = key or cs.name
        if key not in self.made:
            ctx = self.ctx
            h = ctx.mesh_upload(cs.coords, cs.cells)
            rp, cols = ctx.mesh_pattern(h)
            rp_o, cols_o = F.csr_pattern(cs.n, cs.cells)
            assert np.array_equal(rp, rp_o) and np.array_equal(cols, cols_o)
            terms = getattr(cs, "terms", None)
            if terms is None or vals is not None:
                atoms = []
                op = ctx.atom_upload(h, cs.pattern_values() if vals is None else vals)
            else:
                atoms = [ctx.atom_assemble(h, kind, da, 0) for kind, da, _ in terms]
                op = ctx.op_combine(h, atoms, [c for _, _, c in terms], cs.bc)
            self.made[key] = (h, op, atoms)
        return self.made[key]

    def close(self):
        for h, op, atoms in self.made.values():
            for a in [op] + atoms:
                self.ctx.atom_free(a)
            self.ctx.mesh_free(h)
        self.made = {}


@pytest.fixture(scope="module")
def dev(ctx):
    d = Device(ctx)
    yield d
    d.close()


_EXT = {}


def true_relres(cs, x, key=None):
    """(||b - A x|| / ||b||, || |A||x| + |b| || / ||b||) with the sums in the extended type (slot_reference.exact_dot without one)."""
    A, b = cs.A.tocsr(), cs.b
    if R.HAVE_EXTENDED:
        key = key or cs.name
        if key not in _EXT:
            ar = R.Arith("extended")
            _EXT[key] = (ar, R.Matrix(A, ar))
        ar, M = _EXT[key]
        r = ar.vec(b) - M.dot(ar.vec(x))
        rn = float(np.sqrt(ar.dot(r, r)))
    else:
        from tests.slot_reference import exact_dot
        r = np.array([b[i] - exact_dot(A.data[A.indptr[i]:A.indptr[i + 1]], x[A.indices[A.indptr[i]:A.indptr[i + 1]]]) for i in range(cs.n)])
        rn = float(np.sqrt(exact_dot(r, r)))
    bn = float(np.linalg.norm(b))
    return rn / bn, float(np.linalg.norm(abs(A) @ np.abs(x) + np.abs(b))) / bn


def check_honest(cs, x, relres, key=None):
    true, scale = true_relres(cs, x, key)
    assert abs(relres - true) <= 4e-15 * scale, (cs.name, relres, true, scale)


def run(ctx, op, bv, x0, rtol, atol, maxit):
    xv = ctx.vec_from(x0)
    try:
        it, rel = ctx.bicgstab(op, bv, xv, rtol, atol, maxit)
        return it, rel, ctx.vec_download(xv)
    finally:
        ctx.vec_free(xv)


def walk(ctx, cs, op, x0, noise_row, label, key=None):
    """maxit = 1..K against the restatement; returns (K, largest deviation / bound)."""
    K = R.pinned_steps(noise_row)
    assert K >= 6
    traj, ref = R.trajectory(cs.A, cs.b, x0, K)
    assert len(traj) == K and ref.iters == K
    bv = ctx.vec_from(cs.b)
    worst = 0.0
    try:
        for k in range(1, K + 1):
            it, rel, x = run(ctx, op, bv, x0, 1e-30, 0.0, k)
            assert it == k, (label, k, it)
            dist = float(np.linalg.norm(x - traj[k - 1])) / float(np.linalg.norm(traj[k - 1]))
            ratio = dist / R.bound(noise_row[k - 1])
            worst = max(worst, ratio)
            print("bicgstab %s step %d: deviation %.3e, bound %.3e, ratio %.3f" % (label, k, dist, R.bound(noise_row[k - 1]), ratio))
            assert dist <= R.bound(noise_row[k - 1]), (label, k, dist, noise_row[k - 1])
            check_honest(cs, x, rel, key)
    finally:
        ctx.vec_free(bv)
    print("bicgstab %s: last pinned step %d, largest deviation / bound %.3f" % (label, K, worst))
    return K, worst


@pytest.mark.parametrize("start", C.STARTS)
@pytest.mark.parametrize("name", C.NAMES)
def test_trajectory_is_the_restatements(ctx, dev, name, start):
    """Every pinned iterate of every system from both starts; the reported residual of each call is the true one."""
    cs = C.case(name)
    h, op, atoms = dev.get(cs)
    if name == "spd_lattice":
        # the diagonal form exists, so pgd_op_combine has left the CSR values to the first reader: BiCGStab has to form them
        assert all(ctx.atom_product_form(a) != 0 for a in atoms)
    walk(ctx, cs, op, cs.starts[start], NOISE["%s/%s" % (name, start)], "%s/%s" % (name, start))


@pytest.mark.parametrize("name", C.NAMES)
def test_reported_residual_is_honest_through_the_confirmation_legs(ctx, dev, name):
    """rtol = 1e-14 is below what the recurrence residual can promise: the call goes through the confirmation and its second legs.
    Whatever it reaches, relres is ||b - A x|| / ||b|| of the x it returns and iters <= maxit; and the same call again gives the same
    bits."""
    cs = C.case(name)
    h, op, atoms = dev.get(cs)
    bv = ctx.vec_from(cs.b)
    try:
        for rtol, maxit in ((1e-14, 300), (1e-14, 25), (1e-16, 300)):
            # (1e-16 is out of reach: all three legs run; what is reported after the last one is the recurrence's residual, which
            # started from the true one at most 50 iterations before and has to stay within the same bound of it)
            it, rel, x = run(ctx, op, bv, cs.starts["warm"], rtol, 0.0, maxit)
            assert 1 <= it <= maxit and np.all(np.isfinite(x))
            check_honest(cs, x, rel)
            it2, rel2, x2 = run(ctx, op, bv, cs.starts["warm"], rtol, 0.0, maxit)
            assert (it2, rel2) == (it, rel) and np.array_equal(x2, x)
        it, rel, x = run(ctx, op, bv, cs.starts["zero"], 1e-11, 0.0, 20000)
        assert rel <= 1.0000001e-11 and np.linalg.norm(x - cs.xstar) <= 1e-8 * np.linalg.norm(cs.xstar)
        check_honest(cs, x, rel)
    finally:
        ctx.vec_free(bv)


@pytest.mark.parametrize("name", C.RECOMBINED)
def test_recombined_handle_uses_the_new_diagonal_and_values(ctx, name):
    """Solve, combine other coefficients (50 MASS: another diagonal) into the SAME operator handle, and pin the steps 1..6 against
    the restatement of the new matrix: CSR values left from the first combine would move every iterate, and so would its Jacobi
    diagonal on the graded mesh (on the uniform ones the diagonal is constant inside the hull and its scale does not matter)."""
    cs, new = C.recombined(name)
    terms = new.terms
    noise_row = NOISE["%s/warm" % new.name][:6]
    assert R.pinned_steps(noise_row) == 6
    h = ctx.mesh_upload(cs.coords, cs.cells)
    atoms = [ctx.atom_assemble(h, kind, da, 0) for kind, da, _ in cs.terms]
    op = ctx.op_combine(h, atoms, [c for _, _, c in cs.terms], cs.bc)
    bv = ctx.vec_from(cs.b)
    try:
        it, rel, x = run(ctx, op, bv, cs.starts["zero"], 1e-11, 0.0, 20000)
        assert np.linalg.norm(x - cs.xstar) <= 1e-8 * np.linalg.norm(cs.xstar)
        assert ctx.op_combine(h, atoms, [c for _, _, c in terms], cs.bc, op=op) == op
        walk(ctx, new, op, new.starts["warm"], noise_row, new.name, key=new.name)
    finally:
        ctx.vec_free(bv)
        for a in [op] + atoms:
            ctx.atom_free(a)
        ctx.mesh_free(h)


def ordinary_solve(ctx, dev):
    cs = C.case("rect9x7")
    h, op, atoms = dev.get(cs)
    bv = ctx.vec_from(cs.b)
    try:
        it, rel, x = run(ctx, op, bv, cs.starts["zero"], 1e-11, 0.0, 20000)
    finally:
        ctx.vec_free(bv)
    assert rel <= 1.0000001e-11 and np.linalg.norm(x - cs.xstar) <= 1e-8 * np.linalg.norm(cs.xstar)


@pytest.mark.parametrize("row", C.table() + list(C.RECOVERABLE), ids=lambda t: t.name)
def test_breakdown_table(ctx, dev, row):
    """The device does what the restatement does: status, iters, x (bit for bit where the arithmetic is exact), relres; after an
    error return the context still solves."""
    ref = R.solve(row.A, row.b, np.zeros(row.n), rtol=1e-10, atol=0.0, maxit=100)
    assert ref.status == row.status and list(ref.events) == list(row.events) and ref.iters == row.iters
    assert np.array_equal(ref.x, row.x) if row.exact else np.abs(ref.x - row.x).max() <= 1e-15 * np.abs(row.x).max()
    h, op, _ = dev.get(row)
    bv, xv = ctx.vec_from(row.b), ctx.vec_from(np.zeros(row.n))
    try:
        if row.status == R.OK:
            it, rel = ctx.bicgstab(op, bv, xv, 1e-10, 0.0, 100)
            x = ctx.vec_download(xv)
            assert it == ref.iters == row.iters
            assert rel == ref.relres == 0.0 if row.exact else rel <= 1e-14
            check_honest(row, x, rel)
        else:
            with pytest.raises(PgdError) as err:
                ctx.bicgstab(op, bv, xv, 1e-10, 0.0, 100)
            assert err.value.code == R.SINGULAR
            x = ctx.vec_download(xv)
        if row.exact:
            assert np.array_equal(x, row.x) and np.array_equal(x, ref.x), (row.name, x[:6])
        else:
            assert np.abs(x - row.x).max() <= 1e-15 * np.abs(row.x).max(), (row.name, x[:6])
    finally:
        ctx.vec_free(bv)
        ctx.vec_free(xv)
    if row.status != R.OK:
        ordinary_solve(ctx, dev)


def test_zero_diagonal_entry_is_an_error_return(ctx, dev):
    """One exact zero on the diagonal: PGD_ERR_SINGULAR with x unchanged, never PGD_OK with a non-finite x."""
    cs, vals = C.line41_zero_diagonal()
    h, op, _ = dev.get(cs, vals=vals, key="line41_zero_diagonal")
    bv = ctx.vec_from(cs.b)
    try:
        for start in C.STARTS:
            xv = ctx.vec_from(cs.starts[start])
            with pytest.raises(PgdError) as err:
                ctx.bicgstab(op, bv, xv, 1e-10, 0.0, 100)
            assert err.value.code == R.SINGULAR
            assert np.array_equal(ctx.vec_download(xv), cs.starts[start])
            ctx.vec_free(xv)
    finally:
        ctx.vec_free(bv)
    ordinary_solve(ctx, dev)


def test_edges(ctx, dev):
    cs = C.case("rect9x7")
    h, op, _ = dev.get(cs)
    warm = cs.starts["warm"]
    bv = ctx.vec_from(cs.b)
    bnorm = float(np.linalg.norm(cs.b))
    try:
        # maxit = 0: nothing but the residual of the start
        it, rel, x = run(ctx, op, bv, warm, 1e-10, 0.0, 0)
        assert it == 0 and np.array_equal(x, warm)
        check_honest(cs, warm, rel)
        # a start that already meets the tolerance
        it, rel, x = run(ctx, op, bv, cs.xstar, 1e-10, 0.0, 100)
        assert it == 0 and np.array_equal(x, cs.xstar) and rel <= 1e-10
        # atol above rtol ||b|| decides the stop: the restatement's count, far below the count of the rtol run
        ref = R.solve(cs.A, cs.b, cs.starts["zero"], rtol=1e-30, atol=0.05 * bnorm, maxit=100)
        it, rel, x = run(ctx, op, bv, cs.starts["zero"], 1e-30, 0.05 * bnorm, 100)
        assert it == ref.iters and 1 <= it < 10 and rel <= 0.05 * 1.0000001
        check_honest(cs, x, rel)
        it_r, rel_r, _ = run(ctx, op, bv, cs.starts["zero"], 1e-11, 1e-30, 100)
        assert it_r > it and rel_r <= 1.0000001e-11
        # refused before anything is launched: x and b keep their bits
        xv = ctx.vec_from(warm)
        short = ctx.vec_from(warm[:-1])
        for args in ((op, bv, bv, 1e-10, 0.0, 100), (op, bv, short, 1e-10, 0.0, 100), (op, short, xv, 1e-10, 0.0, 100),
                     (op, bv, xv, 1e-10, 0.0, -1)):
            with pytest.raises(PgdError) as err:
                ctx.bicgstab(*args)
            assert err.value.code == R.INVALID
        assert np.array_equal(ctx.vec_download(xv), warm) and np.array_equal(ctx.vec_download(bv), cs.b)
        assert np.array_equal(ctx.vec_download(short), warm[:-1])
        ctx.vec_free(xv)
        ctx.vec_free(short)
    finally:
        ctx.vec_free(bv)
    ordinary_solve(ctx, dev)


def test_two_identical_calls_give_the_same_bits(ctx, dev):
    cs = C.case("rect40x25")                       # four workgroups: the partial sums are added in a fixed order
    h, op, _ = dev.get(cs)
    bv = ctx.vec_from(cs.b)
    try:
        for rtol, maxit in ((1e-30, 7), (1e-11, 20000)):
            a = run(ctx, op, bv, cs.starts["warm"], rtol, 0.0, maxit)
            b = run(ctx, op, bv, cs.starts["warm"], rtol, 0.0, maxit)
            assert a[0] == b[0] and a[1] == b[1] and np.array_equal(a[2], b[2])
    finally:
        ctx.vec_free(bv)
