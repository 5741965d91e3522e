"""The systems of the BiCGStab tests (tests/test_bicgstab_cpu.py, tests/test_bicgstab_gpu.py): the smallest at which the kernels of
pgdrome_amd/csrc/pgd_krylov.hip can still go wrong.  TPB = 256: rect40x25 (1000 rows) takes four workgroups, so the partial sums of
several workgroups are met; everything else is one workgroup and a tail.

Every system has two starts: zero, and 0.3 x* + 0.01 max|x*| noise with the Dirichlet rows zeroed ("warm").

spd_lattice: every box lattice from 3 x 3 x 3 nodes on takes a non-zero pgd_atom_product_form for its STIFF and MASS atoms after
pgd_op_combine (measured on the MI355X: form 2 for all 216 boxes with 3..8 nodes per side), so the CSR values of the combined
operator are deferred on all of them.  The 27-row box has ONE row inside its Dirichlet hull and BiCGStab ends there in one step;
SPD_LATTICE_NODES is the smallest box (by rows, then lexicographically) on which the solve takes more than the 12 recorded steps
and the steps 1..6 are pinned from both starts (found by smallest_pinned_lattice() on the CPU, checked by the CPU test).

The breakdown table: 2- and 3-node interval meshes with integer values uploaded on the tridiagonal pattern, x0 = 0.  Every
quantity up to the event is a small dyadic rational, so any summation order reproduces it bit for bit.  search_recoverable()
looks for further cases (integer entries in -4..4, diagonal in +-1, +-2, +-4, up to 4 rows); what it found is RECOVERABLE.
"""
from __future__ import annotations

import itertools

import numpy as np
import scipy.sparse as sps
import scipy.sparse.linalg as spla

from oracle import fem_numpy as F

SPD_LATTICE_NODES = (4, 6, 4)          # 96 rows, 16 of them inside the hull
BOX_EXTENT = (1.0, 0.7, 1.3)


class Case:
    """name, the layout (coords, cells), the matrix A with its Dirichlet rows (scipy CSR), b, bc, how the device gets the operator
    (terms: [(kind, direction, coefficient)] for pgd_op_combine, or None: the values go up with pgd_atom_upload), x* and the starts."""

    def __init__(self, name, coords, cells, A, bc, terms, seed):
        self.name, self.coords, self.cells, self.bc, self.terms = name, coords, cells, np.asarray(bc, dtype=np.int32), terms
        self.A = A.tocsr()
        self.n = A.shape[0]
        rng = np.random.default_rng(seed)
        self.b = rng.uniform(-1, 1, self.n)
        self.b[self.bc] = 0.0
        self.xstar = spla.spsolve(self.A.tocsc(), self.b)
        warm = 0.3 * self.xstar + 0.01 * np.abs(self.xstar).max() * rng.uniform(-1, 1, self.n)
        warm[self.bc] = 0.0
        self.starts = {"zero": np.zeros(self.n), "warm": warm}

    def pattern_values(self):
        """The values of A in the order of the layout's CSR pattern (what pgd_atom_upload takes), structural zeros included."""
        rp, cols = F.csr_pattern(self.n, self.cells)
        rows = np.repeat(np.arange(self.n), np.diff(rp))
        return np.asarray(self.A[rows, cols]).ravel().astype(np.float64)


def hull(coords):
    lo, hi = coords.min(axis=0), coords.max(axis=0)
    return np.where(np.any((coords <= lo + 1e-12) | (coords >= hi - 1e-12), axis=1))[0].astype(np.int32)


def _assembled(name, coords, cells, terms, seed, sign=1.0, upload=False):
    A = None
    for kind, da, coef in terms:
        T = coef * F.assemble_atom(coords, cells, kind, da, 0)
        A = T if A is None else A + T
    bc = hull(coords)
    A, _ = F.apply_dirichlet(A.tocsr(), np.zeros(coords.shape[0]), bc)
    return Case(name, coords, cells, sign * A, bc, None if upload else terms, seed)


def _cdr(gdim, mass=3.0):
    return [(F.STIFF, 0, 1.0), (F.MASS, 0, mass)] + [(F.CONV, a, c) for a, c in enumerate((30.0, -12.0, 7.0)[:gdim])]


def spd_lattice_case(nodes=SPD_LATTICE_NODES):
    nx, ny, nz = nodes
    # steps (1/4, 1/8, 1/2): every coordinate is dyadic, so the atoms are symmetric to the last bit whatever assembles them
    c, e = F.box_mesh((0, 0, 0), (0.25 * (nx - 1), 0.125 * (ny - 1), 0.5 * (nz - 1)), nx - 1, ny - 1, nz - 1)
    return _assembled("spd_lattice", c, e, [(F.STIFF, 0, 1.0), (F.MASS, 0, 1.0)], 17)


_CASES = {}


def _builders():
    def p2line():
        c, e = F.interval_mesh(40)
        nodes, tab = F.p2_interval_nodes(c, e)
        return _assembled("p2line", nodes, tab, [(F.STIFF, 0, 1.0), (F.MASS, 0, 1.0), (F.CONV, 0, 1.0)], 15)
    return {
        "rect9x7": lambda: _assembled("rect9x7", *F.rectangle_mesh((0, 0), (1, 1), 8, 6), _cdr(2), 11),
        "box6x5x4": lambda: _assembled("box6x5x4", *F.box_mesh((0, 0, 0), BOX_EXTENT, 5, 4, 3), _cdr(3), 12),
        "line41": lambda: _assembled("line41", *F.interval_mesh(40), [(F.STIFF, 0, 1.0), (F.MASS, 0, 3.0), (F.CONV, 0, 5.0)], 13),
        "rect40x25": lambda: _assembled("rect40x25", *F.rectangle_mesh((0, 0), (1, 1), 39, 24), _cdr(2), 14),
        "p2line": p2line,
        "negdiag": lambda: _assembled("negdiag", *F.rectangle_mesh((0, 0), (1, 1), 8, 6), _cdr(2), 16, sign=-1.0, upload=True),
        "spd_lattice": spd_lattice_case,
        "rect9x7_graded": _graded,
    }


NAMES = ("rect9x7", "box6x5x4", "line41", "rect40x25", "p2line", "negdiag", "spd_lattice")
STARTS = ("zero", "warm")


def case(name):
    """Built once, shared and left unchanged."""
    if name not in _CASES:
        _CASES[name] = _builders()[name]()
    return _CASES[name]


def all_cases():
    return [case(n) for n in NAMES]


RECOMBINED = ("rect9x7", "rect9x7_graded", "spd_lattice")


def _graded():
    """rect9x7 with its vertices moved to (x^1.5, y^1.25) (a stronger grading, (x^2, y^1.5), loses step 6 to rounding).  On the
    uniform meshes every row inside the hull has the SAME diagonal entry, and right-Jacobi BiCGStab does not change when the scaling
    is multiplied by a constant: a Jacobi diagonal left over from other coefficients is invisible there.  Here the diagonal of
    STIFF + 3 MASS + ... is not a multiple of that of STIFF + 50 MASS + ..."""
    c, e = F.rectangle_mesh((0, 0), (1, 1), 8, 6)
    c = np.stack([c[:, 0] ** 1.5, c[:, 1] ** 1.25], axis=1)
    return _assembled("rect9x7_graded", c, e, _cdr(2), 18)


def recombined(name):
    """(the case, the case with 50 MASS in place of its MASS coefficient): what the operator handle of the first holds after it
    has been combined a second time."""
    key = name + "_recombined"
    if key not in _CASES:
        base = case(name)
        terms = [(k, da, 50.0 if k == F.MASS else c) for k, da, c in base.terms]
        _CASES[key] = _assembled(key, base.coords, base.cells, terms, 21)
    return case(name), _CASES[key]


def table_cases():
    """Every system with a row in tests/golden/bicgstab_noise.json."""
    return all_cases() + [recombined(n)[1] for n in RECOMBINED]


def line41_zero_diagonal(row=20):
    """The values of line41 on its pattern with the diagonal entry of one row set to 0."""
    cs = case("line41")
    rp, cols = F.csr_pattern(cs.n, cs.cells)
    vals = cs.pattern_values()
    k = rp[row] + int(np.where(cols[rp[row]:rp[row + 1]] == row)[0][0])
    vals[k] = 0.0
    return cs, vals


def smallest_pinned_lattice(max_rows=20000):
    """The first box (rows ascending, then lexicographic) on which the recorded steps mean something: from both starts the solve to
    rtol = 1e-11 needs more than NOISE_STEPS iterations (a box with a handful of rows inside its hull is solved after as many steps,
    and what follows is the recurrence run on rounding errors), and the steps 1..6 are pinned."""
    from tests import bicgstab_reference as R
    shapes = sorted({s for s in itertools.product(range(3, 12), repeat=3)}, key=lambda s: (s[0] * s[1] * s[2], s))
    for s in shapes:
        if s[0] * s[1] * s[2] > max_rows:
            break
        if (s[0] - 2) * (s[1] - 2) * (s[2] - 2) <= R.NOISE_STEPS:
            continue                       # (exact arithmetic ends within as many steps as there are free rows)
        cs = spd_lattice_case(s)
        if all(R.solve(cs.A, cs.b, x0, rtol=1e-11, atol=0.0, maxit=1000).iters > R.NOISE_STEPS for x0 in cs.starts.values()) and \
                all(R.pinned_steps(R.noise(cs.A, cs.b, x0, 6)) >= 6 for x0 in cs.starts.values()):
            return s
    return None


# ------------------------------------------------------------------------------------------------ the breakdown table
class Tiny:
    """A dense integer matrix on the tridiagonal pattern of an interval mesh of its size, replicated `copies` times as uncoupled
    blocks along one interval mesh (zero couplings between the blocks): sums over the copies stay exact, and cross workgroups."""

    def __init__(self, name, A, b, events, status, iters, x, copies=1, exact=True):
        """events, status, iters, x: the expected outcome from x0 = 0 with rtol = 1e-10, atol = 0, maxit = 100 (iters: as reported,
        0 on an error return); exact: x is met bit for bit (else to 1e-15: the quantities after the event are not dyadic)."""
        self.name, self.events, self.status, self.iters, self.copies, self.exact = name, tuple(events), status, iters, copies, exact
        A0 = np.asarray(A, dtype=np.float64)
        m = A0.shape[0]
        assert all(A0[i, j] == 0 for i in range(m) for j in range(m) if abs(i - j) > 1)
        self.block = m
        self.n = m * copies
        self.A = sps.kron(sps.identity(copies), sps.csr_matrix(A0)).tocsr()
        self.b = np.tile(np.asarray(b, dtype=np.float64), copies)
        self.x = None if x is None else np.tile(np.asarray(x, dtype=np.float64), copies)
        self.coords, self.cells = F.interval_mesh(self.n - 1)

    def pattern_values(self):
        rp, cols = F.csr_pattern(self.n, self.cells)
        rows = np.repeat(np.arange(self.n), np.diff(rp))
        return np.asarray(self.A.todense())[rows, cols].astype(np.float64) if self.n <= 64 else \
            np.asarray(self.A.tocsr()[rows, cols]).ravel().astype(np.float64)

    def replicated(self, copies):
        m = self.block
        return Tiny("%s_x%d" % (self.name, copies), self.A[:m, :m].toarray(), self.b[:m], self.events, self.status, self.iters,
                    None if self.x is None else self.x[:m], copies, self.exact)


OK, SINGULAR = 0, -5
FIVE = ("rhat.v=0", "restart") * 4 + ("rhat.v=0", "singular")      # the fifth breakdown of a call ends it
FOUR = FIVE[2:]

TABLE = (
    Tiny("half_step", [[-4, -4], [0, -4]], (-2, 0), ("half-step", "confirm"), OK, 1, (0.5, 0.0)),
    Tiny("rhat_v_at_once", [[-4, -4], [0, -2]], (1, -1), FIVE, SINGULAR, 0, (0.0, 0.0)),
    Tiny("omega_then_rhat_v", [[-4, -4], [0, -2]], (1, 1), ("omega=0", "restart") + FOUR, SINGULAR, 0, (-0.125, -0.25)),
    Tiny("t_t", [[-4, -4], [-2, -2]], (1, 2), ("t.t=0", "restart") + FOUR, SINGULAR, 0, (-0.125, -0.5)),
    Tiny("rho_restart_half_step", [[-1, 0, 0], [-4, -2, 0], [0, 2, -1]], (1, 0, 0), ("rho=0", "restart", "half-step", "confirm"), OK, 3,
         (-1.0, 2.0, 4.0), exact=False),
)
REPLICATED = (0, 4)               # rows of TABLE repeated as 256 uncoupled blocks: 512 and 768 rows, three workgroups


def table():
    return list(TABLE) + [TABLE[i].replicated(256) for i in REPLICATED]


def search_recoverable(rows, seconds=None, seed=1, want=3):
    """Tridiagonal systems of `rows` rows (off-diagonal entries in -4..4, diagonal in +-1, +-2, +-4, b in -2..2, x0 = 0) on which the
    call meets omega == 0 or rhat . v == 0, restarts and still ends with PGD_OK at rtol = 1e-10 - with both float64 orders on the
    same path to the same bits and an exact run that agrees and stays dyadic, so that the device would meet the event exactly.
    seconds = None: every system (2 rows: 69 984 with b != 0); else random systems for that long.  Returns ({event: [(A, b, events, iters, x)]},
    systems tried)."""
    import time
    from tests import bicgstab_reference as R
    D, E, B = (-4, -2, -1, 1, 2, 4), tuple(range(-4, 5)), (-2, -1, 0, 1, 2)
    found = {"omega=0": [], "rhat.v=0": []}

    def systems():
        if seconds is None:
            for d in itertools.product(D, repeat=rows):
                for lo in itertools.product(E, repeat=rows - 1):
                    for up in itertools.product(E, repeat=rows - 1):
                        for b in itertools.product(B, repeat=rows):
                            yield d, lo, up, b
        else:
            rng, t0 = np.random.default_rng(seed), time.time()
            while time.time() - t0 < seconds:
                yield rng.choice(D, rows), rng.choice(E, rows - 1), rng.choice(E, rows - 1), rng.choice(B, rows)

    tried = 0
    for d, lo, up, b in systems():
        b = np.array(b, dtype=np.float64)
        if not b.any():
            continue
        tried += 1
        A = sps.csr_matrix(np.diag(np.array(d, dtype=np.float64)) + np.diag(np.array(lo, dtype=np.float64), -1) + np.diag(np.array(up, dtype=np.float64), 1))
        run = lambda arith, maxit: R.solve(A, b, np.zeros(rows), rtol=1e-10, atol=0.0, maxit=maxit, arith=arith)         # noqa: E731
        r = run("f64_asc", 4 * rows)              # (exact arithmetic ends within `rows` steps per restart)
        if r.status != R.OK or r.relres > 1e-10 or not np.all(np.isfinite(r.x)):
            continue
        for ev in found:
            if ev in r.events and len(found[ev]) < want:
                d2 = run("f64_desc", 4 * rows)
                if d2.events != r.events or not np.array_equal(d2.x, r.x):
                    continue
                e = run("exact", r.iters)
                if e.events == r.events and e.arith.dyadic and np.array_equal(np.array([float(v) for v in e.x]), r.x):
                    found[ev].append((A.toarray().tolist(), b.tolist(), r.events, r.iters, r.x.tolist()))
        if all(len(v) >= want for v in found.values()):
            break
    return found, tried


# What search_recoverable found.  2 rows, all 69 984 systems with b != 0: no recoverable case of either kind.  3 rows, 434 831
# random systems (seed 3; the bound holds 1.8e8): recoverable rhat . v == 0 cases, the first one below; no recoverable omega == 0.
# 4 rows, 370 269 random systems (seed 4; of 4.3e11): none of either kind.  So a recoverable omega == 0 has not been found within the
# bound, but only the 2-row part of the bound has been searched completely.
RECOVERABLE = (
    Tiny("rhat_v_recovered", [[1, 0, 0], [-3, -1, -2], [0, 1, -2]], (1, 0, 1), ("rhat.v=0", "restart", "half-step", "confirm"), OK, 3,
         (1.0, -1.0, -1.0)),
)
