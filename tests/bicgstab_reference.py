"""pgd_bicgstab_solve (pgdrome_amd/csrc/pgd_krylov.hip) restated in plain numpy, control flow and all.

The restatement follows the host loop of the function statement by statement: right-Jacobi BiCGStab, the four breakdown tests
(rhat . v == 0, t . t == 0, omega == 0, rho == 0) with a restart from the current x (five breakdowns end the call with
PGD_ERR_SINGULAR), the half-step exit (x += alpha y), the confirmation of the true residual with its legs of at most 50
iterations and the factor 1.0000001, and the accounting of maxit.  It is independent of oracle/backend_numpy.py (whose bicgstab
is a direct solve) and of pgdrome_amd/dist.py.

The arithmetic is a parameter (ARITHMETICS):

    f64_asc   float64, every sum (dot products, rows of the product) taken in ascending index order
    f64_desc  float64, the same sums in descending order
    extended  np.longdouble, where its epsilon is at most 2^-63 (HAVE_EXTENDED), ascending order
    exact     fractions.Fraction: no rounding at all (the 2- and 3-row breakdown systems)

The device forms its sums in a third order (fused multiply-adds per thread, a tree per workgroup, the partial sums of the
workgroups in fixed order), so float64 iterates agree with the device to rounding only - how far rounding alone moves the k-th
iterate is what noise_table() measures: the larger distance of the two float64 orders from the extended run.
"""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

OK, SINGULAR, INVALID = 0, -5, -1               # PGD_OK, PGD_ERR_SINGULAR, PGD_ERR_INVALID (include/pgd_amd.h)
HAVE_EXTENDED = bool(np.finfo(np.longdouble).eps <= 2.0 ** -63)
ARITHMETICS = ("f64_asc", "f64_desc", "extended", "exact")
VARIANTS = (None, "beta_without_alpha_over_omega", "p_plus_omega_v", "x_without_omega_z")     # None: the recurrence as the device states it
NOISE_STEPS = 12
CAP = 1e-9                                      # a step is pinned only if 32 * noise_k <= CAP
FACTOR = 32.0


class Arith:
    """Vectors, sums in a fixed order and the few scalar functions of one arithmetic."""

    def __init__(self, name):
        assert name in ARITHMETICS, name
        if name == "extended" and not HAVE_EXTENDED:
            raise RuntimeError("np.longdouble is no extended type here")
        self.name = name
        self.exact = name == "exact"
        self.dtype = {"f64_asc": np.float64, "f64_desc": np.float64, "extended": np.longdouble, "exact": object}[name]
        self.descending = name == "f64_desc"
        self.bits, self.dyadic = 0, True       # exact runs: the widest numerator / denominator met, and whether all were dyadic

    def note(self, *values):
        """Exact runs keep book of what they meet: scalars, the terms of every sum and the sums themselves."""
        if not self.exact:
            return
        for v in values:
            for q in (np.asarray(v, dtype=object).ravel() if isinstance(v, np.ndarray) else (v,)):
                q = Fraction(q)
                if q.denominator & (q.denominator - 1):
                    self.dyadic = False
                self.bits = max(self.bits, abs(q.numerator).bit_length(), q.denominator.bit_length())

    def scalar(self, v):
        if self.exact:
            return v if isinstance(v, Fraction) else Fraction(v)
        return self.dtype(v)

    def vec(self, a):
        a = np.asarray(a)
        if self.exact:
            return np.array([self.scalar(v) for v in a.ravel()], dtype=object).reshape(a.shape)
        return a.astype(self.dtype)

    def zeros(self, n):
        return self.vec(np.zeros(n))

    def sum_rows(self, P):
        """Sequential sums along the last axis, in this arithmetic's order (np.add.accumulate adds one term after the other)."""
        if P.shape[-1] == 0:
            return self.zeros(P.shape[:-1]) if P.ndim > 1 else self.scalar(0)
        if self.descending:
            P = P[..., ::-1]
        out = np.add.accumulate(P, axis=-1)[..., -1]
        self.note(P, out)
        return out

    def dot(self, a, b):
        return self.sum_rows(a * b)

    def sqrt(self, q):
        if self.exact:
            return math.sqrt(q)        # (reporting only: the exact run compares squares)
        return np.sqrt(q)

    def is_nan(self, q):
        return (not self.exact) and bool(q != q)


class Matrix:
    """The rows of a sparse matrix padded to one width: y_i = sum_k vals[i, k] x[cols[i, k]] in a fixed order per row."""

    def __init__(self, A, ar):
        A = A.tocsr().copy()
        A.sort_indices()
        n = A.shape[0]
        cnt = np.diff(A.indptr)
        w = int(cnt.max()) if n else 0
        self.n = n
        self.cols = np.zeros((n, w), dtype=np.int64)
        self.mask = np.arange(w)[None, :] < cnt[:, None]
        self.cols[self.mask] = A.indices
        self.vals = ar.zeros((n, w))
        self.vals[self.mask] = ar.vec(A.data)
        self.diag = ar.vec(A.diagonal())
        self.zero = ar.zeros((n, w))
        self.ar = ar

    def dot(self, x):
        # (entries outside the mask stay exact zeros even where x is not finite)
        return self.ar.sum_rows(np.where(self.mask, self.vals * x[self.cols], self.zero))

    def dinv(self):
        ar = self.ar
        if ar.exact:
            return np.array([1 / d for d in self.diag], dtype=object)        # ZeroDivisionError: no exact run of such a system
        with np.errstate(divide="ignore"):
            return ar.scalar(1) / self.diag


class Result:
    def __init__(self):
        self.status, self.iters, self.x, self.relres = OK, 0, None, 0.0
        self.arith = None         # the Arith of the run (exact runs: .bits, .dyadic)
        self.events = []          # what the control flow took, in order
        self.steps = []           # per counted iteration: (x_k, alpha, omega, beta); omega is None where the step ended early
        self.message = ""

    def __repr__(self):
        return "Result(status=%d, iters=%d, relres=%r, events=%r)" % (self.status, self.iters, self.relres, self.events)


def solve(A, b, x0, rtol=1e-10, atol=0.0, maxit=10000, arith="f64_asc", variant=None, diagonal=None):
    """The whole of pgd_bicgstab_solve.  On SINGULAR `x` is what the device vector holds at the return (the function does not
    report iters then: Result.iters stays 0, Result.steps still lists the counted iterations).  diagonal: the Jacobi scaling from
    these numbers instead of A's own diagonal (what a diagonal left over from the operator's previous values would do)."""
    with np.errstate(all="ignore"):          # (infinities and NaN are values the control flow tests for, as on the device)
        return _solve(A, b, x0, rtol, atol, maxit, arith, variant, diagonal)


def _solve(A, b, x0, rtol, atol, maxit, arith, variant, diagonal):
    assert variant in VARIANTS, variant
    ar = arith if isinstance(arith, Arith) else Arith(arith)
    M = A if isinstance(A, Matrix) else Matrix(A, ar)
    n = M.n
    out = Result()
    out.arith = ar
    b = ar.vec(b)
    x = ar.vec(x0).copy()
    out.x = x
    if b.shape != (n,) or x.shape != (n,) or maxit < 0:
        out.status, out.message = INVALID, "invalid handles or size mismatch"
        return out
    if n == 0:
        return out
    dinv = M.dinv() if diagonal is None else ar.scalar(1) / ar.vec(diagonal)
    one = ar.scalar(1)
    st = {}                      # r, and the squared norms of the last residual() call

    def residual():
        r = b - M.dot(x)
        st["r"] = r
        return ar.dot(r, r), ar.dot(b, b)

    rr, bb = residual()
    if ar.exact:
        # no square roots: sqrt(q) <= tol  <=>  q <= tol^2 with tol^2 = max(rtol^2 b.b, atol^2)
        tol2 = max(Fraction(rtol) ** 2 * bb, Fraction(atol) ** 2)
        wide2 = tol2 * Fraction(1.0000001) ** 2
        above = lambda q: q > tol2                               # noqa: E731
        confirmed = lambda q: q <= wide2                         # noqa: E731
        rel = lambda q: math.sqrt(q / bb) if bb > 0 else math.sqrt(q)          # noqa: E731
    else:
        bnorm = ar.sqrt(bb)
        tol = max(ar.scalar(rtol) * bnorm, ar.scalar(atol))
        above = lambda q: bool(ar.sqrt(q) > tol)                  # noqa: E731
        confirmed = lambda q: bool(ar.sqrt(q) <= tol * ar.scalar(1.0000001))   # noqa: E731
        rel = lambda q: float(ar.sqrt(q) / bnorm) if bnorm > 0 else float(ar.sqrt(q))       # noqa: E731
    if ar.is_nan(rr):
        out.status, out.message = INVALID, "the start residual is not finite"
        return out

    def singular(what, it):
        out.status, out.message = SINGULAR, "breakdown (%s) after %d iterations" % (what, it)
        out.events.append("singular")
        return out

    def p_update(p, r, v, beta, omega):
        if variant == "p_plus_omega_v":
            return r + beta * (p + omega * v)
        return r + beta * (p - omega * v)

    def make_beta(rho_new, rho, alpha, omega):
        if variant == "beta_without_alpha_over_omega":
            return rho_new / rho
        return (rho_new / rho) * (alpha / omega)

    def x_update(x, y, z, alpha, omega):
        if variant == "x_without_omega_z":
            x += alpha * y
        else:
            x += alpha * y + omega * z

    it, restarts, fresh = 0, 0, True
    rho = alpha = omega = one
    rho_new = rr
    r = st["r"]
    rhat = p = v = y = z = None
    while above(rr) and it < maxit:
        if fresh:
            rhat, p, v = r.copy(), ar.zeros(n), ar.zeros(n)
            rho = alpha = omega = one
            rho_new = rr
            fresh = False
        beta = make_beta(rho_new, rho, alpha, omega)
        p = p_update(p, r, v, beta, omega)
        y = dinv * p
        v = M.dot(y)
        hv = ar.dot(rhat, v)
        if hv == 0 or ar.is_nan(hv):
            out.events.append("rhat.v=0")
            restarts += 1
            if restarts > 4:
                return singular("rhat . v = 0", it)
            rr, bb = residual()
            r = st["r"]
            fresh = True
            out.events.append("restart")
            continue
        alpha = rho_new / hv
        ar.note(beta, alpha)
        r = r - alpha * v                       # s
        z = dinv * r
        ss = ar.dot(r, r)
        it += 1
        if not above(ss):
            x += alpha * y
            rr = ss
            out.events.append("half-step")
            out.steps.append((x.copy(), alpha, None, beta))
            break
        t = M.dot(z)
        ts, tt = ar.dot(t, r), ar.dot(t, t)
        if tt == 0 or ar.is_nan(tt):
            x += alpha * y
            out.events.append("t.t=0")
            out.steps.append((x.copy(), alpha, None, beta))
            restarts += 1
            if restarts > 4:
                return singular("t . t = 0", it)
            rr, bb = residual()
            r = st["r"]
            fresh = True
            out.events.append("restart")
            continue
        omega = ts / tt
        ar.note(omega)
        x_update(x, y, z, alpha, omega)
        r = r - omega * t
        rr = ar.dot(r, r)
        rho = rho_new
        rho_new = ar.dot(rhat, r)
        out.steps.append((x.copy(), alpha, omega, beta))
        if ar.is_nan(rr):
            out.status, out.message = INVALID, "the residual is not finite after %d iterations" % it
            return out
        if omega == 0 or rho_new == 0:
            out.events.append("omega=0" if omega == 0 else "rho=0")
            if not above(rr):
                break
            restarts += 1
            if restarts > 4:
                return singular("omega or rho = 0", it)
            rr, bb = residual()
            r = st["r"]
            fresh = True
            out.events.append("restart")
    # the confirmation on the true residual, and the second legs from it
    for _ in range(3):
        rr, bb = residual()
        r = st["r"]
        out.events.append("confirm")
        if confirmed(rr) or it >= maxit:
            break
        out.events.append("leg")
        it2 = 0
        rhat, p, v = r.copy(), ar.zeros(n), ar.zeros(n)
        rho = alpha = omega = one
        rho_new = rr
        while above(rr) and it < maxit and it2 < 50:
            beta = make_beta(rho_new, rho, alpha, omega)
            p = p_update(p, r, v, beta, omega)
            y = dinv * p
            v = M.dot(y)
            hv = ar.dot(rhat, v)
            if hv == 0 or ar.is_nan(hv):
                out.events.append("leg:rhat.v=0")
                break
            alpha = rho_new / hv
            r = r - alpha * v
            z = dinv * r
            t = M.dot(z)
            ts, tt = ar.dot(t, r), ar.dot(t, t)
            if tt == 0 or ar.is_nan(tt):
                x += alpha * y
                out.events.append("leg:t.t=0")
                break
            omega = ts / tt
            x_update(x, y, z, alpha, omega)
            r = r - omega * t
            rr = ar.dot(r, r)
            rho, rho_new = rho_new, ar.dot(rhat, r)
            it += 1
            it2 += 1
            out.steps.append((x.copy(), alpha, omega, beta))
            if omega == 0 or rho_new == 0 or ar.is_nan(rr):
                out.events.append("leg:stop")
                break
    # (after a third leg rr is the recurrence's: it started from the true residual at most 50 iterations before)
    out.iters = it
    out.relres = rel(rr)
    ar.note(x)
    return out


def trajectory(A, b, x0, steps, arith="f64_asc", variant=None, diagonal=None):
    """x_1 .. x_K of the run with rtol = 1e-30, atol = 0, maxit = steps: after maxit = k the device vector holds exactly x_k (the
    confirmation pass at it == maxit leaves x alone), as long as no event ends the main loop early - fewer entries come back then."""
    res = solve(A, b, x0, rtol=1e-30, atol=0.0, maxit=steps, arith=arith, variant=variant, diagonal=diagonal)
    return [s[0] for s in res.steps], res


def _norm(v):
    v = np.asarray(v, dtype=np.longdouble)
    return float(np.sqrt(np.add.accumulate(v * v)[-1])) if v.size else 0.0


def noise(A, b, x0, steps=NOISE_STEPS):
    """noise_k for k = 1..steps: max over the two float64 orders of ||x_k(f64) - x_k(extended)|| / ||x_k(extended)||.  inf where
    one of the three runs has no k-th iterate (an event ended it early) or the distance is not finite."""
    te, _ = trajectory(A, b, x0, steps, "extended")
    runs = [trajectory(A, b, x0, steps, name)[0] for name in ("f64_asc", "f64_desc")]
    out = []
    for k in range(steps):
        if k >= len(te) or any(k >= len(t) for t in runs):
            out.append(float("inf"))
            continue
        den = _norm(te[k])
        worst = max(_norm(t[k].astype(np.longdouble) - te[k]) for t in runs) / den if den > 0 else float("inf")
        out.append(worst if math.isfinite(worst) else float("inf"))
    return out


def noise_table(cases):
    """{"<system>/<start>": [noise_1 .. noise_12]} for the systems of tests/bicgstab_cases.py (what tests/golden/bicgstab_noise.json holds)."""
    table = {}
    for case in cases:
        for start, x0 in case.starts.items():
            table["%s/%s" % (case.name, start)] = noise(case.A, case.b, x0)
    return table


def write_noise_table(path, cases):
    """Regenerate tests/golden/bicgstab_noise.json (needs the extended type):
    python -c "from tests import bicgstab_cases as C, bicgstab_reference as R; R.write_noise_table('tests/golden/bicgstab_noise.json', C.table_cases())" """
    import json
    doc = {"about": "noise_k, k = 1..%d, per system/start: tests/bicgstab_reference.py::noise_table" % NOISE_STEPS,
           "steps": NOISE_STEPS, "noise": noise_table(cases)}
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


def pinned_steps(noise_row):
    """K: the steps 1..K are pinned - 32 * noise_k <= CAP for every k up to K."""
    k = 0
    while k < len(noise_row) and FACTOR * noise_row[k] <= CAP:
        k += 1
    return k


def bound(noise_k):
    """Relative distance allowed between the device's x_k and the float64 restatement's."""
    return max(FACTOR * noise_k, 1e-14)
