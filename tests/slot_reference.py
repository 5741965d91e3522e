"""Plain reference of the host-driven PCG pieces (include/pgd_amd.h, "distributed PCG pieces"): a state of numpy vectors, the
64 scalar slots and the three flags, and one function per piece that does what the header says, entry by entry.

Independent of oracle/backend_numpy.py (which is itself checked against this module).

Elementwise results are exact: the kernels form every scalar by one IEEE division, every entry by explicit fma calls and plain
products, so ``fma`` below (one correctly rounded a*b+c through rationals) and float64 products reproduce them bit for bit.
Sums are the exact sums, rounded once (``exact_dot``); every reducing piece also records sum |a_i b_i| of each slot it writes in
``State.mag`` so that a caller can form a rounding bound for a device sum.
"""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

NSLOTS = 64
ERR_SINGULAR = -5
S_TOL2, S_LAST_RR = 5, 6          # written by cg_scalars (both) and check (S_LAST_RR) whatever indices the caller passes
CG_SCRATCH = (40, 41, 42)         # cg_init reduces into these before it places the sums


class State:
    def __init__(self, vecs, slots=None, flags=(0, 0, 0)):
        self.v = {k: np.array(a, dtype=np.float64, copy=True) for k, a in vecs.items()}
        self.S = np.zeros(NSLOTS) if slots is None else np.array(slots, dtype=np.float64, copy=True)
        assert self.S.size == NSLOTS
        self.flags = [int(f) for f in flags]          # done, iterations, status
        self.mag = {}                                 # slot -> sum |a_i b_i| of the last sum written there
        self.vmag = {}                                # vector -> per entry, the sum of the |terms| on the path to its last value
                                                      # (what a rounding bound of another evaluation order is relative to)

    def copy(self):
        c = State(self.v, self.S, self.flags)
        c.mag = dict(self.mag)
        c.vmag = {k: a.copy() for k, a in self.vmag.items()}
        return c


def fma_fraction(a, b, c):
    """One correctly rounded a * b + c: the definition (finite arguments)."""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def fma(a, b, c):
    """One correctly rounded a * b + c.  Same value as ``fma_fraction`` without its gcd work: a float is an integer over a power of
    two, and Python's int / int is correctly rounded."""
    a, b, c = float(a), float(b), float(c)
    if a == 0.0 or b == 0.0 or not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        return a * b + c                              # the product is exact (or the result is not a number to round)
    na, da = a.as_integer_ratio()
    nb, db = b.as_integer_ratio()
    nc, dc = c.as_integer_ratio()
    return (na * nb * dc + nc * da * db) / (da * db * dc)


def fma_vec(a, b, c):
    """fma entry by entry; every argument a scalar or an array of the common length."""
    A, B, Cc = np.broadcast_arrays(*(np.asarray(t, dtype=np.float64) for t in (a, b, c)))
    A, B, Cc = A.reshape(-1), B.reshape(-1), Cc.reshape(-1)
    n = A.size
    return np.array([fma(A[i], B[i], Cc[i]) for i in range(n)], dtype=np.float64)


def two_product(a, b):
    """(h, l) with h + l == a * b exactly, entry by entry (Veltkamp split + Dekker product; no overflow or underflow for the
    magnitudes the tests use: 1e-12 < |a|, |b| < 1e12)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    h = a * b
    f = 134217729.0                                   # 2^27 + 1
    ta, tb = f * a, f * b
    a1 = ta - (ta - a); a2 = a - a1
    b1 = tb - (tb - b); b2 = b - b1
    l = a2 * b2 - (((h - a1 * b1) - a2 * b1) - a1 * b2)
    return h, l


def exact_dot(a, b):
    """sum a_i b_i, exact, rounded once."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.size == 0:
        return 0.0
    if not (np.all(np.isfinite(a)) and np.all(np.isfinite(b))):
        return float(a @ b)
    h, l = two_product(a, b)
    return math.fsum(np.concatenate([h, l]).tolist())


def abs_dot(a, b):
    return float(np.abs(np.asarray(a, dtype=np.longdouble)) @ np.abs(np.asarray(b, dtype=np.longdouble)))


def _range(n, lo, hi):
    if hi < 0:
        hi = n
    assert 0 <= lo <= hi <= n, "bad range"
    return slice(lo, hi)


def _mag(st, name, k, values):
    m = np.zeros(st.v[name].size)
    m[k] = values
    st.vmag[name] = m


def _sum(st, slot, a, b):
    st.S[slot] = exact_dot(a, b)
    st.mag[slot] = abs_dot(a, b)


def _tol2(rtol, atol, bb):
    t1, t2 = rtol * rtol * bb, atol * atol
    return t1 if t1 > t2 else t2


def _nan(x):
    return x != x


# ------------------------------------------------------------------ the two-reduction recurrence
def pcg_init(st, b, q, dinv, r, z, p, lo, hi, slot):
    """r = b - q, z = dinv r, p = z on [lo, hi); S[slot..slot+2] <- (r.z, r.r, b.b).  Not gated by the done flag."""
    v = st.v
    k = _range(v[b].size, lo, hi)
    _mag(st, r, k, np.abs(v[b][k]) + np.abs(v[q][k]))
    v[r][k] = v[b][k] - v[q][k]
    v[z][k] = v[dinv][k] * v[r][k]
    v[p][k] = v[z][k]
    for t in (z, p):
        _mag(st, t, k, v[dinv][k] * st.vmag[r][k])
    _sum(st, slot, v[r][k], v[z][k])
    _sum(st, slot + 1, v[r][k], v[r][k])
    _sum(st, slot + 2, v[b][k], v[b][k])


def pcg_tol(st, rtol, atol, s_rr, s_bb, s_tol2):
    """S[tol2] <- max(rtol^2 S[bb], atol^2); done <- S[rr] <= tol2; a NaN in S[rr] is a breakdown.  Not gated by the done flag."""
    tol2 = _tol2(rtol, atol, st.S[s_bb])
    st.S[s_tol2] = tol2
    rr = st.S[s_rr]
    if _nan(rr):
        st.flags[0], st.flags[2] = 1, ERR_SINGULAR
    elif rr <= tol2:
        st.flags[0] = 1


def pcg_xr(st, x, r, p, q, dinv, z, lo, hi, s_rz, s_pq, s_out):
    """alpha = S[rz] / S[pq]; x += alpha p; r -= alpha q; z = dinv r; S[out..out+1] <- (r.z, r.r)."""
    if st.flags[0]:
        return
    v = st.v
    k = _range(v[x].size, lo, hi)
    alpha = st.S[s_rz] / st.S[s_pq]
    _mag(st, x, k, np.abs(alpha * v[p][k]) + np.abs(v[x][k]))
    _mag(st, r, k, np.abs(alpha * v[q][k]) + np.abs(v[r][k]))
    _mag(st, z, k, v[dinv][k] * st.vmag[r][k])
    v[x][k] = fma_vec(alpha, v[p][k], v[x][k])
    v[r][k] = fma_vec(-alpha, v[q][k], v[r][k])
    v[z][k] = v[dinv][k] * v[r][k]
    _sum(st, s_out, v[r][k], v[z][k])
    _sum(st, s_out + 1, v[r][k], v[r][k])


def pcg_check(st, s_rr, s_tol2):
    """iterations += 1; S[6] <- S[rr]; done <- S[rr] <= S[tol2], or breakdown on a NaN."""
    if st.flags[0]:
        return
    rr = st.S[s_rr]
    st.S[S_LAST_RR] = rr
    st.flags[1] += 1
    if _nan(rr):
        st.flags[0], st.flags[2] = 1, ERR_SINGULAR
    elif rr <= st.S[s_tol2]:
        st.flags[0] = 1


def pcg_p(st, p, z, lo, hi, s_num, s_den):
    """beta = S[num] / S[den]; p = z + beta p."""
    if st.flags[0]:
        return
    v = st.v
    k = _range(v[p].size, lo, hi)
    beta = st.S[s_num] / st.S[s_den]
    _mag(st, p, k, np.abs(beta * v[p][k]) + np.abs(v[z][k]))
    v[p][k] = fma_vec(beta, v[p][k], v[z][k])


# ------------------------------------------------------------------ the single-reduction recurrence
def cg_init(st, b, q, dinv, r, u, p, s, lo, hi, base):
    """r = b - q, u = dinv r, p = s = 0; S[base], S[base+1], S[base+8] <- (r.u, r.r, b.b); slots 40..42 are scratch (they hold the
    same three sums afterwards).  Not gated by the done flag."""
    v = st.v
    k = _range(v[b].size, lo, hi)
    _mag(st, r, k, np.abs(v[b][k]) + np.abs(v[q][k]))
    _mag(st, u, k, v[dinv][k] * st.vmag[r][k])
    _mag(st, p, k, 0.0)
    _mag(st, s, k, 0.0)
    v[r][k] = v[b][k] - v[q][k]
    v[u][k] = v[dinv][k] * v[r][k]
    v[p][k] = 0.0
    v[s][k] = 0.0
    for j, (a_, b_) in zip(CG_SCRATCH, ((r, u), (r, r), (b, b))):
        _sum(st, j, v[a_][k], v[b_][k])
    for dst, src in ((base, 40), (base + 1, 41), (base + 8, 42)):      # (in the order of the device copies: base may overlap 40..42)
        st.S[dst] = st.S[src]
        st.mag[dst] = st.mag[src]


def cg_update(st, x, r, u, w, p, s, dinv, lo, hi, base):
    """p = u + beta p; s = w + beta s; x += alpha p; r -= alpha s; u = dinv r; S[base..base+1] <- (r.u, r.r)."""
    if st.flags[0]:
        return
    v = st.v
    k = _range(v[x].size, lo, hi)
    alpha, beta = st.S[base + 5], st.S[base + 6]
    _mag(st, p, k, np.abs(beta * v[p][k]) + np.abs(v[u][k]))
    _mag(st, s, k, np.abs(beta * v[s][k]) + np.abs(v[w][k]))
    _mag(st, x, k, np.abs(alpha) * st.vmag[p][k] + np.abs(v[x][k]))
    _mag(st, r, k, np.abs(alpha) * st.vmag[s][k] + np.abs(v[r][k]))
    _mag(st, u, k, v[dinv][k] * st.vmag[r][k])
    v[p][k] = fma_vec(beta, v[p][k], v[u][k])
    v[s][k] = fma_vec(beta, v[s][k], v[w][k])
    v[x][k] = fma_vec(alpha, v[p][k], v[x][k])
    v[r][k] = fma_vec(-alpha, v[s][k], v[r][k])
    v[u][k] = v[dinv][k] * v[r][k]
    _sum(st, base, v[r][k], v[u][k])
    _sum(st, base + 1, v[r][k], v[r][k])


def cg_scalars(st, base, init, rtol, atol):
    """After the all-reduce of S[base..base+4]: tol^2 into S[5] (init), iterations += 1 (otherwise), S[6] <- r.r, the stop test,
    then beta = g / S[base+7], alpha = g / (d - beta g / S[base+5]) with d = S[base+2] + S[base+3] + S[base+4]."""
    if st.flags[0]:
        return
    S = st.S
    g, rr = S[base], S[base + 1]
    d = (S[base + 2] + S[base + 3]) + S[base + 4]
    if init:
        S[S_TOL2] = _tol2(rtol, atol, S[base + 8])
    else:
        st.flags[1] += 1
    S[S_LAST_RR] = rr
    if _nan(rr) or _nan(d):
        st.flags[0], st.flags[2] = 1, ERR_SINGULAR
        return
    if rr <= S[S_TOL2]:
        st.flags[0] = 1
        return
    with np.errstate(all="ignore"):
        g, d = np.float64(g), np.float64(d)
        beta = np.float64(0.0) if init else g / S[base + 7]
        alpha = g / d if init else g / (d - (beta * g) / S[base + 5])
    S[base + 5], S[base + 6], S[base + 7] = alpha, beta, g


# ------------------------------------------------------------------ the product
def spmv_dot_slot(st, A, x, y, w, r0, r1, slot):
    """y = A x on the rows [r0, r1); S[slot] <- sum w_i y_i over them.  (The order in which a product kernel adds the terms of a
    row is its own, so y is NOT bit-determined: callers compare it with a rounding bound; the sum is exact for this y.)"""
    if st.flags[0]:
        return
    v = st.v
    k = _range(v[x].size, r0, r1)
    if k.stop > k.start:
        v[y][k] = A[k.start:k.stop] @ v[x]
    _sum(st, slot, v[w][k], v[y][k])


# ------------------------------------------------------------------ the pieces under the backends' method names
class RefBackend:
    """The reference with the method names and argument order of the backends (pgdrome_amd/_lib.py::Context,
    oracle/backend_numpy.py::NumpyBackend); vectors are named by their keys in the state, an operator is a scipy matrix."""

    def __init__(self, st):
        self.st = st

    def flags(self):
        return tuple(self.st.flags)

    def flags_reset(self):
        self.st.flags = [0, 0, 0]

    def slots_get(self, first=0, count=NSLOTS):
        return self.st.S[first:first + count].copy()

    def slots_set(self, vals, first=0):
        vals = np.asarray(vals, dtype=np.float64)
        self.st.S[first:first + vals.size] = vals

    def spmv(self, A, x, y, r0=0, r1=-1):
        k = _range(self.st.v[x].size, r0, r1)
        if k.stop > k.start:
            self.st.v[y][k] = A[k.start:k.stop] @ self.st.v[x]

    def spmv_dot_slot(self, A, x, y, w, r0, r1, slot):
        spmv_dot_slot(self.st, A, x, y, w, r0, r1, slot)

    def pcg_init_slot(self, *a):
        pcg_init(self.st, *a)

    def pcg_tol_slot(self, *a):
        pcg_tol(self.st, *a)

    def pcg_xr_slot(self, *a):
        pcg_xr(self.st, *a)

    def pcg_check_slot(self, *a):
        pcg_check(self.st, *a)

    def pcg_p_slot(self, *a):
        pcg_p(self.st, *a)

    def cg_init_slot(self, *a):
        cg_init(self.st, *a)

    def cg_update_slot(self, *a):
        cg_update(self.st, *a)

    def cg_scalars_slot(self, *a):
        cg_scalars(self.st, *a)


# ------------------------------------------------------------------ whole recurrences, in the call order of pgdrome_amd/dist.py
S_PQ, S_INIT, S_PAIR, CG_BASE = 2, 16, 20, 24
HALF = 27         # slot offset of a second row range in the same bank: clear of 0..32 and of the scratch triple 40..42 (cg form)


class HostAllreduce:
    """Stand-in for the all-reduce between row ranges that share ONE slot bank: the ranges' slot blocks (the first at ``first``, the
    others ``offsets`` further on) are downloaded, added in range order and the sum is uploaded to every block - afterwards every
    range reads the same numbers from its own indices, as every rank does from its own bank.  ``mirror`` copies slots the scalar
    step of the first block wrote (every rank runs that step itself on identical inputs)."""

    def __init__(self, be, offsets):
        self.be, self.offsets = be, [o for o in offsets if o]

    def __call__(self, first, count):
        if not self.offsets:
            return
        S = np.array(self.be.slots_get(0, NSLOTS), dtype=np.float64)
        tot = S[first:first + count].copy()
        for o in self.offsets:
            tot = tot + S[first + o:first + o + count]
        for o in [0] + self.offsets:
            S[first + o:first + o + count] = tot
        self.be.slots_set(S, 0)

    def mirror(self, first, count):
        if not self.offsets:
            return
        S = np.array(self.be.slots_get(0, NSLOTS), dtype=np.float64)
        for o in self.offsets:
            S[first + o:first + o + count] = S[first:first + count]
        self.be.slots_set(S, 0)


def pcg_round(be, op, V, ranges, allreduce, k, rz_old):
    """One iteration of dist.py::pcg; returns the slot that holds r.z afterwards."""
    out = S_PAIR + 2 * (k & 1)
    for lo, hi, o in ranges:
        be.spmv_dot_slot(op, V["p"], V["q"], V["p"], lo, hi, S_PQ + o)
    allreduce(S_PQ, 1)
    for lo, hi, o in ranges:
        be.pcg_xr_slot(V["x"], V["r"], V["p"], V["q"], V["dinv"], V["z"], lo, hi, rz_old + o, S_PQ + o, out + o)
    allreduce(out, 2)
    be.pcg_check_slot(out + 1, S_TOL2)
    for lo, hi, o in ranges:
        be.pcg_p_slot(V["p"], V["z"], lo, hi, out + o, rz_old + o)
    return out


def drive_pcg(be, op, V, ranges, rtol, atol, maxit):
    """dist.py::pcg over the row ranges ``ranges`` = [(lo, hi, slot offset)] of one bank; V: vector name -> the backend's key for
    x b r z p q dinv (dinv filled by the caller).  Returns (rounds run, slot of the last r.z)."""
    allreduce = HostAllreduce(be, [o for _, _, o in ranges])
    be.flags_reset()
    for lo, hi, o in ranges:
        be.spmv(op, V["x"], V["q"], lo, hi)
        be.pcg_init_slot(V["b"], V["q"], V["dinv"], V["r"], V["z"], V["p"], lo, hi, S_INIT + o)
    allreduce(S_INIT, 3)
    be.pcg_tol_slot(rtol, atol, S_INIT + 1, S_INIT + 2, S_TOL2)
    rz_old, k = S_INIT, 0
    while k < maxit and not be.flags()[0]:
        rz_old = pcg_round(be, op, V, ranges, allreduce, k, rz_old)
        k += 1
    return k, rz_old


def cg_round(be, op, V, ranges, allreduce, rtol, atol):
    """One iteration of dist.py::pcg_single_reduction (the three w.u slots: all rows of a range count as interior rows)."""
    B = CG_BASE
    for lo, hi, o in ranges:
        be.cg_update_slot(V["x"], V["r"], V["u"], V["w"], V["p"], V["s"], V["dinv"], lo, hi, B + o)
    for lo, hi, o in ranges:                  # (the products read u on all rows: after every range's update, as after a halo exchange)
        be.spmv_dot_slot(op, V["u"], V["w"], V["u"], lo, hi, B + 2 + o)
    allreduce(B, 5)
    be.cg_scalars_slot(B, 0, rtol, atol)
    allreduce.mirror(B + 5, 3)


def drive_cg(be, op, V, ranges, rtol, atol, maxit):
    """dist.py::pcg_single_reduction over the row ranges; V names x b r u w p s q dinv.  Returns the rounds run."""
    B = CG_BASE
    allreduce = HostAllreduce(be, [o for _, _, o in ranges])
    be.flags_reset()
    for lo, hi, o in ranges:
        be.slots_set(np.zeros(9), B + o)
        be.spmv(op, V["x"], V["q"], lo, hi)
        be.cg_init_slot(V["b"], V["q"], V["dinv"], V["r"], V["u"], V["p"], V["s"], lo, hi, B + o)
    for lo, hi, o in ranges:
        be.spmv_dot_slot(op, V["u"], V["w"], V["u"], lo, hi, B + 2 + o)
    allreduce(B, 9)
    be.cg_scalars_slot(B, 1, rtol, atol)
    allreduce.mirror(B + 5, 3)
    k = 0
    while k < maxit and not be.flags()[0]:
        cg_round(be, op, V, ranges, allreduce, rtol, atol)
        k += 1
    return k


# ------------------------------------------------------------------ cases shared by the CPU and the GPU tests
SIZES = (1, 2, 255, 256, 257, 1000)
LONG = 2 * 2048 * 256 + 259       # 1 048 835: the one-entry-per-lane kernels (grid cap 2048 x 256 lanes) take a third trip, the
                                  # two-entries-per-lane kernels a second one, both with a ragged tail
SENTINEL = -777.25                # prefill of pure output vectors


def ranges_for(n):
    """[(label, lo, hi)]: whole; lo even with an odd / an even count; lo odd; one entry at an even and at an odd lo; empty in the
    middle and at n.  Shapes a size is too small for are left out, duplicates too."""
    def end(lo, parity):
        for hi in (n - 3, n - 2, n - 1, n):
            if hi > lo and (hi - lo) % 2 == parity:
                return hi
        return None
    le, lod = (2, 3) if n > 8 else (0, 1)
    cand = [("whole", 0, -1), ("even_lo_odd_count", le, end(le, 1)), ("even_lo_even_count", le, end(le, 0)),
            ("odd_lo", lod, end(lod, 1) if lod < n else None), ("odd_lo_even_count", lod, end(lod, 0) if lod < n else None),
            ("one_at_even", 2 * (n // 4), 2 * (n // 4) + 1), ("one_at_odd", 2 * (n // 4) + 1, 2 * (n // 4) + 2),
            ("empty_mid", n // 2, n // 2), ("empty_end", n, n)]
    out, seen = [], set()
    for label, lo, hi in cand:
        if hi is None or hi > n or lo > n or (lo, hi) in seen:
            continue
        seen.add((lo, hi))
        out.append((label, lo, hi))
    return out


def all_cases(sizes=SIZES):
    return [(n, label, lo, hi) for n in sizes for label, lo, hi in ranges_for(n)]


def case_id(c):
    return "n%d-%s" % (c[0], c[1])


def wide(rng, n):
    """standard normal times 10^uniform(-3, 3): a lost entry moves a sum visibly."""
    return rng.standard_normal(n) * 10.0 ** rng.uniform(-3.0, 3.0, n)


def make_state(n, seed, outputs=()):
    """All vectors of both recurrences with wide-range data, dinv in [0.5, 2], the pure ``outputs`` prefilled with SENTINEL; slots
    hold 1000 + i."""
    rng = np.random.default_rng(seed)
    v = {k: wide(rng, n) for k in ("x", "b", "r", "z", "u", "w", "p", "s", "q")}
    v["dinv"] = rng.uniform(0.5, 2.0, n)
    for k in outputs:
        v[k][:] = SENTINEL
    return State(v, 1000.0 + np.arange(NSLOTS))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.array_equal(bits(a), bits(b)))


def hull_problem(mesh):
    """(A, b, x*, n): K + M with the hull eliminated on F.box_mesh(..., 8, 7, 6) (``mesh`` = "box") or F.interval_mesh(32), a smooth
    right-hand side, and the direct solution."""
    from oracle import fem_numpy as F
    coords, cells = F.box_mesh((0, 0, 0), (1, 1, 1), 8, 7, 6) if mesh == "box" else F.interval_mesh(32)
    coords = coords.reshape(coords.shape[0], -1)
    n = coords.shape[0]
    K, M = F.assemble_atom(coords, cells, F.STIFF), F.assemble_atom(coords, cells, F.MASS)
    lo, hi = coords.min(axis=0), coords.max(axis=0)
    bc = np.where(np.any((coords <= lo + 1e-12) | (coords >= hi - 1e-12), axis=1))[0].astype(np.int32)
    rhs = M @ (1.0 + np.sin(3.0 * coords).sum(axis=1))
    A, b = F.apply_dirichlet((K + M).tocsr(), rhs, bc)
    return dict(A=A, b=b, sol=F.direct_solve(A, b), n=n, coords=coords, cells=cells, bc=bc)
