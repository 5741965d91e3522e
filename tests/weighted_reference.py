"""Exact rational reference for the weighted derivative atoms (tests only, CPU), on the machinery of tests/exact_reference.py.

Kinds (include/pgd_amd.h, row i = test function, column j = trial function, w the nodal weight in the layout's own space):
wdudv(a, b) int w u_{,a} v_{,b}, wconv(a) int w u_{,a} v, wconvt(b) int w u v_{,b}.

The reference tensors on the reference simplex: WD[i,j,m,k,l] = int N_m d_k N_i d_l N_j (exact_reference.reference_tensors)
and the one added here, WC[i,j,m,l] = int N_i N_m d_l N_j.  A cell maps them through its exact integer adjugate and
determinant as in ExactLayout; values are exact Fractions on the CSR pattern, with the rounding scale S_ij = sum over cells
|K_e,ij|, the same (values, S) contract as ExactLayout.atom.

WeightedNumpyBackend: the numpy oracle with facet atoms (tests/robin_reference.py) that serves kinds 7-9 from this reference,
so that the frontend's grammar for them runs on a machine without a GPU.
"""
from __future__ import annotations

import itertools
from fractions import Fraction

import numpy as np
import scipy.sparse as sps

from tests import exact_reference as X
from tests.robin_reference import FacetNumpyBackend

WDUDV, WCONV, WCONVT = 7, 8, 9
NEW_KINDS = (WDUDV, WCONV, WCONVT)
KIND_NAMES = {WDUDV: "wdudv", WCONV: "wconv", WCONVT: "wconvt"}
_WC = {}


def wc_tensor(D, degree):
    """(integer array, denominator) of WC[i,j,m,l] = int N_i N_m d_l N_j over the reference simplex."""
    key = (D, degree)
    if key not in _WC:
        N = X.lagrange_basis(D, degree)
        nn = len(N)
        T = np.empty((nn, nn, nn, D), dtype=object)
        for i in range(nn):
            for m in range(nn):
                nim = X._mul(N[i], N[m])
                for j in range(nn):
                    for l in range(D):
                        T[i, j, m, l] = X._int_ref(X._mul(nim, X._diff(N[j], l)), D)
        _WC[key] = X._as_int(T)
    return _WC[key]


def kinds_and_pairs(D):
    """Every (kind, a, b) of the weighted derivative kinds on a layout of dimension D."""
    out = []
    for a in range(D):
        out += [(WCONV, a, 0), (WCONVT, 0, a)] + [(WDUDV, a, b) for b in range(D)]
    return out


class WeightedExactLayout(X.ExactLayout):
    """ExactLayout with the atoms of kinds 7-9 (every other kind as before)."""

    def _local(self, kind, a, b, w):
        if kind not in NEW_KINDS:
            return X.ExactLayout._local(self, kind, a, b, w)
        D, s = self.D, self.s
        adj = self.adj
        wi, t = X._dyadic_ints(np.asarray(w, dtype=np.float64)[self.cells])             # (nc, nn)
        if kind == WDUDV:
            Ti, Td = X.reference_tensors(D, self.degree)["WD"]
            P = adj[:, :, b][:, :, None] * adj[:, :, a][:, None, :]                      # P[c,k,l] = adj[k,b] adj[l,a]
            H = np.tensordot(P, Ti, axes=([1, 2], [3, 4]))                                 # (nc, i, j, m)
            num = (H * wi[:, None, None, :]).sum(axis=-1)
            return self._scaled(num, Td * self.absdet, s * (2 - D) - t)
        Ci, Cd = wc_tensor(D, self.degree)
        d = a if kind == WCONV else b
        H = np.tensordot(adj[:, :, d], Ci, axes=([1], [3]))                               # (nc, i, j, m): sum_l adj[l,d] WC[i,j,m,l]
        num = (H * wi[:, None, None, :]).sum(axis=-1) * self.sign[:, None, None]
        if kind == WCONVT:
            num = np.transpose(num, (0, 2, 1))
        return self._scaled(num, np.full(len(self.det), Cd, dtype=object), s * (1 - D) - t)

    def atom(self, kind, a=0, b=0, w=None):
        if kind not in NEW_KINDS:
            return X.ExactLayout.atom(self, kind, a, b, w)
        a = a if kind in (WDUDV, WCONV) else 0
        b = b if kind in (WDUDV, WCONVT) else 0
        key = (kind, a, b, np.asarray(w, dtype=np.float64).tobytes())
        if key not in self._cache:
            num, den = self._local(kind, a, b, w)
            nn = num.shape[1]
            vals = [Fraction(0)] * self.nnz
            S = np.zeros(self.nnz)
            pos = self.pos.reshape(-1, nn * nn)
            numf = num.reshape(-1, nn * nn)
            for c in range(numf.shape[0]):
                dc = den[c]
                for p, q in zip(pos[c], numf[c]):
                    if q:
                        vals[p] += Fraction(q, dc)
                        S[p] += abs(q) / dc
            out = np.empty(self.nnz, dtype=object)
            out[:] = vals
            self._cache[key] = (out, S)
        return self._cache[key]


def self_check(D, degree, coords, cells, seed=0):
    """q . (A p) against sympy's integrate over a small domain for random polynomials p, q, w of the space, every new kind
    and (a, b) - exact equality."""
    import sympy as sp

    rng = np.random.default_rng(seed)
    xs = sp.symbols("x0:%d" % D)
    monos = [e for e in itertools.product(range(degree + 1), repeat=D) if sum(e) <= degree]

    def rand_poly():
        return sum(int(rng.integers(-4, 5)) * sp.prod([xs[k] ** e[k] for k in range(D)]) for e in monos)

    lay = WeightedExactLayout(coords, cells)
    p, q, w = rand_poly(), rand_poly(), rand_poly() + 9
    nodes = [[sp.Rational(Fraction(float(v))) for v in row] for row in lay.coords]
    pf = [Fraction(int(v.p), int(v.q)) for v in (sp.Rational(p.subs(dict(zip(xs, x)))) for x in nodes)]
    qf = [Fraction(int(v.p), int(v.q)) for v in (sp.Rational(q.subs(dict(zip(xs, x)))) for x in nodes)]
    wv = np.array([float(w.subs(dict(zip(xs, x)))) for x in nodes])
    xi = sp.symbols("xi0:%d" % D)

    def integrate(expr):
        tot = sp.Integer(0)
        for c in lay.cells:
            V = [nodes[v] for v in c[:D + 1]]
            sub = {xs[a]: V[0][a] + sum((V[k + 1][a] - V[0][a]) * xi[k] for k in range(D)) for a in range(D)}
            J = sp.Matrix(D, D, lambda a, k: V[k + 1][a] - V[0][a])
            f = sp.expand(expr.subs(sub)) * abs(J.det())
            for k in reversed(range(D)):
                f = sp.integrate(f, (xi[k], 0, 1 - sum(xi[:k])))
            tot += f
        return tot

    for kind, a, b in kinds_and_pairs(D):
        if kind == WDUDV:
            integrand = w * sp.diff(p, xs[a]) * sp.diff(q, xs[b])
        elif kind == WCONV:
            integrand = w * sp.diff(p, xs[a]) * q
        else:
            integrand = w * p * sp.diff(q, xs[b])
        vals, _ = lay.atom(kind, a, b, wv)
        got = X.exact_dot(qf, lay.matvec(vals, pf))
        want = integrate(integrand)
        assert got == Fraction(int(want.p), int(want.q)), (D, degree, KIND_NAMES[kind], a, b, got, want)
    return True


class WeightedNumpyBackend(FacetNumpyBackend):
    """The numpy oracle with facet atoms, and kinds 7-9 from the exact reference (rounded once) - tests only."""
    name = "oracle-numpy+weighted"

    def __init__(self, *args, **kw):
        FacetNumpyBackend.__init__(self, *args, **kw)
        self._exact = {}
        self.assembled = []          # (kind, da, db) of every kind 7-9 atom built, in order

    def atom(self, mh, kind, da, db, w):
        if kind not in NEW_KINDS:
            return FacetNumpyBackend.atom(self, mh, kind, da, db, w)
        m = self._obj[mh]
        if not w or np.asarray(self._obj[w]).size != m.n:
            raise ValueError("weighted kind needs a vertex weight vector")
        lay = self._exact.get(mh)
        if lay is None:
            lay = self._exact[mh] = WeightedExactLayout(m.coords, m.cells)
        vals, _ = lay.atom(kind, da, db, np.asarray(self._obj[w], dtype=np.float64).copy())
        self.assembled.append((kind, da, db))
        A = sps.csr_matrix((np.array([float(v) for v in vals]), m.cols.copy(), m.rp.copy()), shape=(m.n, m.n))
        return self._put((mh, A))
