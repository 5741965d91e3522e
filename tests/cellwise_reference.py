"""Exact rational reference for atoms with a cell-wise constant (DG0) coefficient (pgd_atom_assemble_cellwise), tests only, on
the machinery of tests/subdomain_reference.py.

cellwise_atom(lay, kind, a, b, w, kappa, mask) sums kappa_c times the exact local matrix of every (marked) cell c into the
layout's full CSR pattern, kappa_c taken as the exact rational value of the float.  The rounding scale is
S_ij = sum_c |kappa_c| |K_c,ij|, the (values, S) contract of ExactLayout.atom.

CellwiseNumpyBackend: CellNumpyBackend plus atom_cellwise, so that the frontend's DG0 grammar runs end to end on a machine
without a GPU.  `cellwise_atoms` lists (kind, da, db, nodal weight or None, field bytes, mask bytes or None) of every one built.
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np
import scipy.sparse as sps

from oracle import fem_numpy as F
from tests import exact_reference as X
from tests import subdomain_reference as SR
from tests import weighted_reference as W


def cellwise_atom(lay, kind, a=0, b=0, w=None, kappa=None, mask=None):
    """(exact values on the full CSR pattern, S) of sum_c kappa_c K_c over the cells with mask != 0 (mask None: every cell).
    lay: a WeightedExactLayout (every kind 1-9); kappa: one float per cell."""
    da = a if kind in (X.DUDV, X.CONV, W.WDUDV, W.WCONV) else 0
    db = b if kind in (X.DUDV, X.CONVT, W.WDUDV, W.WCONVT) else 0
    key = ("local", kind, da, db, None if w is None else np.asarray(w, dtype=np.float64).tobytes())
    if key not in lay._cache:
        lay._cache[key] = lay._local(kind, da, db, w)
    num, den = lay._cache[key]
    nn = num.shape[1]
    kappa = np.asarray(kappa, dtype=np.float64)
    assert kappa.shape == (num.shape[0],)
    sel = np.ones(num.shape[0], dtype=bool) if mask is None else np.asarray(mask) != 0
    vals = [Fraction(0)] * lay.nnz
    S = np.zeros(lay.nnz)
    pos = lay.pos.reshape(-1, nn * nn)
    numf = num.reshape(-1, nn * nn)
    for c in np.where(sel)[0]:
        d = den[c]
        k = Fraction(float(kappa[c]))
        ak = abs(float(kappa[c]))
        for p, q in zip(pos[c], numf[c]):
            if q:
                vals[p] += k * Fraction(q, d)
                S[p] += ak * abs(q) / d
    out = np.empty(lay.nnz, dtype=object)
    out[:] = vals
    return out, S


def dyadic_field(nc):
    """The mixed-sign dyadic field of the atom tests: kappa_c = +-(1 + 7 c mod 13) / 8, negative on every fifth cell."""
    c = np.arange(nc)
    return np.where(c % 5 == 4, -1.0, 1.0) * (1 + (7 * c) % 13) / 8.0


def level_field(nc, seed=0):
    """A seeded random 8-level field, kappa_c = 2^(l - 1), l = 0 ... 7 (0.5 ... 64)."""
    return 2.0 ** (np.random.default_rng(seed).integers(0, 8, nc) - 1.0)


def stiffness(coords, cells, kappa, kind=F.STIFF):
    """The oracle's sum_c kappa_c K_c for a field of few distinct values: one oracle atom per value."""
    n = coords.shape[0]
    A = sps.csr_matrix((n, n))
    for v in np.unique(kappa):
        if v != 0.0:
            A = A + float(v) * F.assemble_atom(coords, cells[kappa == v], kind)
    return A.tocsr()


class CellwiseNumpyBackend(SR.CellNumpyBackend):
    """CellNumpyBackend plus cell-weighted atoms (atom_cellwise): a field of at most 64 distinct values by the oracle, one atom
    per value (kinds 1-6); anything else from the exact reference, rounded once - tests only."""
    name = "oracle-numpy+cellwise"

    def __init__(self, *args, **kw):
        SR.CellNumpyBackend.__init__(self, *args, **kw)
        self.cellwise_atoms = []

    def atom_cellwise(self, mh, kind, da, db, w, c, mask=None):
        m = self._obj[mh]
        nc = m.cells.shape[0]
        kappa = np.asarray(self._obj[c], dtype=np.float64).copy()
        if kappa.size != nc:
            raise ValueError("atom_cellwise: the field has %d values, the mesh %d cells" % (kappa.size, nc))
        if mask is not None:
            mask = np.ascontiguousarray(mask).view(np.uint8)
            if mask.size != nc:
                raise ValueError("atom_cellwise: the mask has %d bytes, the mesh %d cells" % (mask.size, nc))
        sel = np.ones(nc, dtype=bool) if mask is None else mask != 0
        wv = np.asarray(self._obj[w], dtype=np.float64).copy() if w else None
        self.cellwise_atoms.append((kind, da, db, None if wv is None else wv.tobytes(), kappa.tobytes(),
                                    None if mask is None else mask.tobytes()))
        levels = np.unique(kappa[sel])
        if kind in W.NEW_KINDS or levels.size > 64:
            lay = self._exact.get(mh)
            if lay is None:
                lay = self._exact[mh] = W.WeightedExactLayout(m.coords, m.cells)
            vals, _ = cellwise_atom(lay, kind, da, db, wv, kappa, None if mask is None else mask)
            A = sps.csr_matrix((np.array([float(v) for v in vals]), m.cols.copy(), m.rp.copy()), shape=(m.n, m.n))
        else:
            A = sps.csr_matrix((m.n, m.n))
            for v in levels:
                if v != 0.0:
                    A = A + float(v) * F.assemble_atom(m.coords, m.cells[sel & (kappa == v)], kind, da, db, wv)
            A = A.tocsr()
        return self._put((mh, A))
