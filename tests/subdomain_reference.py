"""Exact rational reference for cell-subdomain atoms (dx(id): the atom of pgd_atom_assemble over a subset of the cells), tests
only, on the machinery of tests/exact_reference.py and tests/weighted_reference.py.

subset_atom(lay, kind, a, b, w, mask) sums the exact local matrices of the marked cells alone into the layout's FULL CSR
pattern: an entry that no marked cell touches is an exact 0.  The rounding scale S_ij = sum over the marked cells |K_e,ij|,
the (values, S) contract of ExactLayout.atom.

CellNumpyBackend: the numpy oracle with facet atoms and kinds 7-9 (WeightedNumpyBackend) plus masked atoms (atom_cells), so
that the frontend's dx(id) grammar runs end to end on a machine without a GPU.
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np
import scipy.sparse as sps

from oracle import fem_numpy as F
from tests import exact_reference as X
from tests import weighted_reference as W


def subset_atom(lay, kind, a=0, b=0, w=None, mask=None):
    """(exact values on the full CSR pattern, S) of the atom over the cells with mask != 0 (mask None: every cell).
    lay: a WeightedExactLayout (every kind 1-9)."""
    da = a if kind in (X.DUDV, X.CONV, W.WDUDV, W.WCONV) else 0
    db = b if kind in (X.DUDV, X.CONVT, W.WDUDV, W.WCONVT) else 0
    key = ("local", kind, da, db, None if w is None else np.asarray(w, dtype=np.float64).tobytes())
    if key not in lay._cache:
        lay._cache[key] = lay._local(kind, da, db, w)
    num, den = lay._cache[key]
    nn = num.shape[1]
    sel = np.ones(num.shape[0], dtype=bool) if mask is None else np.asarray(mask) != 0
    vals = [Fraction(0)] * lay.nnz
    S = np.zeros(lay.nnz)
    pos = lay.pos.reshape(-1, nn * nn)
    numf = num.reshape(-1, nn * nn)
    for c in np.where(sel)[0]:
        d = den[c]
        for p, q in zip(pos[c], numf[c]):
            if q:
                vals[p] += Fraction(q, d)
                S[p] += abs(q) / d
    out = np.empty(lay.nnz, dtype=object)
    out[:] = vals
    return out, S


def touched(lay, mask):
    """Per CSR entry of the layout: does a marked cell couple its row and column?"""
    out = np.zeros(lay.nnz, dtype=bool)
    out[lay.pos[np.asarray(mask) != 0].ravel()] = True
    return out


def masks(nc, seed=0):
    """The four masks of the atom tests: a seeded random half, one cell, none, all."""
    rng = np.random.default_rng(seed)
    half = np.zeros(nc, dtype=np.uint8)
    half[rng.permutation(nc)[:nc // 2]] = 1
    one = np.zeros(nc, dtype=np.uint8)
    one[int(rng.integers(nc))] = 1
    return {"half": half, "one": one, "none": np.zeros(nc, dtype=np.uint8), "all": np.ones(nc, dtype=np.uint8)}


def on_pattern(A, rp, cols):
    """Values of a scipy matrix at the entries of a CSR pattern, in pattern order."""
    rows = np.repeat(np.arange(rp.size - 1), np.diff(rp))
    return np.asarray(A.tocsr()[rows, cols]).ravel()


class CellNumpyBackend(W.WeightedNumpyBackend):
    """WeightedNumpyBackend plus masked atoms (atom_cells): kinds 1-6 by the oracle over the marked cells, kinds 7-9 from the
    exact reference (rounded once) - tests only.  `cell_atoms` lists (kind, da, db, marked cell count) of every one built."""
    name = "oracle-numpy+cells"

    def __init__(self, *args, **kw):
        W.WeightedNumpyBackend.__init__(self, *args, **kw)
        self.cell_atoms = []

    def atom_cells(self, mh, kind, da, db, w, mask):
        m = self._obj[mh]
        mask = np.ascontiguousarray(mask).view(np.uint8)
        if mask.size != m.cells.shape[0]:
            raise ValueError("atom_cells: the mask has %d bytes, the mesh %d cells" % (mask.size, m.cells.shape[0]))
        sel = mask != 0
        wv = np.asarray(self._obj[w], dtype=np.float64).copy() if w else None
        self.cell_atoms.append((kind, da, db, int(sel.sum())))
        if kind in W.NEW_KINDS:
            lay = self._exact.get(mh)
            if lay is None:
                lay = self._exact[mh] = W.WeightedExactLayout(m.coords, m.cells)
            vals, _ = subset_atom(lay, kind, da, db, wv, mask)
            A = sps.csr_matrix((np.array([float(v) for v in vals]), m.cols.copy(), m.rp.copy()), shape=(m.n, m.n))
        elif sel.any():
            A = F.assemble_atom(m.coords, m.cells[sel], kind, da, db, wv)
        else:
            A = sps.csr_matrix((m.n, m.n))
        return self._put((mh, A))
