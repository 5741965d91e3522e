"""Reference boundary-mass matrices for the Robin tests, written from the closed-form facet masses
(not from the library's kernel): int_Gamma phi_i phi_j ds over facets given as node tuples of a layout
(vertices first, then for P2 the edge nodes in the UFC local order), assembled with scipy.

Also a test-only backend: the numpy oracle plus facet atoms from these matrices, so that the frontend's
ds grammar runs end to end on a machine without a GPU."""
import numpy as np
import scipy.sparse as sps

from oracle.backend_numpy import NumpyBackend

_P2_EDGE = np.array([[4.0, -1.0, 2.0], [-1.0, 4.0, 2.0], [2.0, 2.0, 16.0]]) / 30.0
_P2_TRI = np.array([[6.0, -1.0, -1.0, -4.0, 0.0, 0.0],
                    [-1.0, 6.0, -1.0, 0.0, -4.0, 0.0],
                    [-1.0, -1.0, 6.0, 0.0, 0.0, -4.0],
                    [-4.0, 0.0, 0.0, 32.0, 16.0, 16.0],
                    [0.0, -4.0, 0.0, 16.0, 32.0, 16.0],
                    [0.0, 0.0, -4.0, 16.0, 16.0, 32.0]]) / 180.0


def local_facet_mass(gdim, npf):
    """Facet mass per unit measure: (npf x npf)."""
    if gdim == 1:
        return np.ones((1, 1))
    if npf == gdim:                                      # P1 edge / triangle
        return (np.ones((npf, npf)) + np.eye(npf)) / (npf * (npf + 1))
    return _P2_EDGE if gdim == 2 else _P2_TRI


def facet_measures(coords, facets):
    X = np.asarray(coords, dtype=np.float64)
    if X.ndim == 1:
        X = X.reshape(-1, 1)
    gdim = X.shape[1]
    if gdim == 1:
        return np.ones(facets.shape[0])
    if gdim == 2:
        return np.linalg.norm(X[facets[:, 1]] - X[facets[:, 0]], axis=1)
    a = X[facets[:, 1]] - X[facets[:, 0]]
    b = X[facets[:, 2]] - X[facets[:, 0]]
    return 0.5 * np.linalg.norm(np.cross(a, b), axis=1)


def facet_mass_matrix(coords, facets, n):
    """int_Gamma phi_i phi_j ds as an (n x n) scipy CSR matrix."""
    facets = np.asarray(facets, dtype=np.int64)
    X = np.asarray(coords, dtype=np.float64)
    gdim = 1 if X.ndim == 1 else X.shape[1]
    npf = facets.shape[1]
    loc = local_facet_mass(gdim, npf)
    meas = facet_measures(X, facets)
    rows = np.repeat(facets, npf, axis=1).ravel()
    cols = np.tile(facets, (1, npf)).ravel()
    vals = (meas[:, None, None] * loc[None, :, :]).ravel()
    return sps.coo_matrix((vals, (rows, cols)), shape=(n, n)).tocsr()


def on_pattern(R, rp, cols):
    """Values of R at the entries of a CSR pattern, in pattern order."""
    rows = np.repeat(np.arange(rp.size - 1), np.diff(rp))
    return np.asarray(R[rows, cols]).ravel()


class FacetNumpyBackend(NumpyBackend):
    """The numpy oracle backend with facet atoms (atom_facets) from facet_mass_matrix - tests only."""
    name = "oracle-numpy+facets"

    def atom_facets(self, mh, facets):
        m = self._obj[mh]
        return self._put((mh, facet_mass_matrix(m.coords, facets, m.n)))
