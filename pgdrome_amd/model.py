"""PGD solution container, online evaluation and error computation.

Counterpart of the parts of /root/reference/pgdrome/model.py that sit directly
after the hot path:

* ``PGD`` / ``PGDMesh`` / ``PGDAttribute`` (model.py:25-160, 1573-1663, 1456-1570): what
  ``PGDProblem.return_PGD()`` builds (solver.py:883-907) - per-dimension mesh arrays and the
  stored modes;
* ``PGD.evaluate`` (model.py:724-860): online reconstruction
  ``u(fixed dim) = sum_k F_fixed^k prod_i F_i^k(coord_i)`` - on a large fixed dimension this is a
  tall-skinny product executed on the GPU (``pgd_vec_lincomb``: 8 (K+1) n bytes);
* ``PGD.create_interpolation_fcts`` (model.py:589-722): scipy ``interp1d`` functions of the 1-D
  modes (``interpolationInfo['name'] == 0``) or the mode Functions themselves;
* ``PGDErrorComputation`` (model.py:1666-1825): Latin-hypercube sampling (seed 3452) of the free
  coordinates and relative l2 errors against a full-order model callable.

* result files (model.py:162-575, 1414-1453): ``write_pxdmf`` / ``_write_xdmf`` / ``write_hdf5`` /
  ``load_pxdmf`` / ``save_modes_latex`` in the reference's own file layout: per PGD coordinate ``<grid>.xdmf`` +
  ``<grid>.h5`` (XDMFFile: /Mesh/0/mesh/topology, /Mesh/0/mesh/geometry, /VisualisationVector/<k>) and
  ``<grid>_data.h5`` (HDF5File: mesh + MODE_<k> functions), and one ``<name>.pxdmf`` whose data items point into the
  .h5 files (Grid / Information / Topology / Geometry / Attribute per coordinate - what the ParaView PGD plugin
  reads).  The HDF5 files are real HDF5, written and read by ``pgdrome_amd.h5lite`` (h5py is used for reading
  when it is installed); ``load_pxdmf`` also reads inline-XML items and the raw-binary items of this
  repository's first round.

* sensor responses and parameter derivatives (model.py:107-131, 862-953, 1088-1412): ``eval_fixed_modes``
  (the reference evaluates the fixed-dimension modes at the sensor points with ``fenicstools.Probes``; here by
  point location + shape functions, cached the same way), ``evaluate_sensor_response``,
  ``create_derivation_fct`` (cell-wise derivative of the 1-D modes = the reference's DG(degree - 1)
  projection), ``evaluate_derivative``, ``evaluate_derivative_sensor_response``, and the
  ``evaluate_min_abs / max_abs / max_norm / abs_value`` reductions.
"""
from __future__ import annotations

import logging
import math
import os
import xml.etree.ElementTree as et

import numpy as np
from scipy import interpolate
from scipy.stats import qmc

from . import fem, h5lite

LOGGER = logging.getLogger(__name__)

DEVICE_EVAL_MIN_DOFS = 1 << 16   # fixed dimensions at least this large are reconstructed on the GPU


class PGDAttribute:
    def __init__(self, name="", n_modes=0, _type="Node", field="Scalar"):
        # _type: "Node" | "Cell" (where the values live); field: "Scalar" | "Vector" (model.py:1469-1474)
        self.name, self.n_modes, self._type, self.field = name, n_modes, _type, field
        self.data = []                # vertex values per mode, shape (n, 1)
        self.interpolationfct = []    # callables per mode (Functions or interp1d objects)
        self.derivationfct = []       # d mode / d coordinate, callables (create_derivation_fct)
        self.interpolationInfo = {"name": 1, "family": "P", "degree": 1, "_type": "scalar"}

    def fill_data(self, modes):
        self.interpolationfct = list(modes)
        self.data = []
        for f in modes:
            nc = f.function_space()._ncomp
            v = np.asarray(f.compute_vertex_values())
            self.data.append(v.reshape(nc, -1).T.copy() if nc > 1 else v.reshape(-1, 1))
        if modes and modes[0].function_space()._ncomp > 1:
            self.interpolationInfo = dict(self.interpolationInfo, _type="vector")
        if modes:
            self.interpolationInfo = dict(self.interpolationInfo, degree=modes[0].function_space().ufl_element().degree())

    def print_info(self):
        print("PGDAttribute %s: type %s, field %s, %d modes, interpolation %s" % (
            self.name, self._type, self.field, len(self.data), self.interpolationInfo))


class PGDMesh:
    def __init__(self, name, fmesh=None, info=None):
        self.name = name
        self.info = info or []
        self.attributes = []
        self.fenics_mesh = fmesh
        self.numNodes, self.numElements, self.meshdim = 0, None, 0
        self.dataX = self.dataY = self.dataZ = np.zeros(0)
        self.topology, self.typElements, self.typGeometry = None, None, "XYZ"
        if fmesh is not None:
            self.meshdim = fmesh.topology().dim()
            X = fmesh.coordinates()
            n = fmesh.num_vertices()
            self.numNodes, self.numElements = n, fmesh.num_cells()
            self.dim = fmesh.topology().dim()
            self.dataX = X[:, 0].copy()
            self.dataY = X[:, 1].copy() if X.shape[1] > 1 else np.zeros(n)
            self.dataZ = X[:, 2].copy() if X.shape[1] > 2 else np.zeros(n)
            self.topology = fmesh.cells()
            self.typElements = {1: "Polyline", 2: "Triangle", 3: "Tetrahedron"}[self.dim]


class EvalManyResult:
    """What ``PGD.evaluate_many`` returns; outputs that were not asked for are None."""
    min = max = max_abs = None
    envelope_min = envelope_max = exceedance = None
    fields = None
    coefficients = None
    _fields_owner = None


class SensorManyResult:
    """What ``PGD.evaluate_sensor_response_many`` returns; outputs that were not asked for are None."""
    values = jacobian = coefficients = None
    min = max = max_abs = None


class SensorModes:
    """All modes of a fixed dimension sampled at a point set (``PGD.sensor_modes``): per mode ``m`` entries in the order
    (point, component[, axis]) of ``shape`` - K library vectors on the backend ``be`` (``handles``), or a (K, m) array on the host."""

    def __init__(self, shape, m, be=None, handles=None, host=None):
        self.shape, self.m, self.be, self.handles, self._host = shape, m, be, handles, host

    def host(self):
        """The (K, m) array of the sampled modes (downloads K small vectors the first time on the device path)."""
        if self._host is None:
            self._host = np.stack([self.be.vec_to_host(h) for h in self.handles])
        return self._host

    def contract(self, C, K):
        """(S, m): the first K sampled modes combined with the coefficients C (K, S) - numpy below DEVICE_EVAL_MIN_DOFS entries,
        ``eval_batch`` on the sampled vectors above (device path)."""
        C = np.ascontiguousarray(C, dtype=np.float64)
        S = C.shape[1]
        if self.handles is not None and self.m >= DEVICE_EVAL_MIN_DOFS and K <= 256 and hasattr(self.be, "eval_batch"):
            out = self.be.vec_zeros(self.m * S)
            try:
                self.be.eval_batch(self.handles[:K], C, stats=False, fields=out)
                U = self.be.vec_to_host(out)
            finally:
                self.be.vec_free(out)
            fem.STATS["sensor_eval_batch_calls"] = fem.STATS.get("sensor_eval_batch_calls", 0) + 1
            return U.reshape(S, self.m)
        return C.T @ self.host()[:K]

    def __del__(self):
        if self.handles is not None:
            for h in self.handles:
                try:
                    self.be.vec_free(h)
                except Exception:
                    pass


class _FieldStore:
    """The one library vector (n * S doubles, sample-major) behind the ``fields`` of a device ``evaluate_many``; freed with
    the last reference (the result and every field view hold one)."""

    def __init__(self, be, n, S):
        self.be, self.n = be, n
        self.handle = be.vec_zeros(n * S)

    def read(self, j):
        return self.be.vec_to_host(self.handle, j * self.n, self.n)

    def __del__(self):
        try:
            self.be.vec_free(self.handle)
        except Exception:
            pass


def _p2_point_gradients(lay, U, lam):
    """g[a, e, c * G + d, ...] = d u_c / d x_d at the point of barycentric coordinates ``lam[a]`` of cell e, for nodal values U
    (nodes, ncomp, ...) of the scalar P2 layout ``lay`` (intervals, triangles, tetrahedra).  With N_i = l_i (2 l_i - 1),
    N_ab = 4 l_a l_b and d l_i / d xi_a = [i == a + 1] - [i == 0]: d u / d xi_a = sum_j d N_j / d xi_a u_j - the formula of
    ``pgd_cell_gradient_p2`` (the edge (0, a + 1) with its coefficient 4 l_0 - 4 l_{a+1} in one piece) -, and the Jacobian comes
    from the vertices alone."""
    rec, G = lay.cells, lay.coords.shape[1]
    edges = ((0, 1),) if G == 1 else lay.P2_EDGES[G]
    Xv = lay.coords[rec[:, :G + 1]]
    Einv = np.linalg.inv(Xv[:, 1:] - Xv[:, :1])                                  # rows of E: the edges x_a - x_0; (cells, d, a)
    Un = U[rec]                                                                   # (cells, record entry, c, ...)
    dlam = np.concatenate([-np.ones((1, G)), np.eye(G)])                          # d l_i / d xi_a
    out = []
    for l in np.asarray(lam, dtype=np.float64):
        D = np.array([(4.0 * l[i] - 1.0) * dlam[i] for i in range(G + 1)] +
                     [4.0 * l[b] * dlam[i] + 4.0 * l[i] * dlam[b] for i, b in edges])      # d N_j / d xi_a, (record entry, a)
        du = np.einsum("ja,ejc...->eac...", D, Un)
        g = np.einsum("eda,eac...->ecd...", Einv, du)                            # (cells, c, d, ...)
        out.append(g.reshape((g.shape[0], g.shape[1] * G) + g.shape[3:]))
    return np.stack(out)


class _GradientModes:
    """The planes of the fixed dimension's modes for one gradient quantity (``PGD.evaluate_gradient_many``): on the device one
    library vector of q * entries doubles per mode (``pgd_cell_gradient``; ``pgd_cell_gradient_p2`` at the points ``lam`` of every
    cell for P2 modes), freed with this object; on the host one array (q, entries, K).  Entries: the cells, point-major times the
    points for P2.  ``key`` says what they were built from."""

    def __init__(self, key, be, mesh, V, modes, L, scale_vec, lam=None):
        self.key, self.be, self.planes = key, be, []
        q, nc, ncomp = L.shape[0], mesh.num_cells(), V._ncomp
        if be is not None:
            sc = scale_vec.dev() if scale_vec is not None else 0
            for m in modes:
                out = be.vec_zeros(q * nc * (1 if lam is None else len(lam)))
                self.planes.append(out)
                if lam is None:
                    be.cell_gradient(V._lay.handle(), m.vector().dev(), L, out, sc)
                else:
                    be.cell_gradient_p2(V._lay.handle(), m.vector().dev(), lam, L, out, sc)
            return
        sc = scale_vec.host() if scale_vec is not None else None
        if lam is not None:
            lay = V._lay.base if ncomp > 1 else V._lay
            P = np.empty((q, len(lam) * nc, len(modes)))
            for k, m in enumerate(modes):
                g = _p2_point_gradients(lay, m.vector().host().reshape(-1, ncomp), lam)           # (npt, cells, ncomp * G)
                p = np.einsum("ij,aej->iae", L, g)
                P[:, :, k] = (p if sc is None else p * sc).reshape(q, -1)
            self.planes = P
            return
        X, cells = mesh.coordinates(), mesh.cells()
        G = cells.shape[1] - 1
        Einv = np.linalg.inv(X[cells[:, 1:]] - X[cells[:, :1]])                  # rows of E: the edges x_a - x_0; (cells, d, a)
        P = np.empty((q, nc, len(modes)))
        for k, m in enumerate(modes):
            U = m.vector().host().reshape(-1, ncomp)                              # vertex order, (node, component)
            dU = U[cells[:, 1:]] - U[cells[:, :1]]                                # (cells, a, c)
            g = np.einsum("eda,eac->ecd", Einv, dU).reshape(nc, ncomp * G)        # g[c * G + d] = d u_c / d x_d
            P[:, :, k] = L @ g.T if sc is None else (L @ g.T) * sc
        self.planes = P

    def __del__(self):
        if self.be is not None:
            for h in self.planes:
                try:
                    self.be.vec_free(h)
                except Exception:
                    pass


class _FieldSlice(fem.Vector):
    """Vector of one sample's field: a view into the ``_FieldStore`` until somebody reads or writes it (then an ordinary
    Vector with its own storage)."""

    def __init__(self, V, store, j):
        super().__init__(V)
        self._store, self._j = store, j
        self._zero = False

    def _pull(self):
        if self._store is not None:
            store, self._store = self._store, None
            self._host = store.read(self._j)
            self._host_ok, self._dev_ok = True, False

    def host(self):
        self._pull()
        return super().host()

    def dev(self):
        self._pull()
        return super().dev()

    def dev_for_write(self):
        self._store = None
        return super().dev_for_write()

    def touched_host(self):
        self._store = None
        super().touched_host()

    def touched_dev(self):
        self._store = None
        super().touched_dev()


def _eval_many_device(be, call, V, n, S, stats, envelope, thr, fields):
    """The device half of ``evaluate_many`` / ``evaluate_gradient_many``: allocates the requested outputs on ``V`` (``n`` entries),
    runs ``call(stats, **handles)`` - the backend's batch evaluation, which returns the (3, S) statistics or None - and returns
    the filled ``EvalManyResult``."""
    res = EvalManyResult()

    def out_function():
        f = fem.Function(V)
        return f, f.vector().dev_for_write()
    kw = {}
    if envelope:
        (res.envelope_min, kw["env_min"]), (res.envelope_max, kw["env_max"]) = out_function(), out_function()
    if thr is not None:
        (res.exceedance, kw["exceed"]), kw["threshold"] = out_function(), thr
    if fields:
        res._fields_owner = _FieldStore(be, n, S)
        kw["fields"] = res._fields_owner.handle
    st = call(bool(stats), **kw)
    if stats:
        res.min, res.max, res.max_abs = st[0], st[1], st[2]
    for f in (res.envelope_min, res.envelope_max, res.exceedance):
        if f is not None:
            f.vector().touched_dev()
    if thr is not None:
        v = res.exceedance.vector()
        v._host = v.host() / S                  # counts -> fraction (exactly count / S, as the host path has it)
        v.touched_host()
    if fields:
        res.fields = []
        for j in range(S):
            f = fem.Function(V)
            f._vec = _FieldSlice(V, res._fields_owner, j)
            res.fields.append(f)
    return res


def _eval_many_host(values, n, S, sample_chunk, stats, envelope, thr, fields, wrap, nonnegative=False):
    """The host half: the same outputs in numpy from ``values(j0, step)``, the (n, <= step) matrix of the samples from j0 on,
    ``sample_chunk`` samples at a time.  ``wrap`` turns an array of n entries into what the result holds; ``nonnegative``: the
    values are norms, so ``max_abs`` is a copy of ``max``."""
    res = EvalManyResult()
    if stats:
        res.min, res.max = np.empty(S), np.empty(S)
        if not nonnegative:
            res.max_abs = np.empty(S)
    emn, emx = np.full(n, np.inf), np.full(n, -np.inf)
    cnt = np.zeros(n)
    all_fields = []
    step = max(1, int(sample_chunk))
    for j0 in range(0, S, step):
        U = values(j0, step)
        if stats:
            sl = slice(j0, j0 + U.shape[1])
            res.min[sl], res.max[sl] = U.min(axis=0), U.max(axis=0)
            if not nonnegative:
                res.max_abs[sl] = np.abs(U).max(axis=0)
        if envelope:
            np.minimum(emn, U.min(axis=1), out=emn)
            np.maximum(emx, U.max(axis=1), out=emx)
        if thr is not None:
            cnt += (U > thr).sum(axis=1)
        if fields:
            all_fields.extend(np.ascontiguousarray(U[:, j]) for j in range(U.shape[1]))
    if stats and nonnegative:
        res.max_abs = res.max.copy()
    if envelope:
        res.envelope_min, res.envelope_max = wrap(emn), wrap(emx)
    if thr is not None:
        res.exceedance = wrap(cnt / S)
    if fields:
        res.fields = [wrap(a) for a in all_fields]
    return res


_TENSOR_PLANES = ((0, 0), (1, 1), (2, 2), (0, 1), (1, 2), (0, 2))      # the plane order of fem.stress_quantity


def _quantity_values(U, kind):
    """The values of kind ``kind`` (fem.EVAL_Q_*) of combined planes U (q, ...): the host half of the value epilogue of
    ``pgd_eval_batch_quantity`` - the norm over the planes, the one plane with its sign, or the largest / smallest eigenvalue (or
    their difference) of the symmetric tensors whose planes are xx, yy, zz, xy (, yz, xz), from ``np.linalg.eigvalsh``."""
    if kind == fem.EVAL_Q_NORM:
        return np.sqrt((U * U).sum(axis=0))
    if kind == fem.EVAL_Q_VALUE:
        return U[0]
    T = np.zeros(U.shape[1:] + (3, 3))
    for i in range(U.shape[0]):
        a, b = _TENSOR_PLANES[i]
        T[..., a, b] = T[..., b, a] = U[i]
    w = np.linalg.eigvalsh(T)                        # ascending
    return w[..., 2] if kind == fem.EVAL_Q_EIG_MAX else w[..., 0] if kind == fem.EVAL_Q_EIG_MIN else w[..., 2] - w[..., 0]


def _eval_points_device(be, call, m, stats, envelope):
    """``_eval_many_device`` for entries that are no function space (several points per cell): the statistics as they come, the
    two envelopes of ``m`` entries as numpy arrays."""
    res, hs = EvalManyResult(), []
    try:
        if envelope:
            hs = [be.vec_zeros(m), be.vec_zeros(m)]
        st = call(bool(stats), **({"env_min": hs[0], "env_max": hs[1]} if envelope else {}))
        if stats:
            res.min, res.max, res.max_abs = st[0], st[1], st[2]
        if envelope:
            res.envelope_min, res.envelope_max = be.vec_to_host(hs[0], 0, m), be.vec_to_host(hs[1], 0, m)
    finally:
        for h in hs:
            be.vec_free(h)
    return res


def _host_function(V, a):
    f = fem.Function(V)
    f.vector()._host = np.array(a, dtype=np.float64)
    f.vector().touched_host()
    return f


# ------------------------------------------------------------------ mode compression on Gram matrices
COMPRESS_TOL_FLOOR = 1e-7        # the Gram route carries half the digits: sqrt(2^-53) |u| = 1.05e-8 |u| is its resolution
_GRAM_EIG_DROP = 1e-14           # eigenvalues of a Gram matrix at most this fraction of the largest are rounding


def _gram_coordinates(G):
    """(L, P) of a Gram matrix G = F^T F: row k of L (K x r) holds the coordinates of mode k in an orthonormal basis of span F,
    and F P (P = Q Lambda^-1/2, K x r) IS that basis, so coordinates B (r x R) map back to the modes F (P B)."""
    lam, Q = np.linalg.eigh(0.5 * (G + G.T))
    keep = lam > _GRAM_EIG_DROP * lam[-1] if lam[-1] > 0.0 else np.zeros(len(lam), dtype=bool)
    lam, Q = lam[keep][::-1], Q[:, keep][:, ::-1]
    root = np.sqrt(lam)
    return Q * root, Q / root


def _hadamard_sum(blocks):
    """1^T (o_d blocks[d]) 1: the inner product of two separated functions from the Gram blocks of their dimensions."""
    H = np.ones_like(blocks[0])
    for b in blocks:
        H = H * b
    return float(H.sum())


def _cp_rel_error(Ls, Bs, t2):
    """|T - That| / |T| in the orthonormal coordinates: T = sum_k (x)_d Ls[d][k], That = sum_i (x)_d Bs[d][:, i], t2 = |T|^2.
    The three sums are taken over small matrices of O(1) entries (no 1 / h^d weights of the big norms in them)."""
    cross = _hadamard_sum([L @ B for L, B in zip(Ls, Bs)])
    own = _hadamard_sum([B.T @ B for B in Bs])
    return math.sqrt(max(t2 - 2.0 * cross + own, 0.0) / t2)


def _cp_als(Ls, tol, cap, max_sweeps):
    """CP-ALS on T = sum_k (x)_d Ls[d][k] (D >= 3), deterministic: R grows from 1, the factors that have converged are kept and
    the largest remaining input term joins them; every normal equation is a Hadamard product of cross-Grams.  Returns
    (Bs, rel_error, sweeps) of the first R that meets tol, or of the best R <= cap."""
    D, K = len(Ls), Ls[0].shape[0]
    t2 = _hadamard_sum([L @ L.T for L in Ls])
    order = np.argsort(-np.prod([np.linalg.norm(L, axis=1) for L in Ls], axis=0), kind="stable")
    Bs, best, sweeps = None, None, 0
    for R in range(1, cap + 1):
        new = [L[order[R - 1]].reshape(-1, 1) for L in Ls]
        Bs = new if Bs is None else [np.hstack([B, b]) for B, b in zip(Bs, new)]
        err = _cp_rel_error(Ls, Bs, t2)
        for _ in range(max_sweeps):
            if err <= tol:
                break
            for d in range(D):
                H, M = np.ones((R, R)), np.ones((K, R))
                for e in range(D):
                    if e != d:
                        H, M = H * (Bs[e].T @ Bs[e]), M * (Ls[e] @ Bs[e])
                Bs[d] = np.linalg.lstsq(H, (Ls[d].T @ M).T, rcond=None)[0].T
            sweeps += 1
            last, err = err, _cp_rel_error(Ls, Bs, t2)
            if last - err <= 1e-6 * err:          # stagnation at this R: one more term
                break
        if best is None or err < best[1]:
            best = ([B.copy() for B in Bs], err)
        if err <= tol:
            break
    return best[0], best[1], sweeps


def compress_grams(Gs, tol, max_modes=None, max_sweeps=200):
    """The host half of ``PGD.compress``: from the Gram matrices G_d (K x K) of the modes of every dimension to the matrices
    W_d (K x R) whose products F_d W_d are the new modes.  dict: R, W (None: nothing shorter meets tol - keep the model),
    rel_error, converged, ranks, sweeps."""
    D, K = len(Gs), Gs[0].shape[0]
    LP = [_gram_coordinates(G) for G in Gs]
    Ls, Ps = [lp[0] for lp in LP], [lp[1] for lp in LP]
    ranks = [int(L.shape[1]) for L in Ls]
    out = {"R": K, "W": None, "rel_error": 0.0, "converged": True, "ranks": ranks, "sweeps": 0}
    if min(ranks) == 0:                       # the zero function: one zero term says it all
        return out if K == 1 else dict(out, R=1, W=[np.zeros((K, 1)) for _ in Gs])
    cap = K - 1 if max_modes is None else min(K, int(max_modes))
    if cap < 1:
        return out
    if D == 1:
        Bs, err, sweeps = [Ls[0].sum(axis=0).reshape(-1, 1)], 0.0, 0
    elif D == 2:
        U, sv, Vt = np.linalg.svd(Ls[0].T @ Ls[1], full_matrices=False)      # Eckart-Young: the tail is the best error of its rank
        tails = np.sqrt(np.concatenate([np.cumsum((sv ** 2)[::-1])[::-1], [0.0]])) / np.linalg.norm(sv)
        R = max(1, min(int(np.argmax(tails <= tol)), cap))
        Bs, err, sweeps = [U[:, :R] * sv[:R], Vt[:R].T.copy()], float(tails[R]), 0
    else:
        Bs, err, sweeps = _cp_als(Ls, tol, cap, max_sweeps)
    if max_modes is None and err > tol:
        return out
    # balance: every dimension carries lambda^(1 / D) of a term's weight lambda = prod_d |b_d|; terms by descending weight
    norms = np.array([np.linalg.norm(B, axis=0) for B in Bs])                # (D, R)
    weight = np.prod(norms, axis=0)
    live = weight > 0.0
    if not live.any():
        live[0] = True
    order = np.argsort(-weight[live], kind="stable")
    Ws = []
    for d in range(D):
        B, nd, w = Bs[d][:, live][:, order], norms[d][live][order], weight[live][order]
        Ws.append(Ps[d] @ (B * np.where(nd > 0.0, w ** (1.0 / D) / np.where(nd > 0.0, nd, 1.0), 0.0)))
    return {"R": int(Ws[0].shape[1]), "W": Ws, "rel_error": float(err), "converged": bool(err <= tol), "ranks": ranks,
            "sweeps": int(sweeps)}


def _hadamard(mats):
    out = np.array(mats[0], dtype=np.float64)
    for M in mats[1:]:
        out = out * M
    return out


def variance_forms(moments, random, order=1):
    """The K x K matrices Q with V(x_i) = f_i^T Q f_i for the ANOVA / Sobol decomposition of u = sum_k F_k(x) prod_d G_dk(mu_d)
    with independent parameters.  ``moments`` {d: (m_d, C_d)} over ALL parameter dimensions (``PGD.parameter_moments``; a
    dimension that is given a value has C_d = 0), ``random`` the dimensions that vary.  With M_d = m_d m_d^T and o the
    entrywise product, the keys of the result are

        "total"   sum_j (o_{d<j} (C_d + M_d)) o C_j o (o_{d>j} M_d): the variance, P terms and no subtraction
        (i,)      C_i o (o_{d != i} M_d): the first-order term Var E[u | mu_i]
        (i, j)    C_i o C_j o (o_{d != i, j} M_d), i < j, with ``order`` 2: the second-order interaction
        ("T", i)  C_i o (o_{d != i} (C_d + M_d)): the total effect E Var[u | mu_~i]

    Every matrix is positive semidefinite (Schur products of such)."""
    dims = sorted(moments)
    random = sorted(random)
    C = {d: np.asarray(moments[d][1], dtype=np.float64) for d in dims}
    M = {d: np.outer(moments[d][0], moments[d][0]) for d in dims}
    S = {d: C[d] + M[d] for d in dims}
    forms = {"total": sum(_hadamard([S[d] if d < j else C[d] if d == j else M[d] for d in dims]) for j in random)}
    for i in random:
        forms[(i,)] = _hadamard([C[d] if d == i else M[d] for d in dims])
    if order >= 2:
        for a, i in enumerate(random):
            for j in random[a + 1:]:
                forms[(i, j)] = _hadamard([C[d] if d in (i, j) else M[d] for d in dims])
    for i in random:
        forms[("T", i)] = _hadamard([C[d] if d == i else S[d] for d in dims])
    return forms


class VarianceDecomposition:
    """What ``PGD.variance_decomposition`` returns.  Fields (Functions on the fixed space; None / empty with ``fields=False``):
    ``mean``, ``variance`` (clamped at 0), ``std`` (the root, taken on the host when asked for), ``sobol[(i,)]`` / ``sobol[(i, j)]``
    and ``total[i]`` (ratio fields, 0 where the variance is at or below ``floor``), ``partial[key]`` / ``partial_total[i]`` (the
    partial variances they are ratios of).  Numbers: ``variance_min`` / ``variance_max``, ``extrema[key]`` = (min, max) of every
    form, ``floor``, ``global_variance`` = int V dx and ``global_sobol[key]`` / ``global_total[i]`` = int V_B dx / int V dx (exact,
    from the mass Gram matrix of the fixed modes).  ``forms`` (the Q matrices by key, see ``variance_forms``), ``moments``
    {dim: (m, C)}, ``mean_coefficients``, ``random``, ``given``."""

    def __init__(self):
        self.mean = self.variance = None
        self.sobol, self.total, self.partial, self.partial_total = {}, {}, {}, {}
        self._std = None

    @property
    def std(self):
        if self._std is None and self.variance is not None:
            self._std = _host_function(self.variance.function_space(), np.sqrt(np.maximum(self.variance.vector().host(), 0.0)))
        return self._std


# ----------------------------------------------------------------- Bayesian calibration from sensor data
DEVICE_POSTERIOR_MIN_SAMPLES = 1 << 12   # grids with at least this many samples form their misfits and reductions on the GPU
POST_MARGINALS, POST_THETA, POST_COEF = 1, 2, 4      # what ``grid_posterior`` is asked for (PGD_POST_* of include/pgd_amd.h)
POSTERIOR_MAX_ROWS, POSTERIOR_MAX_MODES, POSTERIOR_MAX_DIMS, POSTERIOR_COEF_MAX_MODES = 256, 256, 6, 64
# sensor_posterior_many takes the device when (data sets) x (samples) reaches this: DEVICE_POSTERIOR_MIN_SAMPLES, one data set on the
# smallest grid sensor_posterior sends to the device.  tools/bench_posterior_many.py (64 data sets on 64^3 samples and up: the device
# call is 20 to 70 times faster than the per-data-set calls) measured nothing near this threshold, so it has not been moved.
DEVICE_POSTERIOR_MANY_MIN_WORK = DEVICE_POSTERIOR_MIN_SAMPLES
POSTERIOR_MANY_MAX_ROWS, POSTERIOR_MANY_MAX_MODES = 64, 64
POSTERIOR_MANY_PARTIALS = 1 << 25                    # doubles of device scratch a chunk of data sets may take (256 MB)


class DeviceArray:
    """A library vector kept with a result (``PosteriorResult.chi2``): ``handle`` on the backend ``be``; ``host()`` downloads it
    and adds ``offset`` (the part of the misfit that the thin QR took out of the kernel's rows).  Freed with the object."""

    def __init__(self, be, handle, n, offset=0.0):
        self.be, self.handle, self.n, self.offset = be, handle, int(n), float(offset)

    def host(self):
        return self.be.vec_to_host(self.handle) + self.offset

    def __array__(self, dtype=None, copy=None):
        a = self.host()
        return a if dtype is None else a.astype(dtype)

    def __len__(self):
        return self.n

    def __del__(self):
        try:
            self.be.vec_free(self.handle)
        except Exception:
            pass


class PosteriorResult:
    """What ``PGD.sensor_posterior`` returns; outputs that were not asked for are None.

    ``chi2_min`` / ``map_index`` / ``map_coords``: the smallest misfit, its grid indices (a tuple; the sample number for scattered
    samples) and coordinates.  ``log_evidence``: log of sum_s w_s N(data | prediction(s), covariance), the prior in w.
    ``marginals[d]`` (masses, sum 1) and ``densities[d]`` (masses over the quadrature weights) per free dimension;
    ``mean`` / ``cov`` of the parameters; ``coef_mean`` = E[c], ``coef_second`` = E[c c^T] of the mode coefficients
    (``PGD.posterior_predictive``); ``ess`` = Z^2 / sum e^2; ``chi2`` with ``keep_chi2`` (numpy array or ``DeviceArray``, the
    grid's shape in C order); ``path``: "device" or "numpy"; ``grids``, ``weights``, ``free_dim``: what the sums ran over."""
    chi2_min = map_index = map_coords = log_evidence = None
    marginals = densities = mean = cov = coef_mean = coef_second = None
    ess = chi2 = path = None
    grids = weights = free_dim = None
    Z = shift = None


class PosteriorManyResult:
    """What ``PGD.sensor_posterior_many`` returns for N data sets (with ``accumulate``: N steps, step n holding all data up to n);
    every array has the leading size N.

    ``chi2_min`` (the smallest misfit, recomputed on the host in the difference form at the MAP sample), ``map_index`` (N, D) and
    ``map_coords`` (N, D), ``log_evidence``, ``ess`` = Z^2 / sum e^2, ``mean`` (N, D) and ``cov`` (N, D, D) with the "theta" output;
    ``Z`` and ``shift`` (the kernel's own minimum of the expanded misfit, what Z is relative to); ``path``: "device" or "numpy";
    ``grids``, ``weights``, ``free_dim``: what the sums ran over."""
    chi2_min = map_index = map_coords = log_evidence = ess = mean = cov = None
    Z = shift = path = None
    grids = weights = free_dim = None


def trapezoid_weights(x):
    """Weights of the trapezoid rule on the non-decreasing abscissae x (one point: weight 1)."""
    x = np.asarray(x, dtype=np.float64)
    if x.size == 1:
        return np.ones(1)
    w = np.zeros(x.size)
    h = np.diff(x)
    w[:-1] += 0.5 * h
    w[1:] += 0.5 * h
    return w


def _grid_coefficients(tables, n, s):
    """(C, idx): the coefficients c_k(s) = 1 * T_0[k, i_0] * T_1[k, i_1] * .. of the samples s (last index fastest) and their indices."""
    idx = np.unravel_index(s, n)
    C = np.ones((tables[0].shape[0], len(s)))
    for d, t in enumerate(tables):
        C *= t[:, idx[d]]
    return C, idx


def grid_misfit_numpy(a, y, tables, sample_chunk=1 << 14):
    """The arithmetic of ``pgd_grid_misfit`` in numpy, ``sample_chunk`` samples at a time: (chi2, min, lowest index of the min)."""
    n = [t.shape[1] for t in tables]
    S = int(np.prod(n, dtype=np.int64))
    chi2 = np.empty(S)
    for s0 in range(0, S, int(sample_chunk)):
        s = np.arange(s0, min(S, s0 + int(sample_chunk)))
        C, _ = _grid_coefficients(tables, n, s)
        r = y[:, None] - a @ C
        chi2[s0:s0 + len(s)] = np.einsum("ps,ps->s", r, r)
    arg = int(np.argmin(chi2))
    return chi2, float(chi2[arg]), arg


def grid_posterior_numpy(chi2, shift, n, weights, tables=None, abscissae=None, want=0, sample_chunk=1 << 14):
    """The arithmetic of ``pgd_grid_posterior`` in numpy, ``sample_chunk`` samples at a time: the dict of ``Context.grid_posterior``."""
    n = [int(v) for v in n]
    S, nd = int(np.prod(n, dtype=np.int64)), len(n)
    out = {"Z": 0.0, "sum_e2": 0.0}
    if want & POST_MARGINALS:
        out["marginals"] = [np.zeros(v) for v in n]
    if want & POST_THETA:
        out["theta1"], out["theta2"] = np.zeros(nd), np.zeros((nd, nd))
    if want & POST_COEF:
        k = tables[0].shape[0]
        out["coef1"], out["coef2"] = np.zeros(k), np.zeros((k, k))
    for s0 in range(0, S, int(sample_chunk)):
        s = np.arange(s0, min(S, s0 + int(sample_chunk)))
        idx = np.unravel_index(s, n)
        w = np.ones(len(s))
        for d in range(nd):
            w *= weights[d][idx[d]]
        e = w * np.exp(-0.5 * (chi2[s] - shift))
        out["Z"] += float(e.sum())
        out["sum_e2"] += float(e @ e)
        if want & POST_MARGINALS:
            for d in range(nd):
                out["marginals"][d] += np.bincount(idx[d], weights=e, minlength=n[d])
        if want & POST_THETA:
            th = np.stack([np.asarray(abscissae[d], dtype=np.float64)[idx[d]] for d in range(nd)])
            out["theta1"] += th @ e
            out["theta2"] += (th * e) @ th.T
        if want & POST_COEF:
            C, _ = _grid_coefficients(tables, n, s)
            out["coef1"] += C @ e
            out["coef2"] += (C * e) @ C.T
    if want & POST_COEF:
        out["coef2"] = np.triu(out["coef2"]) + np.triu(out["coef2"], 1).T        # the upper triangle, mirrored (as the device call)
    return out


def posterior_many_segments(S):
    """(number, length) of the sample segments of ``pgd_grid_posterior_many``: a function of S alone (postmany_segments of the library)."""
    ns = min(max((S + 1023) // 1024, 1), 1024)
    length = ((S + ns - 1) // ns + 255) // 256 * 256
    return max((S + length - 1) // length, 1), length


def grid_posterior_many_numpy(a, u, alpha, beta, tables, weights, abscissae=None, want=0, sample_chunk=1 << 12):
    """The arithmetic of ``pgd_grid_posterior_many`` in numpy, ``sample_chunk`` samples at a time, in two passes over the same
    expanded misfits chi2[j, s] = beta_j - 2 u_j . p_s + alpha_j |p_s|^2: the dict of ``Context.grid_posterior_many``.  Every number
    of a data set is formed by element-wise operations and sums along its own row: it does not depend on the other rows."""
    a, u = np.asarray(a, dtype=np.float64), np.asarray(u, dtype=np.float64)
    alpha, beta = np.asarray(alpha, dtype=np.float64).reshape(-1, 1), np.asarray(beta, dtype=np.float64).reshape(-1, 1)
    n = [t.shape[1] for t in tables]
    S, D, nd, m = int(np.prod(n, dtype=np.int64)), len(n), u.shape[0], a.shape[0]

    def chunk(s0):
        s = np.arange(s0, min(S, s0 + int(sample_chunk)))
        C, idx = _grid_coefficients(tables, n, s)
        Pm = a @ C
        dot = np.zeros((nd, len(s)))
        for p in range(m):
            dot += u[:, p:p + 1] * Pm[p]
        return (beta - 2.0 * dot) + alpha * np.einsum("ps,ps->s", Pm, Pm), idx

    cmin, arg = np.full(nd, np.inf), np.full(nd, -1, dtype=np.int64)
    for s0 in range(0, S, int(sample_chunk)):
        chi2, _ = chunk(s0)
        loc = np.argmin(chi2, axis=1)
        val = chi2[np.arange(nd), loc]
        better = val < cmin                                   # (strict: the lowest sample keeps a tie)
        cmin[better], arg[better] = val[better], s0 + loc[better]
    out = {"chi2_min": cmin, "argmin": arg, "Z": np.zeros(nd), "sum_e2": np.zeros(nd)}
    if want & POST_THETA:
        out["theta1"], out["theta2"] = np.zeros((nd, D)), np.zeros((nd, D, D))
    for s0 in range(0, S, int(sample_chunk)):
        chi2, idx = chunk(s0)
        w = np.ones(chi2.shape[1])
        for d in range(D):
            w *= weights[d][idx[d]]
        e = w * np.exp(-0.5 * (chi2 - cmin[:, None]))
        out["Z"] += e.sum(axis=1)
        out["sum_e2"] += (e * e).sum(axis=1)
        if want & POST_THETA:
            th = [np.asarray(abscissae[d], dtype=np.float64)[idx[d]] for d in range(D)]
            for d in range(D):
                et = e * th[d]
                out["theta1"][:, d] += et.sum(axis=1)
                for f in range(d, D):
                    out["theta2"][:, d, f] += (et * th[f]).sum(axis=1)
    if want & POST_THETA:
        for d in range(D):
            for f in range(d):
                out["theta2"][:, d, f] = out["theta2"][:, f, d]                   # the upper triangle, mirrored (as the device call)
    return out


# ----------------------------------------------------------------- sensor placement by expected information gain
# sensor_placement takes the device when (candidates) x (samples) reaches this.  Measured (tools/bench_placement.py --crossover,
# profiles/placement_crossover_n1.jsonl: whole 8-step calls, 48 modes, three dimensions): at M S = 2^10, the smallest problem timed, the
# two routes take the same time (1.37 against 1.42 ms); from 2^13 on the device call is 1.3 to 2 times faster, from 2^19 on 5 to 60 times.
DEVICE_PLACEMENT_MIN_WORK = 1 << 10
PLACEMENT_MAX_MODES, PLACEMENT_MAX_ROWS = 64, 3      # modes and rows per candidate of pgd_design_gains


class PlacementResult:
    """What ``PGD.sensor_placement`` returns.  ``selected`` (n_select candidate indices in the order they were chosen) and
    ``selected_points``; ``gains`` (n_select marginal gains, in nats); ``installed_gains`` (those of the ``installed`` candidates, in
    order); ``utility``: the expected information gain after 0, 1, .. sensors (installed ones first), from the log-determinants the
    updates report - len(installed) + n_select + 1 values starting at 0; ``first_gains`` (M): every candidate's gain at the first free
    step; ``gain_history`` (n_select, M) with ``keep_gains``; ``expected_cov``: n_select + 1 matrices, the expected posterior
    covariance before the first free step and after each one; ``prior_precision``; ``path``: "device" or "numpy"."""
    selected = selected_points = gains = installed_gains = utility = first_gains = gain_history = expected_cov = None
    prior_precision = path = None


def _grid_derivative_coefficients(tables, dtables, n, s):
    """(CD, idx): CD[d] (K, len(s)) holds cd_t(s) = 1 * U_0[t, i_0] * U_1[t, i_1] * .. with U_f = dtables[f] for f == d, tables[f]
    otherwise - one chain in ascending f per coordinate d (pgd_design_update / pgd_design_gains)."""
    idx = np.unravel_index(s, n)
    D = len(tables)
    CD = np.ones((D, tables[0].shape[0], len(s)))
    for d in range(D):
        for f in range(D):
            CD[d] *= (dtables[f] if f == d else tables[f])[:, idx[f]]
    return CD, idx


def _cholesky_inverse_batch(H):
    """W (.., D, D), the inverse of the lower Cholesky factor of every H (.., D, D): the factor row by row, W by forward substitution
    of the columns of the identity (the arithmetic of k_design_update, vectorised over the leading axes)."""
    D = H.shape[-1]
    L, W = np.zeros_like(H), np.zeros_like(H)
    for i in range(D):
        for j in range(i + 1):
            t = H[..., j, i] - np.einsum("...m,...m->...", L[..., i, :j], L[..., j, :j])
            L[..., i, j] = np.sqrt(t) if i == j else t / L[..., j, j]
    for j in range(D):
        W[..., j, j] = 1.0 / L[..., j, j]
        for i in range(j + 1, D):
            W[..., i, j] = -np.einsum("...m,...m->...", L[..., i, j:i], W[..., j:i, j]) / L[..., i, i]
    return W


def design_state_numpy(n):
    """The state of the numpy route on the grid of ``n`` points per dimension: H_s and W_s as full (S, D, D) arrays."""
    S, D = int(np.prod(n, dtype=np.int64)), len(n)
    return {"H": np.zeros((S, D, D)), "W": np.zeros((S, D, D))}


def design_update_numpy(state, tables, dtables, weights, rows=None, h0=None, sample_chunk=1 << 14):
    """The arithmetic of ``pgd_design_update`` in numpy, ``sample_chunk`` samples at a time: (sum w log det H, sum w H^-1)."""
    n = [t.shape[1] for t in tables]
    S, D = int(np.prod(n, dtype=np.int64)), len(n)
    rows = np.zeros((0, tables[0].shape[0])) if rows is None else np.asarray(rows, dtype=np.float64).reshape(-1, tables[0].shape[0])
    logdet, cov = 0.0, np.zeros((D, D))
    for s0 in range(0, S, int(sample_chunk)):
        s = np.arange(s0, min(S, s0 + int(sample_chunk)))
        sl = slice(s0, s0 + len(s))
        CD, idx = _grid_derivative_coefficients(tables, dtables, n, s)
        H = state["H"][sl]
        if h0 is not None:
            H[:] = np.asarray(h0, dtype=np.float64)
        if rows.shape[0]:
            G = np.einsum("rt,dts->rds", rows, CD)                           # (R, D, s)
            for r in range(rows.shape[0]):
                H += G[r].T[:, :, None] * G[r].T[:, None, :]
        W = _cholesky_inverse_batch(H)
        state["W"][sl] = W
        w = np.ones(len(s))
        for d in range(D):
            w *= weights[d][idx[d]]
        logdet += float(np.sum(w * (-2.0 * np.sum(np.log(np.einsum("sii->si", W)), axis=1))))
        cov += np.einsum("s,smi,smj->ij", w, W, W)
    return logdet, np.triu(cov) + np.triu(cov, 1).T


def design_gains_numpy(a, R, state, tables, dtables, weights, work=1 << 22):
    """The arithmetic of ``pgd_design_gains`` in numpy, in chunks of samples that keep the Jacobians below ``work`` doubles: the gains
    of the M candidates whose R rows each are the rows of ``a`` (M R, k), from the LDL^T pivots of I + V^T V as log1p(pivot - 1)."""
    a = np.asarray(a, dtype=np.float64)
    n = [t.shape[1] for t in tables]
    S, D, M = int(np.prod(n, dtype=np.int64)), len(n), a.shape[0] // R
    chunk = max(int(work) // max(a.shape[0] * D, 1), 1)
    gains = np.zeros(M)
    for s0 in range(0, S, chunk):
        s = np.arange(s0, min(S, s0 + chunk))
        CD, idx = _grid_derivative_coefficients(tables, dtables, n, s)
        G = np.stack([a @ CD[d] for d in range(D)])                           # (D, M R, s)
        W = state["W"][s0:s0 + len(s)]
        V = np.stack([np.einsum("sj,jps->ps", W[:, i, :i + 1], G[:i + 1]) for i in range(D)]).reshape(D, M, R, len(s))
        # LDL^T of I + V^T V without the 1 on the diagonal: mm[p][q] is row p of the Schur complement, mm[p][p] = pivot p less 1
        mm, lf, val = {}, {}, 0.0
        for p in range(R):
            for q in range(p, R):
                t = np.einsum("ims,ims->ms", V[:, :, p], V[:, :, q])
                for r in range(p):
                    t = t - lf[p, r] * mm[r, q]
                mm[p, q] = t
            val = val + np.log1p(mm[p, p])
            for q in range(p + 1, R):
                lf[q, p] = mm[p, q] / (1.0 + mm[p, p])
        w = np.ones(len(s))
        for d in range(D):
            w *= weights[d][idx[d]]
        gains += (val * w).sum(axis=1)
    return 0.5 * gains


class PGD:
    def __init__(self, name=None, n_modes=0, fmeshes=[], pgd_modes=[], name_coord=[], modes_info=[],
                 verbose=False, *args, **kwargs):
        self.logger = logging.getLogger(__name__ + "." + self.__class__.__name__)
        self.name = name
        self.numModes = n_modes
        self.used_numModes = n_modes
        self.problem = None
        self.folder = ""
        self.pos = 0                  # point used by evaluate_abs_value
        self._eval_fixed_modes = {}
        self.name_coord, self.modes_info = name_coord, modes_info
        self.mesh = []
        info = list(modes_info) + ["u", "Node", "Scalar"][len(modes_info):]
        for d, fm in enumerate(fmeshes):
            pm = PGDMesh("PGD%d" % (d + 1), fm, [name_coord[d]] if d < len(name_coord) else [])
            att = PGDAttribute(info[0], n_modes, info[1], info[2])
            att.fill_data(list(pgd_modes[d])[:n_modes] if d < len(pgd_modes) else [])   # the first n_modes (model.py:1483-1487)
            pm.attributes.append(att)
            self.mesh.append(pm)
        if verbose:
            self.print_info()

    @property
    def num_pgd_var(self):
        return len(self.mesh)

    def __str__(self):
        return "PGD(name: %s)(meshes: %s)(modes: %s)" % (self.name, len(self.mesh), self.numModes)

    __repr__ = __str__

    def _info_str(self):
        return ("summary of PGDModel class\n-------------------------------\n"
                "name:                          %s\nnumber of PGD variables:       %s\n"
                "number of modes for each mesh -- max: %s -- used: %s\nnumber of saved meshes:        %s\n"
                "number of elements per mesh:    %s\nfolder:                        %s" % (
                    self.name, self.num_pgd_var, self.numModes, self.used_numModes, len(self.mesh),
                    "".join(" %s, " % m.numElements for m in self.mesh), self.folder))

    def create_from_problem(self, problem=None):
        self.problem = problem
        self.name = problem.name
        self.logger.info("PGDModel created from PGDProblem %s", self.name)
        return self

    def print_info(self):
        print("PGD solution %r: %d modes, %d coordinates" % (self.name, self.numModes, self.num_pgd_var))
        for m in self.mesh:
            print("  %s %s: %d nodes, %d elements" % (m.name, m.info, m.numNodes, m.numElements))

    @property
    def fenics_meshes(self):
        return [m.fenics_mesh for m in self.mesh]

    # ------------------------------------------------------------------------ result files
    def _grid_info(self, d):
        """[dimension, coordinate name, unit] of a PGD coordinate, the three <Information> items of a grid."""
        m = self.mesh[d]
        if len(m.info) >= 3:
            return [int(m.info[0]), str(m.info[1]), str(m.info[2])]
        return [int(m.meshdim), str(m.info[0]) if m.info else "C%d" % d, "-?-"]

    @staticmethod
    def _visual(att, k, pad):
        """Node data of mode k as the reference's XDMF writer lays it out: (N, 1) for a scalar field,
        (N, 3) zero-padded for a vector field."""
        a = np.asarray(att.data[k], dtype=np.float64)
        if a.ndim == 1:
            a = a.reshape(-1, 1)
        if a.shape[1] > 1 or pad:
            out = np.zeros((a.shape[0], 3))
            out[:, :a.shape[1]] = a
            return out
        return a

    def write_hdf5(self, folder):
        """``<grid>_data.h5`` per coordinate: the mesh and the mode FUNCTIONS (dof vectors with their cell -> dof tables)
        as ``dolfin.HDF5File`` lays them out - ``mesh``, ``MODE_0``, ``MODE_1``, ... (model.py:162-181; further attributes
        of a coordinate, which the reference overwrites under the same names, go to ``ATT<a>_MODE_<k>``)."""
        for pm in self.mesh:
            out = fem.HDF5File(fem.MPI.comm_world, os.path.join(folder, pm.name + "_data.h5"), "w")
            out.write(pm.fenics_mesh, "mesh")
            for a, att in enumerate(pm.attributes):
                for k in range(self.numModes):
                    out.write(att.interpolationfct[k], ("MODE_%d" % k) if a == 0 else "ATT%d_MODE_%d" % (a, k))
            out.close()
        self.logger.info("Wrote %i HDF files for Mode data", self.num_pgd_var)

    def _write_xdmf(self, folder):
        """``<grid>.xdmf`` + ``<grid>.h5`` per coordinate through ``XDMFFile``: /Mesh/0/mesh/{topology, geometry} and the
        vertex values of every mode in /VisualisationVector/<k> (model.py:183-196)."""
        for pm in self.mesh:
            out = fem.XDMFFile(os.path.join(folder, pm.name + ".xdmf"))
            out.write(pm.fenics_mesh)
            for att in pm.attributes:
                for k in range(self.numModes):
                    out.write(att.interpolationfct[k], k)
            out.close()

    def _grid_xml(self, pm, pad_vectors, ind, folder):
        """One <Grid> of the pxdmf file, its data items pointing into ``<grid>.h5`` exactly as the reference writes them
        (model.py:236-392)."""
        d = self.mesh.index(pm)
        dims, cname, unit = self._grid_info(d)
        with h5lite.File(os.path.join(folder, pm.name + ".h5"), "r") as hf:
            tshape = np.array(hf.get("Mesh/0/mesh/topology")).shape
            gshape = np.array(hf.get("Mesh/0/mesh/geometry")).shape
            out = [ind + '<Grid Name="%s">' % pm.name,
                   ind + '  <Information Name="Dims" Value="%s" />' % dims,
                   ind + '  <Information Name="Dim0" Value="%s" />' % cname,
                   ind + '  <Information Name="Unit0" Value="%s" />' % unit,
                   ind + '    <Topology NumberOfElements = "%d" TopologyType = "%s" NodesPerElement = "%d" >' % (
                       pm.numElements, pm.typElements, tshape[1]),
                   ind + '      <DataItem Dimensions = "%d %d" NumberType = "UInt" Format = "HDF">%s.h5:/Mesh/0/mesh/topology</DataItem>' % (
                       pm.numElements, tshape[1], pm.name),
                   ind + "    </Topology>",
                   ind + '    <Geometry GeometryType = "%s">' % ("XY" if gshape[1] == 2 else "XYZ"),
                   ind + '      <DataItem Dimensions = "%d %d" Format = "HDF">%s.h5:/Mesh/0/mesh/geometry</DataItem>' % (
                       gshape[0], gshape[1], pm.name),
                   ind + "    </Geometry>"]
            count = 0
            for att in pm.attributes:
                for k in range(len(att.data)):
                    out.append(ind + '    <Attribute Name="%s_%d" AttributeType="%s" Center="Node">' % (att.name, k, att.field))
                    if att.field.lower() == "vector" and pad_vectors:
                        # grids of different dimension in one file: vector attributes carry three components on every grid,
                        # a 1-D coordinate repeating its values (model.py:321-368), written inline
                        raw = np.array(hf.get("/VisualisationVector/%d" % count))
                        v = np.zeros((raw.shape[0], 3))
                        if dims > 1:
                            v[:, :raw.shape[1]] = raw
                        else:
                            v[:] = raw[:, :1]
                        out.append(ind + '      <DataItem Dimensions="%d 3" Format="XML" NumberType="float" >' % v.shape[0])
                        out.extend("%.8e %.8e %.8e" % tuple(r) for r in v)
                        out.append(ind + "      </DataItem>")
                    else:
                        vshape = np.array(hf.get("/VisualisationVector/%d" % count)).shape
                        out.append(ind + '      <DataItem Dimensions="%d %d" Format="HDF">%s.h5:/VisualisationVector/%d</DataItem>' % (
                            vshape[0], vshape[1], pm.name, count))
                    out.append(ind + "    </Attribute>")
                    count += 1
        out.append(ind + "</Grid>")
        return "\n".join(out) + "\n"

    def write_pxdmf(self, folder, xdmf_exist=False):
        """One ``<name>.pxdmf`` with a grid per PGD coordinate and its modes as attributes - the file the
        ParaView PGD plugin opens (model.py:198-416); the heavy data stay in the ``<grid>.h5`` files."""
        if xdmf_exist is False:
            self._write_xdmf(folder)
        dims = [self._grid_info(d)[0] for d in range(self.num_pgd_var)]
        pad = max(dims) != min(dims)
        path = os.path.join(folder, self.name + ".pxdmf")
        with open(path, "w") as f:
            f.write('<?xml version="1.0"?><!--pxdmf written by pgdrome_amd.model.PGD.write_pxdmf-->\n')
            f.write('<!DOCTYPE Xdmf SYSTEM "Xdmf.dtd" []>\n')
            f.write('<Xdmf Version="3.0" xmlns:xi="http://www.w3.org/2001/XInclude">\n')
            f.write('  <Domain Name="%s.pxdmf">\n' % self.name)
            for pm in self.mesh:
                f.write(self._grid_xml(pm, pad, "    ", folder))
            f.write("  </Domain>\n</Xdmf>")
        self.logger.info("Wrote %s ", path)

    @staticmethod
    def _read_item(item, folder):
        """numpy array of a <DataItem>: inline XML, HDF (``file.h5:/path``; h5py when installed, else pgdrome_amd.h5lite)
        or raw Binary (the files round 1 of this repository wrote)."""
        fmt = item.get("Format", "XML")
        dims = tuple(int(v) for v in item.get("Dimensions").split())
        if fmt == "XML":
            return np.array(item.text.split(), dtype=np.float64).reshape(dims)
        if fmt == "Binary":
            kind = item.get("NumberType", "Float").lower()
            dt = np.dtype(("<" if item.get("Endian", "Little") == "Little" else ">") +
                          ("f" if kind == "float" else "u" if kind == "uint" else "i") + item.get("Precision", "8"))
            with open(os.path.join(folder, item.text.strip()), "rb") as fb:
                fb.seek(int(item.get("Seek", "0")))
                return np.frombuffer(fb.read(int(np.prod(dims)) * dt.itemsize), dtype=dt).reshape(dims).copy()
        if fmt == "HDF":
            fname, key = item.text.strip().split(":")
            try:
                import h5py as h5
            except ImportError:
                h5 = h5lite
            with h5.File(os.path.join(folder, fname), "r") as hf:
                node = hf.get(key)
                if node is None:
                    raise RuntimeError("%s has no dataset %s" % (fname, key))
                return np.array(node)
        raise ValueError("unknown DataItem format %r" % fmt)

    def load_pxdmf(self, filepath, verbose=False):
        """Read a pxdmf file into this instance: ``sol = PGD().load_pxdmf(path)`` (model.py:418-572) - one written here or by
        the reference (inline XML or HDF items).  The mesh of every coordinate comes from ``<grid>_data.h5`` when that file
        is there (``write_hdf5``); the mode functions are attached by ``create_interpolation_fcts``."""
        folder = os.path.dirname(os.path.abspath(filepath))
        root = et.parse(filepath).getroot()
        self.folder = folder
        self.name = root.findall("Domain")[0].attrib.get("Name")
        self.mesh = []
        for g in root.iter("Grid"):
            pm = PGDMesh(g.get("Name"))
            try:
                hdf = fem.HDF5File(fem.MPI.comm_world, os.path.join(folder, pm.name + "_data.h5"), "r")
                pm.fenics_mesh = fem.Mesh()
                hdf.read(pm.fenics_mesh, "mesh", False)
                hdf.close()
            except RuntimeError:
                pm.fenics_mesh = None
            info = [[e.attrib.get("Name"), e.attrib.get("Value")] for e in g.iter("Information")]
            pm.info = [int(info[0][1]), info[1][1], info[2][1]] if len(info) >= 3 else [v for _, v in info]
            pm.meshdim = int(info[0][1])
            for e in g.iter("Topology"):
                pm.numElements = int(e.attrib.get("NumberOfElements"))
                pm.typElements = e.attrib.get("TopologyType")
                pm.topology = self._read_item(e[0], folder).astype(np.int64)
            for e in g.iter("Geometry"):
                pm.typGeometry = e.attrib.get("GeometryType")
                geom = self._read_item(e[0], folder)
                pm.numNodes = geom.shape[0]
                pm.dataX = geom[:, 0].copy()
                pm.dataY = geom[:, 1].copy() if geom.shape[1] > 1 else np.zeros(pm.numNodes)
                pm.dataZ = geom[:, 2].copy() if geom.shape[1] > 2 else np.zeros(pm.numNodes)
            for e in g.iter("Attribute"):
                name = "_".join(e.attrib.get("Name").split("_")[:-1])
                att = next((a for a in pm.attributes if a.name == name), None)
                if att is None:
                    att = PGDAttribute(name, 0, e.attrib.get("Center"), e.attrib.get("AttributeType"))
                    pm.attributes.append(att)
                att.data.append(self._read_item(e[0], folder))
                att.n_modes = len(att.data)
            self.mesh.append(pm)
        self.numModes = self.used_numModes = len(self.mesh[0].attributes[0].data)
        if verbose:
            self.print_info()
            for pm in self.mesh:
                for att in pm.attributes:
                    att.print_info()
        return self

    def _load_mode_functions(self, d, attri):
        """Mode functions of coordinate d from ``<grid>_data.h5`` in the space interpolationInfo names (model.py:640-700)."""
        pm = self.mesh[d]
        att = pm.attributes[attri]
        path = os.path.join(self.folder, pm.name + "_data.h5")
        if not os.path.exists(path):
            raise ValueError("mode functions of dimension %d are missing: %s not found (write_hdf5 creates it)" % (d, path))
        info = att.interpolationInfo
        hdf = fem.HDF5File(fem.MPI.comm_world, path, "r")
        try:
            mesh = fem.Mesh()
            hdf.read(mesh, "mesh", False)
            pm.fenics_mesh = mesh
            kind = str(info.get("_type", "scalar")).lower()
            if kind == "scalar":
                V = fem.FunctionSpace(mesh, info.get("family", "P"), int(info.get("degree", 1)))
            elif kind == "vector":
                V = fem.VectorFunctionSpace(mesh, info.get("family", "P"), int(info.get("degree", 1)))
            else:
                raise ValueError("function space type not defined or wrong defined %s" % (kind,))
            out = []
            for k in range(self.numModes):
                f = fem.Function(V)
                try:
                    hdf.read(f, ("MODE_%d" % k) if attri == 0 else "ATT%d_MODE_%d" % (attri, k))
                except RuntimeError as e:
                    raise ValueError(str(e)) from e
                out.append(f)
        finally:
            hdf.close()
        att.interpolationfct = out

    def save_modes_latex(self, folder, attri, prefix="_"):
        """1-D modes as text tables [dof coordinate, mode 1, mode 2, ...] sorted by coordinate (model.py:1414-1453)."""
        for d, pm in enumerate(self.mesh):
            if str(pm.typElements).lower() != "polyline":
                continue
            fcts = pm.attributes[attri].interpolationfct
            x = fcts[0].function_space().tabulate_dof_coordinates().reshape((-1, 1))[:, 0]
            order = np.argsort(x, kind="stable")
            table = np.zeros((x.size, self.numModes + 1))
            table[:, 0] = x[order]
            for m in range(self.numModes):
                table[:, m + 1] = fcts[m].vector()[:][order]
            np.savetxt(os.path.join(folder, "modes_%s_%i_%s.out" % (prefix, attri, self._grid_info(d)[1])), table, delimiter=",")

    # ------------------------------------------------------------------ interpolation
    def create_interpolation_fcts(self, free_dim, attri, verbose=True):
        if len(free_dim) > self.num_pgd_var:
            raise ValueError("given number of Dimensions larger then existing Meshes in PGD solution")
        if attri > len(self.mesh[free_dim[0]].attributes):
            raise ValueError("attribute number not possible")
        for d in free_dim:
            att, pm = self.mesh[d].attributes[attri], self.mesh[d]
            kind = att.interpolationInfo["name"]
            if kind == 0:
                if np.sum(pm.dataY) != 0 and np.sum(pm.dataZ) != 0:
                    raise ValueError("free Dimensions are not 1D, interpolation with INTERP1D not possible")
                how = att.interpolationInfo["kind"]
                att.interpolationfct = [interpolate.interp1d(pm.dataX, att.data[k][:, 0], kind=how)
                                        for k in range(self.numModes)]
            elif kind == 1:
                if len(att.interpolationfct) != self.numModes:
                    self._load_mode_functions(d, attri)
            else:
                self.logger.error("interpolation name not defined: %s", kind)
        self.logger.info("Attribute interpolation functions saved")

    # --------------------------------------------------------------------- evaluation
    def _check_eval(self, fixed_dim, free_dim, coord, attri):
        if len(free_dim) != self.num_pgd_var - 1:
            raise ValueError("given variables are missing or to much, free_dim=%s <-> num_pgd_var=%s",
                             free_dim, self.num_pgd_var - 1)
        if len(coord) != self.num_pgd_var - 1:
            raise ValueError("given variables are missing or to much, coord=%s <-> num_pgd_var=%s",
                             coord, self.num_pgd_var - 1)
        if len(free_dim) != len(coord):
            raise ValueError("Number of free Dimensions and given coordinates are not the same, "
                             "free_dim=%s <-> coord=%s", free_dim, coord)
        if attri >= len(self.mesh[fixed_dim].attributes):
            raise ValueError("attribute number not possible")
        for d in free_dim:
            if len(self.mesh[d].attributes[attri].interpolationfct) == 0:
                self.create_interpolation_fcts(free_dim, attri)
                break
        fixed = self.mesh[fixed_dim].attributes[attri]
        if len(fixed.interpolationfct) == 0 and fixed.interpolationInfo.get("name") == 1:
            self.create_interpolation_fcts([fixed_dim], attri)     # a loaded solution: read the mode functions

    def mode_factors(self, free_dim, coord, attri):
        """c_k = prod_i F_i^k(coord_i) for every used mode."""
        c = np.ones(self.used_numModes)
        for k in range(self.used_numModes):
            for i, d in enumerate(free_dim):
                c[k] *= float(self.mesh[d].attributes[attri].interpolationfct[k](coord[i]))
        return c

    def evaluate(self, fixed_dim, free_dim, coord, attri):
        """PGD solution on the fixed dimension for given coordinates of all other dimensions:
        a numpy array (vertex values) in the interp1d mode, otherwise a Function."""
        self._check_eval(fixed_dim, free_dim, coord, attri)
        att = self.mesh[fixed_dim].attributes[attri]
        c = self.mode_factors(free_dim, coord, attri)
        if self.mesh[free_dim[0]].attributes[attri].interpolationInfo["name"] == 0:
            out = np.zeros(att.data[0].shape)
            for k in range(self.used_numModes):
                out += c[k] * att.data[k]
            return out
        modes = att.interpolationfct
        V = modes[0].function_space()
        out = fem.Function(V)
        if V.dim() >= DEVICE_EVAL_MIN_DOFS:
            be = fem.get_backend()
            be.vec_lincomb(out.vector().dev_for_write(), [modes[k].vector().dev() for k in range(self.used_numModes)], c)
            out.vector().touched_dev()
        else:
            acc = np.zeros(V.dim())
            for k in range(self.used_numModes):
                acc += c[k] * modes[k].vector().host()
            out.vector()._host = acc
            out.vector().touched_host()
        return out

    def _evaluated_values(self, fixed_dim, free_dim, coord, attri):
        """All values of the evaluated field: the array itself (interp1d mode) or the dof vector."""
        u = self.evaluate(fixed_dim, free_dim, coord, attri)
        return u if isinstance(u, np.ndarray) else u.vector()[:]

    def evaluate_min(self, fixed_dim, free_dim, coord, attri, *args, **kwargs):
        return float(np.min(self._evaluated_values(fixed_dim, free_dim, coord, attri)))

    def evaluate_min_abs(self, fixed_dim, free_dim, coord, attri, *args, **kwargs):
        return float(np.min(np.abs(self._evaluated_values(fixed_dim, free_dim, coord, attri))))

    def evaluate_max(self, fixed_dim, free_dim, coord, attri, *args, **kwargs):
        return float(np.max(self._evaluated_values(fixed_dim, free_dim, coord, attri)))

    def evaluate_max_abs(self, fixed_dim, free_dim, coord, attri, *args, **kwargs):
        return float(np.max(np.abs(self._evaluated_values(fixed_dim, free_dim, coord, attri))))

    def evaluate_max_norm(self, fixed_dim, free_dim, coord, attri, *args, **kwargs):
        """Largest Euclidean norm of the field over the nodes (vector-valued fields; model.py:1033-1069)."""
        u = self.evaluate(fixed_dim, free_dim, coord, attri)
        if isinstance(u, np.ndarray):
            return float(np.max(np.linalg.norm(u.reshape(u.shape[0], -1), axis=1)))
        V = u.function_space()
        if V.mesh().geometry().dim() == 1:
            raise ValueError("Function is 1D use evaluate_max instead!!")
        return float(np.max(np.linalg.norm(u.vector()[:].reshape(-1, V._ncomp), axis=1)))

    def evaluate_abs_value(self, fixed_dim, free_dim, coord, attri, *args, **kwargs):
        """max |u(self.pos)| - the field at the point stored in ``pos`` (model.py:1071-1086)."""
        return float(np.max(np.abs(self.evaluate(fixed_dim, free_dim, coord, attri)(self.pos))))

    # ------------------------------------------------------------- batched online evaluation
    def _free_modes_at(self, d, x, attri):
        """All used modes of the free dimension d at the coordinates x (array of S points): shape (used_numModes, S)."""
        att = self.mesh[d].attributes[attri]
        fcts = att.interpolationfct[:self.used_numModes]
        x = np.asarray(x, dtype=np.float64)
        if att.interpolationInfo.get("name") == 0:
            return np.array([np.asarray(f(x), dtype=np.float64).reshape(-1) for f in fcts])     # interp1d: takes the array
        f0 = fcts[0]
        V = f0.function_space() if isinstance(f0, fem.Function) else None
        if (V is not None and V._ncomp == 1 and not V._dg0 and V.mesh().topology().dim() == 1 and x.ndim == 1
                and V._lay.degree in (1, 2) and all(isinstance(f, fem.Function) and f.function_space() is V for f in fcts)):
            # 1-D P1 / P2: cell by searchsorted, basis values, one gather and one contraction for all modes and points
            lay, mesh = V._lay, V.mesh()
            X, cells = mesh.coordinates()[:, 0], mesh.cells()
            a, b = X[cells[:, 0]], X[cells[:, 1]]
            lo = np.minimum(a, b)
            order = np.argsort(lo, kind="stable")
            c = order[np.clip(np.searchsorted(lo[order], x, side="right") - 1, 0, len(order) - 1)]
            l1 = (x - a[c]) * (1.0 / (b[c] - a[c]))
            l0 = 1.0 - l1
            bad = np.minimum(l0, l1) < -1e-10
            if bad.any():
                raise ValueError("point %r outside the mesh of dimension %d" % (float(x[np.argmax(bad)]), d))
            if lay.degree == 1:
                nodes, N = cells[c], np.stack([l0, l1], axis=1)
            else:
                nodes, N = lay.cells[c], np.stack([l0 * (2.0 * l0 - 1.0), l1 * (2.0 * l1 - 1.0), 4.0 * l0 * l1], axis=1)
            G = np.stack([f.vector().host() for f in fcts])                   # (K, dofs)
            return np.einsum("sa,ksa->ks", N, G[:, nodes])
        # anything else (2-D / 3-D free dimensions, vector-valued free modes): the scalar callables, point by point
        out = np.empty((len(fcts), x.shape[0]))
        for j in range(x.shape[0]):
            for k, f in enumerate(fcts):
                try:
                    out[k, j] = float(f(x[j]))
                except RuntimeError as e:           # "point ... outside the mesh"
                    raise ValueError(str(e)) from e
        return out

    def _check_many(self, fixed_dim, free_dim, coords, attri):
        coords = np.asarray(coords, dtype=np.float64)
        if coords.ndim == 1 and len(free_dim) == 1:
            coords = coords.reshape(-1, 1)
        if coords.ndim < 2 or coords.shape[0] < 1:
            raise ValueError("coords must be array-like of shape (samples, len(free_dim)) with at least one sample, got shape %s"
                             % (coords.shape,))
        if coords.shape[1] != len(free_dim):
            raise ValueError("Number of free Dimensions and given coordinates are not the same, free_dim=%s <-> "
                             "coordinates per sample=%s" % (free_dim, coords.shape[1]))
        for d in free_dim:
            if attri >= len(self.mesh[d].attributes) or attri < 0:
                raise ValueError("attribute number not possible")
        if fixed_dim is not None:
            self._check_eval(fixed_dim, free_dim, list(coords[0]), attri)
        else:
            for d in free_dim:
                if len(self.mesh[d].attributes[attri].interpolationfct) == 0:
                    self.create_interpolation_fcts(free_dim, attri)
                    break
        return coords

    def mode_factors_many(self, free_dim, coords, attri):
        """C[k, s] = prod_i F_i^k(coords[s, i]) for every used mode and every sample: shape (used_numModes, S), a handful of
        array operations per free dimension (``mode_factors`` makes used_numModes * len(free_dim) Python calls per sample)."""
        coords = self._check_many(None, free_dim, coords, attri)
        C = np.ones((self.used_numModes, coords.shape[0]))
        for i, d in enumerate(free_dim):
            x = coords[:, i] if coords.ndim == 2 else coords[:, i, ...]
            C *= self._free_modes_at(d, x, attri)
        return C

    def evaluate_many(self, fixed_dim, free_dim, coords, attri, stats=True, envelope=False, threshold=None, fields=False,
                      fields_max_bytes=4 << 30, sample_chunk=256):
        """The PGD solution on the fixed dimension for S coordinate sets of the other dimensions in ONE pass over the modes:
        the product U = F C (fixed-dimension modes times ``mode_factors_many``) with its reductions formed where the product
        is - on the device (``pgd_eval_batch``) when the backend has it, the modes are Functions and the fixed space has
        at least DEVICE_EVAL_MIN_DOFS dofs (as ``evaluate`` decides), otherwise in numpy, ``sample_chunk`` samples at a time.

        Returns an ``EvalManyResult``: ``min`` / ``max`` / ``max_abs`` (numpy, (S,)) when ``stats``; ``envelope_min`` /
        ``envelope_max`` (per dof, over the samples) when ``envelope``; ``exceedance`` (per dof, the fraction of the samples
        with u > threshold) when ``threshold`` is not None; ``fields`` (the S fields themselves) when ``fields``;
        ``coefficients`` = C.  Functions on the fixed space (arrays in the interp1d mode).  NaNs give unspecified statistics."""
        coords = self._check_many(fixed_dim, free_dim, coords, attri)
        S = coords.shape[0]
        att = self.mesh[fixed_dim].attributes[attri]
        as_arrays = self.mesh[free_dim[0]].attributes[attri].interpolationInfo["name"] == 0
        K = self.used_numModes
        modes = att.interpolationfct
        V = None
        if as_arrays:
            n = int(np.prod(att.data[0].shape))
            fmesh = self.mesh[fixed_dim].fenics_mesh
            sharded = fmesh is not None and getattr(fmesh, "part", None) is not None
        else:
            V = modes[0].function_space()
            n = V.dim()
            lay = V._lay.base if V._ncomp > 1 else V._lay
            sharded = V.mesh().part is not None or getattr(lay, "part", None) is not None
        if sharded:
            raise NotImplementedError("evaluate_many on a row-sharded fixed dimension (every rank holds a slab of the modes; "
                                      "the per-sample statistics would need a reduction across ranks)")
        if fields and n * S * 8 > fields_max_bytes:
            raise ValueError("evaluate_many: fields=True would store %d bytes (%d dofs x %d samples x 8), more than "
                             "fields_max_bytes=%d" % (n * S * 8, n, S, fields_max_bytes))
        thr = None if threshold is None else float(threshold)
        C = self.mode_factors_many(free_dim, coords, attri)
        be = fem.get_backend()
        if (not as_arrays and n >= DEVICE_EVAL_MIN_DOFS and K <= 256 and all(isinstance(m, fem.Function) for m in modes[:K])
                and hasattr(be, "eval_batch")):
            handles = [modes[k].vector().dev() for k in range(K)]
            res = _eval_many_device(be, lambda st, **kw: be.eval_batch(handles, C, stats=st, **kw), V, n, S, stats, envelope, thr, fields)
            fem.STATS["eval_batch_calls"] = fem.STATS.get("eval_batch_calls", 0) + 1
        else:
            if as_arrays:
                F = np.stack([np.asarray(att.data[k], dtype=np.float64).reshape(-1) for k in range(K)], axis=1)
                wrap = lambda a: a.reshape(att.data[0].shape)
            else:
                F = np.stack([modes[k].vector().host() for k in range(K)], axis=1)
                wrap = lambda a: _host_function(V, a)
            res = _eval_many_host(lambda j0, step: F @ C[:, j0:j0 + step], n, S, sample_chunk, stats, envelope, thr, fields, wrap)
        res.coefficients = C
        return res

    # ----------------------------------------------- Gram matrices of the modes: norms, distances, compression
    def _gram_family(self, dim, attri):
        """(modes, V) of a dimension for the Gram calls: Functions on one space, not row-sharded."""
        if dim < 0 or dim >= self.num_pgd_var or attri < 0 or attri >= len(self.mesh[dim].attributes):
            raise ValueError("dimension or attribute number not possible")
        att = self.mesh[dim].attributes[attri]
        if att.interpolationInfo.get("name") == 0:
            raise NotImplementedError("Gram matrices of interp1d modes (the modes must be Functions: interpolation name 1)")
        if len(att.interpolationfct) == 0:
            self.create_interpolation_fcts([dim], attri)
        modes = list(att.interpolationfct[:self.used_numModes])
        if not modes or not all(isinstance(m, fem.Function) for m in modes):
            raise NotImplementedError("Gram matrices need the modes as Functions")
        V = modes[0].function_space()
        lay = V._lay.base if V._ncomp > 1 else V._lay
        if V.mesh().part is not None or getattr(lay, "part", None) is not None:
            raise NotImplementedError("Gram matrices on a row-sharded dimension (every rank holds a slab of the modes; the "
                                      "blocks would need a reduction across ranks)")
        if not all(m.function_space() is V for m in modes):
            raise ValueError("the modes of dimension %d live on different spaces" % dim)
        return modes, V

    @staticmethod
    def _same_space(V, W):
        if V is W:
            return True
        if V.dim() != W.dim() or V._ncomp != W._ncomp or V._lay.degree != W._lay.degree or V._dg0 != W._dg0:
            return False
        a, b = V.mesh(), W.mesh()
        return a is b or (np.array_equal(a.coordinates(), b.coordinates()) and np.array_equal(a.cells(), b.cells()))

    @staticmethod
    def _gram_block(V, xs, ys=None):
        """X^T Y of two lists of Functions on V (ys None: X^T X, symmetric bit for bit): ``pgd_vec_gram`` when the backend has
        it and the space has at least DEVICE_EVAL_MIN_DOFS dofs - the rule of ``evaluate_many`` - otherwise numpy."""
        be = fem.get_backend()
        if V.dim() >= DEVICE_EVAL_MIN_DOFS and hasattr(be, "vec_gram"):
            G = be.vec_gram([f.vector().dev() for f in xs], None if ys is None else [f.vector().dev() for f in ys])
            fem.STATS["gram_calls"] = fem.STATS.get("gram_calls", 0) + 1
            return G
        X = np.stack([f.vector().host() for f in xs], axis=1)
        if ys is None:
            G = X.T @ X
            return 0.5 * (G + G.T)
        return X.T @ np.stack([f.vector().host() for f in ys], axis=1)

    def _mass_products(self, dim, attri, modes, V):
        """[M f for f in modes] with M the mass atom of V (u v dx; dot(u, v) dx on vector spaces), assembled once per attribute."""
        att = self.mesh[dim].attributes[attri]
        be = fem.get_backend()
        hit = getattr(att, "_gram_mass", None)
        if hit is None or hit[0] is not be or hit[1] is not V:
            u, v = fem.TrialFunction(V), fem.TestFunction(V)
            hit = (be, V, fem.assemble((fem.dot(u, v) if V._ncomp > 1 else u * v) * fem.dx).op())
            att._gram_mass = hit
        lo, hi = V._lay.owned_range()
        out = []
        for f in modes:
            w = fem.Function(V)
            be.spmv(hit[2], f.vector().dev(), w.vector().dev_for_write(), lo, hi)
            w.vector().touched_dev()
            out.append(w)
        return out

    def mode_gram(self, dim, attri=0, metric="l2", other=None):
        """The Gram matrix G (K x K) of the used modes of dimension ``dim``; with another ``PGD`` on the same space the cross
        block (K x K').  ``metric`` "l2": the Euclidean product of the dof vectors; "mass": F^T M F' with the mass matrix of the
        dimension's space (the L2 product of the functions), symmetrised as (G + G^T) / 2 without ``other``.  One pass over the
        modes on the device (``pgd_vec_gram``) under the rule of ``evaluate_many``, numpy otherwise."""
        if metric not in ("l2", "mass"):
            raise ValueError("mode_gram: metric must be 'l2' or 'mass', got %r" % (metric,))
        if other is not None and not isinstance(other, PGD):
            raise ValueError("mode_gram: other must be a PGD")
        xs, V = self._gram_family(dim, attri)
        ys = None
        if other is not None and other is not self:
            if dim >= other.num_pgd_var:
                raise ValueError("mode_gram: the other model has no dimension %d" % dim)
            ys, W = other._gram_family(dim, attri)
            if not self._same_space(V, W):
                raise ValueError("mode_gram: the two models live on different spaces in dimension %d" % dim)
        if metric == "l2":
            return self._gram_block(V, xs, ys)
        if ys is None:
            G = self._gram_block(V, xs, self._mass_products(dim, attri, xs, V))
            return 0.5 * (G + G.T)
        return self._gram_block(V, xs, other._mass_products(dim, attri, ys, ys[0].function_space()))

    def _inner(self, other, attri, metric):
        return _hadamard_sum([self.mode_gram(d, attri, metric, other) for d in range(self.num_pgd_var)])

    def separated_norm(self, attri=0, metric="l2"):
        """|u| = sqrt(1^T (o_d G_d) 1) of the separated function over all dimensions, from the Gram matrices of its modes."""
        return math.sqrt(max(self._inner(None, attri, metric), 0.0))

    def distance(self, other, attri=0, metric="l2", relative=True):
        """|u - v| of two separated solutions on the same spaces from the three Hadamard products (u, u), (u, v), (v, v) of
        their Gram blocks - no field is reconstructed - divided by |u| when ``relative``.

        The difference of squares cancels: the result is NOT RESOLVED below about 1e-8 |u| (sqrt(2^-53) of the norms that
        cancel).  Values below that floor are returned as they come, clipped at 0 before the root."""
        if not isinstance(other, PGD) or other.num_pgd_var != self.num_pgd_var:
            raise ValueError("distance: another PGD with the same number of dimensions is needed")
        uu = self._inner(None, attri, metric)
        if other is self:
            uv = vv = uu
        else:
            uv, vv = self._inner(other, attri, metric), other._inner(None, attri, metric)
        d = math.sqrt(max(uu - 2.0 * uv + vv, 0.0))
        return d / math.sqrt(uu) if relative and uu > 0.0 else d

    def evaluate_norm_many(self, fixed_dim, free_dim, coords, attri, metric="l2"):
        """(S,) norms sqrt(c_s^T G c_s) of the fixed-dimension field at S coordinate sets of the other dimensions, with
        C = ``mode_factors_many`` and ONE Gram matrix of the fixed dimension's modes: no field is formed."""
        if metric not in ("l2", "mass"):
            raise ValueError("evaluate_norm_many: metric must be 'l2' or 'mass', got %r" % (metric,))
        coords = self._check_many(fixed_dim, free_dim, coords, attri)
        G = self.mode_gram(fixed_dim, attri, metric)
        Cm = self.mode_factors_many(free_dim, coords, attri)
        return np.sqrt(np.maximum(np.einsum("ks,kl,ls->s", Cm, G, Cm), 0.0))

    @staticmethod
    def _combine_modes(V, modes, W):
        """The R Functions F W (W: K x R) that own their vectors: one ``pgd_eval_batch`` with the fields output and R ranged
        copies on the device under the rule of ``evaluate_many``, a numpy product otherwise."""
        be = fem.get_backend()
        n, (K, R) = V.dim(), W.shape
        out = [fem.Function(V) for _ in range(R)]
        if n >= DEVICE_EVAL_MIN_DOFS and K <= 256 and hasattr(be, "eval_batch") and hasattr(be, "vec_copy_range"):
            store = _FieldStore(be, n, R)
            be.eval_batch([m.vector().dev() for m in modes], np.ascontiguousarray(W), stats=False, fields=store.handle)
            for i, f in enumerate(out):
                be.vec_copy_range(f.vector().dev_for_write(), 0, store.handle, i * n, n)
                f.vector().touched_dev()
            fem.STATS["compress_eval_batch_calls"] = fem.STATS.get("compress_eval_batch_calls", 0) + 1
        else:
            F = np.stack([m.vector().host() for m in modes], axis=1) @ W
            for i, f in enumerate(out):
                f.vector()._host = np.ascontiguousarray(F[:, i])
                f.vector().touched_host()
        return out

    def _like(self, modes, attri):
        """A PGD with the meshes, names and modes_info of this one and the given modes (per dimension) as attribute 0."""
        out = PGD(name=self.name, n_modes=len(modes[0]), fmeshes=self.fenics_meshes, pgd_modes=modes,
                  name_coord=list(self.name_coord), modes_info=list(self.modes_info))
        for pm, src in zip(out.mesh, self.mesh):
            pm.name, pm.info = src.name, list(src.info)
            pm.attributes[0].name = src.attributes[attri].name
        out.problem, out.pos = self.problem, self.pos
        return out

    def compress(self, attri=0, tol=1e-6, max_modes=None, metric="l2", max_sweeps=200):
        """A new ``PGD`` with R <= K modes and |u - u_R| <= tol |u| in ``metric``; this model is untouched.

        The Gram matrices G_d of the modes (one pass per dimension, ``mode_gram``) turn the modes into coordinates in
        orthonormal bases of their spans; there two dimensions are a truncated SVD (the optimal rank for ``tol``), three or more
        a deterministic CP-ALS that grows R until ``tol`` is met (at most ``max_sweeps`` sweeps per R).  The new modes are the
        combinations F_d W_d of the old ones (one ``pgd_eval_batch`` per dimension on the device), ordinary Functions that own
        their vectors; every dimension carries the D-th root of a term's weight, terms come by descending weight, and the sign
        makes the entry of largest magnitude of every mode of dimensions 1 .. D - 1 positive.

        Without ``max_modes``: if no R < K meets ``tol`` a copy of the model comes back (modes_out = K, rel_error = 0).  With
        it: the best R <= max_modes found, ``converged`` False if that misses ``tol``.  ``result.compression`` holds modes_in,
        modes_out, rel_error, tol, metric, sweeps, converged, ranks (of the G_d).  Only attribute ``attri`` is carried over (as
        attribute 0 of the result)."""
        tol = float(tol)
        if not tol >= COMPRESS_TOL_FLOOR:
            raise ValueError("compress: tol = %g is below %g: the Gram route carries half the digits, components below "
                             "sqrt(2^-53) |u| = 1.05e-8 |u| are not resolved" % (tol, COMPRESS_TOL_FLOOR))
        if max_modes is not None and int(max_modes) < 1:
            raise ValueError("compress: max_modes must be at least 1")
        if metric not in ("l2", "mass"):
            raise ValueError("compress: metric must be 'l2' or 'mass', got %r" % (metric,))
        D, K = self.num_pgd_var, self.used_numModes
        fam = [self._gram_family(d, attri) for d in range(D)]
        Gs = [self.mode_gram(d, attri, metric) for d in range(D)]
        plan = compress_grams(Gs, tol, max_modes, max_sweeps)
        info = {"modes_in": K, "modes_out": plan["R"], "rel_error": plan["rel_error"], "tol": tol, "metric": metric,
                "sweeps": plan["sweeps"], "converged": plan["converged"], "ranks": plan["ranks"]}
        if plan["W"] is None:
            out = self._like([[m.copy(deepcopy=True) for m in modes] for modes, _ in fam], attri)
            out.compression = info
            return out
        Ws = [W.copy() for W in plan["W"]]
        new = [None] * D
        for d in range(D - 1, -1, -1):                # dimension 0 last: it takes the signs of the others
            new[d] = self._combine_modes(fam[d][1], fam[d][0], Ws[d])
            if d > 0:
                for i, f in enumerate(new[d]):
                    a = f.vector().host()
                    if a.size and a[int(np.argmax(np.abs(a)))] < 0.0:
                        f.vector().scale(-1.0)
                        Ws[0][:, i] *= -1.0
        out = self._like(new, attri)
        out.compression = info
        return out

    # ------------------------------------------- moments over the parameter domain: mean, variance, Sobol index fields
    @staticmethod
    def _apply_atom(V, op, fs):
        """[A f for f in fs] with the operator handle ``op`` on V."""
        be = fem.get_backend()
        lo, hi = V._lay.owned_range()
        out = []
        for f in fs:
            w = fem.Function(V)
            be.spmv(op, f.vector().dev(), w.vector().dev_for_write(), lo, hi)
            w.vector().touched_dev()
            out.append(w)
        return out

    def _density_function(self, dim, V, density):
        """The density of a parameter dimension as a Function on the modes' space (None: uniform), its dof values checked."""
        if density is None:
            return None
        if isinstance(density, fem.Function):
            if not self._same_space(V, density.function_space()):
                raise ValueError("parameter_moments: the density of dimension %d lives on another space than the modes" % dim)
            rho = density
        elif isinstance(density, fem.Expression):
            rho = fem.interpolate(density, V)
        elif callable(density):
            X = V._lay.coords
            rho = _host_function(V, np.array([float(density(float(x[0])) if X.shape[1] == 1 else density(x)) for x in X]))
        else:
            raise ValueError("parameter_moments: density must be None, a Function, an Expression or a callable, got %r"
                             % (type(density),))
        a = rho.vector().host()
        if not np.all(np.isfinite(a)) or a.min() < 0.0:
            raise ValueError("parameter_moments: the density of dimension %d is negative or not finite at a dof" % dim)
        return rho

    def parameter_moments(self, dim, attri=0, density=None, given=None):
        """(m, C) of the used modes G_k of a parameter dimension under the probability density ``density`` (None: uniform; a
        Function on the modes' space, an Expression or a callable interpolated to it; normalised by its own integral):
        m[k] = int rho G_k and C[k, l] = int rho (G_k - m[k]) (G_l - m[l]).  Both come from the (weighted) mass atom of the
        dimension, ``rho*u*v*dx``: m from one product with the constant, C from the CENTRED modes - the constant lies in the
        space, so G - m 1 is a mode vector again; the difference S - m m^T would lose the variance of nearly constant modes.
        ``given=c`` conditions on the value c of the parameter: (G(c), zeros)."""
        modes, V = self._gram_family(dim, attri)
        if V._ncomp > 1:
            raise NotImplementedError("parameter_moments on a vector-valued parameter space")
        if V._dg0:
            raise NotImplementedError("parameter_moments of cell-wise constant modes")
        K = len(modes)
        if given is not None:
            if density is not None:
                raise ValueError("parameter_moments: dimension %d is given a value and a density" % dim)
            x = np.atleast_1d(np.asarray(given, dtype=np.float64))
            x = x if V.mesh().geometry().dim() == 1 and x.size == 1 else x.reshape(1, -1)
            return np.array(self._free_modes_at(dim, x, attri)[:, 0], dtype=np.float64), np.zeros((K, K))
        rho = self._density_function(dim, V, density)
        be = fem.get_backend()
        u, v = fem.TrialFunction(V), fem.TestFunction(V)
        op = fem.assemble((u * v if rho is None else rho * u * v) * fem.dx).op()
        try:
            one = _host_function(V, np.ones(V.dim()))
            w1 = self._apply_atom(V, op, [one])
            Z = float(self._gram_block(V, [one], w1)[0, 0])
            if not Z > 0.0:
                raise ValueError("parameter_moments: the density of dimension %d has no positive integral" % dim)
            m = self._gram_block(V, modes, w1)[:, 0] / Z
            centred = [_host_function(V, f.vector().host() - m[k]) for k, f in enumerate(modes)]
            C = self._gram_block(V, centred, self._apply_atom(V, op, centred)) / Z
        finally:
            be.atom_free(op)
        return m, 0.5 * (C + C.T)

    def quadratic_forms(self, dim, Q, attri=0, clamp=False, fields=True, row_chunk=8192):
        """The quadratic forms f_i^T Q_q f_i of the used modes of dimension ``dim`` at every dof i, f_i = (F_1(x_i) .. F_K(x_i)),
        for ``Q`` of shape (nq, K, K) or (K, K) - any matrices.  Returns (functions, min, max): a list of nq Functions on the
        dimension's space (None with ``fields=False``) and the arrays of the extrema over the dofs; ``clamp`` stores and reduces
        values below 0 as 0.  One pass over the modes on the device (``pgd_quad_forms``, at most 64 forms per call) under the
        rule of ``evaluate_many``, numpy over ``row_chunk`` rows at a time otherwise."""
        modes, V = self._gram_family(dim, attri)
        K, n = len(modes), V.dim()
        Q = np.asarray(Q, dtype=np.float64)
        if Q.ndim == 2:
            Q = Q[None]
        if Q.ndim != 3 or Q.shape[0] < 1 or Q.shape[1:] != (K, K):
            raise ValueError("quadratic_forms: Q has shape %s, (nq, %d, %d) or (%d, %d) is needed" % (Q.shape, K, K, K, K))
        if not np.all(np.isfinite(Q)):
            raise ValueError("quadratic_forms: Q holds a value that is not finite")
        nq = Q.shape[0]
        be = fem.get_backend()
        out = [fem.Function(V) for _ in range(nq)] if fields else None
        if n >= DEVICE_EVAL_MIN_DOFS and K <= 256 and hasattr(be, "quad_forms"):
            outs = None if out is None else [f.vector().dev_for_write() for f in out]
            mn, mx = be.quad_forms([f.vector().dev() for f in modes], Q, outs, clamp)
            for f in out or ():
                f.vector().touched_dev()
            fem.STATS["quad_forms_calls"] = fem.STATS.get("quad_forms_calls", 0) + 1
            return out, mn, mx
        F = np.stack([f.vector().host() for f in modes], axis=1)
        vals = np.empty((nq, n)) if fields else None
        mn, mx = np.full(nq, np.inf), np.full(nq, -np.inf)
        for r0 in range(0, n, int(row_chunk)):
            Fc = F[r0:r0 + int(row_chunk)]
            for q in range(nq):
                v = np.einsum("ik,ik->i", Fc @ Q[q].T, Fc)
                if clamp:
                    v = np.where(v < 0.0, 0.0, v)
                if v.size:
                    mn[q], mx[q] = min(mn[q], v.min()), max(mx[q], v.max())
                if fields:
                    vals[q, r0:r0 + Fc.shape[0]] = v
        for q, f in enumerate(out or ()):
            f.vector()._host = np.ascontiguousarray(vals[q])
            f.vector().touched_host()
        return out, mn, mx

    @staticmethod
    def _ratio_field(V, num, den, floor):
        """num / den where den > floor, 0 elsewhere: ``pgd_vec_ratio`` under the rule of ``evaluate_many``, numpy otherwise."""
        be = fem.get_backend()
        out = fem.Function(V)
        if V.dim() >= DEVICE_EVAL_MIN_DOFS and hasattr(be, "vec_ratio"):
            be.vec_ratio(out.vector().dev_for_write(), num.vector().dev(), den.vector().dev(), floor)
            out.vector().touched_dev()
        else:
            a, b = num.vector().host(), den.vector().host()
            ok = b > floor
            out.vector()._host = np.where(ok, a / np.where(ok, b, 1.0), 0.0)
            out.vector().touched_host()
        return out

    def variance_decomposition(self, fixed_dim, attri=0, densities=None, given=None, order=1, fields=True, variance_floor=1e-12):
        """Mean, variance and Sobol index fields of the solution on ``fixed_dim`` over the domain of the other dimensions, taken
        as independent random parameters - exact integrals of the separated form, no sampling.  ``densities`` {dim: density}
        (see ``parameter_moments``; missing: uniform), ``given`` {dim: value} conditions on fixed values; every other dimension
        is either random or given.  ``order`` 1 or 2: first-order indices, or second-order interactions as well.

        Every partial variance is a quadratic form of the fixed dimension's modes (``variance_forms``, ``quadratic_forms``: one
        pass over the modes for all of them).  Ratio fields are V_B / V where V > variance_floor * max V and 0 elsewhere
        (Dirichlet nodes are such places).  ``fields=False`` forms extrema and global numbers only.  Returns a
        ``VarianceDecomposition``."""
        D = self.num_pgd_var
        if fixed_dim < 0 or fixed_dim >= D:
            raise ValueError("variance_decomposition: fixed dimension %r not possible" % (fixed_dim,))
        if order not in (1, 2):
            raise ValueError("variance_decomposition: order must be 1 or 2, got %r" % (order,))
        if not (float(variance_floor) >= 0.0):
            raise ValueError("variance_decomposition: variance_floor must be >= 0")
        densities, given = dict(densities or {}), dict(given or {})
        dims = [d for d in range(D) if d != fixed_dim]
        for name, table in (("densities", densities), ("given", given)):
            for d in table:
                if d not in dims:
                    raise ValueError("variance_decomposition: %s names dimension %r, the parameter dimensions are %s" % (name, d, dims))
        both = sorted(set(densities) & set(given))
        if both:
            raise ValueError("variance_decomposition: dimensions %s are given a value and a density" % both)
        random = [d for d in dims if d not in given]
        if not random:
            raise ValueError("variance_decomposition: no random dimension is left (every parameter dimension is given)")
        modes, V = self._gram_family(fixed_dim, attri)
        moments = {d: self.parameter_moments(d, attri, densities.get(d), given.get(d)) for d in dims}
        forms = variance_forms(moments, random, order)
        keys = list(forms)
        funcs, mn, mx = self.quadratic_forms(fixed_dim, np.stack([forms[k] for k in keys]), attri, clamp=True, fields=fields)
        res = VarianceDecomposition()
        res.forms, res.moments, res.random, res.given = forms, moments, list(random), given
        it = keys.index("total")
        res.variance_min, res.variance_max = float(mn[it]), float(mx[it])
        res.extrema = {k: (float(mn[i]), float(mx[i])) for i, k in enumerate(keys)}
        res.floor = float(variance_floor) * res.variance_max
        Gm = self.mode_gram(fixed_dim, attri, "mass")
        glob = {k: float(np.sum(Gm * forms[k].T)) for k in keys}
        res.global_variance = glob["total"]
        ratio = (lambda x: x / glob["total"]) if glob["total"] > 0.0 else (lambda x: 0.0)
        res.global_sobol = {k: ratio(glob[k]) for k in keys if isinstance(k, tuple) and k[0] != "T"}
        res.global_total = {k[1]: ratio(glob[k]) for k in keys if isinstance(k, tuple) and k[0] == "T"}
        m = np.ones(len(modes))
        for d in dims:
            m = m * moments[d][0]
        res.mean_coefficients = m
        if fields:
            res.mean = self._combine_modes(V, modes, m.reshape(-1, 1))[0]
            res.variance = funcs[it]
            for i, k in enumerate(keys):
                if k == "total":
                    continue
                r = self._ratio_field(V, funcs[i], res.variance, res.floor)
                if k[0] == "T":
                    res.partial_total[k[1]], res.total[k[1]] = funcs[i], r
                else:
                    res.partial[k], res.sobol[k] = funcs[i], r
        return res

    # ------------------------------------------------- batched evaluation of gradient quantities
    def evaluate_gradient_many(self, fixed_dim, free_dim, coords, attri, quantity="gradient_norm", scale=None, stats=True,
                               envelope=False, threshold=None, fields=False, fields_max_bytes=4 << 30, modes_max_bytes=16 << 30,
                               sample_chunk=256, planes="stored", at=None, nu=None, component=None):
        """``evaluate_many`` for a quantity of the spatial gradient of the solution: per cell of the fixed mesh and per sample
        the value ``scale * |L grad u|`` with L = ``fem.gradient_quantity(quantity, ...)`` - "gradient_norm" (with a conductivity
        as ``scale``: the flux magnitude) or "von_mises" (with ``scale`` = 2 mu = E / (1 + nu): the von Mises stress).  ``scale``:
        None, a float or a DG0 Function of the fixed mesh.

        The P1 gradient is constant per cell and linear in the mode, so every mode is turned ONCE into q = len(L) cell-wise
        planes (``pgd_cell_gradient``; q * cells * 8 bytes per mode, refused above ``modes_max_bytes``) and kept on the attribute
        until the quantity, the number of used modes, the modes or the ``scale`` (its identity or its vector's version) change;
        a sample batch is then the dense product on the planes with a square root before the reductions
        (``pgd_eval_batch_norm``).  Device or host as ``evaluate_many`` decides, with the cell count in the place of the dofs;
        the host path is numpy, ``sample_chunk`` samples at a time.

        ``planes`` says where the planes live.  "stored" (default) is the above.  "fused" stores none: the kernel forms the planes
        of a block of cells from the nodal modes where it would have read them (``pgd_eval_batch_grad``), so nothing is built,
        cached or bounded by ``modes_max_bytes`` - the way to run many modes on a large mesh; every sample chunk gathers the nodal
        values again, and the matrix-unit kernel refuses q * K above about 1250 (a ValueError).  On the host "fused" combines the
        nodal modes per sample chunk and takes the cell gradients of the chunk's fields.  "auto" is "stored" while the planes
        fit ``modes_max_bytes``, else "fused".

        P2 modes: the gradient is affine per cell, so ``at`` says where in the cell the quantity is taken (``None``, the default,
        refuses P2 modes).  "midpoint": at the barycentre, one value per cell - everything above holds as it stands.  "vertices":
        at the G + 1 corners of every cell, (G + 1) * cells entries (``modes_max_bytes`` counts them).  |L grad u| is the norm of an
        affine function on the cell, hence convex, hence largest at a corner: ``max`` is the exact maximum of the quantity over the
        mesh for every sample, and ``envelope_max`` (DG0: the largest of a cell's corners) the exact maximum over the cell and the
        samples.  ``min`` and ``envelope_min`` are minima over the evaluation points, so upper bounds of the true minima.
        ``threshold`` and ``fields`` are refused with "vertices" (a per-cell exceedance needs the per-sample maximum over a cell's
        points, which the entry-wise kernels do not form).  The planes come from ``pgd_cell_gradient_p2``, the fused product is
        ``pgd_eval_batch_grad_p2``; intervals are always served by the host.  P1 modes take ``None`` or "midpoint" (the same
        thing) and refuse "vertices".

        Quantities of the stress tensor itself, for a displacement field of an isotropic material with Poisson's ratio ``nu`` and
        ``scale`` = E (``fem.stress_quantity``; Lame's lambda is in them, so ``nu`` is needed): "max_principal" (the largest
        principal stress: Rankine, tension in brittle materials), "min_principal", "tresca" (largest minus smallest principal
        stress) and "stress_component" with ``component`` = (a, b), the signed sigma_ab.  Everything above holds for them -
        ``planes``, P1 and P2 with ``at``, host and device (``pgd_eval_batch_quantity`` and its fused forms; the host takes the
        eigenvalues from ``np.linalg.eigvalsh``) - with signed values: ``max_abs`` is max |v| (equal to ``max`` for "tresca").
        What ``at="vertices"`` bounds changes with the quantity: the largest eigenvalue and the spread are convex functions of
        a tensor that is affine on the cell, so for "max_principal" and "tresca" ``max`` and ``envelope_max`` are exact over the
        cell and ``min`` / ``envelope_min`` upper bounds; the smallest eigenvalue is concave, so for "min_principal" ``min`` and
        ``envelope_min`` are exact and ``max`` / ``envelope_max`` lower bounds; a component is affine: both are exact.

        Returns an ``EvalManyResult`` whose Functions live on ``FunctionSpace(mesh, "DG", 0)`` of the fixed mesh; for the two
        norms ``max_abs`` equals ``max``."""
        if planes not in ("stored", "fused", "auto"):
            raise ValueError("evaluate_gradient_many: planes=%r, \"stored\", \"fused\" or \"auto\" are possible" % (planes,))
        if at not in (None, "midpoint", "vertices"):
            raise ValueError("evaluate_gradient_many: at=%r, None, \"midpoint\" or \"vertices\" are possible" % (at,))
        coords = self._check_many(fixed_dim, free_dim, coords, attri)
        S = coords.shape[0]
        att = self.mesh[fixed_dim].attributes[attri]
        if self.mesh[free_dim[0]].attributes[attri].interpolationInfo["name"] == 0:
            raise ValueError("evaluate_gradient_many: the interp1d mode keeps the fixed modes as arrays of vertex values, "
                             "without the mesh a gradient needs")
        K = self.used_numModes
        modes = att.interpolationfct
        if not all(isinstance(m, fem.Function) for m in modes[:K]):
            raise ValueError("evaluate_gradient_many: the fixed dimension's modes are not Functions")
        V = modes[0].function_space()
        if V._dg0 or V._lay.degree not in (1, 2):
            raise NotImplementedError("evaluate_gradient_many: P1 or P2 modes only")
        if V._lay.degree == 2 and at is None:
            raise NotImplementedError("evaluate_gradient_many: P1 modes only unless ``at`` says where in the cell the quantity is "
                                      "taken (the gradient of a P2 mode is not constant per cell): at=\"midpoint\" or at=\"vertices\"")
        if V._lay.degree == 1 and at == "vertices":
            raise ValueError("evaluate_gradient_many: at=\"vertices\" with P1 modes (the gradient is constant per cell: there is "
                             "nothing to choose)")
        lay = V._lay.base if V._ncomp > 1 else V._lay
        mesh = V.mesh()
        lam = None                                       # P2: the barycentric coordinates of the points of every cell
        if V._lay.degree == 2:
            G1 = mesh.topology().dim() + 1
            lam = np.full((1, G1), 1.0 / G1) if at == "midpoint" else np.eye(G1)
        npt = 1 if lam is None else lam.shape[0]
        if npt > 1 and (fields or threshold is not None):
            raise ValueError("evaluate_gradient_many: at=\"vertices\" has %d entries per cell: no ``fields`` and no ``threshold`` "
                             "(a per-cell exceedance needs the per-sample maximum over a cell's points)" % npt)
        if mesh.part is not None or getattr(lay, "part", None) is not None:
            raise NotImplementedError("evaluate_gradient_many on a row-sharded fixed dimension (every rank holds a slab of the "
                                      "modes; the per-sample statistics would need a reduction across ranks)")
        if quantity in fem.STRESS_QUANTITIES:
            if V._ncomp != mesh.geometry().dim():
                raise ValueError("evaluate_gradient_many: %r is a quantity of the stress of a displacement field, the modes have %d "
                                 "component%s in %d-D" % (quantity, V._ncomp, "" if V._ncomp == 1 else "s", mesh.geometry().dim()))
            L, kind = fem.stress_quantity(quantity, mesh.geometry().dim(), nu, component)
        else:
            if nu is not None or component is not None:
                raise ValueError("evaluate_gradient_many: nu and component go with the stress quantities (%s), not with %r"
                                 % (", ".join(repr(k) for k in fem.STRESS_QUANTITIES), quantity))
            L, kind = fem.gradient_quantity(quantity, mesh.geometry().dim(), V._ncomp), fem.EVAL_Q_NORM
        nonneg = kind in (fem.EVAL_Q_NORM, fem.EVAL_Q_EIG_SPREAD)
        scale_vec = None
        if isinstance(scale, fem.Function):
            Vs = scale.function_space()
            if not Vs._dg0 or Vs.mesh() is not mesh:
                raise ValueError("evaluate_gradient_many: scale must be a DG0 Function on the mesh of the fixed dimension")
            scale_vec = scale.vector()
            scale_key = (id(scale_vec), scale_vec.version)
        elif scale is None:
            scale_key = None
        else:
            scale_key = float(scale)
            L = L * scale_key
        q, nc = L.shape[0], mesh.num_cells()
        m = npt * nc                                     # entries: one per point and cell, point-major
        if planes == "auto":
            planes = "stored" if K * q * m * 8 <= modes_max_bytes else "fused"
        if planes == "stored" and K * q * m * 8 > modes_max_bytes:
            raise ValueError("evaluate_gradient_many: the derived modes would take %d bytes (%d modes x %d planes x %s%d cells x "
                             "8), more than modes_max_bytes=%d" % (K * q * m * 8, K, q, "%d points x " % npt if npt > 1 else "", nc,
                                                                  modes_max_bytes))
        if fields and nc * S * 8 > fields_max_bytes:
            raise ValueError("evaluate_gradient_many: fields=True would store %d bytes (%d cells x %d samples x 8), more than "
                             "fields_max_bytes=%d" % (nc * S * 8, nc, S, fields_max_bytes))
        thr = None if threshold is None else float(threshold)
        C = self.mode_factors_many(free_dim, coords, attri)
        be = fem.get_backend()
        Vc = fem.FunctionSpace(mesh, "DG", 0)
        if planes == "fused":
            res = self._evaluate_gradient_fused(be, V, Vc, modes[:K], L, scale_vec, C, S, stats, envelope, thr, fields, sample_chunk, lam,
                                                kind)
        else:
            p2dev = lam is not None and lay.coords.shape[1] > 1 and hasattr(be, "cell_gradient_p2")      # (intervals: the host)
            device = (nc >= DEVICE_EVAL_MIN_DOFS and K <= 256 and
                      hasattr(be, "eval_batch_norm" if kind == fem.EVAL_Q_NORM else "eval_batch_quantity") and
                      (hasattr(be, "cell_gradient") if lam is None else p2dev))
            key = (quantity, K, scale_key, device, id(be), tuple((id(f.vector()), f.vector().version) for f in modes[:K]),
                   None if nu is None else float(nu), None if component is None else tuple(component), at if lam is not None else None)
            cache = getattr(att, "_gradient_modes", None)
            if cache is None or cache.key != key:
                att._gradient_modes = None                       # the old planes go before the new ones are allocated
                cache = att._gradient_modes = _GradientModes(key, be if device else None, mesh, V, modes[:K], L, scale_vec, lam)
                fem.STATS["gradient_mode_builds"] = fem.STATS.get("gradient_mode_builds", 0) + 1
            if device:
                if kind == fem.EVAL_Q_NORM:
                    call = lambda st, **kw: be.eval_batch_norm(cache.planes, q, C, stats=st, **kw)
                else:
                    call = lambda st, **kw: be.eval_batch_quantity(cache.planes, q, kind, C, stats=st, **kw)
                res = (_eval_many_device(be, call, Vc, nc, S, stats, envelope, thr, fields) if npt == 1 else
                       _eval_points_device(be, call, m, stats, envelope))
                fem.STATS["eval_gradient_calls"] = fem.STATS.get("eval_gradient_calls", 0) + 1
            else:
                P = cache.planes                                    # (q, entries, K)

                def norms(j0, step):
                    Cc = C[:, j0:j0 + step]
                    if kind != fem.EVAL_Q_NORM:
                        return _quantity_values(np.stack([P[i] @ Cc for i in range(q)]), kind)
                    ss = np.zeros((m, Cc.shape[1]))
                    for i in range(q):
                        U = P[i] @ Cc
                        ss += U * U
                    return np.sqrt(ss)                              # (entries, cs)
                res = _eval_many_host(norms, m, S, sample_chunk, stats, envelope, thr, fields,
                                      (lambda a: _host_function(Vc, a)) if npt == 1 else (lambda a: a), nonnegative=nonneg)
        if npt > 1 and envelope:                         # the corners of a cell -> DG0 (the entries are point-major)
            res.envelope_min = _host_function(Vc, res.envelope_min.reshape(npt, nc).min(axis=0))
            res.envelope_max = _host_function(Vc, res.envelope_max.reshape(npt, nc).max(axis=0))
        res.coefficients = C
        return res

    @staticmethod
    def _evaluate_gradient_fused(be, V, Vc, modes, L, scale_vec, C, S, stats, envelope, thr, fields, sample_chunk, lam=None,
                                 kind=fem.EVAL_Q_NORM):
        """``evaluate_gradient_many(planes="fused")``: no planes are built or kept.  Device: ``pgd_eval_batch_grad`` on the nodal
        modes (``pgd_eval_batch_grad_p2`` at the points ``lam`` for P2 modes).  Host: per sample chunk the nodal product F C, then
        the cell gradients of the chunk's fields - the einsum of ``_GradientModes`` on the fields instead of the modes.  With more
        than one point per cell the envelopes come back as arrays of points x cells entries.  ``kind``: what becomes of the
        planes (fem.EVAL_Q_*; other than the norm: the backend's ``*_quantity`` calls, ``_quantity_values`` on the host)."""
        mesh, K = V.mesh(), len(modes)
        q, nc, ncomp = L.shape[0], mesh.num_cells(), V._ncomp
        npt = 1 if lam is None else len(lam)
        lay = V._lay.base if ncomp > 1 else V._lay
        fem.STATS["eval_gradient_fused_calls"] = fem.STATS.get("eval_gradient_fused_calls", 0) + 1
        norm = kind == fem.EVAL_Q_NORM
        nonneg = kind in (fem.EVAL_Q_NORM, fem.EVAL_Q_EIG_SPREAD)
        p2dev = (lam is not None and lay.coords.shape[1] > 1 and                                            # (intervals: the host)
                 hasattr(be, "eval_batch_grad_p2" if norm else "eval_batch_grad_p2_quantity"))
        if nc >= DEVICE_EVAL_MIN_DOFS and K <= 256 and (hasattr(be, "eval_batch_grad" if norm else "eval_batch_grad_quantity")
                                                        if lam is None else p2dev):
            handles = [m.vector().dev() for m in modes]
            sc = scale_vec.dev() if scale_vec is not None else 0

            def call(st, **kw):
                try:
                    if lam is not None:
                        if not norm:
                            return be.eval_batch_grad_p2_quantity(V._lay.handle(), handles, lam, L, kind, C, scale=sc, stats=st, **kw)
                        return be.eval_batch_grad_p2(V._lay.handle(), handles, lam, L, C, scale=sc, stats=st, **kw)
                    if not norm:
                        return be.eval_batch_grad_quantity(V._lay.handle(), handles, L, kind, C, scale=sc, stats=st, **kw)
                    return be.eval_batch_grad(V._lay.handle(), handles, L, C, scale=sc, stats=st, **kw)
                except RuntimeError as exc:
                    if getattr(exc, "code", None) != -4:                  # PGD_ERR_LIMIT
                        raise
                    raise ValueError("evaluate_gradient_many(planes=\"fused\"): q = %d planes of K = %d modes are more than the "
                                     "fused kernel holds for a block of cells (q * K up to about 1250): %s" % (q, K, exc)) from None
            if npt > 1:
                return _eval_points_device(be, call, npt * nc, stats, envelope)
            return _eval_many_device(be, call, Vc, nc, S, stats, envelope, thr, fields)
        sc = scale_vec.host() if scale_vec is not None else None
        F = np.stack([m.vector().host() for m in modes], axis=1)                 # (nodes * ncomp, K)
        if lam is not None:
            wrap = (lambda a: _host_function(Vc, a)) if npt == 1 else (lambda a: a)

            def norms_p2(j0, step):
                U = (F @ C[:, j0:j0 + step]).reshape(-1, ncomp, min(step, S - j0))
                P = np.einsum("ij,aejs->iaes", L, _p2_point_gradients(lay, U, lam))       # (q, npt, cells, cs)
                if sc is not None:
                    P = P * sc[None, None, :, None]
                return _quantity_values(P, kind).reshape(npt * nc, -1)
            return _eval_many_host(norms_p2, npt * nc, S, sample_chunk, stats, envelope, thr, fields, wrap, nonnegative=nonneg)
        X, cells = mesh.coordinates(), mesh.cells()
        G = cells.shape[1] - 1
        Einv = np.linalg.inv(X[cells[:, 1:]] - X[cells[:, :1]])                  # rows of E: the edges x_a - x_0; (cells, d, a)

        def norms(j0, step):
            U = (F @ C[:, j0:j0 + step]).reshape(-1, ncomp, min(step, S - j0))    # (node, component, sample)
            dU = U[cells[:, 1:]] - U[cells[:, :1]]                                # (cells, a, c, cs)
            g = np.einsum("eda,eacs->ecds", Einv, dU).reshape(nc, ncomp * G, -1)  # g[c * G + d] = d u_c / d x_d
            P = np.einsum("ij,ejs->ies", L, g)                                    # (q, cells, cs)
            if sc is not None:
                P = P * sc[None, :, None]
            return _quantity_values(P, kind)
        return _eval_many_host(norms, nc, S, sample_chunk, stats, envelope, thr, fields, lambda a: _host_function(Vc, a),
                               nonnegative=nonneg)

    # ------------------------------------------------------ sensor responses and derivatives
    def _check_free(self, free_dim, coord, attri, fixed_dim):
        if len(coord) != self.num_pgd_var - 1:
            raise ValueError("given variables are missing or to much, coord=%s <-> num_pgd_var=%s",
                             coord, self.num_pgd_var - 1)
        for d in free_dim:
            if np.sum(self.mesh[d].dataY) != 0 and np.sum(self.mesh[d].dataZ) != 0:
                raise ValueError("free Dimensions are not 1D, interpolation not possible")
        if attri >= len(self.mesh[fixed_dim].attributes):
            raise ValueError("attribute number not possible")
        for d in free_dim:
            if len(self.mesh[d].attributes[attri].interpolationfct) == 0:
                self.create_interpolation_fcts(free_dim, attri)
                break

    def eval_fixed_modes(self, sensor_points, fixed_dim, attri):
        """ALL modes of the fixed dimension at the sensor points, cached per point set: shape (points, modes) for
        a scalar field, (points, components, modes) for a vector field; a single mode drops the mode axis."""
        pts = np.asarray(sensor_points, dtype=np.float64)
        key = (float(np.sum(pts)), pts.shape, fixed_dim, attri)
        hit = self._eval_fixed_modes.get(key)
        if hit is not None:
            return hit
        modes = self.mesh[fixed_dim].attributes[attri].interpolationfct
        V = modes[0].function_space()
        gdim = V.mesh().geometry().dim()
        pts = pts.reshape(-1, gdim)
        nc = V._ncomp
        base = V._lay.base if nc > 1 else V._lay
        out = np.zeros((pts.shape[0], nc, self.numModes))
        vecs = [modes[k].vector().host() for k in range(self.numModes)]
        for i, x in enumerate(pts):
            nodes, N = fem.point_basis(base, x)
            for k in range(self.numModes):
                for c in range(nc):
                    out[i, c, k] = N @ vecs[k][nodes * nc + c]
        if nc == 1:
            out = out[:, 0, :]
        if self.numModes == 1:
            out = out[..., 0]
        self._eval_fixed_modes[key] = out
        return out

    def _contract_modes(self, eval_fixedmode, factors):
        if self.numModes == 1:
            return eval_fixedmode * factors[0]
        return np.sum(eval_fixedmode[..., 0:self.used_numModes] * factors, axis=-1)

    def evaluate_sensor_response(self, fixed_dim, free_dim, coord, attri, sensor_points):
        """The evaluated field at given points of the fixed dimension, as an array (model.py:862-953)."""
        self._check_free(free_dim, coord, attri, fixed_dim)
        fixed = self.eval_fixed_modes(sensor_points, fixed_dim, attri)
        return self._contract_modes(fixed, self.mode_factors(free_dim, coord, attri))

    def create_derivation_fct(self, free_dim, attri):
        """d mode / d coordinate for the given (1-D, scalar) coordinates as callables (model.py:1088-1205)."""
        if len(free_dim) > self.num_pgd_var:
            raise ValueError("given number of Dimensions larger then existing Meshes in PGD solution")
        if attri > len(self.mesh[free_dim[0]].attributes):
            raise ValueError("attribute number not possible")
        for d in free_dim:
            att = self.mesh[d].attributes[attri]
            if att.interpolationInfo["name"] == 0:
                raise ValueError("derivation for interp1 functions not implemented (only fencis functions)")
            if att.interpolationInfo["name"] != 1:
                self.logger.error("interpolation name not defined: %s", att.interpolationInfo["name"])
                continue
            if att.interpolationfct[0].function_space()._ncomp > 1:
                raise NotImplementedError("derivative of vector-valued modes (tensor DG space)")
            att.derivationfct = [fem.DerivativeFunction(att.interpolationfct[k], 0) for k in range(self.numModes)]
        self.logger.info("derivations for dimensions %s are saved in PGD instance" % (free_dim,))

    def _derivative_factors(self, free_dim, coord, attri, d_dim, fixed_dim):
        self._check_free(free_dim, coord, attri, fixed_dim)
        if fixed_dim == d_dim:
            raise ValueError("derivation against fixed dim not possible in the moment")
        if self.mesh[free_dim[0]].attributes[attri].interpolationInfo["name"] == 0:
            self.logger.error("derivation for interp1 functions not implemented (only fencis functions)")
            raise ValueError("derivation for interp1 functions not implemented (only fencis functions)")
        c = np.ones(self.used_numModes)
        for k in range(self.used_numModes):
            for i, d in enumerate(free_dim):
                att = self.mesh[d].attributes[attri]
                fct = att.derivationfct[k] if d == d_dim else att.interpolationfct[k]
                c[k] *= float(fct(coord[i]))
        return c

    def evaluate_derivative(self, fixed_dim, free_dim, coord, attri, d_dim):
        """d u / d coordinate(d_dim) on the fixed dimension, a Function (model.py:1208-1303)."""
        c = self._derivative_factors(free_dim, coord, attri, d_dim, fixed_dim)
        modes = self.mesh[fixed_dim].attributes[attri].interpolationfct
        out = fem.Function(modes[0].function_space())
        for k in range(self.used_numModes):
            out.vector().axpy(c[k], modes[k].vector())
        return out

    def evaluate_derivative_sensor_response(self, fixed_dim, free_dim, coord, attri, d_dim, sensor_points):
        c = self._derivative_factors(free_dim, coord, attri, d_dim, fixed_dim)
        return self._contract_modes(self.eval_fixed_modes(sensor_points, fixed_dim, attri), c)

    # ------------------------------------------------------ sensor responses for many samples
    def sensor_modes(self, sensor_points, fixed_dim, attri, gradient=False, device=None, index=None):
        """ALL ``numModes`` modes of the fixed dimension (``gradient``: their spatial gradients) at the sensor points: a
        ``SensorModes`` of entries (point, component[, axis]) per mode.  The points are located once (``fem.locate_points``).  Where
        the backend samples point sets (``device=None``: then) every mode is sampled on the device into a vector of P * nc (* gdim)
        entries (pgd_points_sample) and no mode is downloaded; otherwise - the numpy backend, ``device=False`` - one gather and one
        contraction over all modes on the host.  The gradient at a point on a face is that of the cell the location chose.
        Cached per (point set, fixed_dim, attri, gradient, path).  ``index``: handed to ``fem.locate_points`` (the bin index of the mesh:
        the same cells and coordinates, located faster for many points on a mesh that is no lattice)."""
        modes = self.mesh[fixed_dim].attributes[attri].interpolationfct
        if len(modes) < self.numModes or not all(isinstance(m, fem.Function) for m in modes[:self.numModes]):
            raise ValueError("sensor_modes: the modes of dimension %d are no Functions (interp1d modes have no mesh to locate points on)"
                             % (fixed_dim,))
        V = modes[0].function_space()
        fem._refuse_dg0(modes[0], "sensor values")
        mesh, nc = V.mesh(), V._ncomp
        base = V._lay.base if nc > 1 else V._lay
        if mesh.part is not None or getattr(base, "part", None) is not None:
            raise NotImplementedError("sensor_modes on a row-sharded fixed dimension (every rank holds a slab of the modes)")
        be = fem.get_backend()
        on_device = hasattr(be, "points_sample") if device is None else bool(device)
        if on_device and not hasattr(be, "points_sample"):
            raise NotImplementedError("sensor_modes(device=True): the backend %r samples no point sets" % (getattr(be, "name", be),))
        located = fem.locate_points(mesh, sensor_points, device=True if on_device else False, index=index)
        key = (located.key, fixed_dim, attri, bool(gradient), on_device)
        cache = self.__dict__.setdefault("_sensor_modes", {})
        fem.SENSOR_CACHES.add(self)              # fem.clear_caches empties the dictionary (the sampled vectors are freed with it)
        # an entry is the samples of THESE mode vectors in their current versions on THIS backend: anything else is sampled again
        vectors = [m.vector() for m in modes[:self.numModes]]
        stamp = [v.version for v in vectors]
        hit = cache.get(key)
        if hit is not None:
            res, be_then, vectors_then, stamp_then = hit
            if be_then is (be if on_device else None) and len(vectors_then) == len(vectors) and stamp_then == stamp and \
                    all(a is b for a, b in zip(vectors_then, vectors)):
                return res
            del cache[key]
        P, D, K = located.cells.shape[0], mesh.geometry().dim(), self.numModes
        if P == 0:
            raise ValueError("sensor_modes: no sensor points")
        shape = (P,) + ((nc,) if nc > 1 else ()) + ((D,) if gradient else ())
        m = P * nc * (D if gradient else 1)
        if on_device:
            pts = located.device_handle(be)
            handles = []
            for k in range(K):
                handles.append(be.vec_zeros(m))
                be.points_sample(pts, V._lay.handle(), modes[k].vector().dev(), handles[-1], gradient=bool(gradient))
            res = SensorModes(shape, m, be=be, handles=handles)
        else:
            nodes = base.cells[located.cells]                                   # (P, nodes per cell)
            G = np.stack([modes[k].vector().host() for k in range(K)])          # (K, dofs)
            Gn = G[:, (nodes[:, :, None] * nc + np.arange(nc)[None, None, :])]  # (K, P, nodes, nc)
            if gradient:
                _, dN = fem.shape_functions(base, located.lam, located.grad_lambda())
                E = np.einsum("pad,kpac->kpcd", dN, Gn)
            else:
                E = np.einsum("pa,kpac->kpc", fem.shape_functions(base, located.lam), Gn)
            res = SensorModes(shape, m, host=np.ascontiguousarray(E.reshape(K, m)))
        cache[key] = (res, be if on_device else None, vectors, stamp)
        return res

    def mode_factor_derivatives_many(self, free_dim, coords, attri, d_dim):
        """C_d[k, s]: ``mode_factors_many`` with the factor of dimension ``d_dim`` replaced by its derivative with respect to that
        coordinate - the coefficients of d u / d coordinate(d_dim), shape (used_numModes, S).  Vectorised for 1-D scalar P1 / P2
        Function modes; at a mesh node the derivative is the one-sided one of the cell ``fem.point_basis`` picks there (the cell
        with the largest smallest barycentric coordinate, the lowest cell among equal ones), as ``fem.DerivativeFunction`` gives."""
        coords = self._check_many(None, free_dim, coords, attri)
        if d_dim not in list(free_dim):
            raise ValueError("derivation against fixed dim not possible in the moment")
        if self.mesh[free_dim[0]].attributes[attri].interpolationInfo["name"] == 0:
            raise ValueError("derivation for interp1 functions not implemented (only fencis functions)")
        C = np.ones((self.used_numModes, coords.shape[0]))
        for i, d in enumerate(free_dim):
            x = coords[:, i] if coords.ndim == 2 else coords[:, i, ...]
            C *= self._free_mode_derivatives_at(d, x, attri) if d == d_dim else self._free_modes_at(d, x, attri)
        return C

    def _free_mode_derivatives_at(self, d, x, attri):
        """d F^k / d x of all used modes of the free dimension d at the coordinates x: shape (used_numModes, S)."""
        att = self.mesh[d].attributes[attri]
        if att.interpolationInfo.get("name") == 0:
            raise ValueError("derivation for interp1 functions not implemented (only fencis functions)")
        fcts = att.interpolationfct[:self.used_numModes]
        f0 = fcts[0]
        V = f0.function_space() if isinstance(f0, fem.Function) else None
        if V is not None and V._ncomp > 1:
            raise NotImplementedError("derivative of vector-valued modes (tensor DG space)")
        x = np.asarray(x, dtype=np.float64)
        if (V is not None and not V._dg0 and V.mesh().topology().dim() == 1 and x.ndim == 1 and V._lay.degree in (1, 2)
                and all(isinstance(f, fem.Function) and f.function_space() is V for f in fcts)):
            lay, mesh = V._lay, V.mesh()
            X, cells = mesh.coordinates()[:, 0], mesh.cells()
            a, b = X[cells[:, 0]], X[cells[:, 1]]
            lo = np.minimum(a, b)
            order = np.argsort(lo, kind="stable")
            slo = lo[order]
            # the two cells that can hold x: the last one starting at or below it and the one before (x on their common node);
            # point_basis's arithmetic decides between them - the larger smallest barycentric coordinate, then the lower cell
            pos = np.clip(np.searchsorted(slo, x, side="right") - 1, 0, len(order) - 1)
            cand = np.stack([order[pos], order[np.maximum(pos - 1, 0)]], axis=1)                     # (S, 2)
            tinv = 1.0 / (b - a)
            l1 = tinv[cand] * (x[:, None] - a[cand])
            l0 = 1.0 - l1
            mins = np.minimum(l0, l1)
            first = (mins[:, 0] > mins[:, 1]) | ((mins[:, 0] == mins[:, 1]) & (cand[:, 0] <= cand[:, 1]))
            pick = np.where(first, 0, 1)
            rows = np.arange(x.shape[0])
            c = cand[rows, pick]
            bad = ~(mins[rows, pick] >= -1e-10)
            if bad.any():
                raise ValueError("point %r outside the mesh of dimension %d" % (float(x[np.argmax(bad)]), d))
            lam = np.stack([l0[rows, pick], l1[rows, pick]], axis=1)
            g = np.stack([-tinv[c], tinv[c]], axis=1)[:, :, None]                                     # (S, 2, 1)
            _, dN = fem.shape_functions(lay, lam, g)
            G = np.stack([f.vector().host() for f in fcts])
            # dN^T u per point and mode as a stack of (1 x nodes) @ (nodes x 1) products: the operation, term order included, of
            # fem.point_gradient behind DerivativeFunction - the terms are of size |u| / h and cancel, so another order of the sum
            # would differ from the per-sample method by rounding errors of the terms, not of the derivative
            return np.matmul(dN[None, :, :, 0][:, :, None, :], G[:, lay.cells[c]][:, :, :, None])[:, :, 0, 0]
        # anything else: the derivative callables, point by point
        out = np.empty((len(fcts), x.shape[0]))
        for j in range(x.shape[0]):
            for k, f in enumerate(fcts):
                try:
                    out[k, j] = float(fem.DerivativeFunction(f, 0)(x[j]))
                except RuntimeError as e:
                    raise ValueError(str(e)) from e
        return out

    def evaluate_sensor_response_many(self, fixed_dim, free_dim, coords, attri, sensor_points, d_dim=None, gradient=False,
                                      stats=False, device=None, index=None):
        """``evaluate_sensor_response`` for S coordinate sets of the free dimensions at once, with the parameter Jacobian: the
        modes are sampled at the points once (``sensor_modes``), the samples are one product with ``mode_factors_many``.

        Returns a ``SensorManyResult``: ``values`` of shape (S, P) for a scalar field, (S, P, nc) for a vector field, with a
        trailing gdim axis when ``gradient`` (the spatial gradient at the points); ``jacobian``: when ``d_dim`` (a free dimension
        or a list of them) is given, the derivatives of ``values`` with respect to those coordinates on a trailing len(d_dim)
        axis; ``coefficients`` = C (used_numModes, S); with ``stats`` ``min`` / ``max`` / ``max_abs`` of ``values`` per sample.
        The product is numpy below DEVICE_EVAL_MIN_DOFS entries per sample, ``pgd_eval_batch`` on the sampled vectors above.
        ``index``: handed to ``sensor_modes``."""
        coords = self._check_many(fixed_dim, free_dim, coords, attri)
        S, K = coords.shape[0], self.used_numModes
        if self.mesh[free_dim[0]].attributes[attri].interpolationInfo["name"] == 0:
            raise ValueError("evaluate_sensor_response_many: interp1d modes have no mesh to locate points on")
        dims = None if d_dim is None else ([int(d_dim)] if np.isscalar(d_dim) else [int(d) for d in d_dim])
        if dims is not None:
            for d in dims:
                if d == fixed_dim or d not in list(free_dim):
                    raise ValueError("derivation against fixed dim not possible in the moment")
        sm = self.sensor_modes(sensor_points, fixed_dim, attri, gradient=gradient, device=device, index=index)
        C = self.mode_factors_many(free_dim, coords, attri)
        res = SensorManyResult()
        res.coefficients = C
        res.values = sm.contract(C, K).reshape((S,) + sm.shape)
        if dims is not None:
            res.jacobian = np.stack([sm.contract(self.mode_factor_derivatives_many(free_dim, coords, attri, d), K).reshape((S,) + sm.shape)
                                     for d in dims], axis=-1)
        if stats:
            flat = res.values.reshape(S, -1)
            if flat.shape[1]:
                res.min, res.max, res.max_abs = flat.min(axis=1), flat.max(axis=1), np.abs(flat).max(axis=1)
        return res


    # ------------------------------------------------------ Bayesian calibration from sensor data
    def _posterior_samples(self, name, fixed_dim, free_dim, attri, grids, coords, prior, quadrature):
        """The samples of ``sensor_posterior`` / ``sensor_posterior_many`` (``name``: who asks, for the messages): the checked free
        dimensions, K, and per dimension the abscissae, mode tables, normalised weights and quadrature weights; the grid's shape,
        S and the checked scattered coordinates (None on a grid)."""
        free_dim = [int(d) for d in free_dim]
        if (grids is None) == (coords is None):
            raise ValueError("%s: exactly one of grids and coords must be given" % name)
        if quadrature not in ("trapezoid", "none"):
            raise ValueError("%s: quadrature must be 'trapezoid' or 'none', got %r" % (name, quadrature,))
        if fixed_dim in free_dim or len(set(free_dim)) != len(free_dim) or not free_dim:
            raise ValueError("%s: free_dim %s must name distinct dimensions other than the fixed one" % (name, free_dim,))
        for d in free_dim:
            if d < 0 or d >= self.num_pgd_var or attri < 0 or attri >= len(self.mesh[d].attributes):
                raise ValueError("dimension or attribute number not possible")
            if self.mesh[d].attributes[attri].interpolationInfo.get("name") == 0:
                raise ValueError("%s: interp1d modes have no mesh to locate points on" % name)
            if len(self.mesh[d].attributes[attri].interpolationfct) == 0:
                self.create_interpolation_fcts(free_dim, attri)
        K = self.used_numModes
        # ---- the samples: tables of the 1-D modes, weights, abscissae
        prior = dict(prior or {})
        for d in prior:
            if d not in free_dim:
                raise ValueError("%s: the prior names dimension %r, the free dimensions are %s" % (name, d, free_dim))
        if grids is not None:
            if len(grids) != len(free_dim):
                raise ValueError("%s: %d grids for %d free dimensions" % (name, len(grids), len(free_dim)))
            if len(free_dim) > POSTERIOR_MAX_DIMS:
                raise ValueError("%s: %d free dimensions, at most %d are possible" % (name, len(free_dim), POSTERIOR_MAX_DIMS))
            absc, tables, weights, quad = [], [], [], []
            for d, g in zip(free_dim, grids):
                f0 = self.mesh[d].attributes[attri].interpolationfct[0]
                V = f0.function_space() if isinstance(f0, fem.Function) else None
                if V is None or V._ncomp > 1 or V.mesh().topology().dim() != 1:
                    raise NotImplementedError("%s: grids need scalar modes on 1-D free dimensions (dimension %d is not)" % (name, d))
                x = np.asarray(g, dtype=np.float64)
                if x.ndim != 1 or x.size < 1 or not np.all(np.isfinite(x)):
                    raise ValueError("%s: the grid of dimension %d must be a finite 1-D array with at least one point" % (name, d))
                if quadrature == "trapezoid" and np.any(np.diff(x) < 0.0):
                    raise ValueError("%s: the trapezoid rule needs non-decreasing abscissae (dimension %d)" % (name, d))
                q = trapezoid_weights(x) if quadrature == "trapezoid" else np.ones(x.size)
                w = q.copy()
                if d in prior:
                    p = prior[d]
                    p = np.asarray([float(p(v)) for v in x]) if callable(p) else np.asarray(p, dtype=np.float64)
                    if p.shape != x.shape or not np.all(np.isfinite(p)) or p.min() < 0.0:
                        raise ValueError("%s: the prior of dimension %d must be finite and >= 0 at the %d abscissae" % (name, d, x.size))
                    w = w * p
                if not w.sum() > 0.0:
                    raise ValueError("%s: the weights of dimension %d have no positive sum" % (name, d))
                w = w / w.sum()
                absc.append(x)
                quad.append(q)
                weights.append(w)
                tables.append(np.ascontiguousarray(self._free_modes_at(d, x, attri)))
            shape = tuple(x.size for x in absc)
        else:
            if prior:
                raise ValueError("%s: scattered samples are draws from the prior; no prior is taken with coords" % name)
            coords = self._check_many(None, free_dim, coords, attri)
            S = coords.shape[0]
            tables = [np.ascontiguousarray(self.mode_factors_many(free_dim, coords, attri))]
            weights, absc, quad, shape = [np.full(S, 1.0 / S)], None, None, (S,)
        S = int(np.prod(shape, dtype=np.int64))
        if S >= 1 << 31:
            raise ValueError("%s: %d samples, fewer than 2^31 are possible" % (name, S))
        return free_dim, K, absc, tables, weights, quad, shape, S, coords

    @staticmethod
    def _posterior_whitening(name, A, m, sigma, cov):
        """(A whitened, whiten, logdet) for the (m, K) sensor modes ``A`` under the noise ``sigma`` or ``cov``: ``whiten(y)`` does to data
        (m,) or (m, N) what was done to A's rows; logdet = log sqrt det of the covariance."""
        if cov is not None:
            cv = np.asarray(cov, dtype=np.float64)
            if cv.shape != (m, m):
                raise ValueError("%s: cov has shape %s, (%d, %d) is needed" % (name, cv.shape, m, m))
            try:
                L = np.linalg.cholesky(cv)
            except np.linalg.LinAlgError as e:
                raise ValueError("%s: cov is not positive definite" % name) from e
            from scipy.linalg import solve_triangular
            A, whiten = solve_triangular(L, A, lower=True), lambda y: solve_triangular(L, y, lower=True)
            logdet = float(np.sum(np.log(np.diag(L))))
        else:
            sg = np.asarray(sigma, dtype=np.float64)
            if sg.ndim > 0 and sg.size != m:
                raise ValueError("%s: sigma has %d entries, a scalar or %d are needed" % (name, sg.size, m))
            sg = np.broadcast_to(sg.reshape(-1) if sg.ndim else sg, (m,))
            if not np.all(np.isfinite(sg)) or sg.min() <= 0.0:
                raise ValueError("%s: sigma must be finite and > 0" % name)
            A, whiten = A / sg[:, None], lambda y: y / (sg if y.ndim == 1 else sg[:, None])
            logdet = float(np.sum(np.log(sg)))
        return A, whiten, logdet

    def sensor_posterior(self, fixed_dim, free_dim, attri, sensor_points, data, grids=None, coords=None, sigma=1.0, cov=None, prior=None,
                         quadrature="trapezoid", gradient=False, outputs=("marginals", "theta", "coef"), keep_chi2=False, device=None,
                         index=None, reduce=True):
        """The posterior of the free coordinates given ``data`` measured at the sensor points (shaped like one sample of
        ``evaluate_sensor_response_many``, or flat; ``gradient``: the spatial gradients there), under Gaussian noise - a scalar
        ``sigma``, an array of it shaped like ``data``, or a full covariance ``cov`` (m x m) - as a ``PosteriorResult``.

        Exactly one of ``grids`` (one 1-D array of abscissae per free dimension: the tensor grid, last dimension fastest) and
        ``coords`` ((S, len(free_dim)) scattered samples drawn from the prior, weights 1 / S: self-normalised importance sampling,
        no marginals) is given.  ``prior``: None (uniform) or {dimension: callable | array on the grid}, separable, multiplied into
        the quadrature weights of that dimension, which are then normalised to sum 1 (``quadrature``: "trapezoid" on non-decreasing
        abscissae, or "none": unit weights).  On the grid the coefficient of mode k is the product of D' small tables of the 1-D
        modes at the abscissae, the prediction is Phi c(s) with Phi the whitened ``sensor_modes``: the misfits are one product whose
        right-hand factor is never stored (``pgd_grid_misfit``), everything else a reduction over them (``pgd_grid_posterior``).
        More data than modes are first reduced exactly by a thin QR, chi2 = |R c - Q^T y|^2 + |y - Q Q^T y|^2 (``reduce``).  On the
        device when the backend has ``grid_misfit`` and S >= DEVICE_POSTERIOR_MIN_SAMPLES (``device``: force either route),
        otherwise the same arithmetic in numpy.  ``outputs``: any of "marginals", "theta" (mean, cov), "coef" (coef_mean,
        coef_second; at most 64 modes on the device).  ``index``: handed to ``sensor_modes``."""
        unknown = set(outputs) - {"marginals", "theta", "coef"}
        if unknown:
            raise ValueError("sensor_posterior: unknown outputs %s" % sorted(unknown))
        free_dim, K, absc, tables, weights, quad, shape, S, coords = self._posterior_samples("sensor_posterior", fixed_dim, free_dim, attri, grids,
                                                                                              coords, prior, quadrature)
        # ---- the whitened sensor modes and data
        sm = self.sensor_modes(sensor_points, fixed_dim, attri, gradient=gradient, device=None, index=index)
        m = sm.m
        y = np.asarray(data, dtype=np.float64)
        if y.size != m or (y.ndim > 1 and y.shape != sm.shape):
            raise ValueError("sensor_posterior: data has shape %s, the sensors give %s (%d entries)" % (y.shape, sm.shape, m))
        y = y.reshape(-1)
        if not np.all(np.isfinite(y)):
            raise ValueError("sensor_posterior: data holds a value that is not finite")
        A = sm.host()[:K].T                                                  # (m, K)
        A, whiten, logdet = self._posterior_whitening("sensor_posterior", A, m, sigma, cov)
        y = whiten(y)
        rest = 0.0
        if reduce and m > K:
            Q, R = np.linalg.qr(A)                                           # thin: Q (m, K), R (K, K)
            z = Q.T @ y
            r = y - Q @ z
            A, y, rest = R, z, float(r @ r)
        if A.shape[0] > POSTERIOR_MAX_ROWS or K > POSTERIOR_MAX_MODES:
            raise ValueError("sensor_posterior: %d rows and %d modes, at most %d and %d are possible: compress the solution first "
                             "(PGD.compress)" % (A.shape[0], K, POSTERIOR_MAX_ROWS, POSTERIOR_MAX_MODES))
        A, y = np.ascontiguousarray(A), np.ascontiguousarray(y)
        want = (POST_MARGINALS if "marginals" in outputs and grids is not None else 0) | \
               (POST_THETA if "theta" in outputs and grids is not None else 0) | (POST_COEF if "coef" in outputs else 0)
        # ---- the route
        be = fem.get_backend()
        has = hasattr(be, "grid_misfit")
        on_device = (has and S >= DEVICE_POSTERIOR_MIN_SAMPLES) if device is None else bool(device)
        if on_device and not has:
            raise NotImplementedError("sensor_posterior(device=True): the backend %r has no grid_misfit" % (getattr(be, "name", be),))
        if on_device and (want & POST_COEF) and K > POSTERIOR_COEF_MAX_MODES:
            raise ValueError("sensor_posterior: the coefficient moments on the device take at most %d modes, the solution uses %d: "
                             "compress it first (PGD.compress) or leave \"coef\" out of the outputs" % (POSTERIOR_COEF_MAX_MODES, K))
        res = PosteriorResult()
        n = [int(v) for v in shape]
        chi2_host = None
        if on_device:
            h = be.vec_zeros(S)
            keep = DeviceArray(be, h, S, rest)
            cmin, arg = be.grid_misfit(A, y, tables, h)
            sums = be.grid_posterior(h, cmin, n, weights, tables=tables, abscissae=absc, want=want)
            fem.STATS["posterior_calls"] = fem.STATS.get("posterior_calls", 0) + 1
            res.path = "device"
            if keep_chi2:
                res.chi2 = keep
            if grids is None and "theta" in outputs:
                chi2_host = be.vec_to_host(h)
        else:
            chi2_host, cmin, arg = grid_misfit_numpy(A, y, tables)
            sums = grid_posterior_numpy(chi2_host, cmin, n, weights, tables=tables, abscissae=absc, want=want)
            res.path = "numpy"
            if keep_chi2:
                res.chi2 = (chi2_host + rest).reshape(shape)
        Z = sums["Z"]
        if not (Z > 0.0 and np.isfinite(Z)):
            raise ValueError("sensor_posterior: the posterior has no mass on the samples (Z = %r)" % (Z,))
        res.Z, res.shift = Z, cmin
        res.chi2_min = cmin + rest
        res.free_dim, res.grids, res.weights = list(free_dim), absc, weights
        if grids is not None:
            res.map_index = tuple(int(i) for i in np.unravel_index(arg, shape))
            res.map_coords = np.array([absc[j][i] for j, i in enumerate(res.map_index)])
        else:
            res.map_index, res.map_coords = int(arg), coords[arg].copy()
        res.log_evidence = math.log(Z) - 0.5 * (cmin + rest) - 0.5 * m * math.log(2.0 * math.pi) - logdet
        res.ess = Z * Z / sums["sum_e2"]
        if want & POST_MARGINALS:
            res.marginals = [mg / Z for mg in sums["marginals"]]
            res.densities = [np.where(q > 0.0, mg / np.where(q > 0.0, q, 1.0), 0.0) for mg, q in zip(res.marginals, quad)]
        if want & POST_THETA:
            res.mean = sums["theta1"] / Z
            res.cov = sums["theta2"] / Z - np.outer(res.mean, res.mean)
        elif grids is None and "theta" in outputs:
            e = np.exp(-0.5 * (chi2_host - cmin)) / S
            th = coords.reshape(S, -1)
            res.mean = (e @ th) / Z
            res.cov = (th.T * e) @ th / Z - np.outer(res.mean, res.mean)
        if want & POST_COEF:
            res.coef_mean, res.coef_second = sums["coef1"] / Z, sums["coef2"] / Z
        return res

    def sensor_posterior_many(self, fixed_dim, free_dim, attri, sensor_points, data, grids=None, coords=None, sigma=1.0, cov=None,
                              prior=None, quadrature="trapezoid", gradient=False, outputs=("theta",), accumulate=False, device=None,
                              index=None, reduce=True, data_chunk=None):
        """The posteriors of ``sensor_posterior`` for a stream of N data sets from the same sensors under the same noise, in one
        pass over the grid - a ``PosteriorManyResult``.  ``data``: (N, *shape of one sample) or (N, m); samples, noise, ``prior``,
        ``quadrature`` and the thin QR (``reduce``; it reduces all N data vectors at once) are ``sensor_posterior``'s.
        ``accumulate``: the posterior of step n is that of ALL data up to n (independent measurements of the same state).
        ``outputs``: () or ("theta",) (mean, cov); marginals and coefficient moments of a step of interest: ``sensor_posterior``.

        The predictions p_s = A c(s) do not depend on the data: the misfits of all data sets are chi2[n, s] = beta_n - 2 u_n . p_s +
        alpha_n |p_s|^2 with (u, alpha, beta) = (y_n, 1, |y_n|^2), or their prefix sums with ``accumulate`` - one more dense product
        behind the one that forms p, reduced where it is formed (``pgd_grid_posterior_many``).  On the device when the backend has
        ``grid_posterior_many`` and N S >= DEVICE_POSTERIOR_MANY_MIN_WORK (``device``: force either route), otherwise the same
        arithmetic in numpy; ``data_chunk`` data sets per call (default: what keeps the scratch of a call under 256 MB).  The
        expanded form cancels where the misfit is small against |y|^2: ``chi2_min`` is therefore recomputed in the difference form at
        the MAP sample, ``shift`` is the kernel's own minimum.  At most 64 modes and 64 rows (after the QR)."""
        name = "sensor_posterior_many"
        if coords is not None:
            raise NotImplementedError("sensor_posterior_many: scattered samples (coords) are not taken; sensor_posterior takes them, one data "
                                      "set at a time")
        unknown = set(outputs) - {"theta"}
        if unknown:
            raise ValueError("sensor_posterior_many: unknown outputs %s (\"theta\" is the only one; sensor_posterior gives marginals and "
                             "coefficient moments)" % sorted(unknown))
        free_dim, K, absc, tables, weights, quad, shape, S, _ = self._posterior_samples(name, fixed_dim, free_dim, attri, grids, None, prior,
                                                                                         quadrature)
        D = len(free_dim)
        # ---- the whitened sensor modes and data
        sm = self.sensor_modes(sensor_points, fixed_dim, attri, gradient=gradient, device=None, index=index)
        m = sm.m
        Y = np.asarray(data, dtype=np.float64)
        if Y.ndim < 2 or Y.shape[0] < 1 or (Y.shape[1:] != (m,) and Y.shape[1:] != tuple(sm.shape)):
            raise ValueError("sensor_posterior_many: data has shape %s, (N, %d) or (N,) + %s is needed" % (Y.shape, m, tuple(sm.shape)))
        N = Y.shape[0]
        Y = Y.reshape(N, m)
        if not np.all(np.isfinite(Y)):
            raise ValueError("sensor_posterior_many: data holds a value that is not finite")
        A = sm.host()[:K].T                                                  # (m, K)
        A, whiten, logdet = self._posterior_whitening(name, A, m, sigma, cov)
        Y = np.ascontiguousarray(whiten(Y.T).T)                              # (N, m), whitened
        rest = np.zeros(N)
        if reduce and m > K:
            Q, R = np.linalg.qr(A)                                           # thin: Q (m, K), R (K, K)
            Z = Y @ Q
            r = Y - Z @ Q.T
            A, Y, rest = R, Z, np.einsum("np,np->n", r, r)
        rows = A.shape[0]
        if rows > POSTERIOR_MANY_MAX_ROWS or K > POSTERIOR_MANY_MAX_MODES:
            raise ValueError("sensor_posterior_many: %d rows and %d modes, at most %d and %d are possible: compress the solution first "
                             "(PGD.compress)" % (rows, K, POSTERIOR_MANY_MAX_ROWS, POSTERIOR_MANY_MAX_MODES))
        A, Y = np.ascontiguousarray(A), np.ascontiguousarray(Y)
        y2 = np.einsum("np,np->n", Y, Y)
        steps = np.arange(1, N + 1, dtype=np.float64)
        if accumulate:
            u, alpha, beta, rest = np.cumsum(Y, axis=0), steps, np.cumsum(y2), np.cumsum(rest)
        else:
            u, alpha, beta = Y, np.ones(N), y2
        want = POST_THETA if "theta" in outputs else 0
        # ---- the route
        be = fem.get_backend()
        has = hasattr(be, "grid_posterior_many")
        on_device = (has and N * S >= DEVICE_POSTERIOR_MANY_MIN_WORK) if device is None else bool(device)
        if on_device and not has:
            raise NotImplementedError("sensor_posterior_many(device=True): the backend %r has no grid_posterior_many" % (getattr(be, "name", be),))
        if data_chunk is None:
            nseg, _ = posterior_many_segments(S)
            nvs = (D + 1) * (D + 2) // 2 + 1
            data_chunk = max(POSTERIOR_MANY_PARTIALS // (nseg * nvs), 1) if on_device else max((1 << 22) // min(S, 1 << 12), 1)
        data_chunk = int(data_chunk)
        if data_chunk < 1:
            raise ValueError("sensor_posterior_many: data_chunk = %d, at least 1 is needed" % data_chunk)
        parts = []
        for n0 in range(0, N, data_chunk):
            sl = slice(n0, min(N, n0 + data_chunk))
            if on_device:
                parts.append(be.grid_posterior_many(A, u[sl], alpha[sl], beta[sl], tables, weights, abscissae=absc, want=want))
                fem.STATS["posterior_many_calls"] = fem.STATS.get("posterior_many_calls", 0) + 1
            else:
                parts.append(grid_posterior_many_numpy(A, u[sl], alpha[sl], beta[sl], tables, weights, abscissae=absc, want=want))
        sums = {key: np.concatenate([p[key] for p in parts]) for key in parts[0]}
        Zs = sums["Z"]
        if not np.all((Zs > 0.0) & np.isfinite(Zs)):
            bad = int(np.flatnonzero(~((Zs > 0.0) & np.isfinite(Zs)))[0])
            raise ValueError("sensor_posterior_many: the posterior of data set %d has no mass on the samples (Z = %r)" % (bad, Zs[bad]))
        res = PosteriorManyResult()
        res.path = "device" if on_device else "numpy"
        res.Z, res.shift = Zs, sums["chi2_min"]
        res.free_dim, res.grids, res.weights = list(free_dim), absc, weights
        arg = sums["argmin"]
        res.map_index = np.stack(np.unravel_index(arg, shape), axis=1)
        res.map_coords = np.stack([absc[d][res.map_index[:, d]] for d in range(D)], axis=1)
        # ---- the misfit at the MAP sample in the difference form: alpha |p - u / alpha|^2 + the scatter of the data about their mean
        Cm = np.ones((K, N))
        for d, t in enumerate(tables):
            Cm *= t[:, res.map_index[:, d]]
        Pm = (A @ Cm).T                                                      # (N, rows): the predictions at the N MAP samples
        ubar = u / alpha[:, None]
        scatter = np.zeros(N)
        if accumulate and N > 1:                                             # Welford: sum_{i <= n} |y_i - mean_n|^2
            scatter[1:] = np.cumsum(np.einsum("np,np->n", Y[1:] - ubar[:-1], Y[1:] - ubar[1:]))
        dlt = Pm - ubar
        res.chi2_min = alpha * np.einsum("np,np->n", dlt, dlt) + scatter + rest
        m_eff = m * alpha
        res.log_evidence = np.log(Zs) - 0.5 * (res.shift + rest) - 0.5 * m_eff * math.log(2.0 * math.pi) - alpha * logdet
        res.ess = Zs * Zs / sums["sum_e2"]
        if want & POST_THETA:
            res.mean = sums["theta1"] / Zs[:, None]
            res.cov = sums["theta2"] / Zs[:, None, None] - res.mean[:, :, None] * res.mean[:, None, :]
        return res

    def sensor_placement(self, fixed_dim, free_dim, attri, candidate_points, n_select, grids=None, coords=None, sigma=1.0, prior=None,
                         prior_precision=None, quadrature="trapezoid", gradient=False, group="point", installed=None, exclude=None,
                         keep_gains=False, device=None, index=None):
        """Of the M places where a sensor could be mounted, the ``n_select`` that make the posterior of the free coordinates narrowest,
        chosen greedily by the expected information gain in the linearised (Laplace) form - Bayesian D-optimality - before any data
        exists: a ``PlacementResult``.

        Samples, ``prior`` and ``quadrature`` are ``sensor_posterior``'s on ``grids`` (scattered ``coords`` are refused); the noise is
        independent, ``sigma`` a scalar or an array shaped like one sample's data (no ``cov``: rank-one gains need independent noise).
        ``group``: "point" - a sensor is everything measured at a point, R = prod(shape[1:]) rows - or "entry": every scalar entry is
        its own candidate, R = 1.  With the parameter Jacobian g_p(s) of row p at sample s (the whitened ``sensor_modes`` against the
        derivative coefficients of ``mode_factor_derivatives_many``) and H_s = prior_precision + sum of g g^T over the rows chosen so
        far, the utility is 1/2 sum_s w_s [log det H_s - log det prior_precision], and a candidate's marginal gain
        1/2 sum_s w_s log det(I + V^T V), V = W_s [g ..], W_s the inverse Cholesky factor of H_s.  ``prior_precision``: a symmetric
        positive definite D x D matrix, or None: diag(1 / var_d) of each dimension's normalised weights over its abscissae.
        ``installed``: candidates applied first, in order (their gains in ``installed_gains``); ``exclude``: never chosen; a chosen
        candidate is not offered again; ties go to the lowest index.

        On the device (``pgd_design_update`` / ``pgd_design_gains``: the M x S x R x D Jacobian is never stored) when the backend has
        ``design_gains``, at most 64 modes, R <= 3 and M S >= DEVICE_PLACEMENT_MIN_WORK (``device``: force either route), otherwise the
        same arithmetic in numpy, in chunks of samples.  ``index``: handed to ``sensor_modes``."""
        name = "sensor_placement"
        if coords is not None:
            raise ValueError("sensor_placement: scattered samples (coords) are not taken, only grids")
        if group not in ("point", "entry"):
            raise ValueError("sensor_placement: group must be 'point' or 'entry', got %r" % (group,))
        free_dim, K, absc, tables, weights, quad, shape, S, _ = self._posterior_samples(name, fixed_dim, free_dim, attri, grids, None, prior,
                                                                                         quadrature)
        D = len(free_dim)
        dtables = [np.ascontiguousarray(self._free_mode_derivatives_at(d, x, attri)) for d, x in zip(free_dim, absc)]
        # ---- the whitened sensor modes of the candidates
        points = np.asarray(candidate_points, dtype=np.float64)
        sm = self.sensor_modes(candidate_points, fixed_dim, attri, gradient=gradient, device=None, index=index)
        m = sm.m
        A = sm.host()[:K].T                                                  # (m, K), rows in the order (point, component[, axis])
        A, _, _ = self._posterior_whitening(name, A, m, sigma, None)
        A = np.ascontiguousarray(A)
        per_point = int(np.prod(sm.shape[1:], dtype=np.int64))
        R = per_point if group == "point" else 1
        M = m // R
        # ---- the prior precision
        if prior_precision is None:
            var = np.array([float(w @ (x * x) - (w @ x) ** 2) for w, x in zip(weights, absc)])
            if not np.all(var > 0.0):
                raise ValueError("sensor_placement: dimension %d has zero variance under its weights; give prior_precision"
                                 % free_dim[int(np.argmin(var > 0.0))])
            H0 = np.diag(1.0 / var)
        else:
            H0 = np.array(prior_precision, dtype=np.float64)
            ok = H0.shape == (D, D) and np.all(np.isfinite(H0)) and np.array_equal(H0, H0.T)
            if ok:
                try:
                    np.linalg.cholesky(H0)
                except np.linalg.LinAlgError:
                    ok = False
            if not ok:
                raise ValueError("sensor_placement: prior_precision must be a symmetric positive definite %d x %d matrix" % (D, D))
        H0 = np.ascontiguousarray(H0)
        # ---- what is on offer
        def indices(what, v):
            v = np.asarray([] if v is None else v, dtype=np.int64).reshape(-1)
            if v.size and (v.min() < 0 or v.max() >= M):
                raise ValueError("sensor_placement: %s names candidate %d, there are %d" % (what, int(v[(v < 0) | (v >= M)][0]), M))
            return [int(j) for j in v]
        installed, exclude = indices("installed", installed), indices("exclude", exclude)
        n_select = int(n_select)
        taken = np.zeros(M, dtype=bool)
        taken[installed] = True
        taken[exclude] = True
        if n_select < 0 or n_select > M - int(taken.sum()):
            raise ValueError("sensor_placement: n_select = %d, %d candidates are on offer" % (n_select, M - int(taken.sum())))
        # ---- the route
        be = fem.get_backend()
        has = hasattr(be, "design_gains")
        fits = K <= PLACEMENT_MAX_MODES and R <= PLACEMENT_MAX_ROWS
        on_device = (has and fits and M * S >= DEVICE_PLACEMENT_MIN_WORK) if device is None else bool(device)
        if on_device and not fits:
            raise ValueError("sensor_placement(device=True): %d modes and %d rows per candidate, the device takes at most %d and %d: "
                             "compress the solution first (PGD.compress), or make every entry a candidate (group=\"entry\")"
                             % (K, R, PLACEMENT_MAX_MODES, PLACEMENT_MAX_ROWS))
        if on_device and not has:
            raise NotImplementedError("sensor_placement(device=True): the backend %r has no design_gains" % (getattr(be, "name", be),))
        n = [int(v) for v in shape]
        if on_device:
            state = be.design_state(n)
            update = lambda **kw: be.design_update(state, tables, dtables, weights, **kw)
            gains_of = lambda a: be.design_gains(a, R, state, tables, dtables, weights)
            fem.STATS["placement_calls"] = fem.STATS.get("placement_calls", 0) + 1
        else:
            state = design_state_numpy(n)
            update = lambda **kw: design_update_numpy(state, tables, dtables, weights, **kw)
            gains_of = lambda a: design_gains_numpy(a, R, state, tables, dtables, weights)
        rows_of = lambda j: A[j * R:(j + 1) * R]
        res = PlacementResult()
        res.path, res.prior_precision = "device" if on_device else "numpy", H0
        try:
            logdet0, cov = update(h0=H0)
            logdets, covs = [logdet0], []
            res.installed_gains = np.zeros(len(installed))
            for i, j in enumerate(installed):
                res.installed_gains[i] = gains_of(rows_of(j))[0]
                ld, cov = update(rows=rows_of(j))
                logdets.append(ld)
            covs.append(cov)
            res.selected, res.gains = np.zeros(n_select, dtype=np.int64), np.zeros(n_select)
            res.gain_history = np.zeros((n_select, M)) if keep_gains else None
            for step in range(n_select):
                g = gains_of(A)
                if step == 0:
                    res.first_gains = g.copy()
                if keep_gains:
                    res.gain_history[step] = g
                j = int(np.argmax(np.where(taken, -np.inf, g)))              # (argmax: the lowest index among equal gains)
                taken[j] = True
                res.selected[step], res.gains[step] = j, g[j]
                ld, cov = update(rows=rows_of(j))
                logdets.append(ld)
                covs.append(cov)
        finally:
            if on_device:
                be.vec_free(state)
        if res.first_gains is None:
            res.first_gains = np.zeros(0)
        res.utility = 0.5 * (np.array(logdets) - logdets[0])
        res.expected_cov = np.stack(covs)
        pts = points.reshape(sm.shape[0], -1) if points.size else points
        res.selected_points = pts[res.selected if group == "point" else res.selected // per_point]
        return res

    def posterior_predictive(self, res, fixed_dim, attri):
        """(mean, variance): the posterior predictive mean and variance Functions on the fixed space from a ``PosteriorResult`` with
        the "coef" output: F E[c] through ``eval_batch`` and f_i^T (E[c c^T] - E[c] E[c]^T) f_i through ``quadratic_forms``
        (clamped at 0), both under the rule of ``evaluate_many``."""
        if res.coef_mean is None or res.coef_second is None:
            raise ValueError("posterior_predictive: the result holds no coefficient moments (outputs must name \"coef\")")
        modes, V = self._gram_family(fixed_dim, attri)
        mbar = np.asarray(res.coef_mean, dtype=np.float64)
        if mbar.shape != (len(modes),):
            raise ValueError("posterior_predictive: %d coefficient moments for %d modes" % (mbar.size, len(modes)))
        mean = self._combine_modes(V, modes, mbar.reshape(-1, 1))[0]
        funcs, _, _ = self.quadratic_forms(fixed_dim, res.coef_second - np.outer(mbar, mbar), attri, clamp=True)
        return mean, funcs[0]


class PGDErrorComputation(object):
    def __init__(self, fixed_dim=0, n_samples=1, data_test=[], FOM_model=[], PGD_model=[], lim_samples=[],
                 fixed_var=[], *args, **kwargs):
        self.logger = logging.getLogger(__name__ + "." + self.__class__.__name__)
        self.fixed_dim = fixed_dim
        self.n_smp = n_samples
        self.data_test = data_test
        self.FOM_sol = FOM_model
        self.PGD_sol = PGD_model
        self.lim_smp = lim_samples
        self.fixed_var = fixed_var
        self.free_dim = [d for d in range(self.PGD_sol.num_pgd_var) if d not in fixed_dim]

    def sampling_LHS(self):
        """Latin-hypercube samples of the free coordinates, scaled to their ranges (seed 3452)."""
        sample = qmc.LatinHypercube(d=len(self.free_dim), seed=3452).random(n=self.n_smp)
        lo, hi = [], []
        for d in self.free_dim:
            if not self.lim_smp:
                X = self.PGD_sol.problem.meshes[d].coordinates()
                if len(X[0]) == 1:
                    lo.append(float(np.min(X)))
                    hi.append(float(np.max(X)))
                else:
                    print("Not implemented")
            elif len(self.lim_smp[d]) == 2:
                lo.append(float(min(self.lim_smp[d])))
                hi.append(float(max(self.lim_smp[d])))
            else:
                print("Not implemented")
        return qmc.scale(sample, lo, hi).tolist()

    def compute_SampleError(self, u_FOM, u_PGD):
        """|u_PGD - u_FOM|_2 / |u_FOM|_2 for arrays, vertex values or two Functions."""
        if isinstance(u_FOM, np.ndarray):
            pgd = u_PGD.reshape(-1) if isinstance(u_PGD, np.ndarray) else u_PGD.compute_vertex_values()[:]
            return np.linalg.norm(pgd - u_FOM.reshape(-1), 2) / np.linalg.norm(u_FOM.reshape(-1), 2)
        diff = u_FOM.vector().copy()
        diff.axpy(-1.0, u_PGD.vector())
        return diff.norm("l2") / u_FOM.vector().norm("l2")

    def evaluate_error(self):
        if not self.data_test:
            self.data_test = self.sampling_LHS()
        errorL2 = np.zeros(len(self.data_test))
        for i, smp in enumerate(self.data_test):
            if not self.FOM_sol:
                self.logger.error("FEM not defined")
                raise ValueError("FEM not defined")
            u_fem = self.FOM_sol(smp)
            if isinstance(u_fem, float):
                u_fem = np.array(u_fem)
            if not self.PGD_sol:
                self.logger.error("PGD model not defined")
                raise ValueError("PGD model not defined")
            u_pgd = self.PGD_sol.evaluate(int(self.fixed_dim[0]), self.free_dim, smp, 0)
            if not self.fixed_var:
                errorL2[i] = self.compute_SampleError(u_fem, u_pgd)
            else:
                errorL2[i] = self.compute_SampleError(u_fem, np.array([u_pgd(x) for x in self.fixed_var]))
        return errorL2, np.mean(errorL2), np.max(errorL2)
