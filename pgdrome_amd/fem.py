"""Host-side form frontend: the subset of the dolfin/UFL surface that PGDrome's
weak-form callbacks and ``PGDProblem`` use, captured
as *operator atoms* and executed by the HIP engine through the C-ABI.

The reference callbacks build every form from one rigid grammar
(/root/reference/tests/integration/test_heat1D.py:55-266,
test_laplace.py:73-366):

    Constant(assemble(F*A*G*dx(m_j)) * ...) * param * u[.dx(0)] * v[.dx(0)] * dx(m_d)

so an integrand is a sum of monomials  coef * prod(factors)  with factors
``field`` or ``field.dx(i)`` (or ``inner(grad f, grad g)``), fields being the
trial / test function or coefficient Functions.  Each monomial maps onto one
P1 atom (mass, stiffness, directional derivative, convection, weighted mass)
that is assembled ONCE per mesh on the GPU and cached; a bilinear form is then
``sum_t c_t A_t`` (one k_combine launch), a linear form ``sum_s c_s A_s g_s``
(SpMV + axpy) and a functional ``f^T A g`` (fused SpMV-dot).

Numbering: device vectors are kept in mesh-vertex order.  ``Function.vector()``
exposes dof order; as in serial dolfin 2019.1.0 the P1 dofs of an IntervalMesh
run opposite to the vertices (pinned by /root/reference/tests/unit/test_FD.py:69,
76-79), for 2-D/3-D meshes dof == vertex (dolfin's reordering there is not
pinned by anything in the reference tree; compare in vertex order).

There is no CPU implementation in this package: the default backend is the HIP
library and creating it without a GPU raises.  Tests inject the oracle backend
explicitly with ``set_backend``.
"""
from __future__ import annotations

import collections
import contextlib
import functools
import hashlib
import itertools
import logging
import math
import numbers
import os
import sys
import time
import weakref

import numpy as np

LOG = logging.getLogger("pgdrome_amd.fem")

MASS, STIFF, DUDV, CONV, CONVT, WMASS, WSTIFF = range(7)   # == include/pgd_amd.h PGD_ATOM_*
WDUDV, WCONV, WCONVT = 7, 8, 9                             # int w u_{,da} v_{,db}, int w u_{,da} v, int w u v_{,db}
# kinds whose (da, db) matter: the trial derivative da, the test derivative db
_DA_KINDS, _DB_KINDS = (DUDV, CONV, WDUDV, WCONV), (DUDV, CONVT, WDUDV, WCONVT)
DS_MASS = "ds_mass"          # int_Gamma phi_i phi_j ds over a facet set (pgd_atom_assemble_facets): the atom of a Robin term

# --------------------------------------------------------------------------- backend
_backend = None


def set_backend(be):
    """Install a backend object (see hip_backend.HipBackend for the interface)."""
    global _backend
    _backend = be
    _FAST_PLANS.clear()          # (plans name atoms of the backend they were made under)
    return be


def get_backend():
    global _backend
    if _backend is None:
        from .hip_backend import HipBackend   # raises without the HIP library or a GPU
        _backend = HipBackend()
    return _backend


# ------------------------------------------------------------------- logging shims
class LogLevel:
    DEBUG, TRACE, PROGRESS, INFO, WARNING, ERROR, CRITICAL = 10, 13, 16, 20, 30, 40, 50


def set_log_level(level):
    LOG.setLevel(level)


parameters = {"form_compiler": {"optimize": True, "cpp_optimize": True, "quadrature_degree": -1},
              "linear_algebra_backend": "pgd_amd"}

DOLFIN_EPS = 3.0e-16


def near(x, x0, eps=DOLFIN_EPS):
    return abs(x - x0) < eps


class Point:
    def __init__(self, *xs):
        if len(xs) == 1 and hasattr(xs[0], "__len__"):
            xs = tuple(xs[0])
        self._x = tuple(float(v) for v in xs)

    def __getitem__(self, i):
        return self._x[i]

    def __len__(self):
        return len(self._x)

    def x(self):
        return self._x[0]

    def y(self):
        return self._x[1] if len(self._x) > 1 else 0.0

    def z(self):
        return self._x[2] if len(self._x) > 2 else 0.0

    def array(self):
        return np.array(self._x + (0.0,) * (3 - len(self._x)))


# ---------------------------------------------------------------------------- meshes
class _Topology:
    def __init__(self, d):
        self._d = d

    def dim(self):
        return self._d


class _Geometry(_Topology):
    pass


class Partition:
    """Row-sharding of a mesh across ranks (pgdrome_amd/dist.py).  The local mesh
    holds the owned vertices [own0, own1) plus one layer of ghost vertices on
    either side; all local vectors have the extended length."""

    def __init__(self, comm, own0, own1, n_global, lo_ghost, hi_ghost, global_offset):
        self.comm = comm
        self.own0, self.own1 = own0, own1
        self.n_global = n_global
        self.lo_ghost, self.hi_ghost = lo_ghost, hi_ghost   # ghost counts before / after
        self.global_offset = global_offset                    # global id of local vertex 0
        # what this rank SENDS down / up - the neighbour's ghost counts.  Equal to its own ghost counts on P1 slabs; a P2 layout
        # (below) receives a whole plane block from below and sends one up, but only vertices + in-plane edge nodes the other way
        self.send_lo, self.send_hi = lo_ghost, hi_ghost

    @property
    def symmetric(self):
        return self.send_lo == self.lo_ghost and self.send_hi == self.hi_ghost


class Mesh:
    _CELL_NAMES = {1: "interval", 2: "triangle", 3: "tetrahedron"}

    def __init__(self, coords=None, cells=None, part=None):
        # ``Mesh()`` is the empty mesh dolfin lets ``HDF5File.read(mesh, name, False)`` fill (model.py:455-458)
        self.part = part
        self._set_geometry(np.zeros((0, 1)) if coords is None else coords,
                           np.zeros((0, 2), dtype=np.int32) if cells is None else cells)

    def _set_geometry(self, coords, cells):
        coords = np.ascontiguousarray(coords, dtype=np.float64)
        if coords.ndim == 1:
            coords = coords.reshape(-1, 1)
        self._coords = coords
        self._cells = np.ascontiguousarray(cells, dtype=np.int32)
        self._gdim = coords.shape[1]
        self._layouts = {}       # degree -> DofLayout
        self._on_boundary = None
        self._facets = None

    def coordinates(self):
        return self._coords

    def cells(self):
        return self._cells

    def num_vertices(self):
        return self._coords.shape[0]

    def num_cells(self):
        return self._cells.shape[0]

    def topology(self):
        return _Topology(self._gdim)

    def geometry(self):
        return _Geometry(self._gdim)

    def ufl_cell(self):
        return self._CELL_NAMES[self._gdim]

    def hmin(self):
        X = self._coords[self._cells]
        return float(np.linalg.norm(X[:, 1:] - X[:, :1], axis=2).min())

    # rows a rank owns (whole mesh when not sharded)
    def owned_range(self):
        return (self.part.own0, self.part.own1) if self.part else (0, self.num_vertices())

    def layout(self, degree=1):
        """Degrees of freedom of the Lagrange space of this degree on the mesh (created once)."""
        lay = self._layouts.get(degree)
        if lay is None:
            lay = DofLayout(self, degree)
            self._layouts[degree] = lay
        return lay

    def handle(self):
        return self.layout(1).handle()

    def atom(self, kind, da=0, db=0, weight=None):
        return self.layout(1).atom(kind, da, db, weight)

    def facets(self):
        """(facet -> sorted vertices, exterior flag): the codimension-1 entities, numbered by sorted vertex
        tuple (in 2-D the same numbering as the edge nodes of the P2 layout)."""
        if getattr(self, "_facets", None) is None:
            c = self._cells.astype(np.int64)
            nv, k = self.num_vertices(), c.shape[1]
            if self._gdim == 1:
                cnt = np.bincount(c.ravel(), minlength=nv)
                self._facets = (np.arange(nv, dtype=np.int64).reshape(-1, 1), cnt == 1)
            else:
                loc = np.concatenate([np.sort(np.delete(c, j, axis=1), axis=1) for j in range(k)], axis=0)
                key = loc[:, 0]
                for j in range(1, k - 1):
                    key = key * nv + loc[:, j]
                uk, idx, cnt = np.unique(key, return_index=True, return_counts=True)
                ext = cnt == 1
                test = getattr(self, "_hull_test", None)
                if self.part is not None and test is not None and ext.any():
                    # a slab's cut planes are facets of one cell too: exterior is what lies on the hull of the WHOLE mesh (builder's test)
                    fv = loc[idx]
                    ext = ext & test(self._coords[fv].mean(axis=1))
                self._facets = (loc[idx], ext)
        return self._facets

    def num_facets(self):
        return self.facets()[0].shape[0]

    def vertex_on_boundary(self):
        """Vertices on exterior facets (facets that belong to exactly one cell)."""
        if self._on_boundary is None:
            nv = self.num_vertices()
            flag = np.zeros(nv, dtype=bool)
            c = self._cells
            if self._gdim == 1:
                cnt = np.bincount(c.ravel(), minlength=nv)
                flag = cnt == 1
            else:
                k = c.shape[1]
                facets = np.concatenate([np.delete(c, j, axis=1) for j in range(k)], axis=0)
                facets = np.sort(facets, axis=1)
                uniq, counts = np.unique(facets, axis=0, return_counts=True)
                flag[uniq[counts == 1].ravel()] = True
            if self.part is not None:
                raise RuntimeError("a sharded mesh must be given its hull mask by its builder")
            self._on_boundary = flag
        return self._on_boundary


class DofLayout:
    """The degrees of freedom of a Lagrange space as the device sees them: node coordinates, cell -> node
    connectivity (uploaded as a "dof mesh"), and the cache of assembled atoms.

    degree 1: nodes = mesh vertices.  degree 2 on intervals: nodes ordered along the interval, vertex i ->
    node 2 i, midpoint of cell i -> node 2 i + 1, cell record (v0, v1, mid).  degree 2 on triangles /
    tetrahedra: the vertices keep their numbers, one node per edge follows (edges numbered by sorted vertex
    pair), cell record (vertices, edge nodes in the UFC local edge order)."""

    P2_EDGES = {2: ((1, 2), (0, 2), (0, 1)), 3: ((2, 3), (1, 3), (1, 2), (0, 3), (0, 2), (0, 1))}

    def __init__(self, mesh, degree):
        self.mesh, self.degree = mesh, int(degree)
        if self.degree == 1:
            self.coords, self.cells = mesh.coordinates(), mesh.cells()
            self.vertex_nodes = None
        elif self.degree == 2 and mesh.topology().dim() == 1:
            if mesh.part is not None:
                raise NotImplementedError("P2 on a sharded mesh")
            X, C = mesh.coordinates()[:, 0], mesh.cells()
            if not (np.all(np.diff(X) > 0) and np.array_equal(C[:, 0] + 1, C[:, 1])):
                raise NotImplementedError("P2 needs an interval mesh with vertices in increasing order")
            nv = X.size
            nodes = np.empty(2 * nv - 1)
            nodes[0::2] = X
            nodes[1::2] = 0.5 * (X[:-1] + X[1:])
            self.coords = nodes.reshape(-1, 1)
            self.cells = np.stack([2 * C[:, 0], 2 * C[:, 1], 2 * C[:, 0] + 1], axis=1).astype(np.int32)
            self.vertex_nodes = np.arange(0, 2 * nv - 1, 2)
            self.edge_nodes = np.arange(1, 2 * nv - 1, 2)
            self.edge_vertices = np.stack([self.vertex_nodes[:-1], self.vertex_nodes[1:]], axis=1)
        elif self.degree == 2 and mesh.topology().dim() == 3 and mesh.part is not None:
            self._init_p2_slab(mesh)
        elif self.degree == 2 and mesh.topology().dim() in (2, 3):
            if mesh.part is not None:
                raise NotImplementedError("P2 on a sharded 2-D mesh")
            X, C = mesh.coordinates(), mesh.cells()
            nv, loc = X.shape[0], self.P2_EDGES[mesh.topology().dim()]
            pairs = np.concatenate([np.sort(C[:, list(e)], axis=1) for e in loc], axis=0).astype(np.int64)
            keys, inv = np.unique(pairs[:, 0] * nv + pairs[:, 1], return_inverse=True)
            ev = np.stack([keys // nv, keys % nv], axis=1)
            self.coords = np.concatenate([X, 0.5 * (X[ev[:, 0]] + X[ev[:, 1]])], axis=0)
            self.cells = np.concatenate([C, nv + inv.reshape(len(loc), C.shape[0]).T], axis=1).astype(np.int32)
            self.vertex_nodes = np.arange(nv)
            self.edge_nodes = nv + np.arange(ev.shape[0])
            self.edge_vertices = ev
        else:
            raise NotImplementedError("Lagrange degree %d on %s cells: P1 everywhere, P2 on intervals "
                                      "/ triangles / tetrahedra (SURVEY 8(f4))" % (self.degree, mesh.ufl_cell()))
        self.n = self.coords.shape[0]
        self._handles, self._atoms, self._atom_weights = {}, {}, {}
        self._p2_bound = weakref.WeakKeyDictionary()     # backend -> has it bound this layout to its vertex lattice (bind_p2_lattice)
        self._facet_atoms = {}
        self._cell_atoms = {}        # cell-subdomain atoms: _atom_key + (cell-set key,) -> (atom, weakref to the MeshFunction, to the weight)
        self._cw_atoms = {}          # cell-weighted atoms: _atom_key + (cell-set key | None, (id, version) of the DG0 field's vector) ->
        #                              (atom, weakref to the field's vector, to the MeshFunction, to the nodal weight)
        self._ones = self._space = None

    def _init_p2_slab(self, mesh):
        """P2 on a z-slab of a box mesh (r04): the nodes are numbered PLANE BY PLANE - block z = [vertices of plane z | nodes of the
        edges inside plane z | nodes of the edges from plane z up to plane z + 1] - so that what a neighbour needs is a contiguous
        range: the rank below sends its last block up (this rank's ghost nodes below: a whole block), the rank above sends the
        vertices and in-plane edge nodes of its first plane down (ghost nodes above; the edges from there upwards touch no cell of
        this slab).  The send sizes therefore differ from the ghost sizes (`Partition.send_lo / send_hi`): such a partition is
        solved by the loops driven from Python (pgdrome_amd/dist.py), whose exchanges take the sizes per direction."""
        mp = mesh.part
        plane = int(getattr(mp, "plane", 0) or 0)
        X, C = mesh.coordinates(), mesh.cells()
        nv = X.shape[0]
        if plane <= 0 or nv % plane:
            raise NotImplementedError("P2 on a sharded mesh needs the slab's plane size (pgdrome_amd.dist.sharded_box_mesh)")
        nzl, loc = nv // plane, self.P2_EDGES[3]
        pairs = np.concatenate([np.sort(C[:, list(e)], axis=1) for e in loc], axis=0).astype(np.int64)
        keys, inv = np.unique(pairs[:, 0] * nv + pairs[:, 1], return_inverse=True)
        ev = np.stack([keys // nv, keys % nv], axis=1)
        za, zb = ev[:, 0] // plane, ev[:, 1] // plane
        if np.any((zb - za < 0) | (zb - za > 1)):
            raise NotImplementedError("P2 on a sharded mesh: an edge spans more than two vertex planes")
        inter = zb > za
        n_in = np.bincount(za[~inter], minlength=nzl)
        n_up = np.bincount(za[inter], minlength=nzl)
        if nzl < 2 or np.any(n_in != n_in[0]) or np.any(n_up[:-1] != n_up[0]) or n_up[-1] != 0:
            raise NotImplementedError("P2 on a sharded mesh: the planes of the slab do not carry the same edges")
        ne_in, ne_up = int(n_in[0]), int(n_up[0])
        B = plane + ne_in + ne_up
        # rank of every edge within its plane and kind (keys are sorted: a stable count per (plane, kind) gives the order)
        kind_key = za * 2 + inter.astype(np.int64)
        order = np.argsort(kind_key, kind="stable")
        rank_in_group = np.empty(ev.shape[0], dtype=np.int64)
        start = np.concatenate([[0], np.cumsum(np.bincount(kind_key, minlength=2 * nzl))])[:-1]
        rank_in_group[order] = np.arange(ev.shape[0]) - start[kind_key[order]]
        edge_node = za * B + plane + np.where(inter, ne_in, 0) + rank_in_group
        vert_node = (np.arange(nv) // plane) * B + np.arange(nv) % plane
        n = (nzl - 1) * B + plane + ne_in
        coords = np.empty((n, X.shape[1]))
        coords[vert_node] = X
        coords[edge_node] = 0.5 * (X[ev[:, 0]] + X[ev[:, 1]])
        self.coords = coords
        self.cells = np.concatenate([vert_node[C], edge_node[inv.reshape(len(loc), C.shape[0]).T]], axis=1).astype(np.int32)
        self.vertex_nodes = vert_node
        self.edge_nodes = edge_node
        self.edge_vertices = ev
        has_lo, has_hi = mp.lo_ghost > 0, mp.hi_ghost > 0
        own_planes = nzl - int(has_lo) - int(has_hi)
        if own_planes < 2 and has_hi:
            raise NotImplementedError("P2 on a sharded mesh: every rank but the last needs two owned vertex planes")
        lo_g = B if has_lo else 0
        hi_g = plane + ne_in if has_hi else 0
        part = Partition(mp.comm, lo_g, n - hi_g, -1, lo_g, hi_g, -1)
        part.send_lo = plane + ne_in if has_lo else 0           # the first plane's vertices and in-plane edge nodes go down
        part.send_hi = B if has_hi else 0                       # the last owned block goes up
        self._p2_part = part

    _p2_part = None

    @property
    def part(self):
        return self._p2_part if self._p2_part is not None else self.mesh.part

    def owned_range(self):
        if self._p2_part is not None:
            return (self._p2_part.own0, self._p2_part.own1)
        return self.mesh.owned_range() if self.degree == 1 else (0, self.n)

    def shard_view(self):
        return _ShardView(self) if self._p2_part is not None else self.mesh

    def on_boundary(self):
        onb = self.mesh.vertex_on_boundary()
        if self.vertex_nodes is None:
            return onb
        flags = np.zeros(self.n, dtype=bool)
        flags[self.vertex_nodes] = onb
        tdim = self.mesh.topology().dim()
        if self._p2_part is not None:
            # a slab's own facets include its cut planes: the builder says which points lie on the hull of the WHOLE mesh
            test = getattr(self.mesh, "_hull_test", None)
            if test is None:
                raise NotImplementedError("P2 on a sharded mesh needs the builder's hull test")
            flags[self.edge_nodes] = test(self.coords[self.edge_nodes])
            return flags
        if tdim > 1:
            # an edge node lies on the boundary when its edge belongs to a boundary facet (a facet of one cell)
            C = self.mesh.cells().astype(np.int64)
            nv = C.max() + 1
            if tdim == 2:
                fe = np.concatenate([np.sort(C[:, list(e)], axis=1) for e in self.P2_EDGES[2]], axis=0)
                keys, cnt = np.unique(fe[:, 0] * nv + fe[:, 1], return_counts=True)
                bkeys = keys[cnt == 1]
            else:
                faces = np.concatenate([np.sort(C[:, [a, b, c]], axis=1)
                                        for a, b, c in ((1, 2, 3), (0, 2, 3), (0, 1, 3), (0, 1, 2))], axis=0)
                fk, idx, cnt = np.unique((faces[:, 0] * nv + faces[:, 1]) * nv + faces[:, 2],
                                         return_index=True, return_counts=True)
                bf = faces[idx[cnt == 1]]
                be = np.concatenate([bf[:, [0, 1]], bf[:, [0, 2]], bf[:, [1, 2]]], axis=0)
                bkeys = np.unique(be[:, 0] * nv + be[:, 1])
            ek = self.edge_vertices[:, 0].astype(np.int64) * nv + self.edge_vertices[:, 1]
            flags[self.edge_nodes] = np.isin(ek, bkeys)
        return flags

    def embed_p1(self, vertex_values):
        """Nodal values of the piecewise-LINEAR interpolant of per-vertex data in this layout (edge nodes
        take the mean of their end points) - how a degree-1 coefficient enters a P2 integrand."""
        if self.vertex_nodes is None:
            return np.asarray(vertex_values, dtype=np.float64)
        out = np.empty(self.n)
        out[self.vertex_nodes] = vertex_values
        vn_of = np.full(self.n, -1, dtype=np.int64)
        vn_of[self.vertex_nodes] = np.arange(len(self.vertex_nodes))
        ev = self.edge_vertices
        if self.mesh.topology().dim() == 1:
            a, b = vn_of[ev[:, 0]], vn_of[ev[:, 1]]
        else:
            a, b = ev[:, 0], ev[:, 1]
        vv = np.asarray(vertex_values, dtype=np.float64)
        out[self.edge_nodes] = 0.5 * (vv[a] + vv[b])
        return out

    def space(self):
        if self._space is None:
            self._space = FunctionSpace(self.mesh, "CG", self.degree)
        return self._space

    def handle(self):
        be = get_backend()
        h = self._handles.get(id(be))
        if h is None:
            h = be.mesh(self.coords, self.cells)
            self._handles[id(be)] = h
        return h

    def bind_p2_lattice(self, be):
        """Bind this layout to the box lattice of its vertices on the backend (pgd_mesh_p2_bind), for the p-multigrid cycle: True
        where the library took it.  Only a degree-2 layout on an unsharded 3-D mesh is offered (its own edge list and the P1 layout
        of its own mesh, as the entry point requires); the answer is kept per backend, so a run asks once per layout."""
        if self.degree != 2 or self.mesh.topology().dim() != 3 or self.part is not None or not hasattr(be, "mesh_p2_bind"):
            return False
        got = self._p2_bound.get(be)
        if got is None:
            got = self._p2_bound[be] = bool(be.mesh_p2_bind(self.handle(), self.mesh.layout(1).handle(), self.edge_vertices))
        return got

    def _atom_key(self, be, kind, da, db, weight):
        if self.mesh.geometry().dim() == 1 and kind in (DUDV, WDUDV):
            kind = STIFF if kind == DUDV else WSTIFF
        wkey = None if weight is None else (id(weight), weight.version)
        return (id(be), kind, da if kind in _DA_KINDS else 0, db if kind in _DB_KINDS else 0, wkey)

    def atom(self, kind, da=0, db=0, weight=None, cells=None, cw=None):
        """Cached device atom; weighted atoms are keyed by the weight's identity + version, the identity checked through
        a weak reference: an address (``id``) is reused as soon as a vector dies, and an iterate can end up as the weight
        of a functional (``assemble(E * F * F * dx)`` with E and F equally "old").  cells: the _CellSet of a dx(id) measure;
        cw: the vector of a DG0 Function (one value per cell) that multiplies the integrand."""
        be = get_backend()
        if cw is not None:
            return self._cellwise_atom(be, kind, da, db, weight, cells, cw)
        if cells is not None:
            return self._cell_atom(be, kind, da, db, weight, cells)
        if kind in (WDUDV, WCONV, WCONVT) and self.part is not None:
            raise NotImplementedError("weighted derivative atoms on a sharded (slab) layout")
        key = self._atom_key(be, kind, da, db, weight)
        kind = key[1]
        a = self._atoms.get(key)
        if a is not None and weight is not None:
            ref = self._atom_weights.get(key)
            if ref is None or ref() is not weight:          # another vector lives at that address now
                self._drop_atom(be, key)
                a = None
        if a is None:
            if weight is not None:
                # drop the atoms of older versions of this weight and those of weights that died (2 GB each at 256^3) - never
                # another atom of the same version: the (da, db) atoms of one weight (weighted elasticity) live side by side
                for k in [k for k in self._atoms if k[0] == id(be) and k[4] and
                          ((k[4][0] == id(weight) and k[4][1] < weight.version) or self._atom_weights[k]() is None)]:
                    self._drop_atom(be, k)
            a = be.atom(self.handle(), kind, key[2], key[3], weight.dev() if weight is not None else 0)
            self._atoms[key] = a
            if weight is not None:
                self._atom_weights[key] = weakref.ref(weight)
        return a

    def facet_atom(self, ids):
        """Cached boundary-mass atom  int_Gamma phi_i phi_j ds  over the facets `ids` (Mesh.facets() numbering), assembled
        on the device; kept per backend and facet set with the layout, like the cell atoms."""
        if self.part is not None:
            raise NotImplementedError("bilinear ds terms (Robin atoms) on a sharded (slab) layout")
        be = get_backend()
        fn = getattr(be, "atom_facets", None)
        if fn is None:
            raise NotImplementedError("bilinear ds terms need a backend that assembles facet atoms (atom_facets); %r has none"
                                      % (getattr(be, "name", type(be).__name__),))
        key = (id(be), ids.tobytes())
        a = self._facet_atoms.get(key)
        if a is None:
            a = fn(self.handle(), _facet_node_tuples(self, ids))
            self._facet_atoms[key] = a
        return a

    def _drop_atom(self, be, key):
        stale = self._atoms.pop(key)
        self._atom_weights.pop(key, None)
        _purge_atom(stale)       # the library recycles handle numbers: forget everything keyed by it
        be.atom_free(stale)

    def _cell_atom(self, be, kind, da, db, weight, cells):
        """The atom over the cells of a dx(id) measure (pgd_atom_assemble_cells), cached per backend, kind, (da, db), weight and
        cell set.  A cell set is keyed by the generation of its MeshFunction's markers (_cell_generation): the atoms of older
        generations of the same MeshFunction, of MeshFunctions that died and of stale weights are freed here, with the
        vector-valued embeddings built from them."""
        if self.part is not None:
            raise NotImplementedError("cell-subdomain integrals dx(id) on a sharded (slab) layout")
        fn = getattr(be, "atom_cells", None)
        if fn is None:
            raise NotImplementedError("cell-subdomain integrals dx(id) need a backend that assembles masked atoms (atom_cells); "
                                      "%r has none" % (getattr(be, "name", type(be).__name__),))
        key = self._atom_key(be, kind, da, db, weight) + (cells.key,)
        hit = self._cell_atoms.get(key)
        if hit is not None and hit[1]() is cells.mf and (weight is None or hit[2]() is weight):
            return hit[0]
        for k, (a, mref, wref) in list(self._cell_atoms.items()):
            bid, _, _, _, wkey, ckey = k
            if bid == id(be) and (k == key or _stale_cells(ckey, mref, cells) or _stale_vector(wkey, wref, weight)):
                self._drop_cell_atom(be, self._cell_atoms, k)
        a = fn(self.handle(), key[1], key[2], key[3], weight.dev() if weight is not None else 0, cells.mask())
        self._cell_atoms[key] = (a, weakref.ref(cells.mf), weakref.ref(weight) if weight is not None else (lambda: None))
        return a

    def _cellwise_atom(self, be, kind, da, db, weight, cells, cw):
        """The atom with a cell-wise constant coefficient (pgd_atom_assemble_cellwise), cached per backend, kind, (da, db), nodal
        weight, cell set and field.  The field is keyed like a nodal weight - identity + version of its vector, the identity
        checked through a weak reference - and evicted like one: atoms of older versions of this field, of fields that died and
        of stale weights / cell sets are freed here with their vector-valued embeddings; the atoms of ONE version (the nine of
        weighted elasticity) live side by side."""
        if self.part is not None:
            raise NotImplementedError("cell-wise constant (DG0) coefficients on a sharded (slab) layout")
        fn = getattr(be, "atom_cellwise", None)
        if fn is None:
            raise NotImplementedError("cell-wise constant (DG0) coefficients need a backend that assembles cell-weighted atoms "
                                      "(atom_cellwise); %r has none" % (getattr(be, "name", type(be).__name__),))
        if cw.V.mesh() is not self.mesh:
            raise ValueError("the DG0 coefficient lives on a different mesh than the integral")
        key = self._atom_key(be, kind, da, db, weight) + (cells.key if cells is not None else None, (id(cw), cw.version))
        hit = self._cw_atoms.get(key)
        if (hit is not None and hit[1]() is cw and (cells is None or hit[2]() is cells.mf)
                and (weight is None or hit[3]() is weight)):
            return hit[0]
        for k, (a, cref, mref, wref) in list(self._cw_atoms.items()):
            bid, _, _, _, wkey, ckey, fkey = k
            if bid == id(be) and (k == key or _stale_vector(fkey, cref, cw) or _stale_cells(ckey, mref, cells)
                                  or _stale_vector(wkey, wref, weight)):
                self._drop_cell_atom(be, self._cw_atoms, k)
        a = fn(self.handle(), key[1], key[2], key[3], weight.dev() if weight is not None else 0, cw.dev(),
               cells.mask() if cells is not None else None)
        none = lambda: None
        self._cw_atoms[key] = (a, weakref.ref(cw), weakref.ref(cells.mf) if cells is not None else none,
                               weakref.ref(weight) if weight is not None else none)
        return a

    def _drop_cell_atom(self, be, store, key):
        """Free the atom of `key` in `store` (_cell_atoms or _cw_atoms), the vector-valued embeddings built from it and
        everything keyed by its handle."""
        stale = store.pop(key)[0]
        for blk in list(self.mesh._layouts.values()):
            if isinstance(blk, BlockLayout) and blk.base is self:
                blk._drop_derived(be, stale)
        _purge_atom(stale)
        be.atom_free(stale)


def _stale_vector(vkey, ref, current):
    """Is a cached atom keyed by a vector (vkey = (id, version) or None: a nodal weight or a DG0 field, `ref` the weak reference
    kept with it) out of date?  Yes when the vector died, and when `current` - the vector of the request at hand - lives at
    that address but is another object or a newer version.  Atoms of the SAME version stay: the (da, db) atoms of one weight
    live side by side."""
    if vkey is None:
        return False
    if ref() is None:
        return True
    return current is not None and vkey[0] == id(current) and (ref() is not current or vkey[1] < current.version)


def _stale_cells(ckey, ref, cells):
    """Is a cached atom keyed by a cell set (ckey = (generation, id) or None, `ref` the weak reference to its MeshFunction) out
    of date?  Yes when the MeshFunction died, and when `cells` - the _CellSet of the request at hand - is of the same
    MeshFunction in another generation of its markers."""
    if ckey is None:
        return False
    if ref() is None:
        return True
    return cells is not None and ref() is cells.mf and ckey[0] != cells.gen


def IntervalMesh(n, a, b):
    n = int(n)
    coords = (a + (b - a) * np.arange(n + 1, dtype=np.float64) / n).reshape(-1, 1)
    cells = np.stack([np.arange(n), np.arange(1, n + 1)], axis=1)
    return Mesh(coords, cells)


def UnitIntervalMesh(n):
    return IntervalMesh(n, 0.0, 1.0)


def _grid_axis(a, b, n):
    return a + (b - a) * np.arange(n + 1, dtype=np.float64) / n


def RectangleMesh(p0, p1, nx, ny, diagonal="right"):
    nx, ny = int(nx), int(ny)
    xs, ys = _grid_axis(p0[0], p1[0], nx), _grid_axis(p0[1], p1[1], ny)
    X, Y = np.meshgrid(xs, ys, indexing="xy")
    coords = np.stack([X.ravel(), Y.ravel()], axis=1)
    ix, iy = np.meshgrid(np.arange(nx), np.arange(ny), indexing="xy")
    v0 = (iy * (nx + 1) + ix).ravel()
    v1, v2, v3 = v0 + 1, v0 + nx + 1, v0 + nx + 2
    if diagonal == "right":
        tris = ((v0, v1, v3), (v0, v2, v3))
    elif diagonal == "left":
        tris = ((v0, v1, v2), (v1, v2, v3))
    elif diagonal == "crossed":
        # four triangles per cell around its midpoint; the midpoints follow the grid vertices
        xm, ym = 0.5 * (xs[:-1] + xs[1:]), 0.5 * (ys[:-1] + ys[1:])
        XM, YM = np.meshgrid(xm, ym, indexing="xy")
        coords = np.concatenate([coords, np.stack([XM.ravel(), YM.ravel()], axis=1)], axis=0)
        vm = (nx + 1) * (ny + 1) + (iy * nx + ix).ravel()
        cells = np.empty((4 * nx * ny, 3), dtype=np.int32)
        for k, t in enumerate(((v0, v1, vm), (v0, v2, vm), (v1, v3, vm), (v2, v3, vm))):
            cells[k::4] = np.sort(np.stack(t, axis=1), axis=1)
        return Mesh(coords, cells)
    else:
        raise NotImplementedError("RectangleMesh diagonal=%r ('right', 'left', 'crossed')" % (diagonal,))
    cells = np.empty((2 * nx * ny, 3), dtype=np.int32)
    for k, t in enumerate(tris):
        cells[k::2] = np.stack(t, axis=1)
    mesh = Mesh(coords, cells)
    jx, jy = np.meshgrid(np.arange(nx + 1), np.arange(ny + 1), indexing="xy")
    mesh._on_boundary = ((jx == 0) | (jx == nx) | (jy == 0) | (jy == ny)).ravel()   # structured: no facet search
    return mesh


def UnitSquareMesh(nx, ny, diagonal="right"):
    return RectangleMesh(Point(0, 0), Point(1, 1), nx, ny, diagonal)


def box_mesh_arrays(p0, p1, nx, ny, nz, z_first=0, z_last=None):
    """Vertices / tetrahedra of dolfin.BoxMesh restricted to the vertex planes
    z_first..z_last (inclusive) - the slab a rank holds when the mesh is sharded."""
    z_last = nz if z_last is None else z_last
    xs, ys, zs = _grid_axis(p0[0], p1[0], nx), _grid_axis(p0[1], p1[1], ny), _grid_axis(p0[2], p1[2], nz)
    zs = zs[z_first:z_last + 1]
    Z, Y, X = np.meshgrid(zs, ys, xs, indexing="ij")
    coords = np.stack([X.ravel(), Y.ravel(), Z.ravel()], axis=1)
    nzl = z_last - z_first
    sx, sy = nx + 1, (nx + 1) * (ny + 1)
    iz, iy, ix = np.meshgrid(np.arange(nzl), np.arange(ny), np.arange(nx), indexing="ij")
    v0 = (iz * sy + iy * sx + ix).ravel().astype(np.int32)
    v1, v2, v3 = v0 + 1, v0 + sx, v0 + sx + 1
    v4, v5, v6, v7 = v0 + sy, v1 + sy, v2 + sy, v3 + sy
    tets = ((v0, v1, v3, v7), (v0, v1, v7, v5), (v0, v5, v7, v4),
            (v0, v3, v2, v7), (v0, v6, v4, v7), (v0, v2, v6, v7))
    cells = np.empty((6 * nx * ny * nzl, 4), dtype=np.int32)
    for k, t in enumerate(tets):
        cells[k::6] = np.stack(t, axis=1)
    return coords, cells


def box_hull_mask(nx, ny, nz, z_first=0, z_last=None):
    """Vertices of the (sub-)grid that lie on the hull of the whole box."""
    z_last = nz if z_last is None else z_last
    jz, jy, jx = np.meshgrid(np.arange(z_first, z_last + 1), np.arange(ny + 1), np.arange(nx + 1), indexing="ij")
    return ((jx == 0) | (jx == nx) | (jy == 0) | (jy == ny) | (jz == 0) | (jz == nz)).ravel()


def BoxMesh(p0, p1, nx, ny, nz):
    nx, ny, nz = int(nx), int(ny), int(nz)
    coords, cells = box_mesh_arrays(p0, p1, nx, ny, nz)
    mesh = Mesh(coords, cells)
    mesh._on_boundary = box_hull_mask(nx, ny, nz)
    return mesh


def UnitCubeMesh(nx, ny, nz):
    return BoxMesh(Point(0, 0, 0), Point(1, 1, 1), nx, ny, nz)


# ------------------------------------------------------------------- function spaces
class _Element:
    def __init__(self, cell, degree):
        self._cell, self._degree = cell, degree

    def __str__(self):
        return "FiniteElement('Lagrange', %s, %d)" % (self._cell, self._degree)

    __repr__ = __str__

    def degree(self):
        return self._degree

    def family(self):
        return "Lagrange"


class _DofMap:
    def __init__(self, V):
        self._V = V

    def dofs(self):
        return np.arange(self._V.dim())


class _CellLayout:
    """The dofs of a DG0 space: one per cell, dof i = cell i of mesh.cells(), located at the cell's midpoint.  It carries
    coefficients only - no device mesh, no atoms."""
    part = None

    def __init__(self, mesh):
        self.mesh, self.degree = mesh, 0
        self.coords = mesh.coordinates()[mesh.cells()].mean(axis=1)
        self.n = self.coords.shape[0]
        self.vertex_nodes = None


class _DG0Element(_Element):
    def __str__(self):
        return "FiniteElement('Discontinuous Lagrange', %s, 0)" % (self._cell,)

    __repr__ = __str__

    def family(self):
        return "Discontinuous Lagrange"


_DG_FAMILIES = ("DG", "Discontinuous Lagrange")


class FunctionSpace:
    _ncomp = 1
    _dg0 = False                 # a DG0 space: coefficients that are constant per cell (one undifferentiated factor of a dx integrand)

    def __init__(self, mesh, family="CG", degree=1):
        if str(family) in _DG_FAMILIES:
            if int(degree) != 0:
                raise NotImplementedError("discontinuous Lagrange spaces of degree %d: only DG0 (cell-wise constant coefficients)"
                                          % int(degree))
            if mesh.part is not None:
                raise NotImplementedError("DG0 coefficients on a row-sharded mesh")
            self._mesh, self._dg0 = mesh, True
            lay = mesh._layouts.get("dg0")
            if lay is None:
                lay = mesh._layouts["dg0"] = _CellLayout(mesh)
            self._lay = lay
            self._element = _DG0Element(mesh.ufl_cell(), 0)
            self._d2v = None     # dof i = cell i on every mesh (intervals included)
            return
        if str(family) not in ("CG", "P", "Lagrange"):
            raise NotImplementedError("FunctionSpace family %r: only Lagrange ('CG'/'P')" % (family,))
        self._mesh = mesh
        self._lay = mesh.layout(int(degree))       # raises for what is not built (P2 beyond intervals, ...)
        self._element = _Element(mesh.ufl_cell(), int(degree))
        n = self._lay.n
        # dof -> node; self-inverse reversal on intervals (as serial dolfin orders P1 there), identity otherwise
        self._d2v = np.arange(n - 1, -1, -1) if mesh.topology().dim() == 1 else None

    def mesh(self):
        return self._mesh

    def dim(self):
        return self._lay.n

    def ufl_element(self):
        return self._element

    def ufl_function_space(self):
        return self

    def dofmap(self):
        return _DofMap(self)

    def tabulate_dof_coordinates(self):
        return self.to_dof_order(self._lay.coords)

    def to_dof_order(self, a):
        return a if self._d2v is None else a[self._d2v]

    def to_vertex_order(self, a):
        return a if self._d2v is None else a[self._d2v]     # the reversal is its own inverse

    def dof_to_vertex(self, dofs):
        return dofs if self._d2v is None else self._d2v[dofs]

    def __eq__(self, other):
        return self is other

    def __hash__(self):
        return id(self)


class _ShardView:
    """A layout seen as pgdrome_amd/dist.py sees a mesh: `.part` and `.num_vertices()` in DOFS (a vector-valued space on a sharded
    mesh has ncomp times the rows of its mesh)."""

    def __init__(self, lay):
        self.lay = lay

    @property
    def part(self):
        return self.lay.part

    def num_vertices(self):
        return self.lay.n


class BlockLayout:
    """Degrees of freedom of a VECTOR-valued Lagrange space: dof (node i, component c) = ncomp i + c over a
    scalar DofLayout.  The device sees it as a layout of its own (pgd_mesh_blocked); its atoms are scalar
    atoms of the base layout embedded in a (test component, trial component) block (pgd_atom_embed)."""

    def __init__(self, base, ncomp):
        self.base, self.ncomp = base, int(ncomp)
        self.mesh, self.degree = base.mesh, base.degree
        self.n = base.n * self.ncomp
        self.coords = np.repeat(base.coords, self.ncomp, axis=0)       # dof coordinates
        self.vertex_nodes = base.vertex_nodes
        self._handles, self._atoms = {}, {}
        self._watoms = {}            # weighted: base atom key + (cv, cu) -> (embedded atom, scalar source, weakref to the weight)
        self._catoms = {}            # cell-subdomain: (backend, scalar source, cv, cu) -> embedded atom (freed with the source)
        self._ones = self._space = None

    @property
    def part(self):
        """Row-sharded base (P1 on z-slabs): dof (node i, component c) = ncomp i + c keeps a slab's dofs contiguous - ghost dofs
        below, owned dofs, ghost dofs above - so the partition of the nodes, times ncomp, is the partition of the dofs."""
        bp = self.base.part
        if bp is None:
            return None
        if self._part is None or self._part[0] is not bp:
            nc = self.ncomp
            part = Partition(bp.comm, nc * bp.own0, nc * bp.own1, nc * bp.n_global, nc * bp.lo_ghost, nc * bp.hi_ghost,
                             nc * bp.global_offset)
            part.send_lo, part.send_hi = nc * bp.send_lo, nc * bp.send_hi          # (a P2 base: sizes per direction)
            self._part = (bp, part)
        return self._part[1]

    _part = None

    def owned_range(self):
        part = self.part
        return (part.own0, part.own1) if part is not None else (0, self.n)

    def shard_view(self):
        """What the communicator's solvers and halo exchanges take for "the mesh" of this layout: its partition and its length."""
        return _ShardView(self)

    def on_boundary(self):
        return np.repeat(self.base.on_boundary(), self.ncomp)

    def space(self):
        if self._space is None:
            self._space = VectorFunctionSpace(self.mesh, "CG", self.degree, dim=self.ncomp)
        return self._space

    def handle(self):
        be = get_backend()
        h = self._handles.get(id(be))
        if h is None:
            h = be.mesh_blocked(self.base.handle(), self.ncomp)
            self._handles[id(be)] = h
        return h

    def bind_p2_lattice(self, be):
        """A vector-valued layout uses the binding of its scalar layout."""
        return self.base.bind_p2_lattice(be)

    def atom(self, kind, da=0, db=0, weight=None, cv=None, cu=None, cells=None, cw=None):
        """Scalar atom (kind, da, db) in block (cv, cu); cv = cu = None: in every diagonal block (norms).  A weight is a
        scalar field of the base layout (_coef_vec(..., weight=True)): the scalar weighted atom, embedded.  cells: the
        _CellSet of a dx(id) measure - the base layout's masked atom, embedded; cw: the vector of a DG0 coefficient - the base
        layout's cell-weighted atom, embedded."""
        if cells is not None or cw is not None:
            if self.part is not None:
                raise NotImplementedError("cell-subdomain integrals dx(id) and DG0 coefficients on a sharded (slab) vector-valued layout")
            if weight is not None and weight.size() != self.base.n:
                raise NotImplementedError("a weight on a vector-valued space is a scalar field of its Lagrange degree")
            be = get_backend()
            src = self.base.atom(kind, da, db, weight, cells=cells, cw=cw)     # (frees stale sources, and their embeddings with them)
            key = (id(be), src, cv, cu)
            a = self._catoms.get(key)
            if a is None:
                a = self._catoms[key] = self._embed(be, src, cv, cu)
            return a
        if weight is None:
            return self._embedded(self.base.atom(kind, da, db), cv, cu)
        if self.part is not None:
            raise NotImplementedError("weighted atoms on a sharded (slab) vector-valued layout")
        if weight.size() != self.base.n:
            raise NotImplementedError("a weight on a vector-valued space is a scalar field of its Lagrange degree")
        be = get_backend()
        src = self.base.atom(kind, da, db, weight)           # (drops the base's atoms of older versions and of dead weights)
        bkey = self.base._atom_key(be, kind, da, db, weight)
        key = bkey + (cv, cu)
        hit = self._watoms.get(key)
        if hit is not None and hit[1] == src and hit[2]() is weight:
            return hit[0]
        # embedded atoms whose scalar source is gone (handle numbers are reused: the source is checked by its key, its handle
        # and its weight) - or whose entry is replaced here
        base_atoms, base_w = self.base._atoms, self.base._atom_weights
        for k, (a, s_, wref) in list(self._watoms.items()):
            if k[0] != id(be):
                continue
            bk = k[:5]
            alive = wref() is not None and base_atoms.get(bk) == s_ and base_w.get(bk) is not None and base_w[bk]() is wref()
            if k == key or not alive:
                del self._watoms[k]
                _purge_atom(a)
                be.atom_free(a)
        a = self._embed(be, src, cv, cu)
        self._watoms[key] = (a, src, weakref.ref(weight))
        return a

    def facet_atom(self, ids, cv=None, cu=None):
        """The base layout's boundary-mass atom over the facets `ids` in block (cv, cu) (cv = cu = None: every diagonal block)."""
        if self.part is not None:
            raise NotImplementedError("bilinear ds terms (Robin atoms) on a sharded (slab) layout")
        return self._embedded(self.base.facet_atom(ids), cv, cu)

    def _drop_derived(self, be, src):
        """Free the embeddings of a scalar cell-subdomain / cell-weighted atom that its base layout frees."""
        for k in [k for k in self._catoms if k[0] == id(be) and k[1] == src]:
            a = self._catoms.pop(k)
            _purge_atom(a)
            be.atom_free(a)

    def _embedded(self, src, cv, cu):
        be = get_backend()
        key = (id(be), src, cv, cu)
        a = self._atoms.get(key)
        if a is None:
            a = self._embed(be, src, cv, cu)
            self._atoms[key] = a
        return a

    def _embed(self, be, src, cv, cu):
        if cv is None:
            a = be.atom_embed(self.handle(), src, 0, 0, 1.0, 0)
            for c in range(1, self.ncomp):
                be.atom_embed(self.handle(), src, c, c, 1.0, a)
            return a
        return be.atom_embed(self.handle(), src, int(cv), int(cu), 1.0, 0)


def _block_layout(mesh, degree, ncomp):
    key = ("vector", int(degree), int(ncomp))
    lay = mesh._layouts.get(key)
    if lay is None:
        lay = BlockLayout(mesh.layout(int(degree)), ncomp)
        mesh._layouts[key] = lay
    return lay


class _VectorElement(_Element):
    def __init__(self, cell, degree, ncomp):
        _Element.__init__(self, cell, degree)
        self._ncomp = ncomp

    def __str__(self):
        return "<vector element with %d components of FiniteElement('Lagrange', %s, %d)>" % (
            self._ncomp, self._cell, self._degree)

    __repr__ = __str__

    def value_shape(self):
        return (self._ncomp,)


class VectorFunctionSpace(FunctionSpace):
    """Vector-valued Lagrange space, dofs interleaved by component (node-major)."""

    def __init__(self, mesh, family="CG", degree=1, dim=None):
        if str(family) in _DG_FAMILIES:
            raise NotImplementedError("vector-valued discontinuous Lagrange spaces (a DG0 coefficient is a scalar field)")
        if str(family) not in ("CG", "P", "Lagrange"):
            raise NotImplementedError("VectorFunctionSpace family %r: only Lagrange ('CG'/'P')" % (family,))
        self._mesh = mesh
        self._ncomp = int(dim) if dim is not None else mesh.geometry().dim()
        if self._ncomp < 2 or self._ncomp > 3:
            raise NotImplementedError("vector-valued spaces with %d components" % self._ncomp)
        self._lay = _block_layout(mesh, int(degree), self._ncomp)
        self._element = _VectorElement(mesh.ufl_cell(), int(degree), self._ncomp)
        self._d2v = None
        self._scalar = None

    def num_sub_spaces(self):
        return self._ncomp

    def scalar_space(self):
        if self._scalar is None:
            self._scalar = self._lay.base.space()
        return self._scalar


def vertex_to_dof_map(V):
    n = V.dim()
    return np.arange(n) if V._d2v is None else V._d2v.copy()


dof_to_vertex_map = vertex_to_dof_map


# ----------------------------------------------------------------------------- vectors
class Vector:
    """A dof vector resident on the device, with a lazily synchronised host mirror.

    Storage is in VERTEX order on both sides; indexing (``v[:]``, ``v[i]``) is in
    DOF order like dolfin's GenericVector."""

    def __init__(self, V, host=None):
        self.V = V
        self.n = V.dim()
        # the host mirror of a fresh (all-zero) vector is only materialised when somebody reads it:
        # a 16.7 M-entry np.zeros + np.any costs 7 ms per vector, several times per fixed-point pass
        self._host = None if host is None else np.array(host, dtype=np.float64)
        self._zero = host is None
        self._dev = None
        self._be = None          # backend that owns _dev
        self._host_ok = True
        self._dev_ok = False
        self.version = 0

    # -- residency
    def host(self):
        if not self._host_ok:
            self._host = self._be.vec_to_host(self._dev)
            self._host_ok = True
        elif self._host is None:
            self._host = np.zeros(self.n)
        return self._host

    def _alloc_dev(self):
        be = get_backend()
        if self._dev is not None and self._be is not be:     # backend was swapped (tests): start over there
            self.host()
            self._drop_dev()
        if self._dev is None:
            self._dev, self._be = be.vec_zeros(self.n), be
            self._dev_ok = bool(self._host_ok and self._zero)
        return be

    def _drop_dev(self):
        if self._dev is not None:
            try:
                self._be.vec_free(self._dev)
            except Exception:
                pass
        self._dev, self._be, self._dev_ok = None, None, False

    def dev(self):
        be = self._alloc_dev()
        if not self._dev_ok:
            be.vec_upload(self._dev, self.host())
            self._dev_ok = True
        return self._dev

    def touched_host(self):
        self._host_ok, self._dev_ok, self._zero = True, False, False
        self.version += 1

    def touched_dev(self):
        self._dev_ok, self._host_ok, self._zero = True, False, False
        self.version += 1

    def __del__(self):
        self._drop_dev()

    # -- GenericVector surface
    def __len__(self):
        return self.n

    def size(self):
        return self.n

    local_size = size

    def get_local(self):
        return self.V.to_dof_order(self.host()).copy()

    def set_local(self, a):
        self._host = np.array(self.V.to_vertex_order(np.asarray(a, dtype=np.float64)), dtype=np.float64)
        self.touched_host()

    def apply(self, mode=""):
        pass

    def __getitem__(self, key):
        return self.V.to_dof_order(self.host())[key].copy() if isinstance(key, slice) \
            else self.V.to_dof_order(self.host())[key]

    def __setitem__(self, key, val):
        a = self.get_local()
        a[key] = val.get_local() if isinstance(val, Vector) else val
        self.set_local(a)

    def __array__(self, dtype=None, copy=None):
        return self.get_local()

    def zero(self):
        self._host = np.zeros(self.n)
        self.touched_host()

    def copy(self):
        out = Vector(self.V)
        out.assign_from(self)
        return out

    def assign_from(self, other):
        if self._small() or not other._dev_ok:
            self._host = other.host().copy()
            self.touched_host()
        else:
            get_backend().vec_copy(self.dev_for_write(), other.dev())
            self.touched_dev()

    def dev_for_write(self):
        """Device handle whose content is about to be overwritten (skips the upload)."""
        self._alloc_dev()
        return self._dev

    def _small(self):
        return self.n <= 4096

    def fill(self, a):
        """All entries (ghosts included) = a; on the device for large vectors (no 134 MB upload)."""
        if self._small():
            self._host = np.full(self.n, float(a))
            self.touched_host()
        else:
            get_backend().vec_fill(self.dev_for_write(), float(a))
            self.touched_dev()

    def scale(self, a):
        if self._dev_ok and not self._small():
            get_backend().vec_scale(self._dev, float(a))
            self.touched_dev()
        else:
            self._host = self.host() * float(a)
            self.touched_host()

    def axpy(self, a, x):
        if not self._small() and (self._dev_ok or x._dev_ok):
            get_backend().vec_axpy(self.dev(), float(a), x.dev())
            self.touched_dev()
        else:
            self._host = self.host() + float(a) * x.host()
            self.touched_host()

    def __imul__(self, a):
        self.scale(a)
        return self

    # GenericVector arithmetic (new vectors)
    def __add__(self, x):
        out = self.copy()
        out.axpy(1.0, x)
        return out

    def __sub__(self, x):
        out = self.copy()
        out.axpy(-1.0, x)
        return out

    def __neg__(self):
        out = self.copy()
        out.scale(-1.0)
        return out

    def __mul__(self, a):
        out = self.copy()
        out.scale(float(a))
        return out

    __rmul__ = __mul__

    def __itruediv__(self, a):
        self.scale(1.0 / a)
        return self

    def __iadd__(self, x):
        self.axpy(1.0, x)
        return self

    def __isub__(self, x):
        self.axpy(-1.0, x)
        return self

    def inner(self, other):
        lo, hi = self.V._lay.owned_range()
        if self._small() and self.V.mesh().part is None:
            return float(self.host() @ other.host())
        return _allreduce_sum(self.V.mesh(), get_backend().vec_dot(self.dev(), other.dev(), lo, hi))

    def norm(self, kind="l2"):
        if kind.lower() == "l2":
            return math.sqrt(self.inner(self))
        if kind.lower() == "linf":
            return float(np.abs(self.host()).max())
        raise NotImplementedError(kind)

    def max(self):
        return float(self.host().max())

    def min(self):
        return float(self.host().min())

    def sum(self):
        return float(self.host().sum())


def _allreduce_sum(mesh, value):
    if mesh.part is None:
        return value
    return mesh.part.comm.allreduce_sum(value)


# ------------------------------------------------------------------ symbolic algebra
class Expr:
    """Anything that can stand in an integrand; normalises to a polynomial (list of Terms)."""

    def _poly(self):
        raise NotImplementedError

    def __mul__(self, o):
        if isinstance(o, Measure):
            return Form([(t, o) for t in self._poly()])
        if isinstance(o, Form):
            return o * _scalar_of(self)
        return Poly(_pmul(self._poly(), _as_poly(o)))

    def __rmul__(self, o):
        return Poly(_pmul(_as_poly(o), self._poly()))

    def __add__(self, o):
        return Poly(self._poly() + _as_poly(o))

    __radd__ = __add__

    def __sub__(self, o):
        return Poly(self._poly() + _pscale(_as_poly(o), -1.0))

    def __rsub__(self, o):
        return Poly(_as_poly(o) + _pscale(self._poly(), -1.0))

    def __neg__(self):
        return Poly(_pscale(self._poly(), -1.0))

    def __truediv__(self, o):
        return Poly(_pscale(self._poly(), 1.0 / _as_float(o)))

    def dx(self, *axes):
        p = self._poly()
        if len(axes) != 1:
            raise NotImplementedError("only first derivatives .dx(i)")
        out = []
        for t in p:
            if len(t.factors) != 1 or t.factors[0].deriv is not None:
                raise NotImplementedError(".dx() of a product / second derivative")
            f = t.factors[0]
            out.append(t.with_factors((Factor(f.leaf, int(axes[0]), None, f.comp),)))
        return Poly(out)


class Factor:
    __slots__ = ("leaf", "deriv", "other", "comp")

    def __init__(self, leaf, deriv=None, other=None, comp=None):
        # deriv: None | axis | "grad" (dot with `other`); comp: component of a vector-valued leaf
        self.leaf, self.deriv, self.other, self.comp = leaf, deriv, other, comp


class Term:
    """coef * prod(factors).  The coefficient is a number times Constant objects that are read when the
    term is USED, so a form built once follows later ``Constant.assign`` calls (time-stepping loops)."""
    __slots__ = ("num", "factors", "consts")

    def __init__(self, num, factors, consts=()):
        self.num, self.factors, self.consts = float(num), tuple(factors), tuple(consts)

    @property
    def coef(self):
        v = self.num
        for c in self.consts:
            v *= c._v
        return v

    def scaled(self, c):
        return Term(self.num * c, self.factors, self.consts)

    def with_factors(self, factors):
        return Term(self.num, factors, self.consts)


class Poly(Expr):
    def __init__(self, terms):
        self.terms = list(terms)

    def _poly(self):
        return self.terms


class _FastProd(Expr):
    """Product of plain scalar Functions - each undifferentiated, differentiated once (``G.dx(0)``) or an
    ``inner(grad(G), grad(F))`` pair - as the operators of Function build it: the integrands of the callbacks' functionals
    (``assemble(G * F * dx(m))``, the reference's call sites solver.py:547-612).  A pass of a D-dimensional problem with n
    stored modes asks for ~6 D n of them, and the general polynomial (a Term and a Factor per operand and product) was half
    of what such a request cost on the host.  `fs`: tuple of (leaf, deriv, other) as in Factor; the polynomial is formed
    only where something other than ``* Function`` / ``* dx`` happens to the product."""
    __slots__ = ("fs",)

    def __init__(self, fs):
        self.fs = fs

    def _poly(self):
        return [Term(1.0, tuple(Factor(l, d, o) for l, d, o in self.fs))]

    def __mul__(self, o):
        t = type(o)
        if t is Measure:
            return _FastForm(self.fs, o)
        if t is Function:
            if o._V._ncomp == 1 and not o._V._dg0:
                return _FastProd(self.fs + ((o, None, None),))
        elif t is _FastProd:
            return _FastProd(self.fs + o.fs)
        return Expr.__mul__(self, o)


def _scalar_of(e):
    """Value of an expression that contains no fields (products of Constants and floats)."""
    p = e._poly()
    if any(t.factors for t in p):
        raise TypeError("only scalars can multiply an integrated form")
    return sum(t.coef for t in p)


def _as_float(o):
    if isinstance(o, Poly):
        return _scalar_of(o)
    if isinstance(o, Constant):
        return float(o)
    if isinstance(o, numbers.Real):
        return float(o)
    if isinstance(o, np.ndarray) and o.ndim == 0:
        return float(o)
    raise TypeError("expected a scalar, got %r" % (type(o),))


def _as_poly(o):
    if isinstance(o, Expr):
        return o._poly()
    return [Term(_as_float(o), ())]


def _pmul(a, b):
    return [Term(s.num * t.num, s.factors + t.factors, s.consts + t.consts) for s in a for t in b]


def _pscale(a, c):
    return [t.scaled(c) for t in a]


class Constant(Expr):
    def __init__(self, value, cell=None, name=None):
        self._vals = None
        if isinstance(value, (tuple, list, np.ndarray)) and np.ndim(value) > 0:
            if np.ndim(value) != 1:
                raise NotImplementedError("tensor-valued Constant")
            self._vals = np.array(value, dtype=np.float64)     # vector valued: used through dot() / [i]
            self._v = float("nan")
            return
        self._v = float(value)

    def assign(self, v):
        if self._vals is not None:
            self._vals[:] = np.asarray(v.values() if isinstance(v, Constant) else v, dtype=np.float64)
        else:
            self._v = float(v)

    def values(self):
        return self._vals.copy() if self._vals is not None else np.array([self._v])

    def ufl_shape(self):
        return () if self._vals is None else (self._vals.size,)

    def __getitem__(self, i):
        if self._vals is None:
            raise TypeError("scalar Constant is not subscriptable")
        return float(self._vals[i])

    def __len__(self):
        if self._vals is None:
            raise TypeError("scalar Constant has no len()")
        return self._vals.size

    def __float__(self):
        if self._vals is not None:
            raise TypeError("vector-valued Constant used as a scalar")
        return self._v

    def _poly(self):
        if self._vals is not None:
            raise TypeError("vector-valued Constant in a scalar expression: use dot() or index it")
        return [Term(1.0, (), (self,))]

    def __call__(self, *a):
        return self._v


class Grad:
    """grad(f): only meaningful inside inner()/dot()."""

    def __init__(self, f):
        if type(f) is Function and f._V._dg0:
            raise NotImplementedError("grad of a DG0 (cell-wise constant) function")
        if type(f) is Function and f._V._ncomp == 1:
            self.num, self.consts, self.leaf, self.comp = 1.0, (), f, None
            return
        p = _as_poly(f)
        if len(p) != 1 or len(p[0].factors) != 1 or p[0].factors[0].deriv is not None:
            raise NotImplementedError("grad() of anything but a plain function")
        # comp: grad(u[c]) of a vector-valued u keeps its component (inner() writes it out per axis)
        self.num, self.consts, self.leaf, self.comp = p[0].num, p[0].consts, p[0].factors[0].leaf, p[0].factors[0].comp


def grad(f):
    return Grad(f)


nabla_grad = grad


class Indexed(Expr):
    """Component i of a vector-valued Function / Argument."""

    def __init__(self, leaf, i):
        n = leaf._V._ncomp
        if not 0 <= int(i) < n:
            raise IndexError("component %r of a %d-vector" % (i, n))
        self.leaf, self.i = leaf, int(i)

    def _poly(self):
        return [Term(1.0, (Factor(self.leaf, None, None, self.i),))]


class ListTensor:
    """as_vector([...]) / as_matrix([[...]]): a rank-1 or rank-2 array of scalar expressions.  Only the
    algebra the elasticity forms of the reference use: M * v, scalar * T, T + T, inner / dot, indexing."""

    def __init__(self, entries):
        a = np.empty(np.shape(entries), dtype=object)
        if a.ndim not in (1, 2):
            raise NotImplementedError("tensors of rank %d" % a.ndim)
        for idx in np.ndindex(a.shape):
            e = entries[idx[0]] if a.ndim == 1 else entries[idx[0]][idx[1]]
            a[idx] = e if isinstance(e, Expr) else float(e)
        self.a = a

    def ufl_shape(self):
        return self.a.shape

    def __getitem__(self, i):
        r = self.a[i]
        return ListTensor(r) if isinstance(r, np.ndarray) else r

    def __len__(self):
        return self.a.shape[0]

    @staticmethod
    def _mul(x, y):
        if isinstance(x, float) and isinstance(y, float):
            return x * y
        if isinstance(x, float):
            return 0.0 if x == 0.0 else (y if x == 1.0 else x * y)
        if isinstance(y, float):
            return 0.0 if y == 0.0 else (x if y == 1.0 else x * y)
        return x * y

    @staticmethod
    def _add(x, y):
        if isinstance(x, float) and x == 0.0:
            return y
        if isinstance(y, float) and y == 0.0:
            return x
        return x + y

    def __mul__(self, o):
        if isinstance(o, Measure):
            raise TypeError("a tensor-valued integrand: contract it with inner() / dot() first")
        comps = _vector_components(o)
        if comps is not None:
            if self.a.ndim != 2 or self.a.shape[1] != len(comps):
                raise ValueError("shape mismatch in matrix * vector")
            out = []
            for i in range(self.a.shape[0]):
                acc = 0.0
                for k in range(self.a.shape[1]):
                    acc = self._add(acc, self._mul(self.a[i, k], comps[k]))
                out.append(acc)
            return ListTensor(out)
        c = o if isinstance(o, Expr) else float(o)
        out = np.empty(self.a.shape, dtype=object)
        for idx in np.ndindex(self.a.shape):
            out[idx] = self._mul(self.a[idx], c)
        return ListTensor(out.tolist())

    def __rmul__(self, o):
        c = o if isinstance(o, Expr) else float(o)
        out = np.empty(self.a.shape, dtype=object)
        for idx in np.ndindex(self.a.shape):
            out[idx] = self._mul(c, self.a[idx])
        return ListTensor(out.tolist())

    def __add__(self, o):
        b = o.a if isinstance(o, ListTensor) else np.array(_vector_components(o), dtype=object)
        if b.shape != self.a.shape:
            raise ValueError("shape mismatch in tensor sum")
        out = np.empty(self.a.shape, dtype=object)
        for idx in np.ndindex(self.a.shape):
            out[idx] = self._add(self.a[idx], b[idx])
        return ListTensor(out.tolist())

    def __neg__(self):
        return self.__rmul__(-1.0)

    def __sub__(self, o):
        return self + (-1.0) * (o if isinstance(o, ListTensor) else ListTensor(_vector_components(o)))


def as_vector(entries):
    return ListTensor(list(entries))


def as_matrix(entries):
    return ListTensor(np.asarray(entries, dtype=object).tolist())


as_tensor = as_matrix


def _vector_components(o):
    """Components of a vector-valued operand (ListTensor of rank 1, vector Constant, vector-valued
    Function / Argument) or None for scalars."""
    if isinstance(o, ListTensor):
        return list(o.a) if o.a.ndim == 1 else None
    if isinstance(o, Constant) and o._vals is not None:
        return [float(v) for v in o._vals]
    V = getattr(o, "_V", None)
    if V is not None and getattr(V, "_ncomp", 1) > 1 and isinstance(o, (Function, Argument)):
        return [Indexed(o, i) for i in range(V._ncomp)]
    if isinstance(o, (tuple, list, np.ndarray)) and np.ndim(o) == 1:
        return [e if isinstance(e, Expr) else float(e) for e in o]
    return None


def inner(a, b):
    ca, cb = _vector_components(a), _vector_components(b)
    if ca is not None or cb is not None:
        if ca is None or cb is None or len(ca) != len(cb):
            raise ValueError("inner / dot of operands of different shape")
        acc = 0.0
        for x, y in zip(ca, cb):
            acc = ListTensor._add(acc, ListTensor._mul(x, y))
        return acc if isinstance(acc, Expr) else Poly([Term(float(acc), ())])
    if isinstance(a, ListTensor) and isinstance(b, ListTensor):      # rank 2: full contraction
        acc = 0.0
        for idx in np.ndindex(a.a.shape):
            acc = ListTensor._add(acc, ListTensor._mul(a.a[idx], b.a[idx]))
        return acc if isinstance(acc, Expr) else Poly([Term(float(acc), ())])
    if isinstance(a, Grad) and isinstance(b, Grad):
        if a.comp is not None or b.comp is not None:
            # components of vector-valued functions: sum_k u[c]_{,k} v[d]_{,k}, each term an atom in block (d, c)
            if a.comp is None or b.comp is None:
                raise NotImplementedError("inner(grad(u[c]), grad(f)) with f not a component of a vector-valued function")
            gdim = a.leaf._V.mesh().geometry().dim()
            return Poly([Term(a.num * b.num, (Factor(a.leaf, k, None, a.comp), Factor(b.leaf, k, None, b.comp)),
                              a.consts + b.consts) for k in range(gdim)])
        if type(a.leaf) is Function and type(b.leaf) is Function and a.num == 1.0 and b.num == 1.0 and not a.consts and not b.consts:
            return _FastProd(((a.leaf, "grad", b.leaf),))
        return Poly([Term(a.num * b.num, (Factor(a.leaf, "grad", b.leaf),), a.consts + b.consts)])
    if isinstance(a, Grad) or isinstance(b, Grad):
        raise NotImplementedError("inner(grad f, g) with a non-gradient g")
    return Poly(_pmul(_as_poly(a), _as_poly(b)))


dot = inner


class Measure:
    """dx: cell integrals over a whole mesh, or over the cells a cell MeshFunction marks with ``subdomain_id``
    (``dx(1)`` of ``Measure("dx", domain=mesh, subdomain_data=cf)``; data without an id: the whole mesh).  ds:
    exterior-facet integrals, optionally restricted to the facets a MeshFunction marks with ``subdomain_id`` (``ds(2)``)."""

    def __init__(self, kind="dx", domain=None, subdomain_data=None, subdomain_id=None):
        if kind not in ("dx", "ds"):
            raise NotImplementedError("Measure %r: cell integrals dx and exterior-facet integrals ds" % (kind,))
        if kind == "dx":
            subdomain_id = _check_cell_subdomain(domain, subdomain_data, subdomain_id)
        self.kind, self.mesh = kind, domain
        self.subdomain_data, self.subdomain_id = subdomain_data, subdomain_id
        if self.mesh is None and subdomain_data is not None:
            self.mesh = subdomain_data.mesh()

    def __call__(self, *args, **kw):
        mesh, sid = kw.get("domain", self.mesh), kw.get("subdomain_id", self.subdomain_id)
        data = kw.get("subdomain_data", self.subdomain_data)
        for a in args:
            if isinstance(a, Mesh):
                mesh = a
            elif isinstance(a, numbers.Integral):
                sid = int(a)
            elif isinstance(a, (tuple, list, numbers.Real)) and self.kind == "dx":
                sid = a                          # (refused by _check_cell_subdomain)
            elif a is not None:
                raise NotImplementedError("%s(%r)" % (self.kind, a))
        return Measure(self.kind, mesh, data, sid)

    def __rmul__(self, o):
        return Form([(t, self) for t in _as_poly(o)])


def _check_cell_subdomain(domain, data, sid):
    """The subdomain arguments of a dx measure: a cell MeshFunction with integer values of the integration mesh and an
    integer id (or no id: the whole mesh).  Returns the id as an int."""
    if isinstance(sid, (tuple, list)):
        raise NotImplementedError("dx over a tuple of subdomain ids (write one integral per id)")
    if sid is not None:
        if not isinstance(sid, numbers.Integral) or isinstance(sid, bool):
            raise ValueError("dx: the subdomain id must be an integer, got %r" % (sid,))
        if data is None:
            raise ValueError("dx(%r) without subdomain_data (a cell MeshFunction)" % (sid,))
        sid = int(sid)
    if data is not None:
        if not isinstance(data, MeshFunction):
            raise ValueError("dx: subdomain_data must be a cell MeshFunction, got %r" % (type(data).__name__,))
        mesh = data.mesh()
        if data.dim() != mesh.topology().dim():
            raise ValueError("dx: subdomain_data marks entities of dimension %d, not the cells (%d)"
                             % (data.dim(), mesh.topology().dim()))
        if domain is not None and domain is not mesh:
            raise ValueError("dx: subdomain_data belongs to another mesh than the measure's domain")
        if data.array().dtype.kind not in "iu":
            raise ValueError("dx: subdomain_data must hold integer values, not %s" % (data.array().dtype,))
    return sid


dx = Measure("dx")
ds = Measure("ds")


class Form:
    """Sum of (Term, Measure) integrals."""

    def __init__(self, integrals):
        self.integrals = list(integrals)

    def __add__(self, o):
        if isinstance(o, numbers.Real) and o == 0:
            return self
        return Form(self.integrals + o.integrals)

    __radd__ = __add__

    def __neg__(self):
        return Form([(t.scaled(-1.0), m) for t, m in self.integrals])

    def __sub__(self, o):
        if isinstance(o, numbers.Real) and o == 0:
            return self
        return self + (-o)

    def __rsub__(self, o):
        return (-self) + o

    def __mul__(self, c):
        c = _as_float(c)
        return Form([(t.scaled(c), m) for t, m in self.integrals])

    __rmul__ = __mul__

    def __truediv__(self, c):
        return self * (1.0 / _as_float(c))

    def __eq__(self, o):
        return Equation(self, o)

    __hash__ = None

    def mesh(self):
        for t, m in self.integrals:
            if m.mesh is not None:
                return m.mesh
            for f in t.factors:
                V = getattr(f.leaf, "_V", None)
                if V is not None:
                    return V.mesh()
        raise ValueError("cannot determine the integration domain of this form")

    def rank(self):
        first = None
        for t, _ in self.integrals:
            n = 0
            for f in t.factors:
                if isinstance(f.leaf, Argument):
                    n += 1
                if f.deriv == "grad" and isinstance(f.other, Argument):
                    n += 1
            if first is None:
                first = n
            elif n != first:
                raise ValueError("form mixes integrands of different arity: %s" % sorted({first, n}))
        return first or 0


class _FastForm(Form):
    """``_FastProd * dx(mesh)``: a functional of plain Functions.  assemble() takes it from its operands (_fast_scalar);
    the general list of integrals is formed on first use by anything else (sums, scalings, ds integrals)."""

    def __init__(self, fs, measure):
        self.fs, self.measure = fs, measure

    def __getattr__(self, name):
        if name == "integrals":
            v = [(Term(1.0, tuple(Factor(l, d, o) for l, d, o in self.fs)), self.measure)]
            self.integrals = v
            return v
        raise AttributeError(name)

    def rank(self):
        return 0


class Equation:
    def __init__(self, lhs, rhs):
        self.lhs, self.rhs = lhs, rhs


class Argument(Expr):
    def __init__(self, V, number):
        if V._dg0:
            raise NotImplementedError("DG0 trial / test functions: a DG0 space carries coefficients only")
        self._V, self.number = V, number

    def function_space(self):
        return self._V

    def _poly(self):
        if self._V._ncomp > 1:
            raise TypeError("vector-valued argument in a scalar expression: index it (v[i]) or use dot()")
        return [Term(1.0, (Factor(self),))]

    def __getitem__(self, i):
        if self._V._ncomp == 1:
            raise TypeError("scalar argument is not subscriptable")
        return Indexed(self, i)

    def __len__(self):
        if self._V._ncomp == 1:
            raise TypeError("scalar argument has no len()")
        return self._V._ncomp

    def ufl_shape(self):
        return () if self._V._ncomp == 1 else (self._V._ncomp,)


def TestFunction(V):
    return Argument(V, 0)


def TrialFunction(V):
    return Argument(V, 1)


# --------------------------------------------------------------------------- functions
class Function(Expr):
    def __init__(self, V, src=None, name=None):
        if isinstance(V, Function):       # copy constructor
            src, V = V, V._V
        self._V = V
        self._vec = Vector(V)
        self._name = name or "f"
        if isinstance(src, Function):
            self._vec.assign_from(src._vec)
        elif isinstance(src, Vector):
            self._vec.assign_from(src)

    def function_space(self):
        return self._V

    def vector(self):
        return self._vec

    def name(self):
        return self._name

    def rename(self, name, label=None):
        self._name = name

    def ufl_element(self):
        return self._V.ufl_element()

    def compute_vertex_values(self, mesh=None):
        if self._V._dg0:
            raise NotImplementedError("compute_vertex_values of a DG0 function (it has one value per cell, not per vertex)")
        vn = self._V._lay.vertex_nodes
        nc = self._V._ncomp
        if nc > 1:     # dolfin: all vertex values of component 0, then component 1, ...
            a = self._vec.host().reshape(-1, nc)
            return (a if vn is None else a[vn]).T.reshape(-1).copy()
        return self._vec.host().copy() if vn is None else self._vec.host()[vn]

    def __getitem__(self, i):
        if self._V._ncomp == 1:
            raise TypeError("scalar Function is not subscriptable")
        return Indexed(self, i)

    def __len__(self):
        if self._V._ncomp == 1:
            raise TypeError("scalar Function has no len()")
        return self._V._ncomp

    def ufl_shape(self):
        return () if self._V._ncomp == 1 else (self._V._ncomp,)

    def copy(self, deepcopy=False):
        return Function(self._V, self) if deepcopy else self

    def assign(self, other):
        if isinstance(other, Function):
            self._vec.assign_from(other._vec)
        else:
            self._vec._host = interpolate(other, self._V)._vec.host().copy()
            self._vec.touched_host()

    def interpolate(self, other):
        self.assign(other)

    def __mul__(self, o):
        # products of plain scalar (nodal) Functions and their integrals: _FastProd; a DG0 factor takes the general path
        if self._V._ncomp == 1 and not self._V._dg0:
            t = type(o)
            if t is Function:
                if o._V._ncomp == 1 and not o._V._dg0:
                    return _FastProd(((self, None, None), (o, None, None)))
            elif t is _FastProd:
                return _FastProd(((self, None, None),) + o.fs)
            elif t is Measure:
                return _FastForm(((self, None, None),), o)
        return Expr.__mul__(self, o)

    def dx(self, *axes):
        if self._V._dg0:
            raise NotImplementedError("derivative of a DG0 (cell-wise constant) function")
        if self._V._ncomp == 1 and len(axes) == 1:
            return _FastProd(((self, int(axes[0]), None),))
        return Expr.dx(self, *axes)

    def _poly(self):
        if self._V._ncomp > 1:
            raise TypeError("vector-valued Function in a scalar expression: index it (u[i]) or use dot()")
        # (not cached on the Function: the term refers back to it, and a reference cycle would keep iterates - 134 MB of HBM each at
        # 256^3 - alive until the cycle collector runs)
        return [Term(1.0, (Factor(self),))]

    def __call__(self, *x):
        _refuse_dg0(self, "point evaluation")
        if len(x) == 1 and hasattr(x[0], "__len__"):
            x = tuple(x[0])
        return _point_eval(self, np.array([float(v) for v in x]))


def _refuse_dg0(f, what):
    """A DG0 Function is a coefficient of dx integrands and nothing else: say so where anything else is asked of it."""
    if isinstance(f, Function) and f._V._dg0:
        raise NotImplementedError("%s of a DG0 (cell-wise constant) function: it can only multiply a dx integrand" % (what,))


def point_basis(lay, x, grad=False):
    """Nodes of the scalar layout `lay` whose shape functions are non-zero at the point x, their values
    and (grad=True) their gradients there: the cell containing x is found from the barycentric
    coordinates of x in every cell (the mesh's inverse affine maps are cached on the mesh)."""
    mesh = lay.mesh
    x = np.atleast_1d(np.asarray(x, dtype=np.float64))
    X, cells = mesh.coordinates(), mesh.cells()
    D = mesh.topology().dim()
    inv = getattr(mesh, "_affine_inv", None)
    if inv is None:
        P = X[cells]
        T = np.transpose(P[:, 1:, :] - P[:, :1, :], (0, 2, 1))
        inv = (np.linalg.inv(T), P[:, 0, :].copy())
        mesh._affine_inv = inv
    Tinv, P0 = inv
    lam = np.einsum("cij,cj->ci", Tinv, x[None, :] - P0)
    L = np.concatenate([(1.0 - lam.sum(axis=1))[:, None], lam], axis=1)
    k = int(np.argmax(L.min(axis=1)))
    if L[k].min() < -1e-10:
        raise RuntimeError("point %r outside the mesh" % (x,))
    l = L[k]
    g = np.concatenate([-Tinv[k].sum(axis=0)[None, :], Tinv[k]], axis=0)       # grad lambda_i, (D+1) x D
    if lay.degree == 1:
        nodes, N, dN = cells[k], l, g
    else:
        edges = ((0, 1),) if D == 1 else lay.P2_EDGES[D]
        N = np.array([l[i] * (2.0 * l[i] - 1.0) for i in range(D + 1)] + [4.0 * l[a_] * l[b_] for a_, b_ in edges])
        dN = np.array([(4.0 * l[i] - 1.0) * g[i] for i in range(D + 1)] +
                      [4.0 * (l[b_] * g[a_] + l[a_] * g[b_]) for a_, b_ in edges])
        nodes = lay.cells[k]
    return (nodes, N, dN) if grad else (nodes, N)


def _point_eval(f, x):
    V = f._V
    nc = V._ncomp
    base = V._lay.base if nc > 1 else V._lay
    nodes, N = point_basis(base, x)
    vals = f._vec.host()
    if nc > 1:
        return np.array([float(N @ vals[nodes * nc + c]) for c in range(nc)])
    return float(N @ vals[nodes])


def point_gradient(f, x):
    """Gradient of a scalar Function at a point, taken in the cell that contains it (a cell-wise polynomial:
    what projecting the derivative onto DG(degree - 1) gives, model.py:1088-1205)."""
    _refuse_dg0(f, "point gradient")
    V = f._V
    if V._ncomp > 1:
        raise NotImplementedError("gradient of a vector-valued function")
    nodes, N, dN = point_basis(V._lay, x, grad=True)
    return dN.T @ f._vec.host()[nodes]


# ---- point sets: many points located at once (the sensor side of the online phase, model.PGD.evaluate_sensor_response_many)
def affine_inverse(X, cells):
    """(Tinv, P0) of the given cell records: the inverse of the edge matrix T (columns: vertex a + 1 minus vertex 0) and vertex 0 -
    the arithmetic ``point_basis`` caches for the whole mesh, here for any subset of the cells."""
    P = X[cells]
    T = np.transpose(P[:, 1:, :] - P[:, :1, :], (0, 2, 1))
    return np.linalg.inv(T), P[:, 0, :].copy()


def barycentric(Tinv, P0, x):
    """L[p, c, :]: the barycentric coordinates of the points x (P, D) in the cells behind (Tinv, P0), ``point_basis``'s formula."""
    lam = np.einsum("cij,pcj->pci", Tinv, x[:, None, :] - P0[None, :, :])
    return np.concatenate([(1.0 - lam.sum(axis=2))[:, :, None], lam], axis=2)


def shape_functions(lay, lam, g=None):
    """N (P, nodes per cell) of the scalar layout at barycentric coordinates lam (P, D + 1), in the order of the layout's cell
    records; with g (P, D + 1, D), the gradients of the barycentric coordinates, also dN (P, nodes, D).  ``point_basis``'s formulas."""
    D = lam.shape[1] - 1
    if lay.degree == 1:
        return (lam, g) if g is not None else lam
    edges = ((0, 1),) if D == 1 else lay.P2_EDGES[D]
    N = np.stack([lam[:, i] * (2.0 * lam[:, i] - 1.0) for i in range(D + 1)] + [4.0 * lam[:, a] * lam[:, b] for a, b in edges], axis=1)
    if g is None:
        return N
    dN = np.stack([(4.0 * lam[:, i] - 1.0)[:, None] * g[:, i] for i in range(D + 1)] +
                  [4.0 * (lam[:, b, None] * g[:, a] + lam[:, a, None] * g[:, b]) for a, b in edges], axis=1)
    return N, dN


class LocatedPoints:
    """Cells (int32, (P,)) and barycentric coordinates ((P, D + 1)) of a set of points of a mesh; ``handle``: the library's point set
    on ``backend`` where the device located them (None on the host path).  ``key``: the digest the mesh caches it under."""

    def __init__(self, mesh, points, cells, lam, key, backend=None, handle=None, path="host"):
        self.mesh, self.points, self.cells, self.lam, self.key = mesh, points, cells, lam, key
        self.backend, self.handle = backend, handle
        self.path = path      # what located them: "host", or the library's "general", "lattice" or "index" (the same cells and lam)

    def grad_lambda(self):
        """g (P, D + 1, D): the gradients of the barycentric coordinates in the points' cells (rows of Tinv, and minus their sum)."""
        Tinv, _ = affine_inverse(self.mesh.coordinates(), self.mesh.cells()[self.cells])
        return np.concatenate([-Tinv.sum(axis=1)[:, None, :], Tinv], axis=1)

    def device_handle(self, be):
        """The library's point set on ``be``: the one the location made, or one built from the cells and lam (pgd_points_from)."""
        if self.handle is None or self.backend is not be:
            self.free()
            self.backend, self.handle = be, be.points_from(self.mesh.layout(1).handle(), self.cells, self.lam)
        return self.handle

    def free(self):
        if self.handle is not None:
            try:
                self.backend.points_free(self.handle)
            except Exception:
                pass
        self.backend = self.handle = None

    def __del__(self):
        self.free()


_LOCATED_MESHES = weakref.WeakSet()      # meshes that hold located point sets (clear_caches frees their device handles)
SENSOR_CACHES = weakref.WeakSet()        # model.PGD objects that hold sampled modes (PGD.sensor_modes): clear_caches empties their dictionaries
LOCATE_CHUNK_ENTRIES = 1 << 21           # host location: points x cells per chunk (the 96 bytes per cell are per chunk, not per mesh)
# locate_points(index=None) builds the bin index of a mesh from this many points x cells on: the smallest measured size at which
# the FIRST indexed call, build included, beats the general kernel by more than the spread of the rounds, rounded up to a power of
# ten (profiles/locate_index_bench_n1.jsonl: 1.6e10 - 10^4 points on 1.6 M cells, 1.9 ms against 106 ms - is the smallest such size
# measured; the three sizes up to 1.0e10, all with 100 points, lose to the general kernel by the time of the build)
LOCATE_INDEX_MIN_WORK = 1e11
_LOCATE_PATHS = {1: "general", 2: "lattice", 3: "index"}      # pgd_points_last_path


def _locate_host(mesh, pts):
    X, cells = mesh.coordinates(), mesh.cells()
    P, nc = pts.shape[0], cells.shape[0]
    whole = getattr(mesh, "_affine_inv", None)       # point_basis's cache, where somebody has paid for it already
    best = np.full(P, -np.inf)
    where = np.full(P, -1, dtype=np.int64)
    lam = np.zeros((P, X.shape[1] + 1))
    step = max(1, LOCATE_CHUNK_ENTRIES // max(P, 1))
    for c0 in range(0, nc, step):
        c1 = min(nc, c0 + step)
        Tinv, P0 = (whole[0][c0:c1], whole[1][c0:c1]) if whole is not None else affine_inverse(X, cells[c0:c1])
        L = barycentric(Tinv, P0, pts)
        mins = L.min(axis=2)
        k = np.argmax(mins, axis=1)                  # the first of equal minima: the lowest cell, as point_basis's argmax
        m = mins[np.arange(P), k]
        take = m > best                              # strictly: an earlier chunk keeps an equal minimum
        best[take], where[take] = m[take], c0 + k[take]
        lam[take] = L[np.arange(P), k][take]
    return where, lam, best


def locate_points(mesh, points, tol=1e-10, device=None, index=None):
    """The cells and barycentric coordinates of many points of a mesh at once: a ``LocatedPoints``.  The cell of a point is the one
    with the largest smallest barycentric coordinate, the lowest cell among equal ones (``point_basis``'s choice).

    device=None: on the device where the backend locates points (pgd_points_locate on the P1 layout; the set stays there for
    ``points_sample``), else on the host; device=False: on the host - ``point_basis``'s own arithmetic over all points and chunks of
    cells, giving its cells and its lam bit for bit.  A point whose best cell has a barycentric coordinate below -tol (or a NaN
    coordinate) raises ValueError naming the first such point.  Cached on the mesh per (point bytes, tol, path).

    index: whether the device tests a point against the cells of its bin of a uniform grid over the mesh (pgd_points_locate under
    PGD_TUNE_LOCATE_INDEX; built by the first such call and kept with the mesh) instead of against every cell: True / False decide,
    None indexes where the mesh holds an index already or points x cells >= LOCATE_INDEX_MIN_WORK.  The same cells and lam, bit for
    bit, so the cache does not tell the two apart; ``path`` of the result says what ran.  The library uses the index in 2-D and 3-D for
    tol <= 2^-10 where no lattice path applies, and the general kernel elsewhere.  index=True on the host path or on a backend without
    the index is a NotImplementedError."""
    if index is not None and index is not True and index is not False:
        raise ValueError("locate_points: index = %r (True, False or None)" % (index,))
    if getattr(mesh, "part", None) is not None:
        raise NotImplementedError("locate_points on a row-sharded mesh (every rank holds a slab of the cells)")
    D = mesh.geometry().dim()
    pts = np.ascontiguousarray(np.asarray(points, dtype=np.float64).reshape(-1, D))
    tol = float(tol)
    if not (tol >= 0.0 and math.isfinite(tol)):
        raise ValueError("locate_points: tol = %r, a finite tolerance >= 0 is needed" % (tol,))
    be = get_backend()
    on_device = hasattr(be, "points_locate") if device is None else bool(device)
    if on_device and not hasattr(be, "points_locate"):
        raise NotImplementedError("locate_points(device=True): the backend %r locates no points" % (getattr(be, "name", be),))
    can_index = on_device and hasattr(be, "points_index_info")
    if index is True and not can_index:
        raise NotImplementedError("locate_points(index=True): %s" % ("the host path has no index" if not on_device else
                                                                     "the backend %r has no point index" % (getattr(be, "name", be),)))
    key = (hashlib.blake2b(pts.tobytes(), digest_size=16).hexdigest(), pts.shape[0], tol, on_device)
    cache = mesh.__dict__.setdefault("_located", {})
    hit = cache.get(key)
    if hit is not None:
        if not on_device or hit.backend is be:
            return hit
        cache.pop(key).free()                    # located on a backend that is no longer the current one: again, on this one
    handle, path = None, "host"
    if on_device:
        mh = mesh.layout(1).handle()
        if can_index:
            use = index if index is not None else bool(be.points_index_info(mh)["built"]) or pts.shape[0] * mesh.num_cells() >= LOCATE_INDEX_MIN_WORK
            if use:
                held = mesh.__dict__.setdefault("_index_on", [])      # clear_caches drops the index there
                if not any(b is be for b in held):
                    held.append(be)
                _LOCATED_MESHES.add(mesh)
            handle = be.points_locate(mh, pts, tol, index=bool(use))
        else:
            handle = be.points_locate(mh, pts, tol)
        path = _LOCATE_PATHS.get(be.points_last_path(), "general") if hasattr(be, "points_last_path") else "general"
        cells, lam = be.points_download(handle)
        bad = cells < 0
    else:
        cells, lam, best = _locate_host(mesh, pts)
        bad = ~(best >= -tol)
    if bad.any():
        if handle is not None:
            be.points_free(handle)
        i = int(np.argmax(bad))
        raise ValueError("point %d (%r) outside the mesh" % (i, pts[i]))
    out = LocatedPoints(mesh, pts, cells.astype(np.int32), lam, key, be if on_device else None, handle, path)
    cache[key] = out
    _LOCATED_MESHES.add(mesh)
    return out


def gradient_quantity(name, gdim, ncomp):
    """The matrix L (q x ncomp * gdim) of a gradient quantity: the quantity is the Euclidean norm of L g, with
    g[c * gdim + a] = d u_c / d x_a the (cell-wise constant) gradient of a P1 field of ``ncomp`` components.

    "gradient_norm": L is the identity - |grad u| of a scalar field, the Frobenius norm of the gradient of a vector field.
    "von_mises": ncomp == gdim in (2, 3); the rows are sqrt(3 / 2) times s_xx, s_yy, s_zz, sqrt(2) s_xy (, sqrt(2) s_yz,
    sqrt(2) s_xz) of the strain deviator s = eps - tr(eps) / 3 I, in 2-D for plane strain (eps_zz = 0, s_zz = -tr(eps) / 3, as
    problems._voigt_C has it).  The stress deviator is 2 mu s, so the von Mises stress is 2 mu = E / (1 + nu) times the
    quantity: the material enters through the ``scale`` alone, Lame's lambda drops out."""
    gdim, ncomp = int(gdim), int(ncomp)
    if gdim not in (1, 2, 3) or ncomp not in (1, 2, 3):
        raise ValueError("gradient_quantity: gdim and ncomp are 1, 2 or 3, got %r and %r" % (gdim, ncomp))
    qin = gdim * ncomp
    if name == "gradient_norm":
        return np.eye(qin)
    if name == "von_mises":
        if ncomp != gdim or gdim < 2:
            raise ValueError("gradient_quantity: von_mises needs a displacement field, ncomp == gdim in (2, 3), got gdim = %d, "
                             "ncomp = %d" % (gdim, ncomp))
        G = gdim
        eps = np.zeros((3, 3, qin))                   # eps[a, b] as a row over g
        for a in range(G):
            for b in range(G):
                eps[a, b, a * G + b] += 0.5
                eps[a, b, b * G + a] += 0.5
        tr = eps[0, 0] + eps[1, 1] + eps[2, 2]
        rows = [eps[a, a] - tr / 3.0 for a in range(3)]
        rows += [math.sqrt(2.0) * eps[a, b] for a, b in (((0, 1),) if G == 2 else ((0, 1), (1, 2), (0, 2)))]
        return math.sqrt(1.5) * np.array(rows)
    raise ValueError("gradient_quantity: unknown quantity %r ('gradient_norm', 'von_mises')" % (name,))


# What becomes of the rows of L g (pgd_eval_quantity of include/pgd_amd.h): their norm, the one row with its sign, an eigenvalue of the
# symmetric tensor they are
from ._lib import EVAL_Q_EIG_MAX, EVAL_Q_EIG_MIN, EVAL_Q_EIG_SPREAD, EVAL_Q_NORM, EVAL_Q_VALUE      # noqa: E402  (plain integers)
STRESS_QUANTITIES = {"max_principal": EVAL_Q_EIG_MAX, "min_principal": EVAL_Q_EIG_MIN, "tresca": EVAL_Q_EIG_SPREAD,
                     "stress_component": EVAL_Q_VALUE}


def stress_quantity(name, gdim, nu, component=None):
    """(L, kind) of a quantity of the stress tensor of a displacement field (ncomp == gdim in (2, 3)) of an isotropic material with
    Poisson's ratio ``nu`` in (-1, 1/2): the rows of L (q x gdim^2, on g[c * gdim + a] = d u_c / d x_a as ``gradient_quantity``) are
    the components xx, yy, zz, xy (, yz, xz) of sigma / E = eps / (1 + nu) + nu / ((1 + nu) (1 - 2 nu)) tr(eps) I - Lame's lambda
    does not drop out of a principal stress as it does out of the deviator - so Young's modulus is the ``scale``; in 2-D for plane
    strain (eps_zz = 0, sigma_zz = nu (sigma_xx + sigma_yy), no yz and xz).  ``kind`` says what becomes of them:

    "max_principal", "min_principal": the largest / smallest eigenvalue of sigma (EVAL_Q_EIG_MAX / EVAL_Q_EIG_MIN);
    "tresca": their difference, twice the largest shear stress (EVAL_Q_EIG_SPREAD);
    "stress_component": the one row sigma_ab of ``component`` = (a, b) with its sign (EVAL_Q_VALUE); in 2-D a, b in (0, 1), or
    (2, 2) for sigma_zz."""
    gdim = int(gdim)
    if gdim not in (2, 3):
        raise ValueError("stress_quantity: a displacement field in 2 or 3 dimensions, got gdim = %r" % (gdim,))
    if name not in STRESS_QUANTITIES:
        raise ValueError("stress_quantity: unknown quantity %r (%s)" % (name, ", ".join(repr(k) for k in STRESS_QUANTITIES)))
    if nu is None:
        raise ValueError("stress_quantity: %r needs Poisson's ratio nu (Lame's lambda is in the stress)" % (name,))
    nu = float(nu)
    if not -1.0 < nu < 0.5:
        raise ValueError("stress_quantity: nu = %r, Poisson's ratio lies in (-1, 1/2)" % (nu,))
    G = gdim
    eps = np.zeros((3, 3, G * G))                     # eps[a, b] as a row over g
    for a in range(G):
        for b in range(G):
            eps[a, b, a * G + b] += 0.5
            eps[a, b, b * G + a] += 0.5
    tr = eps[0, 0] + eps[1, 1] + eps[2, 2]
    lam = nu / ((1.0 + nu) * (1.0 - 2.0 * nu))
    sig = eps / (1.0 + nu)
    for a in range(3):
        sig[a, a] += lam * tr
    kind = STRESS_QUANTITIES[name]
    if kind == EVAL_Q_VALUE:
        try:
            a, b = (int(i) for i in component)
        except (TypeError, ValueError):
            raise ValueError("stress_quantity: \"stress_component\" needs component=(a, b), got %r" % (component,)) from None
        if not ((0 <= a < G and 0 <= b < G) or (a, b) == (2, 2)):
            raise ValueError("stress_quantity: unknown component %r in %d-D (a, b below %d%s)"
                             % (component, G, G, ", or (2, 2)" if G == 2 else ""))
        return sig[a, b][None, :].copy(), kind
    if component is not None:
        raise ValueError("stress_quantity: component=%r goes with \"stress_component\" only" % (component,))
    planes = ((0, 0), (1, 1), (2, 2), (0, 1)) + (((1, 2), (0, 2)) if G == 3 else ())
    return np.array([sig[a, b] for a, b in planes]), kind


class DerivativeFunction:
    """d f / d x_axis of a scalar Function as a callable of the point."""

    def __init__(self, f, axis=0):
        self.f, self.axis = f, int(axis)

    def function_space(self):
        return self.f.function_space()

    def __call__(self, *x):
        if len(x) == 1 and hasattr(x[0], "__len__"):
            x = tuple(x[0])
        return float(point_gradient(self.f, np.array([float(v) for v in x]))[self.axis])


_EXPR_FUNCS = {
    "pow": np.power, "exp": np.exp, "sqrt": np.sqrt, "sin": np.sin, "cos": np.cos, "tan": np.tan,
    "fabs": np.abs, "abs": np.abs, "log": np.log, "log10": np.log10, "sinh": np.sinh, "cosh": np.cosh,
    "tanh": np.tanh, "atan": np.arctan, "atan2": np.arctan2, "asin": np.arcsin, "acos": np.arccos,
    "floor": np.floor, "ceil": np.ceil, "fmin": np.minimum, "fmax": np.maximum, "min": np.minimum,
    "max": np.maximum, "erf": None, "pi": math.pi, "DOLFIN_PI": math.pi, "DOLFIN_EPS": DOLFIN_EPS,
    "where": np.where, "logical_and": np.logical_and, "logical_or": np.logical_or,
    "logical_not": np.logical_not,
}


def _split_top(s, op):
    """Split s at top-level occurrences of the operator string `op`."""
    out, depth, last, i = [], 0, 0, 0
    while i < len(s):
        c = s[i]
        if c in "([":
            depth += 1
        elif c in ")]":
            depth -= 1
        elif depth == 0 and s.startswith(op, i):
            out.append(s[last:i])
            i += len(op)
            last = i
            continue
        i += 1
    out.append(s[last:])
    return out


def _c_to_py(s):
    """Translate the C++ expression dialect of dolfin.Expression to numpy-evaluable Python."""
    s = s.strip()
    # ternary  c ? a : b  (right-associative, lowest precedence)
    depth = 0
    for i, ch in enumerate(s):
        if ch in "([":
            depth += 1
        elif ch in ")]":
            depth -= 1
        elif ch == "?" and depth == 0:
            cond, rest = s[:i], s[i + 1:]
            d2, nest = 0, 0
            for j, cj in enumerate(rest):
                if cj in "([":
                    d2 += 1
                elif cj in ")]":
                    d2 -= 1
                elif cj == "?" and d2 == 0:
                    nest += 1
                elif cj == ":" and d2 == 0:
                    if nest == 0:
                        return "where(%s, %s, %s)" % (_c_to_py(cond), _c_to_py(rest[:j]), _c_to_py(rest[j + 1:]))
                    nest -= 1
            raise ValueError("malformed ternary in Expression: %r" % s)
    parts = _split_top(s, "||")
    if len(parts) > 1:
        out = _c_to_py(parts[0])
        for p in parts[1:]:
            out = "logical_or(%s, %s)" % (out, _c_to_py(p))
        return out
    parts = _split_top(s, "&&")
    if len(parts) > 1:
        out = _c_to_py(parts[0])
        for p in parts[1:]:
            out = "logical_and(%s, %s)" % (out, _c_to_py(p))
        return out
    # recurse into parenthesised groups / call arguments that may contain the operators above
    if "?" in s or "&&" in s or "||" in s:
        out, i = "", 0
        while i < len(s):
            if s[i] == "(":
                depth, j = 1, i + 1
                while j < len(s) and depth:
                    depth += s[j] == "("
                    depth -= s[j] == ")"
                    j += 1
                inner_s = s[i + 1:j - 1]
                out += "(" + ", ".join(_c_to_py(a) for a in _split_top(inner_s, ",")) + ")"
                i = j
            else:
                out += s[i]
                i += 1
        return out
    return s


class Expression(Expr):
    """dolfin.Expression("C++ string", degree=k, **parameters), scalar valued.

    Used as a form coefficient it is interpolated into the P1 space of the
    integration mesh (exact for the degree <= 1 data of the benchmark configs;
    for higher ``degree`` FFC would integrate a degree-k interpolant instead -
    documented deviation)."""

    def __init__(self, code=None, degree=None, element=None, cell=None, domain=None, name=None, **params):
        object.__setattr__(self, "_params", dict(params))
        self._components = None
        if isinstance(code, (tuple, list)):
            # vector valued: one scalar Expression per component; usable with interpolate() / DirichletBC
            self._components = [Expression(c, degree=degree, **params) for c in code]
            self._code, self._py, self._degree, self._cache = None, None, degree, {}
            return
        self._code = code
        self._py = compile(_c_to_py(code), "<Expression %r>" % (code,), "eval") if code is not None else None
        self._degree = degree
        self._cache = {}

    def __setattr__(self, k, v):
        if k in self.__dict__.get("_params", {}):
            self._params[k] = v
            self._cache.clear()
        else:
            object.__setattr__(self, k, v)

    def __getattr__(self, k):
        p = self.__dict__.get("_params", {})
        if k in p:
            return p[k]
        raise AttributeError(k)

    def _param_values(self):
        out = {}
        for k, v in self._params.items():
            if isinstance(v, Function):
                raise NotImplementedError("Function-valued Expression parameter")
            out[k] = float(v)
        return out

    def is_constant(self):
        if self._components is not None:
            return all(c.is_constant() for c in self._components)
        return "x[" not in self._code

    def eval_at(self, coords):
        """Vectorised evaluation at points (n x gdim) -> (n,)."""
        coords = np.asarray(coords, dtype=np.float64)
        if coords.ndim == 1:
            coords = coords.reshape(1, -1)
        ns = dict(_EXPR_FUNCS)
        ns.update(self._param_values())
        ns["x"] = [coords[:, k] for k in range(coords.shape[1])]
        val = eval(self._py, {"__builtins__": {}}, ns)
        return np.broadcast_to(np.asarray(val, dtype=np.float64), (coords.shape[0],)).copy()

    def __call__(self, *x):
        if len(x) == 1 and hasattr(x[0], "__len__"):
            x = tuple(x[0])
        return float(self.eval_at(np.array([[float(v) for v in x]]))[0])

    def as_function(self, lay):
        key = (id(lay), tuple(sorted(self._param_values().items())))
        f = self._cache.get(key)
        if f is None:
            f = Function(lay.space())
            if lay.degree == 2 and getattr(self, "_degree", 2) == 1:
                # a degree-1 Expression is interpolated into P1 cell by cell (as the form compiler does)
                f._vec._host = lay.embed_p1(self.eval_at(lay.coords[lay.vertex_nodes]))
            else:
                f._vec._host = self.eval_at(lay.coords)
            f._vec.touched_host()
            self._cache = {key: f}
        return f

    def _poly(self):
        if self._components is not None:
            raise TypeError("vector-valued Expression in a scalar expression")
        return [Term(1.0, (Factor(self),))]


def _interpolate_vector(v, V):
    """Nodal interpolation into a vector-valued space (dofs interleaved by component)."""
    f = Function(V)
    nc, base = V._ncomp, V._lay.base
    vals = np.empty((base.n, nc))
    if isinstance(v, Function) and v._V._ncomp == nc:
        if v._V._lay is V._lay:
            f._vec.assign_from(v._vec)
            return f
        vals[:] = np.array([v(x) for x in base.coords])
    elif isinstance(v, Expression) and v._components is not None and len(v._components) == nc:
        for c, e in enumerate(v._components):
            vals[:, c] = e.eval_at(base.coords)
    elif isinstance(v, Expression) and v._components is None:
        vals[:] = v.eval_at(base.coords)[:, None]          # the same scalar in every component
    elif isinstance(v, Constant) and v._vals is not None and v._vals.size == nc:
        vals[:] = v._vals[None, :]
    elif isinstance(v, (Constant, numbers.Real)):
        vals[:] = float(v)
    elif isinstance(v, (tuple, list, np.ndarray)) and len(v) == nc:
        vals[:] = np.asarray(v, dtype=np.float64)[None, :]
    else:
        raise TypeError("cannot interpolate %r into a %d-vector space" % (type(v), nc))
    f._vec._host = vals.reshape(-1)
    f._vec.touched_host()
    return f


def interpolate(v, V):
    if V._ncomp > 1:
        return _interpolate_vector(v, V)
    f = Function(V)
    if isinstance(v, Function):
        if v._V._lay is V._lay:
            f._vec.assign_from(v._vec)
        elif V._dg0 and v._V._ncomp > 1:
            raise NotImplementedError("interpolation of a vector-valued function into a DG0 space")
        else:
            _refuse_dg0(v, "interpolation into another space")
            f._vec._host = np.array([v(x) for x in V._lay.coords])
            f._vec.touched_host()
    elif isinstance(v, Expression):
        if v.is_constant():
            f._vec.fill(v.eval_at(np.zeros((1, V.mesh().geometry().dim())))[0])
        else:
            f._vec._host = v.eval_at(V._lay.coords)
            f._vec.touched_host()
    elif isinstance(v, (Constant, numbers.Real)):
        f._vec.fill(float(v))
    else:
        raise TypeError("cannot interpolate %r" % (type(v),))
    return f


def project(v, V, bcs=None, **kw):
    """L2 projection onto P1.  With P1-interpolated data the projection of the
    interpolant is the interpolant itself."""
    if V._dg0:
        raise NotImplementedError("project onto a DG0 space (interpolate takes the value at the cell midpoint)")
    return interpolate(v, V)


# ----------------------------------------------------------------- boundary conditions
class MeshFunction:
    """dolfin.MeshFunction("size_t", mesh, dim[, value]): one value per mesh entity of dimension `dim`
    (cells, facets or vertices)."""

    def __init__(self, value_type, mesh, dim, value=0):
        tdim = mesh.topology().dim()
        self._mesh, self._dim = mesh, int(dim)
        if self._dim == tdim:
            n = mesh.num_cells()
        elif self._dim == tdim - 1:
            n = mesh.num_facets()
        elif self._dim == 0:
            n = mesh.num_vertices()
        else:
            raise NotImplementedError("MeshFunction over entities of dimension %d of a %d-D mesh" % (self._dim, tdim))
        dt = {"size_t": np.int64, "int": np.int64, "bool": bool, "double": np.float64}[str(value_type)]
        self._a = np.full(n, value, dtype=dt)

    def mesh(self):
        return self._mesh

    def dim(self):
        return self._dim

    def set_all(self, v):
        self._a[:] = v

    def array(self):
        return self._a

    def size(self):
        return self._a.size

    def __getitem__(self, i):
        return self._a[i]

    def __setitem__(self, i, v):
        self._a[i] = v

    def entity_vertices(self):
        """(entity -> vertices, on-boundary flag per entity)."""
        tdim = self._mesh.topology().dim()
        if self._dim == tdim:
            return self._mesh.cells().astype(np.int64), np.zeros(self._mesh.num_cells(), dtype=bool)
        if self._dim == tdim - 1:
            return self._mesh.facets()
        return np.arange(self._mesh.num_vertices()).reshape(-1, 1), self._mesh.vertex_on_boundary()


def _eval_inside(fn, P, onb):
    """inside(x, on_boundary) at the points P (m x gdim): vectorised when the marker allows it, point by
    point (as dolfin calls it) otherwise."""
    try:
        res = np.asarray(fn([P[:, k] for k in range(P.shape[1])], onb))
        if res.shape == (P.shape[0],) and res.dtype == bool:
            return res
    except (ValueError, TypeError):
        pass
    return np.array([bool(fn(P[i], bool(onb[i]))) for i in range(P.shape[0])], dtype=bool)


class SubDomain:
    def inside(self, x, on_boundary):
        raise NotImplementedError

    def mark(self, meshfunction, value, check_midpoint=True):
        """Entities all of whose vertices (and whose midpoint) lie inside get `value` (dolfin's rule;
        ``on_boundary`` is the entity's flag).  Every vertex is evaluated at most once per flag value, and
        midpoints only for the entities whose vertices passed."""
        ent, onb = meshfunction.entity_vertices()
        X = meshfunction.mesh().coordinates()
        ok = np.ones(ent.shape[0], dtype=bool)
        for flag in (True, False):
            sel = np.where(onb == flag)[0]
            if sel.size == 0:
                continue
            verts = np.unique(ent[sel])
            inside_v = np.zeros(X.shape[0], dtype=bool)
            inside_v[verts] = _eval_inside(self.inside, X[verts], np.full(verts.size, flag))
            ok[sel] = inside_v[ent[sel]].all(axis=1)
        if check_midpoint and ent.shape[1] > 1:
            cand = np.where(ok)[0]
            if cand.size:
                ok[cand] = _eval_inside(self.inside, X[ent[cand]].mean(axis=1), onb[cand])
        meshfunction._a[ok] = value


def _eval_marker(marker, lay):
    """Nodes selected by a dolfin-style marker ``f(x, on_boundary)``: vectorised when the marker accepts
    coordinate arrays, otherwise node by node as dolfin does."""
    fn = marker.inside if isinstance(marker, SubDomain) else marker
    return _eval_inside(fn, lay.coords, lay.on_boundary())


def _facet_nodes(lay, facet_ids):
    """Nodes of a scalar layout on the given facets of its mesh: their vertices and, for P2, the nodes of
    their edges."""
    mesh = lay.mesh
    fv = mesh.facets()[0][facet_ids]
    vn = lay.vertex_nodes
    nodes = [fv.ravel() if vn is None else np.asarray(vn)[fv.ravel()]]
    if lay.degree == 2 and fv.shape[1] >= 2:
        nv = mesh.num_vertices()
        ekeys = lay.edge_vertices[:, 0].astype(np.int64) * nv + lay.edge_vertices[:, 1]
        order = np.argsort(ekeys)
        for a in range(fv.shape[1]):
            for b in range(a + 1, fv.shape[1]):
                lo, hi = np.minimum(fv[:, a], fv[:, b]), np.maximum(fv[:, a], fv[:, b])
                if mesh.topology().dim() == 1:
                    continue
                pos = order[np.searchsorted(ekeys[order], lo * nv + hi)]
                nodes.append(np.asarray(lay.edge_nodes)[pos])
    return np.unique(np.concatenate(nodes))


class DirichletBC:
    def __init__(self, V, value, marker, tag=None, method="topological"):
        if V._dg0:
            raise NotImplementedError("DirichletBC on a DG0 space: it carries coefficients only")
        self._V, self._value = V, value
        lay = V._lay
        if isinstance(marker, MeshFunction):
            if tag is None:
                raise TypeError("DirichletBC(V, g, meshfunction, tag): the tag is missing")
            if marker.mesh() is not V.mesh() or marker.dim() != V.mesh().topology().dim() - 1:
                raise ValueError("DirichletBC needs a facet MeshFunction of the space's mesh")
            scalar = lay.base if V._ncomp > 1 else lay
            nodes = _facet_nodes(scalar, np.where(marker.array() == tag)[0])
            if V._ncomp > 1:
                nodes = (nodes[:, None] * V._ncomp + np.arange(V._ncomp)[None, :]).ravel()
            self._vertices = nodes.astype(np.int32)
        else:
            if tag is not None:
                raise TypeError("DirichletBC(V, g, marker): a tag needs a MeshFunction")
            mask = _eval_marker(marker, lay)
            self._vertices = np.where(mask)[0].astype(np.int32)
        self._vals = self._values_at(self._vertices)

    def _values_at(self, verts):
        g, X = self._value, self._V._lay.coords
        nc = self._V._ncomp
        if nc > 1:
            comp = verts % nc
            if isinstance(g, Constant) and g._vals is not None:
                return g._vals[comp].astype(np.float64)
            if isinstance(g, (tuple, list, np.ndarray)):
                return np.asarray(g, dtype=np.float64)[comp]
            if isinstance(g, Expression) and g._components is not None:
                out = np.empty(verts.size)
                for c, e in enumerate(g._components):
                    out[comp == c] = e.eval_at(X[verts[comp == c]])
                return out
            if isinstance(g, Function) and g._V._ncomp == nc:
                return g._vec.host()[verts]
            if isinstance(g, (numbers.Real, Constant)):
                return np.full(verts.size, float(g))
            raise TypeError("unsupported Dirichlet value %r on a vector-valued space" % (type(g),))
        if isinstance(g, (numbers.Real, Constant)):
            return np.full(verts.size, float(g))
        if isinstance(g, Expression):
            return g.eval_at(X[verts])
        if isinstance(g, Function):
            return g._vec.host()[verts]
        raise TypeError("unsupported Dirichlet value %r" % (type(g),))

    def function_space(self):
        return self._V

    def vertices(self):
        return self._vertices

    def vertex_values(self):
        return self._vals

    def get_boundary_values(self):
        inv = vertex_to_dof_map(self._V)
        return {int(inv[v]): float(g) for v, g in zip(self._vertices, self._vals)}

    def homogeneous(self):
        # (asked once per solve; 0.4 ms per look at the 390 152 boundary values of a 256^3 grid)
        h = self.__dict__.get("_homog")
        if h is None or h[0] is not self._vals:
            h = self._homog = (self._vals, not np.any(self._vals))
        return h[1]

    def _sorted_unique(self):
        s = self.__dict__.get("_su")
        if s is None or s[0] is not self._vertices:
            v = self._vertices
            s = self._su = (v, bool(v.dtype == np.int32 and (v.size < 2 or np.all(v[1:] > v[:-1]))))
        return s[1]

    def apply(self, *args):
        for a in args:
            if isinstance(a, Vector):
                if a._small() or not a._dev_ok:
                    h = a.host()
                    h[self._vertices] = self._vals
                    a.touched_host()
                else:
                    get_backend().vec_set(a.dev(), self._vertices, self._vals)
                    a.touched_dev()
            elif isinstance(a, Matrix):
                a.apply_dirichlet(self)
            else:
                raise TypeError("DirichletBC.apply(%r)" % (type(a),))


def _bc_list(bcs):
    if bcs is None or (isinstance(bcs, numbers.Real) and bcs == 0):
        return []
    return list(bcs) if isinstance(bcs, (list, tuple)) else [bcs]


def _bc_vertices(bcs):
    """Merged (vertices, values) of several conditions; later ones win like dolfin."""
    bcs = _bc_list(bcs)
    if not bcs:
        return np.zeros(0, dtype=np.int32), np.zeros(0)
    if len(bcs) == 1:
        return bcs[0].vertices(), bcs[0].vertex_values()
    verts = np.concatenate([bc.vertices() for bc in bcs])
    vals = np.concatenate([bc.vertex_values() for bc in bcs])
    # keep the LAST occurrence of every vertex: unique on the reversed arrays keeps the first it meets
    uniq, first = np.unique(verts[::-1], return_index=True)
    return uniq.astype(np.int32), vals[::-1][first]


# ---------------------------------------------------------------------------- assembly
class _AtomRef:
    """One atom of one mesh with a scalar coefficient; on a vector-valued space the atom sits in the block
    (test component cv, trial component cu)."""
    __slots__ = ("coef", "kind", "da", "db", "weight", "cv", "cu", "cells", "cw")

    def __init__(self, coef, kind, da=0, db=0, weight=None, cv=None, cu=None, cells=None, cw=None):
        self.coef, self.kind, self.da, self.db, self.weight, self.cv, self.cu = coef, kind, da, db, weight, cv, cu
        self.cells = cells           # the _CellSet of a dx(id) integral, None: the whole mesh
        self.cw = cw                 # the vector of a DG0 coefficient of the integrand, None: no cell-wise factor

    def _wkey(self):
        # (the facet set of a DS_MASS atom by its contents: every assemble() of the same ds(tag) builds a new one)
        if self.weight is None:
            return None
        return self.weight.key if self.kind == DS_MASS else id(self.weight)

    def key(self):
        return (self.kind, self.da if self.kind in _DA_KINDS else 0, self.db if self.kind in _DB_KINDS else 0,
                self._wkey(), self.cv or 0, self.cu or 0, self.cells.key if self.cells is not None else None,
                (id(self.cw), self.cw.version) if self.cw is not None else None)

    def transposed_key(self):
        kind = {CONV: CONVT, CONVT: CONV, WCONV: WCONVT, WCONVT: WCONV}.get(self.kind, self.kind)
        k = self.key()
        return (kind, k[2], k[1], k[3], k[5], k[4], k[6], k[7])


def _lay_atom(lay, kind, da, db, w, cv=None, cu=None, cells=None, cw=None):
    """Atom of a layout; on a vector-valued layout in block (cv, cu), a side without a vector-valued factor
    (the all-ones function of a functional) using component 0.  DS_MASS: w is the _FacetSet of the ds measure.
    cells: the _CellSet of a dx(id) measure (None: the whole mesh); cw: the vector of a DG0 coefficient (None: none)."""
    if kind == DS_MASS:
        if isinstance(lay, BlockLayout):
            return lay.facet_atom(w.ids, cv or 0, cu or 0)
        if cv is not None or cu is not None:
            raise ValueError("component of a vector-valued function in an integrand over a scalar space")
        return lay.facet_atom(w.ids)
    if isinstance(lay, BlockLayout):
        return lay.atom(kind, da, db, w, cv or 0, cu or 0, cells=cells, cw=cw)
    if cv is not None or cu is not None:
        raise ValueError("component of a vector-valued function in an integrand over a scalar space")
    return lay.atom(kind, da, db, w, cells=cells, cw=cw)


def _coef_vec(leaf, lay, weight=False):
    """Device-resident nodal representation of a coefficient leaf in the layout of the integral.  weight=True: the leaf
    weights an atom, and on a vector-valued layout it is a scalar field of the base layout (same mesh, same degree)."""
    if weight and isinstance(lay, BlockLayout):
        if isinstance(leaf, Function) and leaf._V._ncomp > 1:
            raise NotImplementedError("vector-valued weight function (write the components' terms out)")
        lay = lay.base
    if isinstance(leaf, Function):
        if leaf._V._lay is not lay:
            if leaf._V.mesh() is not lay.mesh:
                raise ValueError("coefficient lives on a different mesh than the integral")
            raise NotImplementedError("mixing Lagrange degrees in one integrand")
        return leaf._vec
    if isinstance(leaf, Expression):
        return leaf.as_function(lay)._vec
    raise TypeError("unsupported coefficient %r" % (type(leaf),))


def _atom_for(test, trial, weights, lay):
    """Map (test factor, trial factor, extra undifferentiated weights) to an atom."""
    if test.deriv == "grad" or trial.deriv == "grad":
        raise AssertionError("grad factors are handled by the caller")
    if len(weights) > 1:
        raise NotImplementedError("more than one weight function in one integrand")
    if weights and weights[0].deriv is not None:
        raise NotImplementedError("differentiated weight function")
    w = _coef_vec(weights[0].leaf, lay, weight=True) if weights else None
    dt, du = test.deriv, trial.deriv
    if dt is None and du is None:
        return (WMASS, 0, 0, w) if w is not None else (MASS, 0, 0, None)
    if w is not None:
        if dt is not None and du is not None:
            return (WSTIFF, 0, 0, w) if lay.mesh.topology().dim() == 1 else (WDUDV, du, dt, w)
        return (WCONV, du, 0, w) if du is not None else (WCONVT, 0, dt, w)
    if dt is not None and du is not None:
        return (DUDV, du, dt, None)
    if du is not None:
        return (CONV, du, 0, None)
    return (CONVT, 0, dt, None)


def _weight_last(plain, lay):
    """Order undifferentiated coefficients so that the one best suited as the atom's weight comes last:
    an Expression (fixed data) before anything else, then the vector that changes least often."""
    def key(c):
        # ties (equally "old" vectors): the factor that occurs once in the integrand is the weight, the repeated one
        # (F * F) the function the functional is evaluated on.  On a vector-valued layout only a scalar field can weight.
        scalar = not isinstance(lay, BlockLayout) or isinstance(c.leaf, Expression) or c.leaf._V._ncomp == 1
        return (1 if scalar else 0, 1 if isinstance(c.leaf, Expression) else 0, -_coef_vec(c.leaf, lay, weight=scalar).version,
                -sum(1 for o in plain if o.leaf is c.leaf))
    return sorted(plain, key=key)


def _classify(term, lay):
    """Split a Term into (test factor, trial factor, coefficient factors, graddot factor)."""
    test = trial = gd = None
    coefs = []
    for f in term.factors:
        if f.deriv == "grad":
            if gd is not None:
                raise NotImplementedError("two inner(grad, grad) factors in one integrand")
            gd = f
        elif isinstance(f.leaf, Argument):
            if f.leaf.number == 0:
                if test is not None:
                    raise ValueError("two test functions in one integrand")
                test = f
            else:
                if trial is not None:
                    raise ValueError("two trial functions in one integrand")
                trial = f
        else:
            coefs.append(f)
    return test, trial, coefs, gd


_SCALAR_MEMO = {}
_SCALAR_MEMO_MAX = 65536


def _memo_make_room(extra=1):
    """Called before inserting: when the memo is full, drop what can never hit again - entries whose vectors have died or
    moved on to another version (the iterates of earlier passes) - and, if that is not enough, the oldest half.  Never
    everything: with 50 stored modes in four dimensions one pass asks for ~1200 functionals, most of them several times,
    and a wholesale clear() in mid-pass had every one of them recomputed on the device (cfg5: 0.66 s per pass at mode 50)."""
    if len(_SCALAR_MEMO) + extra <= _SCALAR_MEMO_MAX:
        return
    dead = []
    for key, (_val, wf, wg) in _SCALAR_MEMO.items():
        f, g = wf(), wg()
        if f is None or g is None or f.version != key[2] or g.version != key[4]:
            dead.append(key)
    for key in dead:
        del _SCALAR_MEMO[key]
    if len(_SCALAR_MEMO) + extra > (3 * _SCALAR_MEMO_MAX) // 4:       # still three quarters full of live entries: the oldest go, down to half
        for key in list(_SCALAR_MEMO)[:len(_SCALAR_MEMO) + extra - _SCALAR_MEMO_MAX // 2]:
            del _SCALAR_MEMO[key]
_MV_CACHE = {}        # (atom handle, id(vec)) -> (version, result Vector)   A @ g for immutable g


def _purge_atom(atom):
    for k in [k for k, p in _FAST_PLANS.items() if p[1] == atom]:
        del _FAST_PLANS[k]
    for k in [k for k in _MV_CACHE if k[0] == atom]:
        del _MV_CACHE[k]
    for k in [k for k in _SCALAR_MEMO if k[0] == atom]:
        del _SCALAR_MEMO[k]
    for tag, plan in list(_FUNCTIONAL_PLANS.items()):
        if any(e[1] == atom for e in plan):
            _FUNCTIONAL_PLANS[tag] = [e for e in plan if e[1] != atom]


def _matvec_cached(lay, atom, g):
    """A g as a Vector; cached while g is unchanged (stored modes and loads never change)."""
    key = (atom, id(g))
    hit = _MV_CACHE.get(key)
    if hit is not None and hit[0] == g.version and hit[2]() is g:
        return hit[1]
    be = get_backend()
    out = Vector(g.V)
    _halo(lay, g)
    lo, hi = lay.owned_range()
    be.spmv(atom, g.dev(), out.dev_for_write(), lo, hi)
    out.touched_dev()
    if len(_MV_CACHE) > 4096:
        _MV_CACHE.clear()
    # g is held WEAKLY: the cache must not keep an iterate (134 MB of HBM at 256^3) alive, and the product goes with it
    _MV_CACHE[key] = (g.version, out, weakref.ref(g, lambda _r, key=key: _MV_CACHE.pop(key, None)))
    return out


def _halo(lay, vec):
    if lay.part is not None:
        lay.part.comm.halo_exchange(lay.shard_view(), vec)


_SYMMETRIC_KINDS = (MASS, STIFF, WMASS, WSTIFF)


def _cached_product(atom, v):
    hit = _MV_CACHE.get((atom, id(v)))
    if hit is not None and hit[0] == v.version and hit[2]() is v:
        return hit[1]
    return None


KEEP_FUNCTIONAL_PRODUCTS = os.environ.get("PGD_KEEP_FUNCTIONAL_PRODUCTS", "1") != "0"      # 0: fused product-dot per functional (A/B)
_MULTIDOT_MAX = max(1, min(256, int(os.environ.get("PGD_BATCH_FUNCTIONALS", "256"))))   # 1: one dot per request (A/B)


def _dots_with_stored_products(be, atom, other, Ag, swapped, lo, hi, lay=None):
    """other . Ag, and in the same device pass other . (A v) for every other stored product of this atom.

    The driver asks for the functionals of one iterate against ALL stored modes of its dimension, one
    assemble() at a time (solver.py:568-612), and each answer costs a host synchronisation; the products A v
    of the stored modes are cached by the right-hand-side assembly, so the first request computes all of them
    in one launch sequence with one synchronisation and memoises the rest (same keys _bilinear_scalar looks up).

    Row-sharded dimension (``lay.part``): the local dots of the whole batch travel in ONE all-reduce of fixed length
    instead of one collective per functional.  The ranks run the same program on the same cache history, so they
    hold the same candidate list; the message still carries (count, count^2) so that every rank sees - from the same
    all-reduced numbers - whether all counts were equal (world * sum count^2 == (sum count)^2), and if they were not
    all of them fall back to the single all-reduced dot together."""
    part = lay.part if lay is not None else None
    outs, keys, refs = [Ag], [None], [None]
    oid, over = id(other), other.version
    for (a, _vid), (ver, out, ref) in _MV_CACHE.items():
        if a != atom or out is Ag:
            continue
        v = ref()
        if v is None or v.version != ver or v is other:
            continue
        key = (atom, id(v), ver, oid, over) if swapped else (atom, oid, over, id(v), ver)
        if key in _SCALAR_MEMO:
            continue
        outs.append(out)
        keys.append(key)
        refs.append(v)
        if len(outs) == _MULTIDOT_MAX:
            break
    if part is None:
        if len(outs) == 1:
            return be.vec_dot(other.dev(), Ag.dev(), lo, hi)
        vals = be.vec_multidot(other.dev(), [o.dev() for o in outs], lo, hi)
    else:
        if _MULTIDOT_MAX == 1:
            return part.comm.allreduce_sum(be.vec_dot(other.dev(), Ag.dev(), lo, hi))
        k = len(outs)
        local = be.vec_multidot(other.dev(), [o.dev() for o in outs], lo, hi) if k > 1 else \
            np.array([be.vec_dot(other.dev(), Ag.dev(), lo, hi)])
        msg = np.zeros(_MULTIDOT_MAX + 2)
        msg[0], msg[1], msg[2:2 + k] = k, k * k, local
        msg = part.comm.allreduce_array(msg)
        world = part.comm.world
        if world * msg[1] != msg[0] * msg[0]:          # the ranks' candidate lists differ in length: the one dot, together
            LOG.warning("batched functionals: the ranks hold different product caches; single dot")
            return part.comm.allreduce_sum(float(local[0]))
        vals = msg[2:2 + k]
        if k == 1:
            return float(vals[0])
    _memo_make_room(len(outs))
    wo = weakref.ref(other)
    for key, v, val in zip(keys[1:], refs[1:], vals[1:]):
        wv = weakref.ref(v)
        _SCALAR_MEMO[key] = (float(val), wv, wo) if swapped else (float(val), wo, wv)
    return float(vals[0])


# ---- learned prefetch of the functionals of one call site -----------------------------------------------------------
# A user callback asks for its functionals one assemble() at a time and uses each answer on the spot (solver.py:547-612):
# every answer on a large or row-sharded dimension is a device pass + a host synchronisation (+ an all-reduce across the
# ranks).  Which functionals a call site asks for hardly changes from pass to pass - the same atoms, the current iterates
# of the other dimensions, the stored modes, the loads - so a call site RECORDS its requests (functional_scope) and the next
# time it is entered they are computed ahead of the callback in one batch: the missing products, one multi-dot per left
# factor, ONE host synchronisation and ONE fixed-length all-reduce; the callback's assemble() calls then find their values
# in the memo.  Nothing depends on the guess being right: a request that was not prefetched takes the ordinary path.
PREFETCH_FUNCTIONALS = os.environ.get("PGD_PREFETCH_FUNCTIONALS", "1") != "0"
PAIR_FUNCTIONALS = os.environ.get("PGD_PAIR_FUNCTIONALS", "1") != "0"        # 0: one left factor per multi-dot (A/B)
_PREFETCH_MAX = 510                      # values per batch (the all-reduced message has a fixed length)
_FUNCTIONAL_PLANS = {}                   # call-site tag -> [(lay, atom, f_ref, g_ref, symmetric)]
_RECORDING = None
STATS_PREFETCH = {"batches": 0, "values": 0, "requests": 0, "hits": 0}


def drop_functional_plans(scope_id):
    """Forget the plans of the call sites tagged (.., scope_id, ..): their problem has died (solver.PGDProblem)."""
    for tag in [t for t in _FUNCTIONAL_PLANS if isinstance(t, tuple) and len(t) > 1 and t[1] == scope_id]:
        _FUNCTIONAL_PLANS.pop(tag, None)


class functional_scope:
    """``with functional_scope(tag, iterates):`` around the evaluation of a call site's functionals.  `iterates`: the vectors
    that change from call to call (the current factors of all dimensions), in an order that is the same every time; every
    other vector of a request is taken to be immutable (a stored mode, a load) and referenced weakly."""

    def __init__(self, tag, iterates):
        self.tag, self.iterates = tag, list(iterates)
        self.roles = {id(v): k for k, v in enumerate(self.iterates)}      # (_fast_scalar: an iterate is named by its position)

    def _ref(self, v):
        k = self.roles.get(id(v))
        if k is not None:
            return ("it", k)
        return ("obj", weakref.ref(v), v.version)

    def _deref(self, ref):
        if ref[0] == "it":
            return self.iterates[ref[1]] if ref[1] < len(self.iterates) else None
        v = ref[1]()
        return v if v is not None and v.version == ref[2] else None

    def note(self, lay, atom, f, g, symmetric):
        self.seen.append((lay, atom, self._ref(f), self._ref(g), symmetric))

    def __enter__(self):
        global _RECORDING
        self.outer, self.seen = _RECORDING, []
        if PREFETCH_FUNCTIONALS:
            plan = _FUNCTIONAL_PLANS.get(self.tag)
            if plan:
                # A row-sharded layout takes part in ONE fixed-length all-reduce per entry of the scope.  Whether a rank issues it
                # must not depend on anything rank-local (memo hits, weak references that died, what the product caches hold:
                # ADVICE r03) - it depends on the recorded plan alone, which every rank records from the same sequence of
                # assemble() calls: a layout's requests are numbered by their position in the plan (the SLOT of the message
                # a value travels in), and the collective is issued whenever the plan names 2 ... _PREFETCH_MAX of them.
                reqs, slots = [], {}
                for lay, atom, fr, gr, sym in plan:
                    slot = None
                    if lay.part is not None:
                        ent = slots.setdefault(id(lay), [lay, 0])
                        slot, ent[1] = ent[1], ent[1] + 1
                    f, g = self._deref(fr), self._deref(gr)
                    if f is not None and g is not None:
                        reqs.append((lay, atom, f, g, sym, slot))
                _prefetch_functionals(reqs, [tuple(e) for e in slots.values()])
            _RECORDING = self
        return self

    def __exit__(self, *exc):
        global _RECORDING
        if PREFETCH_FUNCTIONALS:
            _RECORDING = self.outer
            if exc[0] is None:
                _FUNCTIONAL_PLANS[self.tag] = self.seen
        return False


def _prefetch_functionals(reqs, sharded_plan=()):
    """`reqs`: (layout, atom, f, g, symmetric, slot) of the requests to compute ahead; `sharded_plan`: (layout, number of
    requests the PLAN holds for it) of every row-sharded layout of the plan, in plan order - the same on every rank."""
    be = get_backend()
    todo = {}
    for lay, n_slots in sharded_plan:
        if 2 <= n_slots <= _PREFETCH_MAX:
            todo[id(lay)] = (lay, [])                    # takes part in the collective even with nothing to bring
    for lay, atom, f, g, sym, slot in reqs:
        if lay.part is not None and id(lay) not in todo:
            continue                                     # (a plan with 1 or too many requests on this layout: no batch, on any rank)
        key = (atom, id(f), f.version, id(g), g.version)
        hit = _SCALAR_MEMO.get(key)
        if hit is not None and hit[1]() is f and hit[2]() is g:
            continue
        if lay.part is None and g._small():
            continue                                     # host arithmetic: nothing to batch
        # f^T A g as a dot of one factor with the stored product of the other: either way round where A is symmetric and both
        # products are kept.  Which way is decided below, per layout: the way that shares its left factor with the most requests
        # (stored modes against the iterate: ONE multi-dot with the iterate on the left, not one per stored mode)
        ways = []
        Ag = _cached_product(atom, g)
        if Ag is not None:
            ways.append((f, Ag))
        if sym and f is not g:
            Af = _cached_product(atom, f)
            if Af is not None:
                ways.append((g, Af))
        if not ways:
            if lay.part is None and not (KEEP_FUNCTIONAL_PRODUCTS and be.atom_product_form(atom) > 0):
                continue                                 # the fused product-dot over the CSR atom stays the cheaper way
            ways.append((f, _matvec_cached(lay, atom, g)))
        todo.setdefault(id(lay), (lay, []))[1].append((key, f, g, ways, slot))
    for lay, requests in todo.values():
        if lay.part is None and (len(requests) < 2 or len(requests) > _PREFETCH_MAX):
            continue
        lo, hi = lay.owned_range()
        vals, order = [], []
        # Two PRODUCTS that many requests can take as their left factor - K F and M F of the iterate F, against the stored modes
        # m_j - go through ONE pass that reads every m_j once for both (pgd_vec_multidot_pair): 2 + k vector reads for 2 k
        # functionals, where F . (K m_j), F . (M m_j) read a stored product per mode and atom.  Taken where it reads less.
        if PAIR_FUNCTIONALS and hasattr(be, "vec_multidot_pair"):
            by_prod = {}
            for rq in requests:
                for other, prod in rq[3]:
                    by_prod.setdefault(id(prod), (prod, []))[1].append((rq, other))
            cands = sorted((e for e in by_prod.values() if len(e[1]) >= 2), key=lambda e: -len(e[1]))
            while len(cands) >= 2:
                (p0, c0), (p1, c1) = cands[0], cands[1]
                cands = cands[2:]
                done = {id(it[0]) for it in order}
                rights, covered = {}, []
                for left, cs in ((0, c0), (1, c1)):
                    for rq, other in cs:
                        if id(rq[0]) in done:
                            continue
                        done.add(id(rq[0]))
                        rights.setdefault(id(other), other)
                        covered.append((rq, left, other))
                rl = list(rights.values())
                if len(rl) > 128 or 2 + len(rl) >= len(covered):
                    continue
                a = be.vec_multidot_pair(p0.dev(), p1.dev(), [r.dev() for r in rl], lo, hi)
                pos = {id(r): i for i, r in enumerate(rl)}
                for rq, left, other in covered:
                    vals.append(float(a[left][pos[id(other)]]))
                    order.append((rq[0], rq[1], rq[2], other, None, rq[4]))
                STATS_PREFETCH["pair_values"] = STATS_PREFETCH.get("pair_values", 0) + len(covered)
            if order:
                taken = {id(it[0]) for it in order}
                requests = [rq for rq in requests if id(rq[0]) not in taken]
        shared = {}
        for _key, _f, _g, ways, _slot in requests:
            for other, _prod in ways:
                shared[id(other)] = shared.get(id(other), 0) + 1
        items = []
        for key, f, g, ways, slot in requests:
            other, prod = max(ways, key=lambda w: shared[id(w[0])])      # (ties: the first way, as before)
            items.append((key, f, g, other, prod, slot))
        groups = {}
        for it in items:
            groups.setdefault(id(it[3]), (it[3], []))[1].append(it)
        for other, its in groups.values():
            outs = [it[4].dev() for it in its]
            local = be.vec_multidot(other.dev(), outs, lo, hi) if len(outs) > 1 else [be.vec_dot(other.dev(), outs[0], lo, hi)]
            vals.extend(float(v) for v in local)
            order.extend(its)
        if lay.part is not None:
            # a value travels in the slot of its request's position in the plan, its presence count in the second half: a
            # functional is kept only where EVERY rank has brought its share (a rank whose memo already holds one, or whose
            # weak reference has died, brings nothing for that slot - on any rank the ordinary path then answers the request)
            msg = np.zeros(2 * _PREFETCH_MAX)
            for it, val in zip(order, vals):
                msg[it[5]] += val
                msg[_PREFETCH_MAX + it[5]] += 1.0
            msg = lay.part.comm.allreduce_array(msg)
            world = float(lay.part.comm.world)
            kept = [(it, msg[it[5]]) for it in order if msg[_PREFETCH_MAX + it[5]] == world]
            if len(kept) != len(order):
                LOG.debug("prefetched functionals: %d of %d values not brought by every rank; ordinary path for those",
                          len(order) - len(kept), len(order))
            order, vals = [it for it, _ in kept], [v for _, v in kept]
            if not order:
                continue
        _memo_make_room(len(order))
        for (key, f, g, _o, _a, _s), val in zip(order, vals):
            _SCALAR_MEMO[key] = (float(val), weakref.ref(f), weakref.ref(g))
        STATS_PREFETCH["batches"] += 1
        STATS_PREFETCH["values"] += len(order)


def _bilinear_scalar(lay, atom, f, g, symmetric=False):
    """f^T A g with memoisation on (atom, vector identity, vector version).

    When A g (or, for a symmetric atom, A f) is already cached - stored modes and loads never
    change, and the right-hand-side assembly has multiplied them once - the functional is a dot
    product (2 vector reads) instead of a pass over the matrix."""
    key = (atom, id(f), f.version, id(g), g.version)
    if _RECORDING is not None:
        _RECORDING.note(lay, atom, f, g, symmetric)
        STATS_PREFETCH["requests"] += 1
    hit = _SCALAR_MEMO.get(key)
    if hit is not None and hit[1]() is f and hit[2]() is g:
        if _RECORDING is not None:
            STATS_PREFETCH["hits"] += 1
        return hit[0]
    be = get_backend()
    lo, hi = lay.owned_range()
    Ag = _cached_product(atom, g)
    other, swapped = f, False
    if Ag is None and symmetric and f is not g:
        Ag, other, swapped = _cached_product(atom, f), g, True
    if Ag is not None and (lay.part is not None or not Ag._small()):
        val = _dots_with_stored_products(be, atom, other, Ag, swapped, lo, hi, lay)
    elif Ag is not None:
        val = float(other.host() @ Ag.host())
    elif lay.part is None and KEEP_FUNCTIONAL_PRODUCTS and not g._small() and be.atom_product_form(atom) > 0:
        # the atom has its diagonal form (a structured grid; mass and stiffness of a uniform one: a code byte per row): product
        # + dot move 17 + 16 bytes per row where the fused product-dot over the CSR atom moves 200, and the product stays for
        # the next functional with this g (the norms and the stop test of solver.py:754, 836-842 ask for the same M F twice)
        Ag = _matvec_cached(lay, atom, g)
        val = be.vec_dot(f.dev(), Ag.dev(), lo, hi)
    else:
        _halo(lay, g)
        val = _allreduce_sum(lay.mesh, be.bilinear(atom, f.dev(), g.dev(), lo, hi))
    _memo_make_room()
    _SCALAR_MEMO[key] = (val, weakref.ref(f), weakref.ref(g))       # weak: a memoised scalar pins no vector
    return val


def _ones(lay):
    if lay._ones is None:
        v = Vector(lay.space(), np.ones(lay.n))
        lay._ones = v
    return lay._ones


def _term_operands(term, lay, cells=None, cw=None):
    """(atom, f, g, symmetric) with  integral of the term = coef * f^T A g  for a term without arguments (over the cells of
    a dx(id) measure: `cells`; with the DG0 coefficient `cw`, already split off the term by _cellwise)."""
    test, trial, coefs, gd = _classify(term, lay)
    if test is not None or trial is not None:
        raise ValueError("scalar assemble of a form with arguments")
    if gd is not None:
        if isinstance(gd.leaf, Argument) or isinstance(gd.other, Argument):
            raise ValueError("scalar assemble of a form with arguments")
        if len(coefs) > 1:
            raise NotImplementedError("weighted inner(grad, grad) functional with several weights")
        f, g = _coef_vec(gd.leaf, lay), _coef_vec(gd.other, lay)
        if coefs:
            atom = lay.atom(WSTIFF, 0, 0, _coef_vec(coefs[0].leaf, lay), cells=cells, cw=cw)
        else:
            atom = lay.atom(STIFF, cells=cells, cw=cw)
        return atom, f, g, True
    if len(coefs) == 0:
        one = _ones(lay)
        return _lay_atom(lay, MASS, 0, 0, None, cells=cells, cw=cw), one, one, False
    if len(coefs) == 1:
        c = coefs[0]
        kind, da, db, w = _atom_for(Factor(None, None), Factor(None, c.deriv), [], lay)
        return _lay_atom(lay, kind, da, db, w, None, c.comp, cells, cw), _ones(lay), _coef_vec(c.leaf, lay), False
    # f (test side) is the first factor, g (trial side) the second, further undifferentiated ones weight
    der = [c for c in coefs if c.deriv is not None]
    plain = [c for c in coefs if c.deriv is None]
    if len(der) > 2:
        raise NotImplementedError("more than two differentiated factors in a functional")
    if len(der) + len(plain) > 2:
        plain = _weight_last(plain, lay)
    ordered = der + plain
    f, g, rest = ordered[0], ordered[1], ordered[2:]
    kind, da, db, w = _atom_for(Factor(None, f.deriv), Factor(None, g.deriv), rest, lay)
    return (_lay_atom(lay, kind, da, db, w, f.comp, g.comp, cells, cw), _coef_vec(f.leaf, lay), _coef_vec(g.leaf, lay),
            (kind in _SYMMETRIC_KINDS or (kind in (DUDV, WDUDV) and da == db)) and f.comp == g.comp)


def _term_scalar(term, lay, cells=None, cw=None):
    atom, f, g, symmetric = _term_operands(term, lay, cells, cw)
    return term.coef * _bilinear_scalar(lay, atom, f, g, symmetric=symmetric)


# ---- functionals of plain Functions (_FastForm): the structure of a request is resolved once ------------------------------
# What _term_operands works out for a functional - layout, atom, which operand stands on which side - depends on WHICH
# vectors the integrand names and how, not on their values.  A request names its vectors by role: the iterates of the
# enclosing functional_scope by their position (they are new objects after every solve, solver.py:746), every other vector -
# stored modes, loads, weights: long-lived - by identity.  The plan of a structure is kept with weak references to those
# long-lived vectors (an address is reused once a vector has died) and, for a weighted atom, the version of the weight the
# atom was assembled from; the value itself goes through _bilinear_scalar and its memo as before.
_FAST_PLANS = {}
_FAST_PLANS_MAX = 65536
STATS_FAST = {"requests": 0, "planned": 0}


def _fast_scalar(form):
    fs, mesh = form.fs, form.measure.mesh
    scope = _RECORDING
    roles = scope.roles if scope is not None else {}
    vecs = []
    key = [id(_backend), id(mesh)]
    for l, d, o in fs:
        v = l._vec
        vecs.append(v)
        key.append(roles.get(id(v), id(v)))
        key.append(d)
        if o is not None:
            v = o._vec
            vecs.append(v)
            key.append(roles.get(id(v), id(v)))
    key = tuple(key)
    STATS_FAST["requests"] += 1
    plan = _FAST_PLANS.get(key)
    if plan is not None:
        lref, atom, fi, gi, sym, refs, wi, wver, mref = plan
        lay = lref()
        ok = mref() is mesh and lay is not None
        if ok:
            for r, v in zip(refs, vecs):
                if (r is not None and r() is not v) or v.V._lay is not lay:
                    ok = False
                    break
        if ok and wi >= 0:
            w = vecs[wi]
            ok = w.version == wver and w.version < vecs[fi].version and w.version < vecs[gi].version
        if ok:
            STATS_FAST["planned"] += 1
            return _bilinear_scalar(lay, atom, vecs[fi] if fi >= 0 else _ones(lay), vecs[gi] if gi >= 0 else _ones(lay), sym)
        del _FAST_PLANS[key]
    term = Term(1.0, tuple(Factor(l, d, o) for l, d, o in fs))
    m = mesh if mesh is not None else Form([(term, form.measure)]).mesh()
    lay = _integral_layout(term, m)
    atom, f, g, sym = _term_operands(term, lay)
    # keep the plan where every operand of the atom's product is one of the named vectors (or the layout's vector of ones)
    # and a weight - the one vector that is neither side - is a long-lived vector, strictly older than both sides (which
    # of three undifferentiated factors weights the other two is decided by their versions: _weight_last)
    ones = lay._ones
    fi = next((i for i, v in enumerate(vecs) if v is f), -1)
    gi = next((i for i, v in enumerate(vecs) if v is g and i != fi), -1)
    rest = [i for i in range(len(vecs)) if i != fi and i != gi]
    plannable = mesh is not None and (fi >= 0 or f is ones) and (gi >= 0 or g is ones) and len(rest) <= 1
    wi, wver = -1, 0
    if plannable and rest:
        wi = rest[0]
        w = vecs[wi]
        wver = w.version
        plannable = (fi >= 0 and gi >= 0 and id(w) not in roles and w.version < vecs[fi].version and w.version < vecs[gi].version)
    if plannable:
        if len(_FAST_PLANS) >= _FAST_PLANS_MAX:
            _FAST_PLANS.clear()
        refs = tuple(None if id(v) in roles else weakref.ref(v) for v in vecs)
        _FAST_PLANS[key] = (weakref.ref(lay), atom, fi, gi, sym, refs, wi, wver, weakref.ref(mesh))
    return _bilinear_scalar(lay, atom, f, g, symmetric=sym)


def _term_vector(term, lay, cells=None, cw=None):
    """(coef, atom handle, coefficient Vector g) with  b += coef * A g  (A over the cells of a dx(id) measure: `cells`, with
    the DG0 coefficient `cw`)."""
    test, trial, coefs, gd = _classify(term, lay)
    if trial is not None:
        raise ValueError("linear form with a trial function")
    if gd is not None:
        a, b = gd.leaf, gd.other
        if isinstance(b, Argument):
            a, b = b, a
        if not isinstance(a, Argument) or a.number != 0 or isinstance(b, Argument):
            raise ValueError("linear form: inner(grad, grad) needs exactly one test function")
        if test is not None:
            raise ValueError("two test functions in one integrand")
        if len(coefs) > 1:
            raise NotImplementedError("several weights on inner(grad, grad)")
        atom = (lay.atom(WSTIFF, 0, 0, _coef_vec(coefs[0].leaf, lay), cells=cells, cw=cw) if coefs
                else lay.atom(STIFF, cells=cells, cw=cw))
        return term.coef, atom, _coef_vec(b, lay)
    if test is None:
        raise ValueError("linear form without a test function")
    if not coefs:
        return term.coef, _lay_atom(lay, MASS, 0, 0, None, test.comp, None, cells, cw), _ones(lay)
    der = [c for c in coefs if c.deriv is not None]
    plain = [c for c in coefs if c.deriv is None]
    if len(der) > 1:
        raise NotImplementedError("two differentiated coefficients in a linear form")
    if len(der) + len(plain) > 1:
        # w g v is symmetric in (w, g): weight the atom with fixed data / the coefficient that changes less often
        plain = _weight_last(plain, lay)
    ordered = der + plain
    g, rest = ordered[0], ordered[1:]
    kind, da, db, w = _atom_for(test, Factor(None, g.deriv), rest, lay)
    return term.coef, _lay_atom(lay, kind, da, db, w, test.comp, g.comp, cells, cw), _coef_vec(g.leaf, lay)


def _term_matrix(term, lay, cells=None, cw=None):
    test, trial, coefs, gd = _classify(term, lay)
    if gd is not None:
        a, b = gd.leaf, gd.other
        if not (isinstance(a, Argument) and isinstance(b, Argument) and {a.number, b.number} == {0, 1}):
            raise ValueError("bilinear form: inner(grad, grad) needs the trial and the test function")
        if test is not None or trial is not None:
            raise ValueError("too many arguments in one integrand")
        if len(coefs) > 1 or (coefs and coefs[0].deriv is not None):
            raise NotImplementedError("several / differentiated weights on inner(grad, grad)")
        w = _coef_vec(coefs[0].leaf, lay) if coefs else None
        return _AtomRef(term.coef, WSTIFF if w is not None else STIFF, 0, 0, w, cells=cells, cw=cw)
    if test is None or trial is None:
        raise ValueError("bilinear form needs a trial and a test function")
    kind, da, db, w = _atom_for(test, trial, coefs, lay)
    return _AtomRef(term.coef, kind, da, db, w, test.comp, trial.comp, cells, cw)


class AssembledVector(Vector):
    """Result of assemble(linear form)."""


class Matrix:
    """sum_t c_t A_t on one mesh, optionally with Dirichlet rows/columns eliminated."""

    def __init__(self, V, refs):
        self.V, self.refs, self.lay = V, refs, V._lay
        self.bc_vertices = np.zeros(0, dtype=np.int32)
        self._op = 0

    def mesh(self):
        return self.V.mesh()

    def is_symmetric(self):
        """The SUM is symmetric when every atom's coefficient equals that of its transposed partner
        (DUDV(a,b) in block (cv,cu) <-> DUDV(b,a) in block (cu,cv); CONV <-> CONVT)."""
        acc = {}
        for r in self.refs:
            acc[r.key()] = acc.get(r.key(), 0.0) + r.coef
        scale = max((abs(v) for v in acc.values()), default=0.0)
        for r in self.refs:
            if abs(acc[r.key()] - acc.get(r.transposed_key(), 0.0)) > 1e-14 * scale:
                return False
        return True

    def apply_dirichlet(self, bc):
        if self.bc_vertices.size == 0 and bc._sorted_unique():
            self.bc_vertices = bc.vertices()       # the usual case, one condition per solve: its own sorted list (union1d: 3 ms at 256^3)
        else:
            self.bc_vertices = np.union1d(self.bc_vertices, bc.vertices()).astype(np.int32)
        self._op = 0

    def merged(self):
        """Atoms with equal keys summed: (handles, coefs)."""
        acc = {}
        for r in self.refs:
            h = _lay_atom(self.lay, r.kind, r.da, r.db, r.weight, r.cv, r.cu, r.cells, r.cw)
            acc[h] = acc.get(h, 0.0) + r.coef
        return list(acc), [acc[h] for h in acc]

    def op(self, reuse=0):
        handles, coefs = self.merged()
        return get_backend().combine(self.lay.handle(), handles, coefs, self.bc_vertices, reuse)

    def array(self):
        """Dense copy in dof order (small systems / tests only)."""
        be = get_backend()
        op = self.op()
        rp, cols = be.mesh_pattern(self.lay.handle())
        vals = be.atom_values(op, cols.size)
        be.atom_free(op)
        n = self.lay.n
        A = np.zeros((n, n))
        rows = np.repeat(np.arange(n), np.diff(rp))
        A[rows, cols] = vals
        p = vertex_to_dof_map(self.V)
        return A[np.ix_(p, p)]


def _integral_layout(term, mesh):
    """Layout (mesh + Lagrange degree) an integrand lives in: that of its functions / arguments on the
    integration mesh, a vector-valued one before a scalar one (which can only weight it); pure-Expression integrands are P1."""
    for f in term.factors:
        for leaf in (f.leaf, f.other):
            V = getattr(leaf, "_V", None)
            if V is not None and V.mesh() is mesh and V._ncomp > 1:
                return V._lay
    for f in term.factors:
        for leaf in (f.leaf, f.other):
            V = getattr(leaf, "_V", None)
            if V is not None and V.mesh() is mesh:
                return V._lay
    return mesh.layout(1)


def assemble(form, tensor=None, **kw):
    """Scalar, vector or matrix of a Form - dolfin.assemble."""
    if isinstance(form, numbers.Real):
        return float(form)
    if type(form) is _FastForm and form.measure.kind == "dx" and form.measure.subdomain_id is None:
        return _fast_scalar(form)            # (its plans know meshes, not cell sets: dx(id) takes the general path, and so does
        #                                       a DG0 factor, which never enters a _FastProd)
    rank = form.rank()
    if rank == 0:
        total = 0.0
        for t, m in form.integrals:
            mesh = m.mesh if m.mesh is not None else Form([(t, m)]).mesh()
            t, cw = _cellwise(t, m)
            if m.kind == "ds":
                total += _ds_scalar(t, _integral_layout(t, mesh), m)
            else:
                lay = _integral_layout(t, mesh)
                total += _term_scalar(t, lay, _dx_cells(lay, m), cw)
        return total
    mesh = form.mesh()
    V = _argument_space(form, 0)
    if rank == 1:
        out = AssembledVector(V)
        _assemble_vector_into(form, V._lay, out)
        return out
    return Matrix(V, [_ds_matrix(t, V._lay, m) if m.kind == "ds" else _term_matrix(t, V._lay, _dx_cells(V._lay, m), cw)
                      for (t, cw), m in ((_cellwise(t, m), m) for t, m in form.integrals)])


def _cellwise(term, measure):
    """Split the DG0 factor off an integrand: (the term without it, the vector of its cell values), or (term, None).  A cell-wise
    constant scales a cell's finished local matrix, so everything else about the term is classified as if it were not there."""
    dg = [f for f in term.factors if (getattr(getattr(f.leaf, "_V", None), "_dg0", False)
                                      or getattr(getattr(f.other, "_V", None), "_dg0", False))]
    if not dg:
        return term, None
    if len(dg) > 1:
        raise NotImplementedError("more than one DG0 (cell-wise constant) factor in one integrand")
    f = dg[0]
    if f.deriv is not None:
        raise NotImplementedError("derivative of a DG0 (cell-wise constant) function in an integrand")
    if measure.kind != "dx":
        raise NotImplementedError("DG0 coefficients in exterior-facet integrals ds")
    return term.with_factors(tuple(g for g in term.factors if g is not f)), f.leaf._vec


# cell-subdomain integrals dx(id): the atoms of the marked cells (pgd_atom_assemble_cells), cached with the layout per cell
# set.  A cell set is named by the GENERATION of its MeshFunction's markers: every lookup compares the live markers with the
# snapshot taken when they were last seen (one vectorised pass, like the facet selection of ds(tag) on every call) and a
# change of any kind - set_all, item assignment, SubDomain.mark, a write into array() - starts a new generation, whose atoms
# are built afresh; unchanged markers find the atoms already assembled.
_CELL_GENERATIONS = itertools.count(1)


def _cell_generation(mf):
    a = mf.array()
    snap = getattr(mf, "_cells_snapshot", None)
    if snap is None or snap.shape != a.shape or snap.dtype != a.dtype or not np.array_equal(snap, a):
        mf._cells_snapshot = a.copy()
        mf._cells_generation = next(_CELL_GENERATIONS)
    return mf._cells_generation


class _CellSet:
    """The cells of one dx(id) measure: MeshFunction, generation of its markers and id; keyed by (generation, id)."""
    __slots__ = ("mf", "gen", "sid", "key")

    def __init__(self, mf, sid):
        self.mf, self.sid = mf, int(sid)
        self.gen = _cell_generation(mf)
        self.key = (self.gen, self.sid)

    def mask(self):
        """One byte per cell (1: marked), from the snapshot of this generation."""
        return (self.mf._cells_snapshot == self.sid).view(np.uint8)


def _dx_cells(lay, measure):
    """The _CellSet of a dx measure on the layout's mesh; None for the whole mesh (no subdomain id)."""
    if measure.subdomain_id is None:
        return None
    if measure.subdomain_data.mesh() is not lay.mesh:
        raise ValueError("dx: subdomain_data belongs to another mesh than the integrand")
    return _CellSet(measure.subdomain_data, measure.subdomain_id)


# exterior-facet integrals.  Loads - a constant times one (component of a) test function:  int_Gamma N_i ds  is computed ON THE
# DEVICE by treating the marked facets as a mesh of their own (one disconnected interval / triangle per facet, same polynomial
# degree), assembling its mass atom and multiplying by ones; the boundary-sized result is scattered into a vector of the space
# once and cached.  Everything with a second function on the facets - the Robin term c*u*v*ds, the functional F*G*ds, the load
# F*v*ds - goes through the boundary-mass atom R of the facet set on the layout's own pattern (DofLayout.facet_atom): a Matrix
# term like any dx atom, F^T R G through _bilinear_scalar, R F through the cached products.
_DS_CACHE = {}


def _ds_facet_ids(mesh, measure):
    """Ids (Mesh.facets() numbering, ascending) of the exterior facets a ds measure integrates over: those a facet
    MeshFunction marks with ``subdomain_id``, or all of them."""
    ext = mesh.facets()[1]
    if measure.subdomain_data is not None and measure.subdomain_id is not None:
        mf = measure.subdomain_data
        if mf.mesh() is not mesh or mf.dim() != mesh.topology().dim() - 1:
            raise ValueError("ds: subdomain_data must be a facet MeshFunction of the integration mesh")
        return np.where((mf.array() == measure.subdomain_id) & ext)[0]
    if measure.subdomain_id is None:
        return np.where(ext)[0]
    raise ValueError("ds(%r) without subdomain_data" % (measure.subdomain_id,))


def _facet_node_tuples(scalar_lay, ids):
    """(len(ids), nodes per facet) node ids of a scalar layout on the given facets: the facet's vertices (sorted), then for P2
    the nodes of its edges in the UFC local order - (0, 1) on an edge, (1, 2), (0, 2), (0, 1) on a triangle."""
    mesh = scalar_lay.mesh
    f = mesh.facets()[0][ids]
    tdim, deg = mesh.topology().dim(), scalar_lay.degree
    m, nvert = f.shape
    pairs = [] if deg == 1 or tdim == 1 else [(0, 1)] if tdim == 2 else [(1, 2), (0, 2), (0, 1)]
    gl = np.empty((m, nvert + len(pairs)), dtype=np.int64)
    vn = scalar_lay.vertex_nodes
    for j in range(nvert):
        gl[:, j] = f[:, j] if vn is None else np.asarray(vn)[f[:, j]]
    if pairs:
        nv = mesh.num_vertices()
        ekeys = scalar_lay.edge_vertices[:, 0].astype(np.int64) * nv + scalar_lay.edge_vertices[:, 1]
        order = np.argsort(ekeys)
        for k, (a_, b_) in enumerate(pairs):
            lo, hi = np.minimum(f[:, a_], f[:, b_]), np.maximum(f[:, a_], f[:, b_])
            gl[:, nvert + k] = np.asarray(scalar_lay.edge_nodes)[order[np.searchsorted(ekeys[order], lo * nv + hi)]]
    return gl


class _FacetSet:
    """The facets of one ds measure: the weight slot of a DS_MASS _AtomRef (keyed by its contents)."""
    __slots__ = ("ids", "key")

    def __init__(self, ids):
        self.ids = np.ascontiguousarray(ids, dtype=np.int64)
        self.key = self.ids.tobytes()


def _boundary_load(scalar_lay, measure):
    mesh = scalar_lay.mesh
    ids = _ds_facet_ids(mesh, measure)
    key = (id(get_backend()), id(scalar_lay), ids.tobytes())
    hit = _DS_CACHE.get(key)
    if hit is not None and hit[1]() is scalar_lay:       # (an address is reused once a layout has died: check who lives there)
        return hit[0]
    out = np.zeros(scalar_lay.n)
    tdim, deg = mesh.topology().dim(), scalar_lay.degree
    if ids.size and tdim == 1:
        out[_facet_nodes(scalar_lay, ids)] = 1.0                    # point evaluation at boundary vertices
    elif ids.size:
        X = mesh.coordinates()
        f = mesh.facets()[0][ids]
        m = f.shape[0]
        if tdim == 2:      # facets = edges -> intervals laid end to end
            length = np.linalg.norm(X[f[:, 1]] - X[f[:, 0]], axis=1)
            start = np.concatenate([[0.0], np.cumsum(length)[:-1]])
            per = 2 if deg == 1 else 3
            co = np.empty((m, per))
            co[:, 0], co[:, 1] = start, start + length
            if deg == 2:
                co[:, 2] = start + 0.5 * length
            bcoords = co.reshape(-1, 1)
            bcells = np.arange(m * per, dtype=np.int32).reshape(m, per)
        else:              # facets = triangles -> congruent triangles in the plane, side by side
            a = X[f[:, 1]] - X[f[:, 0]]
            b = X[f[:, 2]] - X[f[:, 0]]
            la = np.linalg.norm(a, axis=1)
            bx = np.einsum("ij,ij->i", a, b) / la
            by = np.sqrt(np.maximum(np.einsum("ij,ij->i", b, b) - bx * bx, 0.0))
            off = np.concatenate([[0.0], np.cumsum(la + np.abs(bx) + 1.0)[:-1]]) + np.abs(np.minimum(bx, 0.0))
            P0 = np.stack([off, np.zeros(m)], axis=1)
            P1 = np.stack([off + la, np.zeros(m)], axis=1)
            P2_ = np.stack([off + bx, by], axis=1)
            pts = [P0, P1, P2_]
            if deg == 2:
                pts += [0.5 * (P1 + P2_), 0.5 * (P0 + P2_), 0.5 * (P0 + P1)]      # UFC edge order (1,2),(0,2),(0,1)
            per = len(pts)
            bcoords = np.stack(pts, axis=1).reshape(-1, 2)
            bcells = np.arange(m * per, dtype=np.int32).reshape(m, per)
        be = get_backend()
        bm = be.mesh(bcoords, bcells)
        at = be.atom(bm, MASS, 0, 0, 0)
        one, res = be.vec_from(np.ones(bcells.size)), be.vec_zeros(bcells.size)
        be.spmv(at, one, res)
        loads = be.vec_to_host(res).reshape(m, per)
        for h in (one, res):
            be.vec_free(h)
        be.atom_free(at)
        be.mesh_free(bm)
        gl = _facet_node_tuples(scalar_lay, ids)             # global node of every local boundary node
        np.add.at(out, gl.ravel(), loads.ravel())
    if len(_DS_CACHE) > 64:
        _DS_CACHE.clear()
    _DS_CACHE[key] = (out, weakref.ref(scalar_lay))
    return out


def _ds_load_vector(lay, measure, comp):
    """int_Gamma N_i ds as a Vector of the space of `lay` (in component `comp` of a vector-valued space)."""
    scalar = lay.base if isinstance(lay, BlockLayout) else lay
    L = _boundary_load(scalar, measure)
    key = ("vec", id(get_backend()), id(lay), id(L), comp)
    v = _DS_CACHE.get(key)
    if v is None:
        full = np.zeros(lay.n)
        if isinstance(lay, BlockLayout):
            full[(comp or 0)::lay.ncomp] = L
        else:
            full[:] = L
        v = Vector(lay.space(), full)
        v._keep = L
        _DS_CACHE[key] = v
    return v


def _ds_split(term, lay):
    test, trial, coefs, gd = _classify(term, lay)
    if gd is not None or any(f is not None and f.deriv is not None for f in [test, trial] + coefs):
        raise NotImplementedError("derivatives in a ds integrand (only  c * u * v,  c * F * v,  c * F * G  and loads)")
    return test, trial, coefs


def _ds_atom(lay, measure, cv=None, cu=None):
    """The boundary-mass atom of the measure's facets on `lay` (block (cv, cu) of a vector-valued layout)."""
    return _lay_atom(lay, DS_MASS, 0, 0, _FacetSet(_ds_facet_ids(lay.mesh, measure)), cv, cu)


def _ds_matrix(term, lay, measure):
    """c * u * v * ds(tag): the Robin term, a Matrix term over the facet set's boundary-mass atom."""
    test, trial, coefs = _ds_split(term, lay)
    if test is None or trial is None:
        raise ValueError("bilinear form needs a trial and a test function")
    if coefs:
        raise NotImplementedError("a Function-valued coefficient in a bilinear ds term (only constants: c * u * v * ds)")
    if lay.part is not None:
        raise NotImplementedError("bilinear ds terms (Robin atoms) on a sharded (slab) layout")
    if not hasattr(get_backend(), "atom_facets"):
        lay.facet_atom(np.zeros(0, dtype=np.int64))          # (raises: no facet atoms on this backend)
    return _AtomRef(term.coef, DS_MASS, 0, 0, _FacetSet(_ds_facet_ids(lay.mesh, measure)), test.comp, trial.comp)


def _ds_scalar(term, lay, measure):
    test, trial, coefs = _ds_split(term, lay)
    if test is not None or trial is not None:
        raise ValueError("scalar assemble of a form with arguments")
    part = lay.part
    if len(coefs) == 0:
        scalar = lay.base if isinstance(lay, BlockLayout) else lay
        L0 = _boundary_load(scalar, measure)
        if part is None:
            return term.coef * float(L0.sum())
        lo0, hi0 = scalar.owned_range()              # row-sharded: this rank's rows, summed over the ranks
        return term.coef * part.comm.allreduce_sum(float(L0[lo0:hi0].sum()))
    if len(coefs) == 2:
        # F^T R G: the memo, the stored products and the batched functionals of every other functional
        f, g = coefs
        atom = _ds_atom(lay, measure, f.comp, g.comp)
        return term.coef * _bilinear_scalar(lay, atom, _coef_vec(f.leaf, lay), _coef_vec(g.leaf, lay),
                                            symmetric=f.comp == g.comp)
    if len(coefs) != 1:
        raise NotImplementedError("ds functional of a product of more than two functions")
    c = coefs[0]
    f, L = _coef_vec(c.leaf, lay), _ds_load_vector(lay, measure, c.comp)
    if part is not None:
        lo, hi = lay.owned_range()
        return term.coef * part.comm.allreduce_sum(get_backend().vec_dot(f.dev(), L.dev(), lo, hi))
    if f._small():
        return term.coef * float(f.host() @ L.host())
    return term.coef * get_backend().vec_dot(f.dev(), L.dev())


def _ds_vector(term, lay, measure):
    """(coef, None, load Vector): b += coef * load;  with a coefficient F: (coef, R, F), b += coef * R F."""
    test, trial, coefs = _ds_split(term, lay)
    if trial is not None:
        raise ValueError("linear form with a trial function")
    if test is None:
        raise ValueError("linear form without a test function")
    if len(coefs) > 1:
        raise NotImplementedError("ds linear form with more than one coefficient function")
    if coefs:
        g = coefs[0]
        return term.coef, _ds_atom(lay, measure, test.comp, g.comp), _coef_vec(g.leaf, lay)
    return term.coef, None, _ds_load_vector(lay, measure, test.comp)


def _argument_space(form, number):
    for t, _ in form.integrals:
        for f in t.factors:
            for leaf in (f.leaf, f.other):
                if isinstance(leaf, Argument) and leaf.number == number:
                    return leaf._V
    raise ValueError("form has no argument %d" % number)


def _assemble_vector_into(form, lay, out):
    """out = sum_s c_s A_s g_s.  Small systems on the host mirror, large ones by axpy on the device."""
    pieces = [_ds_vector(t, lay, m) if m.kind == "ds" else _term_vector(t, lay, _dx_cells(lay, m), cw)
              for (t, cw), m in ((_cellwise(t, m), m) for t, m in form.integrals)]
    merged = {}
    for c, atom, g in pieces:
        key = (atom, id(g))
        if key in merged:
            merged[key][0] += c
        else:
            merged[key] = [c, atom, g]
    be = get_backend()
    if out._small() and lay.part is None:
        acc = np.zeros(out.n)
        for c, atom, g in merged.values():
            acc += c * (g if atom is None else _matvec_cached(lay, atom, g)).host()
        out._host = acc
        out.touched_host()
        return
    # one k_lincomb pass per 8 terms (9 vector passes) instead of an axpy each (24): the same chain of fused multiply-adds in
    # the same order, starting from 0 - bit-identical; the right-hand side of an enrichment step with 50 stored modes has 100 terms
    terms = [(float(c), (g if atom is None else _matvec_cached(lay, atom, g)).dev()) for c, atom, g in merged.values() if c != 0.0]
    if terms:
        be.vec_lincomb(out.dev_for_write(), [v for _, v in terms], [c for c, _ in terms])
    else:
        be.vec_fill(out.dev_for_write(), 0.0)
    out.touched_dev()


def norm(f, norm_type="L2", mesh=None):
    """dolfin.norm: L2 norm of a Function (consistent mass), l2 of a Vector."""
    if isinstance(f, Vector):
        return f.norm("l2")
    _refuse_dg0(f, "norm")
    kind = norm_type.lower()
    m = f._V._lay
    if kind == "l2":
        return math.sqrt(abs(_bilinear_scalar(m, m.atom(MASS), f._vec, f._vec)))
    if kind in ("h10", "h1"):
        s = _bilinear_scalar(m, m.atom(STIFF), f._vec, f._vec)
        if kind == "h1":
            s += _bilinear_scalar(m, m.atom(MASS), f._vec, f._vec)
        return math.sqrt(abs(s))
    raise NotImplementedError("norm type %r" % (norm_type,))


def errornorm(u, uh, norm_type="L2", degree_rise=3, mesh=None):
    """L2 distance between two P1 functions (or an Expression and a function) on uh's mesh."""
    _refuse_dg0(uh, "errornorm")
    _refuse_dg0(u, "errornorm")
    V = uh._V
    a = interpolate(u, V) if not (isinstance(u, Function) and u._V is V) else u
    d = Function(V)
    d._vec._host = a._vec.host() - uh._vec.host()
    d._vec.touched_host()
    return norm(d, norm_type)


# --------------------------------------------------------------------- variational solvers
def derivative(form, u, du=None):
    """Gateaux derivative of a form that is LINEAR in the Function `u`:
    integrands containing `u` get it replaced by a trial function, the rest vanish."""
    trial = du if du is not None else TrialFunction(u._V)
    out = []
    for t, m in form.integrals:
        hits = [i for i, f in enumerate(t.factors) if f.leaf is u or f.other is u]
        if not hits:
            continue
        if len(hits) > 1:
            raise NotImplementedError("form is nonlinear in the unknown (u appears twice in an integrand)")
        i = hits[0]
        f = t.factors[i]
        nf = Factor(trial if f.leaf is u else f.leaf, f.deriv, trial if f.other is u else f.other, f.comp)
        out.append((t.with_factors(t.factors[:i] + (nf,) + t.factors[i + 1:]), m))
    return Form(out)


def _has_trial(term):
    return any((isinstance(f.leaf, Argument) and f.leaf.number == 1) or
               (isinstance(f.other, Argument) and f.other.number == 1) for f in term.factors)


def lhs(form):
    """Bilinear part of a residual form written with a TrialFunction (dolfin.lhs)."""
    return Form([(t, m) for t, m in form.integrals if _has_trial(t)])


def rhs(form):
    """Right-hand side of a residual form: minus its linear part (dolfin.rhs)."""
    return Form([(t.scaled(-1.0), m) for t, m in form.integrals if not _has_trial(t)])


class _Params(dict):
    """Nested solver-parameter dictionary accepting any key (settings are forwarded verbatim)."""

    def __missing__(self, k):
        v = _Params()
        self[k] = v
        return v


SMALL_DIRECT_N = 20000   # systems up to this size on 1-D meshes take the banded direct path
WARM_START_RESCALE = True  # scale the PCG start vector to its energy-optimal length (see _rescale_start)
START_SPACE_MAX = int(os.environ.get("PGD_START_SPACE_MAX", "8"))   # stored modes that may join the Galerkin start of a solve (most recent ones; <= 8)


def _rescale_start(lay, op, b, x):
    """The warm start of a PCG solve is the previous iterate of the same dimension, NORMALISED by the fixed-point loop:
    the right shape, an arbitrary length.  gamma = (x . b) / (x . A x) is the best multiple of it in the energy norm
    (one product, two dots); on the bench problem it saves 23 % of the PCG iterations of a pass.

    When the caller names further vectors (``x._start_space``: the stored modes of this dimension - the right-hand side
    of an enrichment step is the load minus the operator applied to them) the start is the Galerkin projection onto
    span{x, v_1, ..., v_k}: k + 1 products, (k + 1)(k + 4) / 2 dots and a (k + 1) x (k + 1) solve on the host; it is
    never worse than the scaled x in the energy norm.

    Returns the coefficients of the start in [x (as it came), v_1 ... v_k], or None where x was left as it was."""
    be = get_backend()
    lo, hi = lay.owned_range()
    extras = [v for v in getattr(x, "_start_space", ()) if v is not x][-START_SPACE_MAX:]
    vecs = [x] + extras
    for v in vecs:
        _halo(lay, v)
    k = len(vecs)
    # k products from the operator's fastest storage form and all (k + 1)(k + 2) / 2 - 1 dots on the device: one host
    # synchronisation (one D2H copy), and ONE all-reduce of the packed result when the rows are sharded
    G, g = be.start_gram(op, [v.dev() for v in vecs], b.dev(), lo, hi)
    STATS["host_syncs_start"] = STATS.get("host_syncs_start", 0) + 1
    if lay.part is not None:
        packed = lay.part.comm.allreduce_array(np.concatenate([G.ravel(), g]))
        G, g = packed[:k * k].reshape(k, k), packed[k * k:]
    if not (np.all(np.isfinite(G)) and np.all(np.isfinite(g)) and G[0, 0] > 0.0):
        return None
    if k == 1:
        coef = np.array([g[0] / G[0, 0]])
    else:
        d = np.sqrt(np.abs(np.diag(G)))
        d[d == 0.0] = 1.0
        coef = np.linalg.lstsq(G / np.outer(d, d), g / d, rcond=1e-10)[0] / d        # equilibrated, rank-revealing
    if not np.all(np.isfinite(coef)) or not np.any(coef):
        return None
    if k == 1:
        be.vec_scale(x.dev(), float(coef[0]))
    elif hasattr(be, "vec_lincomb_inplace"):
        # straight into x, which is the first term: every entry of the terms is read before that entry of x is written
        be.vec_lincomb_inplace(x.dev(), [v.dev() for v in vecs], [float(c) for c in coef])
    else:
        out = be.vec_zeros(lay.n)
        be.vec_lincomb(out, [v.dev() for v in vecs], [float(c) for c in coef])
        be.vec_copy(x.dev(), out)
        be.vec_free(out)
    x.touched_dev()
    if lay.part is not None:
        x._halo_version = x.version        # a combination of vectors with current ghost planes
    return coef


STATS = {"linear_solves": 0, "pcg_iterations": 0, "pcg_seconds": 0.0, "mg_solves": 0, "vmg_solves": 0, "cmg_solves": 0, "pmg_solves": 0}
# values of settings["preconditioner"] that select the geometric multigrid V-cycle (dolfin's names of its algebraic ones included)
MULTIGRID_NAMES = ("amg", "hypre_amg", "petsc_amg", "ml_amg", "gmg", "multigrid", "mg")
# ... and those that select the V-cycle for variable-coefficient operators (pgd_vmg.hip): opt-in, none of the names above
VARIABLE_MULTIGRID_NAMES = ("vmg", "variable_multigrid")
# ... and those that select one such cycle per component of a vector-valued P1 space on a box lattice: opt-in, its own names
COMPONENT_MULTIGRID_NAMES = ("cmg", "component_multigrid")
# ... and those that select the p-multigrid cycle of a P2 space on a 3-D box lattice (pgd_pmg.hip): opt-in, its own names
P_MULTIGRID_NAMES = ("pmg", "p_multigrid")
# values of settings["block_product"]: the product of a vector-valued P1 operator on a box lattice from CSR or from its row-diagonal form
BLOCK_PRODUCT_NAMES = ("csr", "diagonal")
# values of settings["p2_product"]: the product of a P2 operator on a 3-D box lattice from CSR or from its row-class form
P2_PRODUCT_NAMES = ("csr", "lattice")

# One row per cycle that settings["preconditioner"] can ask for: its names, the backend's selector with its on / off arguments
# (the selector returns the number of solves the cycle has preconditioned so far), the communicator's solve that stands in for it on
# a row-sharded layout (None: that layout has the Jacobi form only), whether a request offers DofLayout.bind_p2_lattice first, what
# info["method"] says where the cycle was used and the STATS key that counts those solves.
_Cycle = collections.namedtuple("_Cycle", "names selector on off sharded binds method stat")
PRECONDITIONERS = (
    # settings["preconditioner"] (forwarded to PETSc by the reference, solver.py:593-594): the multigrid family asks for
    # the V-cycle of pgd_mg.hip, which the library uses where the operator has the structure for it and says so in its
    # counters; every other value is the Jacobi-PCG.  The row-sharded solve has the Jacobi form only - but for this family on
    # a row-sharded lattice: the V-cycle with level 0 on the slabs and levels >= 1 replicated (dist.pcg_mg); where it does not
    # apply on some rank every rank takes the Jacobi-PCG (decided by an all-reduce)
    _Cycle(MULTIGRID_NAMES, "precondition", 1, 0, "pcg_mg", False, "mg_pcg", "mg_solves"),
    # VARIABLE_MULTIGRID_NAMES (opt-in) ask for the V-cycle of pgd_vmg.hip instead: any scalar P1 operator on a lattice
    # mesh, any Dirichlet set.  A backend without it (the numpy oracle) and a row-sharded layout answer with the Jacobi-PCG.
    _Cycle(VARIABLE_MULTIGRID_NAMES, "precondition_variable", True, False, None, False, "vmg_pcg", "vmg_solves"),
    # COMPONENT_MULTIGRID_NAMES (opt-in) ask for one such cycle per component of a vector-valued P1 space on a box lattice
    # (the diagonal blocks of the operator); "amg" and "vmg" on a vector space stay the Jacobi-PCG.
    _Cycle(COMPONENT_MULTIGRID_NAMES, "precondition_component", True, False, None, False, "cmg_pcg", "cmg_solves"),
    # P_MULTIGRID_NAMES (opt-in) ask for the p-multigrid cycle of pgd_pmg.hip: P2 spaces (scalar or vector-valued) on a 3-D box
    # lattice, through the P1 V-cycles on P^T A P.  A degree-2 layout on a 3-D mesh is bound to its vertex lattice on the first
    # such request (DofLayout.bind_p2_lattice).  The degree and the dimension decide only whether a binding is OFFERED, not
    # whether the library is asked: the request reaches it for every unsharded space - a departure from routing "pmg" in the
    # frontend only for degree 2 on a 3-D mesh - so that a P1 or a 2-D space under these names is a fallback the library
    # COUNTS (pgd_pmg_counts), like a 3-D P2 space it refuses to bind; all of them are the Jacobi-PCG.
    _Cycle(P_MULTIGRID_NAMES, "precondition_p", True, False, None, True, "pmg_pcg", "pmg_solves"),
)

# One row per product form: the settings key, its allowed values (the first is the default) and the one that switches the form on,
# the backend's selector (True / False; returns the number of products launched from the form so far) and its stats method (whose
# "products" is that number), which layouts can have the form, whether a request offers DofLayout.bind_p2_lattice first, what
# info["product"] says where the form was used (the later row where two were) and the STATS key that counts those solves.
_Form = collections.namedtuple("_Form", "key values on selector stats applies binds product stat")
PRODUCT_FORMS = (
    # settings["block_product"] = "diagonal" (opt-in, default "csr"): the products of a vector-valued P1 space on a box
    # lattice from the operator's row-diagonal form (csrc/pgd_bdia.hip) - the same numbers, bit for bit; the library says
    # in its counters whether the operator had one.  A backend without it and a row-sharded layout ignore the key.
    # (the counter is read either way: PGD_TUNE=58=1 switches whole runs without the key)
    _Form("block_product", BLOCK_PRODUCT_NAMES, "diagonal", "block_product", "bdia_stats",
          lambda lay: getattr(lay, "ncomp", 1) > 1, False, "block_dia", "block_dia_solves"),
    # settings["p2_product"] = "lattice" (opt-in, default "csr"): the products of a P2 space (scalar or vector-valued) on a 3-D
    # box lattice from the operator's row-class form (csrc/pgd_p2lat.hip) - the same numbers, bit for bit.  The request binds
    # a degree-2 layout on a 3-D mesh to its vertex lattice like a "pmg" request does; the library says in its counters
    # whether the operator had a form.  A backend without it, a row-sharded layout and a degree-1 space ignore
    # the key.  (on a degree-2 space the counter is read either way: PGD_TUNE=59=1 switches whole runs without the key)
    _Form("p2_product", P2_PRODUCT_NAMES, "lattice", "p2_product", "p2lat_stats",
          lambda lay: getattr(lay, "degree", 1) == 2, True, "p2_lattice", "p2_lattice_solves"),
)
# the settings a nonlinear solve hands on to its linear solves
LINEAR_SOLVE_KEYS = ("linear_solver", "preconditioner") + tuple(f.key for f in PRODUCT_FORMS)


def _setting(prm, key, default, cast=None):
    """settings[key], cast; the default where the key is absent or was touched but never set (an empty _Params sits there)."""
    v = prm.get(key, default)
    if isinstance(v, _Params):
        v = default
    return v if cast is None else cast(v)


def _tolerances(prm):
    return (_setting(prm, "relative_tolerance", 1e-10, float), _setting(prm, "absolute_tolerance", 0.0, float),
            _setting(prm, "maximum_iterations", 20000, int))


def _report_nonconvergence(prm, failed, solver, rtol, it, rel):
    """dolfin's Krylov solvers raise on non-convergence unless told otherwise (error_on_nonconvergence,
    default True): an unconverged mode must not be stored silently"""
    if not failed:
        return
    msg = "%s did not reach rtol %g in %d iterations (relres %g)" % (solver, rtol, it, rel)
    if _setting(prm, "error_on_nonconvergence", True):
        raise RuntimeError(msg)
    LOG.error(msg)


@contextlib.contextmanager
def _switched_on(be, lay, cycle, forms):
    """Switch on the cycle (a row of PRECONDITIONERS or None) and the product forms ([(row of PRODUCT_FORMS, asked for)]; a form
    not asked for is only watched through its stats) for the solve inside; on the way out, exception or not, switch every one of
    them off again.  Yields a dict that then holds, per row's STATS key, how far its counter advanced."""
    for row, wanted in [(cycle, cycle is not None)] + forms:
        if wanted and row.binds:
            lay.bind_p2_lattice(be)
    used, watch = {}, []         # watch: (STATS key, the counter at the start, what switches off and reads it again)
    try:
        if cycle is not None:
            select = getattr(be, cycle.selector)
            watch.append((cycle.stat, select(cycle.on), functools.partial(select, cycle.off)))
        for row, wanted in forms:
            if wanted:
                select = getattr(be, row.selector)
                watch.append((row.stat, select(True), functools.partial(select, False)))
            else:
                read = getattr(be, row.stats)
                watch.append((row.stat, read()["products"], lambda read=read: read()["products"]))
        yield used
    finally:
        for stat, start, off in watch:
            used[stat] = off() - start


def _solve_band(be, A, op, b, x, prm):
    be.band_solve(op, b.dev(), x.dev_for_write())
    x.touched_dev()
    return dict(method="band_lu", iterations=1)


def _solve_bicgstab(be, A, op, b, x, prm):
    """A convection atom on a 2-D / 3-D space (or a 1-D system beyond the banded LU): BiCGStab with Jacobi scaling on the
    CSR product (csrc/pgd_krylov.hip) where the reference's MUMPS solves whatever the callbacks produce
    (solver.py:627-636); same relative_tolerance / maximum_iterations / error_on_nonconvergence semantics as the PCG"""
    rtol, atol, maxit = _tolerances(prm)
    part = A.lay.part
    t_solve = time.perf_counter()
    if part is not None:
        # (row-sharded: the same recurrence driven over the communicator - pgdrome_amd/dist.py::TorchComm.bicgstab;
        # is_symmetric() reads the forms' coefficients, which are all-reduced numbers: every rank takes this branch or none)
        it, rel = part.comm.bicgstab(A.lay.shard_view(), op, b, x, rtol, atol, maxit)
    else:
        it, rel = be.bicgstab(op, b.dev(), x.dev(), rtol, atol, maxit)
    x.touched_dev()
    STATS["bicgstab_seconds"] = STATS.get("bicgstab_seconds", 0.0) + time.perf_counter() - t_solve
    STATS["bicgstab_iterations"] = STATS.get("bicgstab_iterations", 0) + it
    _report_nonconvergence(prm, rel > max(rtol, 1e-14) * 1.0001 and (atol <= 0.0 or it >= maxit), "BiCGStab", rtol, it, rel)
    return dict(method="jacobi_bicgstab", iterations=it, relres=rel)


def _solve_pcg(be, A, op, b, x, prm):
    """Jacobi-PCG, or the PCG under the cycle of PRECONDITIONERS that settings["preconditioner"] names, with the products from the
    forms of PRODUCT_FORMS that the settings ask for: where the backend has them and the rows are not sharded."""
    lay, part = A.lay, A.lay.part
    rtol, atol, maxit = _tolerances(prm)
    prec_name = _setting(prm, "preconditioner", "default", lambda v: str(v).lower())
    asked = next((row for row in PRECONDITIONERS if prec_name in row.names), None)
    cycle = asked if asked is not None and part is None and hasattr(be, asked.selector) else None
    forms = []
    for row in PRODUCT_FORMS:        # (both keys are checked before anything is bound or switched)
        value = _setting(prm, row.key, row.values[0])
        if str(value).lower() not in row.values:
            raise ValueError("settings['%s']: expected one of %s, got %r" % (row.key, row.values, value))
        if part is None and row.applies(lay) and hasattr(be, row.selector) and hasattr(be, row.stats):
            forms.append((row, str(value).lower() == row.on))
    # settings["spectral_start"] = k: the second level of the Galerkin start, over k Ritz vectors harvested once per space
    # and Dirichlet set (pgdrome_amd/spectral.py); the harvest itself is one-time work and stays out of the solve's clock
    k_spec = spectral.requested(prm) if lay.n >= spectral.MIN_ROWS else 0
    spec = spectral.get(sys.modules[__name__], A, b, k_spec, prm) if k_spec != 0 else None
    t_solve = time.perf_counter()
    start_coefs = None
    if WARM_START_RESCALE and not x._zero:
        start_coefs = _rescale_start(lay, op, b, x)
    if spec is not None:
        spec.correct(sys.modules[__name__], A, op, b, x, start_coefs)
    got = None
    with _switched_on(be, lay, cycle, forms) as used:
        if part is None:
            it, rel = be.pcg(op, b.dev(), x.dev(), rtol, atol, maxit)
            x.touched_dev()
        else:
            # the rows' partition and what the communicator takes for "the mesh": the layout's (a vector-valued space has ncomp rows per vertex)
            view = lay.shard_view()
            if asked is not None and asked.sharded and hasattr(part.comm, asked.sharded):
                got = getattr(part.comm, asked.sharded)(view, op, b, x, rtol, atol, maxit)
            it, rel = got if got is not None else part.comm.pcg(view, op, b, x, rtol, atol, maxit)
    if got is not None:
        used[asked.stat] = 1
    STATS["pcg_seconds"] += time.perf_counter() - t_solve      # the solve returns synchronised
    for stat, advanced in used.items():
        if advanced > 0:
            STATS[stat] = STATS.get(stat, 0) + 1
    info = dict(method=next((row.method for row in PRECONDITIONERS if used.get(row.stat, 0) > 0), "jacobi_pcg"), iterations=it, relres=rel,
                product=next((row.product for row in reversed(PRODUCT_FORMS) if used.get(row.stat, 0) > 0), "csr"))
    _report_nonconvergence(prm, rel > max(rtol, 1e-14) * 1.0001 and it >= maxit, "PCG", rtol, it, rel)
    return info


def _solve_linear(A, b, x, prm):
    """Solve A x = b on the device.  A: Matrix (BCs already registered), b: Vector (BC values set).

    1-D meshes (time / parameter dimensions, possibly non-symmetric) use the banded
    LU kernel - the counterpart of the reference's MUMPS solve; larger SPD systems
    use Jacobi-PCG with `relative_tolerance` (default 1e-10) from the settings."""
    be = get_backend()
    op = A.op()
    try:
        use_direct = A.mesh().topology().dim() == 1 and A.lay.n <= SMALL_DIRECT_N and A.lay.part is None
        solve = _solve_band if use_direct else _solve_pcg if A.is_symmetric() else _solve_bicgstab
        info = solve(be, A, op, b, x, prm)
        LOG.debug("linear solve (%s requested): %s", str(prm.get("linear_solver", "default")), info)
    finally:
        be.atom_free(op)
    STATS["linear_solves"] += 1
    STATS["pcg_iterations"] += info["iterations"] if solve is _solve_pcg else 0
    return info


def _apply_bcs_system(A, b, bcs):
    """Symmetric elimination: lift non-zero values, then identity rows/cols + b[bc] = g."""
    verts, vals = _bc_vertices(bcs)
    if verts.size == 0:
        return
    one = _bc_list(bcs)
    if (not one[0].homogeneous()) if len(one) == 1 else np.any(vals):
        g = Vector(A.V)
        g.host()[verts] = vals
        g.touched_host()
        handles, coefs = A.merged()
        for h, c in zip(handles, coefs):
            b.axpy(-c, _matvec_cached(A.lay, h, g))
    for bc in _bc_list(bcs):
        A.apply_dirichlet(bc)
    tmp = DirichletBC.__new__(DirichletBC)
    tmp._vertices, tmp._vals = verts, vals
    tmp.apply(b)


class LinearVariationalProblem:
    def __init__(self, a, L, u, bcs=None, form_compiler_parameters=None):
        self.a, self.L, self.u, self.bcs = a, L, u, _bc_list(bcs)


class LinearVariationalSolver:
    def __init__(self, problem):
        self.problem = problem
        self.parameters = _Params(linear_solver="default")
        self.info = {}

    def solve(self):
        p = self.problem
        A = assemble(p.a)
        b = assemble(p.L)
        _apply_bcs_system(A, b, p.bcs)
        self.info = _solve_linear(A, b, p.u.vector(), self.parameters)
        return self.info


class NonlinearVariationalProblem:
    def __init__(self, F, u, bcs=None, J=None, form_compiler_parameters=None):
        self.F, self.u, self.bcs = F, u, _bc_list(bcs)
        self.J = J if J is not None else derivative(F, u)


class NonlinearVariationalSolver:
    """Newton's method.  The forms PGDrome's callbacks can express are linear in
    the unknown, so the first step solves the problem and the second residual
    evaluation confirms it (solver.py:579-595, 651-674)."""

    def __init__(self, problem):
        self.problem = problem
        self.parameters = _Params()
        ns = self.parameters["newton_solver"]
        ns.update(linear_solver="default", maximum_iterations=50, relative_tolerance=1e-9,
                  absolute_tolerance=1e-10)
        self.info = {}

    def _residual(self, bcs_h):
        p = self.problem
        r = assemble(p.F)          # F(u; v): u enters as a coefficient
        for bc in bcs_h:
            bc.apply(r)
        return r

    def solve(self):
        p, ns = self.problem, self.parameters["newton_solver"]
        u = p.u.vector()
        # start from a state that satisfies the Dirichlet values; updates are homogeneous there
        for bc in p.bcs:
            bc.apply(u)
        bcs_h = []
        for bc in p.bcs:
            h = DirichletBC.__new__(DirichletBC)
            h._V, h._vertices, h._vals = bc._V, bc._vertices, np.zeros_like(bc._vals)
            bcs_h.append(h)
        lin = _Params({k: v for k, v in ns.items() if k in LINEAR_SOLVE_KEYS})
        lin["relative_tolerance"] = _setting(ns, "krylov_relative_tolerance", 1e-10)
        rtol, atol, maxit = float(ns["relative_tolerance"]), float(ns["absolute_tolerance"]), int(ns["maximum_iterations"])
        r = self._residual(bcs_h)
        r0 = r.norm("l2")
        it = 0
        res = r0
        while it < maxit and res > atol and (it == 0 or res > rtol * r0):
            A = assemble(p.J)
            for bc in bcs_h:
                A.apply_dirichlet(bc)
            r.scale(-1.0)
            du = Vector(u.V)
            _solve_linear(A, r, du, lin)
            u.axpy(1.0, du)
            it += 1
            r = self._residual(bcs_h)
            res = r.norm("l2")
        self.info = {"newton_iterations": it, "residual": res, "residual0": r0}
        return it, res <= atol or res <= rtol * r0


def solve(eq, u, bcs=None, solver_parameters=None, **kw):
    """solve(a == L, u, bcs) for linear problems."""
    if not isinstance(eq, Equation):
        raise TypeError("solve() expects `a == L`")
    if isinstance(eq.rhs, numbers.Real):
        prob = NonlinearVariationalProblem(eq.lhs, u, bcs)
        s = NonlinearVariationalSolver(prob)
        if solver_parameters:
            s.parameters["newton_solver"].update(solver_parameters.get("newton_solver", {}))
        return s.solve()
    s = LinearVariationalSolver(LinearVariationalProblem(eq.lhs, eq.rhs, u, bcs))
    if solver_parameters:
        s.parameters.update(solver_parameters)
    return s.solve()


def clear_caches():
    spectral.clear()
    _FUNCTIONAL_PLANS.clear()
    _FAST_PLANS.clear()
    _SCALAR_MEMO.clear()
    _MV_CACHE.clear()
    _DS_CACHE.clear()
    for mesh in list(_LOCATED_MESHES):          # located point sets: the cache entries go, and the library's point sets with them
        for located in mesh.__dict__.pop("_located", {}).values():
            located.free()
        for be in mesh.__dict__.pop("_index_on", []):      # ... and the bin indexes that locate_points(index=...) had built
            h = mesh.layout(1)._handles.get(id(be))
            if h is not None:
                try:
                    be.points_index_drop(h)
                except Exception:
                    pass
    _LOCATED_MESHES.clear()
    for sol in list(SENSOR_CACHES):
        sol.__dict__.pop("_sensor_modes", None)
    SENSOR_CACHES.clear()


from . import spectral                       # noqa: E402  (the spectral start space of the large SPD solves)
# result files: dolfin.HDF5File / dolfin.XDMFFile / dolfin.MPI (pgdrome_amd/io.py, real HDF5 through pgdrome_amd.h5lite)
from .io import HDF5File, MPI, XDMFFile      # noqa: E402,F401
