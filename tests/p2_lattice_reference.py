"""CPU restatement (numpy / scipy.sparse, tests only) of the row-class form of a P2 operator on a 3-D box lattice
(pgdrome_amd/csrc/pgd_p2lat.hip: k_p2lat_extract / k_spmv_p2lat, PGD_TUNE_SPMV_P2_LATTICE, settings["p2_product"] = "lattice"):

  * nodes: the vertices of the lattice in lattice order (vertex = x + nx (y + ny z)), then one node per mesh edge with the keys
    lo * nvert + hi ascending (DofLayout.edge_vertices); dof = ncomp * node + c;
  * every node is a pair (anchor vertex I, class g): g = 0 the vertex itself, g = dx + 2 dy + 4 dz in 1..7 the midpoint of the edge
    from I to I + (dx, dy, dz); in half steps the node sits at 2 I + (dx, dy, dz), so the P2 nodes fill the lattice of half steps;
  * the columns of a row of class g are a fixed table of (vertex offset in {-1, 0, 1}^3, class) pairs, built from the six
    tetrahedra of the unit cube: the vertex columns first, in lattice order of the offset, then the edge columns in lattice order
    of the anchor's offset and ascending class inside it.  With at least 3 vertices per axis that is ascending node order;
  * the form: one value per (row, slot, column component) - 65 ncomp arrays over the vertex rows, 27 ncomp arrays over the edge rows
    (the 19-wide classes padded with 0.0);
  * the product of row r: acc = 0.0, then for the slots ascending and d ascending inside a slot acc += a[slot, d][r] * x[column];
    a neighbour that does not exist meets the coefficient 0.0 and the row's own x.
"""
import itertools

import numpy as np
import scipy.sparse as sps

WIDTHS = (65, 27, 27, 19, 27, 19, 19, 27)
VERTEX_WIDTH, EDGE_WIDTH = 65, 27


def tetrahedra():
    """The six tetrahedra of the unit cube: the monotone paths 0 -> e_a -> e_a + e_b -> (1, 1, 1), as 4 vertices each."""
    out = []
    for perm in itertools.permutations(range(3)):
        v, path = [0, 0, 0], [(0, 0, 0)]
        for a in perm:
            v[a] = 1
            path.append(tuple(v))
        out.append(path)
    return out


def tables():
    """tables()[g]: the slots of a row of class g in order, each (ox, oy, oz, class of the column node)."""
    pairs = [set() for _ in range(8)]
    for tet in tetrahedra():
        # the 10 nodes of the tetrahedron in half steps: 2 v for a vertex, va + vb for the midpoint of an edge
        nodes = [tuple(2 * c for c in v) for v in tet]
        nodes += [tuple(a + b for a, b in zip(tet[i], tet[j])) for i in range(4) for j in range(i + 1, 4)]
        for p in nodes:
            g = (p[0] & 1) + 2 * (p[1] & 1) + 4 * (p[2] & 1)
            par = (p[0] & 1, p[1] & 1, p[2] & 1)
            for q in nodes:
                # translated so that the row's anchor is the origin: the column sits at parity + (q - p)
                h = tuple(par[k] + q[k] - p[k] for k in range(3))
                off = tuple(c // 2 for c in h)                     # (floor division: -1 -> -1, 2 -> 1)
                cls = (h[0] & 1) + 2 * (h[1] & 1) + 4 * (h[2] & 1)
                pairs[g].add(off + (cls,))
    order = lambda e: (e[3] != 0, e[2], e[1], e[0], e[3])
    return [sorted(s, key=order) for s in pairs]


def slot_maps():
    """slot_maps()[g]: {(ox, oy, oz, class): slot}."""
    return [{e: s for s, e in enumerate(t)} for t in tables()]


def bindable(shape, edge_vertices):
    """What the binding records for the form: at least 3 vertices along every axis, the edge list strictly ascending in (va, vb) with
    va < vb, 3 nnode < 2^31."""
    ev = np.asarray(edge_vertices, dtype=np.int64).reshape(-1, 2)
    nvert = int(np.prod(shape))
    if min(shape) < 3 or 3 * (nvert + ev.shape[0]) >= 2 ** 31:
        return False
    if np.any(ev[:, 0] >= ev[:, 1]):
        return False
    key = ev[:, 0] * nvert + ev[:, 1]
    return bool(np.all(key[1:] > key[:-1]))


def vertex_position(i, shape):
    nx, ny, _ = shape
    return i % nx, (i // nx) % ny, i // (nx * ny)


class Lattice:
    """The (anchor, class) of every node and the node of every (anchor, class)."""

    def __init__(self, shape, edge_vertices):
        self.shape = tuple(int(s) for s in shape)
        nx, ny, nz = self.shape
        self.nvert = nx * ny * nz
        ev = np.asarray(edge_vertices, dtype=np.int64).reshape(-1, 2)
        self.nnode = self.nvert + ev.shape[0]
        self.anchor = np.concatenate([np.arange(self.nvert), ev[:, 0]])
        self.cls = np.zeros(self.nnode, dtype=np.int64)
        self.node_of = {(i, 0): i for i in range(self.nvert)}
        for e, (va, vb) in enumerate(ev):
            pa, pb = vertex_position(int(va), self.shape), vertex_position(int(vb), self.shape)
            d = tuple(b - a for a, b in zip(pa, pb))
            if min(d) < 0 or max(d) > 1 or d == (0, 0, 0):
                raise ValueError("edge %d leaves the pattern" % e)
            g = d[0] + 2 * d[1] + 4 * d[2]
            self.cls[self.nvert + e] = g
            self.node_of[(int(va), g)] = self.nvert + e

    def neighbour(self, node, entry):
        """The node at (offset, class) = entry from the anchor of `node`, None where there is none."""
        ox, oy, oz, gc = entry
        x, y, z = vertex_position(int(self.anchor[node]), self.shape)
        q = (x + ox, y + oy, z + oz)
        if any(c < 0 or c >= n for c, n in zip(q, self.shape)):
            return None
        return self.node_of.get((q[0] + self.shape[0] * (q[1] + self.shape[1] * q[2]), gc))

    def entry(self, row_node, col_node):
        """(offset, class) of col_node seen from the anchor of row_node."""
        pa = vertex_position(int(self.anchor[row_node]), self.shape)
        pb = vertex_position(int(self.anchor[col_node]), self.shape)
        return tuple(b - a for a, b in zip(pa, pb)) + (int(self.cls[col_node]),)


def walk(lat, r, ncomp, tabs=None):
    """The columns row r visits - slots ascending, d ascending inside a slot - neighbours that do not exist left out."""
    tabs = tabs or tables()
    node = r // ncomp
    out = []
    for e in tabs[int(lat.cls[node])]:
        j = lat.neighbour(node, e)
        if j is not None:
            out.extend(ncomp * j + d for d in range(ncomp))
    return out


def to_form(M, lat, ncomp):
    """(vertex segment [65 ncomp, ncomp nvert], edge segment [27 ncomp, ncomp n_edges]) of a CSR matrix.  Raises ValueError on an
    entry without a slot in its row's class and on stored entries whose slots do not ascend."""
    M = sps.csr_matrix(M)
    M.sort_indices()
    maps = slot_maps()
    nv = ncomp * lat.nvert
    vform = np.zeros((VERTEX_WIDTH * ncomp, nv))
    eform = np.zeros((EDGE_WIDTH * ncomp, M.shape[0] - nv))
    for r in range(M.shape[0]):
        node = r // ncomp
        last = -1
        for k in range(M.indptr[r], M.indptr[r + 1]):
            col = int(M.indices[k])
            s = maps[int(lat.cls[node])].get(lat.entry(node, col // ncomp))
            if s is None:
                raise ValueError("row %d: column %d has no slot" % (r, col))
            idx = s * ncomp + col % ncomp
            if idx <= last:
                raise ValueError("row %d: the slots do not ascend" % r)
            last = idx
            if r < nv:
                vform[idx, r] = M.data[k]
            else:
                eform[idx, r - nv] = M.data[k]
    return vform, eform


def from_form(form, lat, ncomp, pattern):
    """The CSR matrix with the sparsity of `pattern` and the values of the form."""
    vform, eform = form
    P = sps.csr_matrix(pattern)
    P.sort_indices()
    maps = slot_maps()
    nv = ncomp * lat.nvert
    data = np.zeros(P.nnz)
    for r in range(P.shape[0]):
        node = r // ncomp
        for k in range(P.indptr[r], P.indptr[r + 1]):
            col = int(P.indices[k])
            idx = maps[int(lat.cls[node])][lat.entry(node, col // ncomp)] * ncomp + col % ncomp
            data[k] = vform[idx, r] if r < nv else eform[idx, r - nv]
    return sps.csr_matrix((data, P.indices.copy(), P.indptr.copy()), shape=P.shape)


def product(form, lat, ncomp, x):
    """y = A x from the form, the chain of k_spmv_p2lat (plain multiply-add here: exact on integer data)."""
    vform, eform = form
    tabs = tables()
    nv = ncomp * lat.nvert
    n = nv + eform.shape[1]
    y = np.zeros(n)
    for r in range(n):
        node = r // ncomp
        a, rl = (vform, r) if r < nv else (eform, r - nv)
        acc = 0.0
        for s, e in enumerate(tabs[int(lat.cls[node])]):
            j = lat.neighbour(node, e)
            for d in range(ncomp):
                acc += a[s * ncomp + d, rl] * (x[ncomp * j + d] if j is not None else x[r])
        y[r] = acc
    return y


def chain(M, x):
    """The sequential ascending-column chain of the CSR product, row by row."""
    M = sps.csr_matrix(M)
    M.sort_indices()
    y = np.zeros(M.shape[0])
    for r in range(M.shape[0]):
        acc = 0.0
        for k in range(M.indptr[r], M.indptr[r + 1]):
            acc += M.data[k] * x[M.indices[k]]
        y[r] = acc
    return y
