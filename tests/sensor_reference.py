"""Restatement of point location and point sampling on simplicial meshes, for the sensor tests.

Everything is formed in np.longdouble straight from the vertex coordinates: the barycentric coordinates of a point in EVERY cell
(adjugate and determinant of the edge matrix, written out per dimension), the cell of a point (largest smallest barycentric
coordinate, lowest cell among equal ones), the P1 / P2 shape functions l (2 l - 1), 4 l_a l_b and their gradients.  Nothing is
taken from pgdrome_amd.fem.point_basis or from the library."""
import itertools

import numpy as np

LD = np.longdouble
U53 = 2.0 ** -53
P2_EDGES = {1: ((0, 1),), 2: ((1, 2), (0, 2), (0, 1)), 3: ((2, 3), (1, 3), (1, 2), (0, 3), (0, 2), (0, 1))}


def edge_matrices(X, cells):
    """T (nc, D, D) in longdouble, column a = vertex a + 1 minus vertex 0, and the vertices 0 (nc, D)."""
    X = np.asarray(X, dtype=LD).reshape(len(X), -1)
    P = X[np.asarray(cells)[:, :X.shape[1] + 1]]
    return np.transpose(P[:, 1:, :] - P[:, :1, :], (0, 2, 1)), P[:, 0, :]


def inverse(T):
    """The inverses of the edge matrices: adjugate over determinant, written out."""
    D = T.shape[1]
    inv = np.empty_like(T)
    if D == 1:
        inv[:, 0, 0] = LD(1) / T[:, 0, 0]
    elif D == 2:
        det = T[:, 0, 0] * T[:, 1, 1] - T[:, 0, 1] * T[:, 1, 0]
        inv[:, 0, 0], inv[:, 0, 1] = T[:, 1, 1] / det, -T[:, 0, 1] / det
        inv[:, 1, 0], inv[:, 1, 1] = -T[:, 1, 0] / det, T[:, 0, 0] / det
    else:
        cof = np.empty_like(T)
        for i in range(3):
            for j in range(3):
                i1, i2, j1, j2 = (i + 1) % 3, (i + 2) % 3, (j + 1) % 3, (j + 2) % 3
                cof[:, i, j] = T[:, i1, j1] * T[:, i2, j2] - T[:, i1, j2] * T[:, i2, j1]
        det = T[:, 0, 0] * cof[:, 0, 0] + T[:, 0, 1] * cof[:, 0, 1] + T[:, 0, 2] * cof[:, 0, 2]
        inv = np.transpose(cof, (0, 2, 1)) / det[:, None, None]
    return inv


def cond_F(X, cells):
    """||T||_F ||T^-1||_F per cell, as float64."""
    T, _ = edge_matrices(X, cells)
    Ti = inverse(T)
    return np.asarray(np.sqrt((T * T).sum(axis=(1, 2)) * (Ti * Ti).sum(axis=(1, 2))), dtype=np.float64)


def barycentric_all(X, cells, pts):
    """L (P, nc, D + 1), longdouble: the barycentric coordinates of every point in every cell."""
    T, P0 = edge_matrices(X, cells)
    Ti = inverse(T)
    pts = np.asarray(pts, dtype=LD).reshape(-1, T.shape[1])
    lam = np.einsum("cij,pcj->pci", Ti, pts[:, None, :] - P0[None, :, :])
    return np.concatenate([(LD(1) - lam.sum(axis=2))[:, :, None], lam], axis=2)


def locate(X, cells, pts):
    """(cell (P,), lam (P, D + 1) longdouble, mins (P, nc) longdouble): the rule, on exact-to-longdouble coordinates."""
    L = barycentric_all(X, cells, pts)
    mins = L.min(axis=2)
    k = np.argmax(mins, axis=1)          # the first of equal maxima: the lowest cell
    return k, L[np.arange(L.shape[0]), k], mins


def grad_lambda(X, cells, which):
    """g (P, D + 1, D) longdouble: the gradients of the barycentric coordinates of the cells `which`."""
    T, _ = edge_matrices(X, np.asarray(cells)[np.asarray(which)])
    Ti = inverse(T)
    return np.concatenate([-Ti.sum(axis=1)[:, None, :], Ti], axis=1)


def shape(degree, lam):
    """N (P, nodes per cell) at lam (P, D + 1), in record order: the vertices, then the edges of P2_EDGES."""
    lam = np.asarray(lam, dtype=LD)
    D = lam.shape[1] - 1
    if degree == 1:
        return lam
    return np.stack([lam[:, i] * (2 * lam[:, i] - 1) for i in range(D + 1)] + [4 * lam[:, a] * lam[:, b] for a, b in P2_EDGES[D]], axis=1)


def dshape(degree, lam, g):
    """dN (P, nodes per cell, D) at lam, g the gradients of the barycentric coordinates."""
    lam, g = np.asarray(lam, dtype=LD), np.asarray(g, dtype=LD)
    D = lam.shape[1] - 1
    if degree == 1:
        return g
    return np.stack([(4 * lam[:, i] - 1)[:, None] * g[:, i] for i in range(D + 1)] +
                    [4 * (lam[:, b, None] * g[:, a] + lam[:, a, None] * g[:, b]) for a, b in P2_EDGES[D]], axis=1)


def sample(degree, records, which, lam, u, ncomp, g=None):
    """values (P, ncomp) - with g: gradients (P, ncomp, D) - of the nodal field u (node * ncomp + c) at (cell, lam), longdouble,
    and the sums of the absolute terms sum_a |N_a u_a| (values) or sum_a |dN_a| |u_a| (gradients) of the same shape."""
    nodes = np.asarray(records)[np.asarray(which)]
    un = np.asarray(u, dtype=LD)[nodes[:, :, None] * ncomp + np.arange(ncomp)[None, None, :]]      # (P, nodes, ncomp)
    if g is None:
        N = shape(degree, lam)
        return np.einsum("pa,pac->pc", N, un), np.einsum("pa,pac->pc", np.abs(N), np.abs(un))
    dN = dshape(degree, lam, g)
    return np.einsum("pad,pac->pcd", dN, un), np.einsum("pad,pac->pcd", np.abs(dN), np.abs(un))


def interior_points(X, cells, seed, floor=0.05):
    """One point per cell with seeded barycentric coordinates >= floor: (points (nc, D) float64, lam (nc, D + 1) float64)."""
    X = np.asarray(X, dtype=np.float64).reshape(len(X), -1)
    D = X.shape[1]
    rng = np.random.default_rng(seed)
    w = rng.dirichlet(np.ones(D + 1), size=len(cells))
    lam = floor + (1.0 - (D + 1) * floor) * w
    V = X[np.asarray(cells)[:, :D + 1]]
    return np.einsum("ca,cad->cd", lam, V), lam


def tie_points(X, cells):
    """All vertices, edge midpoints and (3-D: face, 2-D: cell) centroids of the mesh: points that several cells share."""
    X = np.asarray(X, dtype=np.float64).reshape(len(X), -1)
    D = X.shape[1]
    C = np.asarray(cells)[:, :D + 1]
    out = [X]
    if D >= 1:
        pairs = np.unique(np.concatenate([np.sort(C[:, list(e)], axis=1) for e in itertools.combinations(range(D + 1), 2)]), axis=0)
        out.append(0.5 * (X[pairs[:, 0]] + X[pairs[:, 1]]))
    if D >= 2:
        tri = np.unique(np.concatenate([np.sort(C[:, list(f)], axis=1) for f in itertools.combinations(range(D + 1), 3)]), axis=0)
        out.append((X[tri[:, 0]] + X[tri[:, 1]] + X[tri[:, 2]]) / 3.0)
    return np.concatenate(out, axis=0)


def jitter(mesh_coords, h, seed, amount=0.2):
    """The coordinates moved by at most amount * h per axis (seeded)."""
    rng = np.random.default_rng(seed)
    X = np.asarray(mesh_coords, dtype=np.float64)
    return X + amount * h * rng.uniform(-1.0, 1.0, size=X.shape)
