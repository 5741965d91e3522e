"""CPU restatement (numpy / scipy.sparse, tests only) of the p-multigrid preconditioner for P2 operators on box lattices
(pgdrome_amd/csrc/pgd_pmg.hip, PGD_TUNE_PCG_PRECOND = 4, settings["preconditioner"] = "pmg"), with EXPLICIT matrices where the device
gathers through tables; built on tests/vmg_reference.py (the V-cycle) and the helpers of tests/cmg_reference.py:

  * nodes: the vertices of the lattice in lattice order (node = x + nx (y + ny z)), then one node per mesh edge
    (DofLayout.edge_vertices); dof = ncomp * node + c;
  * an ELIMINATED dof is a row of A without a non-zero off-diagonal entry (identity rows);
  * per component c the interpolation P_c from P1 on the vertex lattice: 1 from a vertex to its own node, 1/2 from each end
    vertex to an edge node, rows of eliminated P2 dofs and columns of eliminated vertex dofs dropped;
  * B_c = P_c^T A[c::ncomp, c::ncomp] P_c with the identity on the eliminated vertices - A is NOT scaled; M_c: one V(1,1) cycle of
    vmg_reference on B_c (l1-Jacobi, Galerkin coarse operators, coarsest level <= 4096 nodes);
  * preconditioner: z = D^-1 r + sum_c P_c M_c(P_c^T r[c::ncomp]) in component c, z = 0 on eliminated dofs;
  * PCG: the textbook two-reduction recurrence on A itself, x = b on the eliminated dofs before the first residual, stop test
    r.r <= max(rtol^2 b.b, atol^2) on the residual of the recurrence.
"""
import numpy as np
import scipy.sparse as sps

from tests import cmg_reference as CM
from tests import vmg_reference as V


def interpolation(nvert, edge_vertices):
    """P of one component without eliminations: (nvert + n_edges) x nvert, entries 1 and 1/2."""
    ev = np.asarray(edge_vertices, dtype=np.int64).reshape(-1, 2)
    ne = ev.shape[0]
    rows = np.concatenate([np.arange(nvert), nvert + np.arange(ne), nvert + np.arange(ne)])
    cols = np.concatenate([np.arange(nvert), ev[:, 0], ev[:, 1]])
    vals = np.concatenate([np.ones(nvert), np.full(2 * ne, 0.5)])
    return sps.csr_matrix((vals, (rows, cols)), shape=(nvert + ne, nvert))


def eliminated_dofs(A):
    """Boolean mask over the dofs: rows of A without couplings."""
    return V.eliminated_rows(A)


class Hierarchy:
    pass


def component(A, nvert, edge_vertices, ncomp, c, el=None):
    """(B_c, P_c, eliminated vertices of component c): the Galerkin block with the identity on the eliminated vertices."""
    A = sps.csr_matrix(A, dtype=np.float64)
    el = eliminated_dofs(A) if el is None else el
    elc = el[c::ncomp]
    elv = elc[:nvert]
    P = (sps.diags((~elc).astype(np.float64)) @ interpolation(nvert, edge_vertices) @ sps.diags((~elv).astype(np.float64))).tocsr()
    P.eliminate_zeros()
    Acc = A[c::ncomp, :][:, c::ncomp].tocsr()
    B = (P.T @ Acc @ P + sps.diags(elv.astype(np.float64))).tocsr()
    return B, P, elv


def build(A, shape, edge_vertices, ncomp):
    """What the solve prepares: eliminated dofs, D^-1, and per component (P_c, levels of vmg_reference on B_c).  None: the vertex
    lattice has at most 4096 nodes, no hierarchy."""
    A = sps.csr_matrix(A, dtype=np.float64)
    nvert = int(np.prod(shape))
    H = Hierarchy()
    H.ncomp, H.el, H.dinv = ncomp, eliminated_dofs(A), 1.0 / A.diagonal()
    H.P, H.levels, H.B = [], [], []
    for c in range(ncomp):
        B, P, _ = component(A, nvert, edge_vertices, ncomp, c, H.el)
        levels = V.build(B, shape)
        if levels is None:
            return None
        H.P.append(P); H.levels.append(levels); H.B.append(B)
    return H


def apply(H, r):
    """z = M r."""
    z = H.dinv * r
    for c in range(H.ncomp):
        z[c::H.ncomp] += H.P[c] @ V.vcycle(H.levels[c], H.P[c].T @ r[c::H.ncomp])
    z[H.el] = 0.0
    return z


def pcg(A, b, shape=None, edge_vertices=None, ncomp=1, rtol=1e-10, maxit=5000, precond="pmg", atol=0.0):
    """The unscaled recurrence of pgd_pcg_solve with z = M r (precond="pmg") or z = D^-1 r ("jacobi") from a zero start.
    Returns (x, iterations, relres)."""
    A = sps.csr_matrix(A, dtype=np.float64)
    x = np.zeros(A.shape[0])
    if precond == "pmg":
        H = build(A, shape, edge_vertices, ncomp)
        assert H is not None
        x[H.el] = b[H.el]
        M = lambda v: apply(H, v)
    else:
        dinv = 1.0 / A.diagonal()
        M = lambda v: dinv * v
    r = b - A @ x
    bb = float(b @ b)
    tol2 = max(rtol * rtol * bb, atol * atol)
    rr = float(r @ r)
    it = 0
    if rr > tol2:
        z = M(r)
        p = z.copy()
        rz = float(r @ z)
        while it < maxit:
            q = A @ p
            a = rz / float(p @ q)
            x += a * p
            r -= a * q
            it += 1
            rr = float(r @ r)
            if rr <= tol2:
                break
            z = M(r)
            rz2 = float(r @ z)
            p = z + (rz2 / rz) * p
            rz = rz2
    return x, it, (rr / bb) ** 0.5 if bb > 0 else 0.0


def galerkin_bound(A, nvert, edge_vertices, ncomp, c, el=None):
    """(|P_c|^T |A_cc| |P_c|, the number of terms summed into every entry of B_c): what bounds the rounding of a Galerkin block
    formed in any order - the weights 1, 1/2 and 1/4 are exact, only the additions round."""
    A = sps.csr_matrix(A, dtype=np.float64)
    _, P, _ = component(A, nvert, edge_vertices, ncomp, c, el)
    Acc = A[c::ncomp, :][:, c::ncomp].tocsr()
    Acc.eliminate_zeros()
    mag = (P.T @ abs(Acc) @ P).tocsr()
    Pn, An = P.copy(), Acc.copy()
    Pn.data[:] = 1.0
    An.data[:] = 1.0
    return mag, (Pn.T @ An @ Pn).tocsr()


def slots_of(B, shape):
    """The 8 upper slot arrays of the diagonal form of a 15-point operator B: slot dx + 2 dy + 4 dz of node I = B[I, I + (dx, dy, dz)]
    (0 where the neighbour lies outside the lattice or nothing is stored), and the mask of the entries B stores."""
    nx, ny, nz = shape
    n = nx * ny * nz
    x, y, z = V.node_coords(shape)
    B = sps.csr_matrix(B)
    S = sps.csr_matrix((np.ones(B.nnz), B.indices, B.indptr), shape=B.shape)
    vals, stored = np.zeros((8, n)), np.zeros((8, n), dtype=bool)
    for t in range(8):
        dx, dy, dz = t & 1, (t >> 1) & 1, t >> 2
        ok = (x + dx < nx) & (y + dy < ny) & (z + dz < nz)
        I = np.where(ok)[0]
        J = I + dx + nx * (dy + ny * dz)
        vals[t, I] = np.asarray(B[I, J]).ravel()
        stored[t, I] = np.asarray(S[I, J]).ravel() != 0
    return vals, stored


# ---- P2 spaces and operators of the tests, through the frontend (whatever backend is set) -------------------------------------

def space(shape, ncomp, step=1.0 / 16):
    """P2 space on the 6-tets-per-cube box with shape = (nx, ny, nz) VERTICES and dyadic vertex coordinates: a FunctionSpace
    (ncomp = 1) or a VectorFunctionSpace."""
    from pgdrome_amd import fem
    if ncomp > 1:
        return CM.vector_space(shape, degree=2, step=step)
    cells = tuple(n - 1 for n in shape)
    mesh = fem.BoxMesh(fem.Point(0.0, 0.0, 0.0), fem.Point(*(c * step for c in cells)), *cells)
    return fem.FunctionSpace(mesh, "P", 2)


def base_layout(Vh):
    """The scalar P2 layout behind a space."""
    lay = Vh._lay
    return getattr(lay, "base", lay)


def node_sets(Vh):
    """P2 node index sets: the face x = 0, the face z = 0, the hull."""
    X = base_layout(Vh).coords
    lo, hi = X.min(axis=0), X.max(axis=0)
    return {"x0": np.where(X[:, 0] == lo[0])[0], "z0": np.where(X[:, 2] == lo[2])[0],
            "hull": np.where(np.any((X == lo) | (X == hi), axis=1))[0]}


def dirichlet_dofs(Vh, ncomp, case):
    """The Dirichlet sets of the tests on P2 nodes: "clamped" (all components on x = 0), "hull", "roller" (only u_x on x = 0 and only
    u_z on z = 0: three different eliminated sets)."""
    sets = node_sets(Vh)
    if case == "clamped":
        return CM.dofs_of(sets["x0"], ncomp)
    if case == "hull":
        return CM.dofs_of(sets["hull"], ncomp)
    if case == "roller":
        return np.unique(np.concatenate([CM.dofs_of(sets["x0"], ncomp, [0]), CM.dofs_of(sets["z0"], ncomp, [2])])).astype(np.int32)
    raise ValueError(case)


def scalar_operator(Vh, bc):
    """(fem.Matrix of the P2 stiffness form with the Dirichlet dofs `bc` registered, the combined operator read back as scipy CSR):
    the scalar counterpart of cmg_reference.frontend_operator (the same two statements of Matrix.apply_dirichlet)."""
    from pgdrome_amd import fem
    u, v = fem.TrialFunction(Vh), fem.TestFunction(Vh)
    A = fem.assemble(fem.inner(fem.grad(u), fem.grad(v)) * fem.dx)
    A.bc_vertices = np.unique(np.asarray(bc, dtype=np.int32))
    A._op = 0
    return A, CM.read_back(A)


# (name -> (ncomp, Dirichlet set, k_found)): elasticity (nu = 0.3) clamped on x = 0 with a foundation term; the same with the hull
# eliminated; roller supports (+ foundation: SPD); the scalar stiffness with the hull eliminated
CASES = {"clamped": (3, "clamped", 2.0), "hull": (3, "hull", 0.0), "roller": (3, "roller", 2.0), "scalar_hull": (1, "hull", 0.0)}


def operator(Vh, name):
    """(fem.Matrix, scipy CSR, Dirichlet dofs) of a case of CASES on the space Vh."""
    ncomp, case, k_found = CASES[name]
    bc = dirichlet_dofs(Vh, ncomp, case)
    if ncomp == 1:
        A, M = scalar_operator(Vh, bc)
    else:
        A, M = CM.frontend_operator(Vh, "elastic", bc, k_found=k_found)
    return A, M, bc


def direct_solve(A, b, Vh, ncomp):
    """scipy.sparse.linalg.spsolve of A x = b on the free dofs (x = b / diagonal on the identity rows), the unknowns renumbered by a
    geometric nested dissection first: the P2 nodes fill the lattice of half steps, and a plane of VERTEX coordinates separates
    the nodes on its two sides (no tetrahedron crosses it).  The same direct solution; SuperLU's own orderings fill far more."""
    import scipy.sparse.linalg as spla
    A = sps.csr_matrix(A, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    X = base_layout(Vh).coords
    H = np.stack([np.searchsorted(np.unique(X[:, d]), X[:, d]) for d in range(3)], axis=0)      # half-step indices: even = vertex planes
    parts = []

    def dissect(ix, lo, hi):
        d = int(np.argmax([h - l for l, h in zip(lo, hi)]))
        mid = 2 * ((lo[d] + hi[d] + 2) // 4)
        if ix.size <= 96 or not lo[d] < mid < hi[d]:
            parts.append(ix)
            return
        c = H[d][ix]
        dissect(ix[c < mid], lo, hi[:d] + (mid - 1,) + hi[d + 1:])
        dissect(ix[c > mid], lo[:d] + (mid + 1,) + lo[d + 1:], hi)
        parts.append(ix[c == mid])
    dissect(np.arange(X.shape[0]), (0, 0, 0), tuple(int(H[d].max()) for d in range(3)))
    p = (np.concatenate(parts)[:, None] * ncomp + np.arange(ncomp)[None, :]).ravel()
    free = ~eliminated_dofs(A)
    p = p[free[p]]
    x = b / A.diagonal()
    x[p] = spla.spsolve(A[p][:, p].tocsc(), b[p], permc_spec="NATURAL")
    return x
