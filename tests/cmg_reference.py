"""CPU restatement (numpy / scipy.sparse, tests only) of the component-wise multigrid preconditioner for vector-valued P1 operators
on box lattices (pgdrome_amd/csrc/pgd_vmg.hip: k_cmg_extract / k_cmg_split / k_cmg_merge, PGD_TUNE_PCG_PRECOND = 3,
settings["preconditioner"] = "cmg"), built on tests/vmg_reference.py:

  * dofs node-major, dof = ncomp * node + c, node = x + nx (y + ny z);  s = diag(A)^-1/2;
  * per component c the scalar operator B_c = (S A S)[c::ncomp, c::ncomp] on the base lattice, its diagonal SET to exactly 1
    (identity rows stay identity); an eliminated node of component c is a row of B_c without couplings - the components may have
    different eliminated sets;
  * M_c: one V(1,1) cycle of vmg_reference on B_c (l1-Jacobi, Galerkin coarse operators, coarsest level <= 4096 nodes);
  * preconditioner of the UNSCALED system: z[c::ncomp] = s_c * M_c(s_c * r[c::ncomp]);
  * PCG: the textbook two-reduction recurrence on A itself, x = b on the eliminated dofs before the first residual, stop test
    r.r <= max(rtol^2 b.b, atol^2) on the true residual of the recurrence.
"""
import numpy as np
import scipy.sparse as sps

from tests import vmg_reference as V


def scaling(A):
    """s = diag(A)^-1/2 as the library forms it: the square root of the inverse diagonal."""
    return np.sqrt(1.0 / sps.csr_matrix(A).diagonal())


def component_operator(A, ncomp, c, s=None):
    """B_c = (S A S)[c::ncomp, c::ncomp] with its diagonal set to exactly 1."""
    A = sps.csr_matrix(A, dtype=np.float64)
    s = scaling(A) if s is None else s
    S = sps.diags(s)
    B = (S @ A @ S).tocsr()[c::ncomp, :][:, c::ncomp].tocsr()
    B = (B - sps.diags(B.diagonal()) + sps.identity(B.shape[0])).tocsr()      # (d - d = 0 exactly, then + 1)
    assert np.all(B.diagonal() == 1.0)
    return B


def build(A, shape, ncomp):
    """The ncomp hierarchies (lists of vmg_reference levels) of the diagonal blocks of the scaled operator; None: the base lattice
    has at most 4096 nodes, no hierarchy."""
    s = scaling(A)
    levels = [V.build(component_operator(A, ncomp, c, s), shape) for c in range(ncomp)]
    return None if any(l is None for l in levels) else levels


def eliminated_dofs(levels):
    """Boolean mask over the dofs: eliminated in its component's hierarchy."""
    ncomp = len(levels)
    el = np.zeros(ncomp * levels[0][0].el.size, dtype=bool)
    for c in range(ncomp):
        el[c::ncomp] = levels[c][0].el
    return el


def apply(levels, s, r):
    """z = M r of the unscaled system."""
    ncomp = len(levels)
    z = np.empty_like(r)
    for c in range(ncomp):
        z[c::ncomp] = s[c::ncomp] * V.vcycle(levels[c], s[c::ncomp] * r[c::ncomp])
    return z


def pcg(A, b, shape=None, ncomp=3, rtol=1e-10, maxit=5000, precond="cmg", atol=0.0, x0=None):
    """The unscaled recurrence of pgd_pcg_solve with z = M r (precond="cmg") or z = D^-1 r ("jacobi").
    Returns (x, iterations, relres)."""
    A = sps.csr_matrix(A, dtype=np.float64)
    x = np.zeros(A.shape[0]) if x0 is None else np.array(x0, dtype=np.float64)
    if precond == "cmg":
        levels = build(A, shape, ncomp)
        assert levels is not None
        s = scaling(A)
        el = eliminated_dofs(levels)
        x[el] = b[el]
        M = lambda v: apply(levels, s, v)
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


# ---- lattice helpers of the tests ---------------------------------------------------------------------------------------------

def node_sets(shape):
    """Node index sets of the lattice: the face x = 0, the face z = 0, the hull."""
    nx, ny, nz = shape
    x, y, z = V.node_coords(shape)
    hull = (x == 0) | (y == 0) | (z == 0) | (x == nx - 1) | (y == ny - 1) | (z == nz - 1)
    return {"x0": np.where(x == 0)[0], "z0": np.where(z == 0)[0], "hull": np.where(hull)[0]}


def dofs_of(nodes, ncomp, comps=None):
    """Sorted int32 dofs of the given components (default: all) on the given nodes."""
    comps = range(ncomp) if comps is None else comps
    return np.unique(np.concatenate([np.asarray(nodes) * ncomp + c for c in comps])).astype(np.int32)


def dirichlet_dofs(shape, ncomp, case):
    """The Dirichlet sets of the tests: "clamped" (all components on x = 0), "hull" (all on the hull), "roller" (only u_x on x = 0
    and only u_z on z = 0: three different eliminated sets)."""
    sets = node_sets(shape)
    if case == "clamped":
        return dofs_of(sets["x0"], ncomp)
    if case == "hull":
        return dofs_of(sets["hull"], ncomp)
    if case == "roller":
        return np.unique(np.concatenate([dofs_of(sets["x0"], ncomp, [0]), dofs_of(sets["z0"], ncomp, [2])])).astype(np.int32)
    raise ValueError(case)


# ---- the operator families of the tests, through the frontend (whatever backend is set) -----------------------------------------

def vector_space(shape, degree=1, step=1.0 / 16):
    """VectorFunctionSpace on the 6-tets-per-cube box with shape = (nx, ny, nz) NODES and dyadic vertex coordinates."""
    from pgdrome_amd import fem
    cells = tuple(n - 1 for n in shape)
    mesh = fem.BoxMesh(fem.Point(0.0, 0.0, 0.0), fem.Point(*(c * step for c in cells)), *cells)
    return fem.VectorFunctionSpace(mesh, "P", degree)


def frontend_operator(Vh, family, bc, nu=0.3, k_found=2.0):
    """(fem.Matrix with the Dirichlet dofs `bc` registered, the combined operator read back from the backend as scipy CSR in the
    backend's own dof order - node-major on the lattice - so that device and numpy see the same numbers).
    family "elastic": the spatial operator of problems.elastic_block, eps(v) : C(nu) eps(u) + k_found v . u;
    "graded": the one of problems.graded_block at theta = 1, (1 + g) eps(v) : C eps(u) + k_found v . u with g = x0 + 4 x1 x2."""
    from pgdrome_amd import fem, problems
    u, v = fem.TrialFunction(Vh), fem.TestFunction(Vh)
    energy = fem.inner(problems._voigt_C(nu) * problems._strain(u), problems._strain(v))
    if family == "elastic":
        a = energy * fem.dx
    elif family == "graded":
        S = fem.FunctionSpace(Vh.mesh(), "P", 1)
        g = fem.interpolate(fem.Expression("x[0] + 4*x[1]*x[2]", degree=1), S)
        a = energy * fem.dx + g * energy * fem.dx
    else:
        raise ValueError(family)
    if k_found:
        a = a + fem.Constant(k_found) * fem.inner(u, v) * fem.dx
    A = fem.assemble(a)
    # `bc` is a dof list (the roller case fixes single components of a node, which DirichletBC on the whole space cannot say), so
    # the two statements of Matrix.apply_dirichlet are restated here: the sorted eliminated dofs, and the reset of the cached
    # combined operator (`_op`), which Matrix.op() must not hand out for another Dirichlet set.  tests/test_cmg_gpu.py checks that
    # the eliminated dofs of the solve are exactly these, so a frontend that stops honouring the two fields fails there.
    A.bc_vertices = np.unique(np.asarray(bc, dtype=np.int32))
    A._op = 0
    return A, read_back(A)


def read_back(A):
    from pgdrome_amd import fem
    be = fem.get_backend()
    op = A.op()
    try:
        rp, cols = be.mesh_pattern(A.lay.handle())
        vals = be.atom_values(op, cols.size)
    finally:
        be.atom_free(op)
    return sps.csr_matrix((np.asarray(vals, dtype=np.float64), np.asarray(cols), np.asarray(rp)), shape=(A.lay.n, A.lay.n))


def direct_solve(A, b, shape, ncomp):
    """scipy.sparse.linalg.spsolve of A x = b, the unknowns renumbered by a geometric nested dissection of the lattice first (the
    same direct solution; SuperLU's own orderings fill three times as much on a 3-D block operator)."""
    import scipy.sparse.linalg as spla
    X = V.node_coords(shape)
    parts = []

    def dissect(ix, lo, hi):
        if ix.size <= 64:
            parts.append(ix)
            return
        d = int(np.argmax([h - l for l, h in zip(lo, hi)]))
        mid = (lo[d] + hi[d]) // 2
        c = X[d][ix]
        dissect(ix[c < mid], lo, hi[:d] + (mid - 1,) + hi[d + 1:])
        dissect(ix[c > mid], lo[:d] + (mid + 1,) + lo[d + 1:], hi)
        parts.append(ix[c == mid])
    dissect(np.arange(X[0].size), (0, 0, 0), tuple(s - 1 for s in shape))
    p = (np.concatenate(parts)[:, None] * ncomp + np.arange(ncomp)[None, :]).ravel()
    A = sps.csr_matrix(A)
    x = np.empty(A.shape[0])
    x[p] = spla.spsolve(A[p][:, p].tocsc(), np.asarray(b)[p], permc_spec="NATURAL")
    return x
