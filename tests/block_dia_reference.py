"""CPU restatement (numpy / scipy.sparse, tests only) of the row-diagonal form of a vector-valued P1 operator on a box lattice
(pgdrome_amd/csrc/pgd_bdia.hip: k_bdia_extract / k_spmv_bdia, PGD_TUNE_SPMV_BLOCK_DIA, settings["block_product"] = "diagonal"):

  * dofs node-major, dof = ncomp * node + c, node = x + nx (y + ny z), P = nx ny;
  * the 15 lattice steps of the 6-tetrahedra-per-cube pattern are +-(dx, dy, dz) with (dx, dy, dz) in {0, 1}^3; slot t = 0..14
    numbers them in ascending node offset: t = 7 - s for the step -(dx, dy, dz), t = 7 + s for +(dx, dy, dz), s = dx + 2 dy + 4 dz
    (t = 7: the node itself);
  * array (t, d) holds at row r = ncomp i + c the entry a(r, ncomp (i + off_t) + d), 0.0 where the row stores none;
  * the product of row r: acc = 0.0, then for t ascending and d ascending acc += a_td[r] * x[column] - with nx, ny >= 2 that is
    the sorted CSR row.
"""
import numpy as np
import scipy.sparse as sps

NT = 15


def step_of(t):
    """(dx, dy, dz) of slot t, each in {-1, 0, 1}."""
    s = abs(t - 7)
    sign = -1 if t < 7 else 1
    return sign * (s & 1), sign * ((s >> 1) & 1), sign * (s >> 2)


def slot_of(step):
    """Slot t of a lattice step, None where the step is not one of the 15."""
    dx, dy, dz = step
    lo, hi = min(step), max(step)
    if lo < -1 or hi > 1 or (lo < 0 and hi > 0):
        return None
    s = abs(dx) + 2 * abs(dy) + 4 * abs(dz)
    return 7 - s if lo < 0 else 7 + s


def node_offset(t, shape):
    dx, dy, dz = step_of(t)
    return dx + shape[0] * dy + shape[0] * shape[1] * dz


def node_position(i, shape):
    nx, ny, _ = shape
    return i % nx, (i // nx) % ny, i // (nx * ny)


def neighbour(i, t, shape):
    """Node i + off_t, None where it lies outside the lattice."""
    pos = node_position(i, shape)
    q = tuple(p + d for p, d in zip(pos, step_of(t)))
    if any(c < 0 or c >= n for c, n in zip(q, shape)):
        return None
    return q[0] + shape[0] * (q[1] + shape[1] * q[2])


def walk(r, shape, ncomp):
    """The columns row r visits, t ascending and d ascending inside t, neighbours outside the lattice left out."""
    i = r // ncomp
    out = []
    for t in range(NT):
        j = neighbour(i, t, shape)
        if j is not None:
            out.extend(ncomp * j + d for d in range(ncomp))
    return out


def pattern(shape, ncomp):
    """The blocked 15-point pattern as a scipy CSR matrix of ones with sorted indices."""
    n = shape[0] * shape[1] * shape[2] * ncomp
    rows, cols = [], []
    for r in range(n):
        w = walk(r, shape, ncomp)
        rows.extend([r] * len(w))
        cols.extend(w)
    M = sps.csr_matrix((np.ones(len(rows)), (rows, cols)), shape=(n, n))
    M.sort_indices()
    return M


def to_form(M, shape, ncomp):
    """The 15 ncomp arrays of a CSR matrix on the blocked lattice: form[t * ncomp + d, r].  Raises on an entry off the pattern."""
    M = sps.csr_matrix(M)
    n = M.shape[0]
    form = np.zeros((NT * ncomp, n))
    for r in range(n):
        pi = node_position(r // ncomp, shape)
        for k in range(M.indptr[r], M.indptr[r + 1]):
            col = int(M.indices[k])
            pj = node_position(col // ncomp, shape)
            t = slot_of(tuple(b - a for a, b in zip(pi, pj)))
            if t is None:
                raise ValueError("row %d: column %d is off the pattern" % (r, col))
            form[t * ncomp + col % ncomp, r] = M.data[k]
    return form


def product(form, shape, ncomp, x):
    """y = A x from the form, the chain of k_spmv_bdia (plain multiply-add here: exact on integer data).  A neighbour outside the
    lattice meets the coefficient 0.0 and the row's own x."""
    n = form.shape[1]
    y = np.zeros(n)
    for r in range(n):
        i = r // ncomp
        acc = 0.0
        for t in range(NT):
            j = neighbour(i, t, shape)
            for d in range(ncomp):
                acc += form[t * ncomp + d, r] * (x[ncomp * j + d] if j is not None else x[r])
        y[r] = acc
    return y
