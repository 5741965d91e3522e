"""CPU restatement (numpy / scipy.sparse, tests only) of the variable-coefficient multigrid preconditioner of
pgdrome_amd/csrc/pgd_vmg.hip (PGD_TUNE_PCG_PRECOND = 2, settings["preconditioner"] = "vmg").

It restates the build's own algorithm with EXPLICIT matrices - P as a sparse matrix, the coarse operators as the sparse products
P^T A P - where the device gathers through slot arrays, so that the two share nothing but the mathematics:

  * lattice of nx x ny x nz nodes, row = x + nx (y + ny z); the 15-point pattern E = {+-(dx, dy, dz), d in {0, 1}^3};
  * an ELIMINATED node is a row without couplings (identity rows, columns zeroed); coarse node k is fine node 2k and is
    eliminated iff that node is; a far face with an even node count has no coarse counterpart (the last coarse node keeps its
    own state, beyond it zero);
  * P: weight 1 at the node, 1/2 at its 14 pattern neighbours, rows of eliminated fine nodes and columns of eliminated coarse
    nodes dropped; coarse operator P^T A P, identity on the eliminated coarse nodes;
  * levels: coarsen while a level has more than 4096 nodes; a lattice of at most 4096 nodes has no hierarchy;
  * smoother l1-Jacobi w_i = 1 / sum_j |a_ij| (0 on eliminated nodes); V(1,1) with the pre-smoothing step from a zero start
    folded in: u = W b, t = b - A u, e = cycle(P^T t), v = u + P e, x = v + W (b - A v); coarsest level: x = W b, then 23 more
    steps x += W (b - A x);
  * PCG on the scaled system A~ = D^-1/2 A D^-1/2 (unit diagonal), x~ = s b on the eliminated rows from the start, stop test on
    the TRUE residual: |b - A x|_2 <= rtol |b|_2.
"""
from fractions import Fraction

import numpy as np
import scipy.sparse as sps

PATTERN = [(dx, dy, dz) for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)]
PATTERN = PATTERN + [(-dx, -dy, -dz) for dx, dy, dz in PATTERN[1:]]           # 15 vectors, the zero vector first
BOTTOM_MAX = 4096
BOTTOM_SWEEPS = 24


def node_coords(shape):
    nx, ny, nz = shape
    i = np.arange(nx * ny * nz)
    return i % nx, (i // nx) % ny, i // (nx * ny)


def on_pattern_mask(A, shape):
    """Per stored entry of A (COO order): does column - row lie on the 15-point pattern of the lattice?"""
    A = A.tocoo()
    x, y, z = node_coords(shape)
    dx, dy, dz = x[A.col] - x[A.row], y[A.col] - y[A.row], z[A.col] - z[A.row]
    up = (dx >= 0) & (dy >= 0) & (dz >= 0) & (dx <= 1) & (dy <= 1) & (dz <= 1)
    dn = (dx <= 0) & (dy <= 0) & (dz <= 0) & (dx >= -1) & (dy >= -1) & (dz >= -1)
    return A, up | dn


def off_pattern_max(A, shape):
    """Largest |entry| of A off the 15-point pattern (0 if none is stored), and the largest |entry| at all."""
    A, on = on_pattern_mask(A, shape)
    d = np.abs(A.data)
    off = d[~on]
    return (off.max() if off.size else 0), (d.max() if d.size else 0)


def eliminated_rows(A):
    """Rows of A without couplings."""
    A = sps.csr_matrix(A)
    off = A - sps.diags(A.diagonal())
    off.eliminate_zeros()
    return np.diff(off.indptr) == 0


def coarse_shape(shape):
    return tuple((s + 1) // 2 for s in shape)


def interpolation(shape, el, dtype=np.float64):
    """(P, coarse shape, eliminated coarse nodes): P is n_f x n_c with entries 1 and 1/2 (dtype=object: Fractions; dtype=np.int64:
    2 P, entries 2 and 1)."""
    nx, ny, nz = shape
    cs = coarse_shape(shape)
    cx, cy, cz = node_coords(cs)
    K = np.arange(cx.size)
    elc = el[2 * cx + nx * (2 * cy + ny * 2 * cz)]
    rows, cols, vals = [], [], []
    one, half = (2, 1) if dtype == np.int64 else (1.0, 0.5)
    for k, (dx, dy, dz) in enumerate(PATTERN):
        fx, fy, fz = 2 * cx + dx, 2 * cy + dy, 2 * cz + dz
        ok = (fx >= 0) & (fy >= 0) & (fz >= 0) & (fx < nx) & (fy < ny) & (fz < nz) & ~elc
        i = (fx + nx * (fy + ny * fz))[ok]
        keep = ~el[i]
        rows.append(i[keep]); cols.append(K[ok][keep]); vals.append(np.full(keep.sum(), one if k == 0 else half))
    P = sps.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(nx * ny * nz, K.size), dtype=dtype)
    return P, cs, elc


def galerkin(A, P, elc):
    """P^T A P with the identity on the eliminated coarse nodes."""
    Ac = (P.T @ sps.csr_matrix(A) @ P).tocsr()
    return (Ac + sps.diags(elc.astype(Ac.dtype))).tocsr()


def exact_integer_form(vals, rp, cols, n):
    """Exact Fractions on a CSR pattern -> (int64 CSR matrix L A, L): L the least common multiple of the denominators."""
    import math
    L = 1
    for v in vals:
        L = L * v.denominator // math.gcd(L, v.denominator)
    ints = [int(v * L) for v in vals]
    assert max(abs(t) for t in ints) < 2 ** 62
    return sps.csr_matrix((np.array(ints, dtype=np.int64), cols, rp), shape=(n, n)), L


def apply_dirichlet_exact(A, bc):
    """Integer / float CSR matrix with the rows and columns of bc replaced by the identity."""
    n = A.shape[0]
    keep = np.ones(n, dtype=A.dtype)
    keep[bc] = 0
    Dk = sps.diags(keep, dtype=A.dtype, format="csr")
    out = (Dk @ A @ Dk + sps.diags(1 - keep, dtype=A.dtype, format="csr")).tocsr()
    assert out.dtype == A.dtype
    out.eliminate_zeros()
    return out


def integer_hierarchy(A, shape, el):
    """The Galerkin operators of an INTEGER matrix A in exact integer arithmetic: level l holds 4^l P^T..A..P (2 P has integer
    entries).  Yields (level matrix, shape) for every level below the finest down to the first with at most 4096 nodes - and one
    beyond, so that small boxes show at least two coarse levels."""
    out = []
    while True:
        P2, cs, elc = interpolation(shape, el, dtype=np.int64)
        # no sum of the product can leave int64: the same product of the absolute values, in floating point, bounds every one
        assert (P2.T.astype(np.float64) @ abs(A).astype(np.float64) @ P2.astype(np.float64)).max() < 2.0 ** 62
        A = ((P2.T @ A @ P2).tocsr() + sps.diags(elc.astype(np.int64), dtype=np.int64, format="csr")).tocsr()
        assert A.dtype == np.int64
        shape, el = cs, elc
        out.append((A, shape))
        if min(shape) < 3 or len(out) >= 2 and A.shape[0] <= BOTTOM_MAX:
            return out


def scale_unit(A):
    """(D^-1/2 A D^-1/2 with its diagonal SET to exactly 1, s = d^-1/2): the operator the scaled recurrence of pgd_pcg_solve
    works on."""
    A = sps.csr_matrix(A, dtype=np.float64)
    d = A.diagonal()
    s = np.sqrt(1.0 / d)
    S = sps.diags(s)
    B = (S @ A @ S).tolil()
    B.setdiag(1.0)
    return B.tocsr(), s


class Level:
    pass


def build(A, shape):
    """The hierarchy of a (scaled) operator on a lattice; None: at most 4096 nodes, no hierarchy."""
    A = sps.csr_matrix(A, dtype=np.float64)
    if A.shape[0] <= BOTTOM_MAX:
        return None
    levels = []
    el = eliminated_rows(A)
    while True:
        L = Level()
        L.A, L.shape, L.el = A, shape, el
        l1 = np.asarray(abs(A).sum(axis=1)).ravel()
        L.w = np.where(el, 0.0, 1.0 / l1)
        levels.append(L)
        if A.shape[0] <= BOTTOM_MAX:
            return levels
        L.P, shape, el = interpolation(shape, el)
        A = galerkin(A, L.P, el)


def vcycle(levels, b, l=0):
    L = levels[l]
    if l == len(levels) - 1:
        x = L.w * b
        for _ in range(BOTTOM_SWEEPS - 1):
            x = x + L.w * (b - L.A @ x)
        return x
    u = L.w * b
    t = np.where(L.el, 0.0, b - L.A @ u)
    e = vcycle(levels, L.P.T @ t, l + 1)
    v = u + L.P @ e
    return v + L.w * (b - L.A @ v)


def pcg(A, b, shape=None, x0=None, rtol=1e-10, maxit=2000, precond="vmg"):
    """PCG of pgd_pcg_solve on A x = b (A with identity rows on the eliminated nodes): the scaled recurrence, preconditioned by
    the V-cycle (shape given, precond="vmg") or by nothing more than the scaling (= Jacobi-PCG).
    Returns (x, iterations, relres)."""
    At, s = scale_unit(A)
    levels = build(At, shape) if precond == "vmg" else None
    x = np.zeros(A.shape[0]) if x0 is None else np.asarray(x0, dtype=np.float64) / s
    if levels is not None:
        el = levels[0].el
        x[el] = (s * b)[el]
        M = lambda v: vcycle(levels, v)
    else:
        M = lambda v: v
    r = s * b - At @ x
    bb = float(b @ b)
    rr = float((r / s) @ (r / s))
    it = 0
    if rr > rtol * rtol * bb:
        z = M(r)
        p = z.copy()
        rz = float(r @ z)
        while it < maxit:
            q = At @ p
            a = rz / float(p @ q)
            x += a * p
            r -= a * q
            it += 1
            rr = float((r / s) @ (r / s))
            if rr <= rtol * rtol * bb:
                break
            z = M(r)
            rz2 = float(r @ z)
            p = z + (rz2 / rz) * p
            rz = rz2
    return s * x, it, (rr / bb) ** 0.5 if bb > 0 else 0.0


def apply_preconditioner(A, shape):
    """v -> M v of the scaled operator of A (for the symmetry test)."""
    At, _ = scale_unit(A)
    levels = build(At, shape)
    return (lambda v: vcycle(levels, v)), levels


# ---- the operator families of the tests, from the exact references -------------------------------------------------------------

def box(shape_nodes, origin=(0.0, 0.0, 0.0), steps=None):
    """(coords, cells) of the 6-tets-per-cube box with shape_nodes = (nx, ny, nz) NODES; dyadic vertex coordinates."""
    from oracle import fem_numpy as F
    cells = tuple(n - 1 for n in shape_nodes)
    steps = steps or tuple(1.0 / 16 for _ in cells)
    p1 = tuple(o + n * h for o, n, h in zip(origin, cells, steps))
    return F.box_mesh(origin, p1, *cells)


def dirichlet_sets(coords):
    lo, hi = coords.min(axis=0), coords.max(axis=0)
    hull = np.where(np.any((coords <= lo) | (coords >= hi), axis=1))[0]
    face = np.where(coords[:, 2] <= lo[2])[0]
    return {"hull": hull, "face": face, "none": np.zeros(0, dtype=np.int64)}


def inclusion_mask(coords, cells):
    """Cells whose centroid lies in the middle third of the box along every axis (the inclusion of a two-material block)."""
    lo, hi = coords.min(axis=0), coords.max(axis=0)
    c = (coords[cells[:, :4]].mean(axis=1) - lo) / (hi - lo)
    return np.all((c > 1.0 / 3) & (c < 2.0 / 3), axis=1).astype(np.uint8)


def ball_cells(coords, cells, center=None, radius=None):
    """The cells problems.inclusion_heat marks: all four vertices and the midpoint inside the ball (default: centred in the box,
    radius a quarter of its smallest side)."""
    lo, hi = coords.min(axis=0), coords.max(axis=0)
    c = 0.5 * (lo + hi) if center is None else np.asarray(center, dtype=np.float64)
    r = 0.25 * float((hi - lo).min()) if radius is None else float(radius)
    inside = ((coords - c) ** 2).sum(axis=1) <= r * r * (1.0 + 1e-12)
    mid = ((coords[cells[:, :4]].mean(axis=1) - c) ** 2).sum(axis=1) <= r * r * (1.0 + 1e-12)
    return inside[cells[:, :4]].all(axis=1) & mid


def inclusion_operator(n_cells, kappa):
    """(A with the hull eliminated, b = 1 on the free nodes, shape): the spatial operator K_out + kappa K_in of
    problems.inclusion_heat on the unit box with n_cells^3 cells, from the numpy oracle's assembly."""
    from oracle import fem_numpy as F
    coords, cells = F.box_mesh((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), n_cells, n_cells, n_cells)
    sel = ball_cells(coords, cells)
    n = coords.shape[0]
    A = F.assemble_atom(coords, cells[~sel], F.STIFF) + kappa * F.assemble_atom(coords, cells[sel], F.STIFF)
    hull = dirichlet_sets(coords)["hull"]
    A = apply_dirichlet_exact(sps.csr_matrix(A), hull)
    b = np.ones(n)
    b[hull] = 0.0
    return A, b, (n_cells + 1,) * 3


def float_csr(vals, lay):
    return sps.csr_matrix((np.array([float(v) for v in vals]), lay.cols, lay.rp), shape=(lay.n, lay.n))


def frac(x):
    return Fraction(x).limit_denominator(10 ** 6)
