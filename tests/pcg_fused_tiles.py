"""numpy restatement of the overlapped tiles of k_pcg1_fused_march (PGD_TUNE_PCG_FUSED_MARCH): the index logic, no arithmetic claims.

A workgroup owns a patch of 64 x PY rows on the planes [za, zb) of its march.  It stages the direction p with a halo of TWO cells in
x and y on the planes za - 2 .. zb + 1, forms q = A p, r' = r - alpha q and p' = r' + beta p on patch + a one-cell ring for the planes
za - 1 .. zb, and then A p' on the patch for the planes za .. zb - 1.  It reads nothing else: `tile_results` poisons everything outside
those windows with NaN before it computes.

The operator is one 15-point stencil c[dx + 2 dy + 4 dz] with eliminated nodes: q_i = p_i on an eliminated row, else the sum over the
neighbours of c_s p~_j with p~ = 0 on eliminated rows and outside the grid.  Products and sums are plain numpy operations in the order
of the kernel's chain - on both sides of every comparison, so results compare with np.array_equal.
"""
import numpy as np

PAD_LO = 2          # cells below the grid in every direction of the padded arrays (a halo of two)
# the chain of k_spmv_stencil_march: (dz, dy, dx, slot) in its order
CHAIN = ((-1, -1, -1, 7), (-1, -1, 0, 6), (-1, 0, -1, 5), (-1, 0, 0, 4),
         (0, -1, -1, 3), (0, -1, 0, 2), (0, 0, -1, 1), (0, 0, 0, 0), (0, 0, 1, 1), (0, 1, 0, 2), (0, 1, 1, 3),
         (1, 0, 0, 4), (1, 0, 1, 5), (1, 1, 0, 6), (1, 1, 1, 7))


def padded(a, shape, py, fill=0.0):
    """`a` (nz, ny, nx) inside an array with PAD_LO cells below and room for partial tiles and their halos above."""
    nz, ny, nx = shape
    out = np.full((nz + 2 * PAD_LO, ny + 2 * PAD_LO + py, nx + 2 * PAD_LO + 64), fill, dtype=a.dtype)
    out[PAD_LO:PAD_LO + nz, PAD_LO:PAD_LO + ny, PAD_LO:PAD_LO + nx] = a
    return out


def chain(xm, c, z0, z1, y0, y1, x0, x1):
    """The 15 products of the cells [z0, z1) x [y0, y1) x [x0, x1) (padded indices) of the masked vector xm, summed in chain order."""
    acc = None
    for dz, dy, dx, s in CHAIN:
        t = c[s] * xm[z0 + dz:z1 + dz, y0 + dy:y1 + dy, x0 + dx:x1 + dx]
        acc = t if acc is None else acc + t
    return acc


def global_results(c, free, p, r, alpha, beta, py=16):
    """(r - alpha A p, r' + beta p, A p') on the whole grid, padded like everything else."""
    shape = p.shape
    nz, ny, nx = shape
    fm = padded(free, shape, py, False)
    L = PAD_LO
    box = (L, L + nz, L, L + ny, L, L + nx)

    def apply(v):
        vp = padded(v, shape, py)
        q = chain(np.where(fm, vp, 0.0), c, *box)
        return np.where(free, q, v)
    q = apply(p)
    rn = r - alpha * q
    pn = rn + beta * p
    return rn, pn, apply(pn)


def tiles(shape, L, py=16):
    """(x0, y0, za, zb) of every workgroup: 64 x py patches, marches of L planes."""
    nz, ny, nx = shape
    L = max(3, L)
    return [(x0, y0, za, min(nz, za + L)) for za in range(0, nz, L) for y0 in range(0, ny, py) for x0 in range(0, nx, 64)]


def tile_results(c, free, p, r, alpha, beta, tile, py=16):
    """What one workgroup forms: (r', p', A p') on its patch rows inside the grid, as (slices into the grid, three arrays)."""
    shape = p.shape
    nz, ny, nx = shape
    x0, y0, za, zb = tile
    P = PAD_LO
    fm = padded(free, shape, py, False)
    ing = padded(np.ones(shape, bool), shape, py, False)

    def poisoned(v, zlo, zhi, halo):
        """v padded, NaN outside the planes [zlo, zhi) x the patch with `halo` cells around it; planes outside the grid stay zeros."""
        vp = padded(v, shape, py)
        out = np.full_like(vp, np.nan)
        zs = slice(max(zlo, -P) + P, min(zhi, nz + P) + P)
        ys, xs = slice(y0 - halo + P, y0 + py + halo + P), slice(x0 - halo + P, x0 + 64 + halo + P)
        out[zs, ys, xs] = vp[zs, ys, xs]
        return out
    pw = poisoned(p, za - 2, zb + 2, 2)                     # p: halo of two, planes za - 2 .. zb + 1
    rw = poisoned(r, za - 1, zb + 1, 1)                     # r: patch + ring, planes za - 1 .. zb
    # A(z): patch + ring on the planes za - 1 .. zb
    rz = (za - 1 + P, zb + 1 + P, y0 - 1 + P, y0 + py + 1 + P, x0 - 1 + P, x0 + 64 + 1 + P)
    reg = (slice(rz[0], rz[1]), slice(rz[2], rz[3]), slice(rz[4], rz[5]))
    pmask = np.where(np.isnan(pw), np.nan, np.where(fm, pw, 0.0))      # staged: eliminated nodes read as 0, the poison stays
    q = np.where(fm[reg], chain(pmask, c, *rz), pw[reg])
    rn = rw[reg] - alpha * q
    pn = rn + beta * pw[reg]
    # p' staged: masked like any staged plane; everything beyond patch + ring is unknown to this workgroup
    pm = np.full_like(pw, np.nan)
    pm[reg] = np.where(fm[reg], pn, 0.0)
    # B(z): the patch on the planes za .. zb - 1
    bz = (za + P, zb + P, y0 + P, y0 + py + P, x0 + P, x0 + 64 + P)
    breg = (slice(bz[0], bz[1]), slice(bz[2], bz[3]), slice(bz[4], bz[5]))
    inner = (slice(1, -1), slice(1, -1), slice(1, -1))      # the patch within patch + ring
    apn = np.where(fm[breg], chain(pm, c, *bz), pn[inner])
    # the rows of the patch that lie inside the grid
    y1, x1 = min(ny, y0 + py), min(nx, x0 + 64)
    own = (slice(za, zb), slice(y0, y1), slice(x0, x1))
    cut = (slice(None), slice(0, y1 - y0), slice(0, x1 - x0))
    assert ing[breg][cut].all()
    return own, rn[inner][cut], pn[inner][cut], apn[cut]
