"""Reference and bounds for the products of an operator on a box lattice, whatever kernel instance computes them
(tests/test_product_variants_gpu.py; held to exact and scipy products in tests/test_product_variants_cpu.py).

The reference is formed from the operator's OWN CSR values - downloaded after pgd_op_combine, on the row pattern of the mesh - so it does not
depend on a second assembly: y_ref = A x in np.longdouble, one np.add.reduceat over the row segments.  A row has at most 15 entries; with
u = the unit roundoff of longdouble (2^-64 where it is the x87 format) every order of the sum leaves |y_ref,i - (A x)_i| <= 16 u (|A||x|)_i
= 8.7e-19 (|A||x|)_i, 4600 times below the bar the kernels are held to.

Bars:
* per row, the project's bound for a product (tests/test_kernels_gpu.py):  |y_i - y_ref,i| <= 4e-15 (|A||x|)_i;
* the fused dot over a row range [r0, r1), against math.fsum of w_i y_i over the kernel's OWN y (so the dot's summation is judged alone):
  1e-12 sum_range |w_i y_i| - the bar tests/test_product_plan_gpu.py derives for the partial sums of the marches, here taken over the rows of
  the range only, which is never more than that module's sum over all rows.

The dot condition keeps the second bar meaningful: at least 95 % of the rows of a tested range must carry |w_i y_i| above the bar itself, so
that a row left out of the dot, or added twice, moves the dot by more than the bar.  x and w are uniform in +-[0.5, 1] for that (no entry
near 0; identity rows give |w_i x_i| >= 1/4)."""
import math

import numpy as np

ROW_TOL = 4e-15
DOT_TOL = 1e-12
DOT_SHARE = 0.95

# nx x ny x nz, each the smallest case of a seam of the marches (64-column x tiles, 8- and 16-row y patches, groups of 3 and 6 planes)
SHAPES = {
    "65x4x9": (65, 4, 9),        # two x tiles, the second with one column; ny below every patch height; nz below 12
    "65x9x14": (65, 9, 14),      # one full 8-row patch plus one row; 12 planes + 2; the slab [1, 13) is exactly 12 planes
    "64x16x6": (64, 16, 6),      # exactly one 64 x 16 patch and exactly one group of six
    "66x17x20": (66, 17, 20),    # partial tiles on both axes; 18 planes + 2
}
BOX = (1.0, 0.7, 1.3)
COEFS = (1.0, 0.37)              # K + 0.37 M
BOUNDARIES = ("hull", "hull + column", "hull + one interior node", "natural", "one face")
ONE_STENCIL = ("hull", "hull + column")      # the sets whose operator is one stencil + eliminated nodes (test_stencil_form_is_lossless)
RANGES = ("whole", "slab", "one plane")


def boundary_sets(coords, shape):
    """The five Dirichlet sets of test_stencil_form_is_lossless (tests/test_kernels_gpu.py) on an nx x ny x nz lattice."""
    nx, ny, nz = shape
    plane = nx * ny
    lo, hi = coords.min(axis=0), coords.max(axis=0)
    hull = np.where(np.any((coords <= lo + 1e-12) | (coords >= hi - 1e-12), axis=1))[0].astype(np.int32)
    face = np.where(coords[:, 2] <= 1e-12)[0].astype(np.int32)
    ix, iy = min(5, nx - 2), min(2, ny - 2)
    column = (ix + nx * iy + plane * np.arange(nz)).astype(np.int32)
    single = np.array([ix + nx * iy + plane * (nz // 2)], dtype=np.int32)
    return dict(zip(BOUNDARIES, (hull, np.union1d(hull, column).astype(np.int32), np.union1d(hull, single).astype(np.int32),
                                 np.zeros(0, dtype=np.int32), face)))


def row_ranges(shape):
    """The whole grid, the plane-aligned slab [1, nz - 1) and the single plane nz // 2, as row ranges."""
    nx, ny, nz = shape
    plane = nx * ny
    return dict(zip(RANGES, ((0, plane * nz), (plane, (nz - 1) * plane), ((nz // 2) * plane, (nz // 2 + 1) * plane))))


def vectors(n, seed=7):
    """x and w, uniform in +-[0.5, 1]."""
    rng = np.random.default_rng(seed)
    return tuple(rng.uniform(0.5, 1.0, n) * rng.choice((-1.0, 1.0), n) for _ in range(2))


def csr_product(rp, cols, vals, x):
    """(y_ref, rowabs): A x in longdouble and (|A||x|)_i in double, per row of the CSR matrix (rp, cols, vals)."""
    rp, cols = np.asarray(rp, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    vals, x = np.asarray(vals, dtype=np.float64), np.asarray(x, dtype=np.float64)
    assert rp[0] == 0 and rp[-1] == cols.size == vals.size and np.all(np.diff(rp) > 0), "a CSR pattern without empty rows"
    prod = vals.astype(np.longdouble) * x[cols].astype(np.longdouble)
    y_ref = np.add.reduceat(prod, rp[:-1])
    assert y_ref.dtype == np.longdouble
    rowabs = np.add.reduceat(np.abs(vals) * np.abs(x[cols]), rp[:-1])
    return y_ref, rowabs


def reference_error_bound(rp, rowabs):
    """What csr_product itself may be off by, per row: (entries + 1) u (|A||x|)_i."""
    return (np.diff(np.asarray(rp, dtype=np.int64)) + 1) * float(np.finfo(np.longdouble).eps) * rowabs


def row_excess(y, y_ref, rowabs, r0, r1):
    """Largest |y_i - y_ref,i| / (4e-15 (|A||x|)_i) over the rows [r0, r1): <= 1 passes.  A row with (|A||x|)_i = 0 must be exact."""
    err = np.abs(np.asarray(y, dtype=np.float64)[r0:r1].astype(np.longdouble) - y_ref[r0:r1]).astype(np.float64)
    bound = ROW_TOL * rowabs[r0:r1]
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    return float(q.max()) if q.size else 0.0


def dot_reference(w, y, r0, r1):
    """(math.fsum of w_i y_i over [r0, r1), the bar 1e-12 sum |w_i y_i|)."""
    t = np.asarray(w, dtype=np.float64)[r0:r1] * np.asarray(y, dtype=np.float64)[r0:r1]       # (one rounding per term: 1.1e-16 of the bar's sum)
    return math.fsum(t), DOT_TOL * math.fsum(np.abs(t))


def dot_share(w, y, r0, r1):
    """Share of the rows of [r0, r1) whose |w_i y_i| is above the dot's bar."""
    t = np.abs(np.asarray(w, dtype=np.float64)[r0:r1] * np.asarray(y, dtype=np.float64)[r0:r1])
    return float(np.count_nonzero(t > DOT_TOL * math.fsum(t))) / max(t.size, 1)
