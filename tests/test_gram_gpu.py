"""pgd_vec_gram on the MI355X, through the C-ABI: the f64-MFMA kernel and the plain fma kernel against the restatement of
tests/gram_reference.py - exact on integer data (fragment map, tile order, padded rows and vectors, ragged blocks, segments),
inside the derived rounding bound on floating-point data, bit-identical across grid sizes, bit-symmetric in the symmetric
case - the blocked binding above 128 vectors, the ranged copy, and every refusal."""
import ctypes as C

import numpy as np
import pytest

from pgdrome_amd import _lib
from tests.gram_reference import bound, gram_exact, scale

pytestmark = pytest.mark.gpu

VARIANTS = {"mfma": 1, "plain": 0}
POISON = -12345.678


class Knobs:
    def __init__(self, ctx, variant=1, grid_max=0):
        self.ctx, self.values = ctx, (variant, grid_max)

    def __enter__(self):
        self.ctx.tune(_lib.TUNE_GRAM_VARIANT, self.values[0])
        self.ctx.tune(_lib.TUNE_GRAM_GRID_MAX, self.values[1])

    def __exit__(self, *exc):
        self.ctx.tune(_lib.TUNE_GRAM_VARIANT, 1)
        self.ctx.tune(_lib.TUNE_GRAM_GRID_MAX, 0)


def upload(ctx, F):
    return [ctx.vec_from(np.ascontiguousarray(F[:, k], dtype=np.float64)) for k in range(F.shape[1])]


def free_all(ctx, vs):
    for v in vs:
        ctx.vec_free(v)


def raw_gram(ctx, xs, ys, lo, hi, kx=None, ky=None, out=None):
    """One call of the C entry point into a poisoned buffer: (return code, array)."""
    kx = len(xs) if kx is None else kx
    ky = (kx if ys is None else len(ys)) if ky is None else ky
    buf = np.full((max(kx, 1), max(ky, 1)), POISON) if out is None else out
    xa = (_lib.H * max(len(xs), 1))(*[int(v) for v in xs]) if xs is not None else None
    ya = (_lib.H * max(len(ys), 1))(*[int(v) for v in ys]) if ys is not None else None
    rc = ctx.lib.pgd_vec_gram(ctx.h, xa, kx, ya, ky, int(lo), int(hi), buf.ctypes.data_as(C.POINTER(C.c_double)))
    return rc, buf


# (n, kx, ky (None: symmetric), lo, hi, grid_max): every n of {1, 3, 4, 5, 15, 16, 17, 293, 1541, 70001} (the last: 274 segments
# of 8 row blocks and a ragged last block), every k of {1, 3, 16, 17, 48, 49, 128} on either side, sub-ranges whose lo is no
# multiple of 4, both cases
SHAPES = [
    (1, 1, None, 0, -1, 0), (3, 3, None, 0, -1, 0), (4, 16, None, 0, -1, 0), (5, 17, None, 1, 5, 0), (15, 48, None, 0, -1, 0),
    (16, 49, None, 3, 16, 0), (17, 128, None, 0, -1, 0), (293, 48, None, 5, 290, 2), (1541, 17, None, 0, -1, 3),
    (70001, 3, None, 7, 69999, 0), (70001, 16, None, 0, -1, 0), (1541, 128, None, 33, 1500, 0),
    (1, 1, 1, 0, -1, 0), (3, 3, 17, 1, 3, 0), (4, 1, 128, 0, -1, 0), (5, 16, 3, 0, -1, 0), (15, 17, 49, 2, 15, 0),
    (16, 128, 1, 0, -1, 0), (17, 49, 48, 0, -1, 0), (293, 48, 16, 0, -1, 1), (1541, 3, 48, 9, 1540, 0),
    (293, 128, 128, 6, 293, 0), (70001, 17, 3, 0, -1, 5), (1541, 49, 17, 0, -1, 0),
]
IDS = ["n%d-kx%d-ky%s-lo%d-hi%d-g%d" % s for s in SHAPES]


@pytest.mark.parametrize("sign", ["mixed", "positive"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_exact_layout_on_integer_data(ctx, shape, sign):
    """Integers in [-7, 7]: every product and sum is an exact integer far below 2^53, so both variants must EQUAL the int64
    result whatever the order.  All-positive data turns a padded row or vector that entered, or a row counted twice, into
    a wrong number; the poisoned output shows an entry that was never written."""
    n, kx, ky, lo, hi, grid_max = shape
    rng = np.random.default_rng(100000 * kx + 1000 * (ky or 0) + n)
    lim = (-7, 8) if sign == "mixed" else (1, 8)
    X = rng.integers(*lim, size=(n, kx))
    Y = None if ky is None else rng.integers(*lim, size=(n, ky))
    h = n if hi < 0 else hi
    ref = gram_exact(X[lo:h], None if Y is None else Y[lo:h]).astype(np.float64)
    xs = upload(ctx, X)
    ys = None if Y is None else upload(ctx, Y)
    try:
        for name, variant in VARIANTS.items():
            with Knobs(ctx, variant=variant, grid_max=grid_max):
                rc, out = raw_gram(ctx, xs, ys, lo, hi)
            assert rc == 0, (name, ctx.last_error() if hasattr(ctx, "last_error") else rc)
            assert np.array_equal(out, ref), name
    finally:
        free_all(ctx, xs + (ys or []))


@pytest.fixture(scope="module", params=[(70001, 17, 3), (1541, 48, 49)], ids=["n70001-17x3", "n1541-48x49"])
def float_case(request):
    """Seeded normal data with its exact references, computed once: many segments with few vectors, many tiles with few rows."""
    n, kx, ky = request.param
    rng = np.random.default_rng(20250611 + n)
    X, Y = rng.standard_normal((n, kx)), rng.standard_normal((n, ky))
    lo, hi = 3, n - 2
    return {"n": n, "X": X, "Y": Y, "lo": lo, "hi": hi,
            "sym": gram_exact(X[lo:hi]), "cross": gram_exact(X[lo:hi], Y[lo:hi]),
            "Bsym": scale(X[lo:hi]), "Bcross": scale(X[lo:hi], Y[lo:hi])}


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_floating_point_inside_the_bound_and_grid_invariant(ctx, float_case, variant):
    """Against the exact sums: (m + 2) 2^-53 sum |x||y| holds for any order of the m products and additions.  The grid changes
    which workgroup takes a segment, never the segments or the order of their partials: not a bit moves.  The symmetric block
    is symmetric bit for bit."""
    c = float_case
    m = c["hi"] - c["lo"]
    xs, ys = upload(ctx, c["X"]), upload(ctx, c["Y"])
    try:
        base = None
        for grid_max in (0, 1, 3):
            with Knobs(ctx, variant=VARIANTS[variant], grid_max=grid_max):
                rs, sym = raw_gram(ctx, xs, None, c["lo"], c["hi"])
                rc, cross = raw_gram(ctx, xs, ys, c["lo"], c["hi"])
            assert rs == 0 and rc == 0
            if base is None:
                base = (sym, cross)
                err_s, err_c = np.abs(sym - c["sym"]), np.abs(cross - c["cross"])
                print("max error / bound: symmetric %.3g, cross %.3g" % ((err_s / bound(m, c["Bsym"])).max(),
                                                                         (err_c / bound(m, c["Bcross"])).max()))
                assert np.all(err_s <= bound(m, c["Bsym"])) and np.all(err_c <= bound(m, c["Bcross"]))
                assert np.array_equal(sym, sym.T)
            else:
                assert np.array_equal(sym, base[0]) and np.array_equal(cross, base[1]), grid_max
    finally:
        free_all(ctx, xs + ys)


@pytest.mark.parametrize("K", [129, 256])
def test_blocked_binding_above_128_vectors(ctx, K):
    n = 293
    rng = np.random.default_rng(K)
    X, Y = rng.integers(-7, 8, size=(n, K)), rng.integers(-7, 8, size=(n, 130))
    xs, ys = upload(ctx, X), upload(ctx, Y)
    try:
        G = ctx.vec_gram(xs)
        assert G.shape == (K, K) and np.array_equal(G, gram_exact(X).astype(np.float64)) and np.array_equal(G, G.T)
        assert np.array_equal(ctx.vec_gram(xs, ys, 5, 290), gram_exact(X[5:290], Y[5:290]).astype(np.float64))
    finally:
        free_all(ctx, xs + ys)


def test_refusals_and_the_empty_range(ctx):
    """Everything the header names is PGD_ERR_INVALID before a launch (the output keeps its poison), an empty range is zeros."""
    n = 40
    xs = upload(ctx, np.ones((n, 3)))
    other = ctx.vec_from(np.ones(n + 1))
    try:
        bad = [
            raw_gram(ctx, xs, None, 0, -1, kx=3, ky=2),                 # symmetric case with ky != kx
            raw_gram(ctx, xs, None, 0, -1, kx=0, ky=0),                 # k out of range
            raw_gram(ctx, xs * 43, None, 0, -1),                        # 129 vectors
            raw_gram(ctx, xs, xs * 43, 0, -1),
            raw_gram(ctx, None, None, 0, -1, kx=3, ky=3),               # null handles
            raw_gram(ctx, [xs[0], 999999, xs[1]], None, 0, -1),         # an invalid handle
            raw_gram(ctx, xs, [xs[0], 0], 0, -1),
            raw_gram(ctx, xs, [other], 0, -1),                          # vectors of different lengths
            raw_gram(ctx, [xs[0], other], None, 0, -1),
            raw_gram(ctx, xs, None, 5, n + 1),                          # a range outside the vectors
            raw_gram(ctx, xs, None, -1, 4),
            raw_gram(ctx, xs, None, 9, 8),
        ]
        for i, (rc, out) in enumerate(bad):
            assert rc == -1 and np.all(out == POISON), i
        xa = (_lib.H * 3)(*xs)
        assert ctx.lib.pgd_vec_gram(ctx.h, xa, 3, None, 3, 0, -1, None) == -1            # no output
        rc, out = raw_gram(ctx, xs, None, 7, 7)
        assert rc == 0 and np.array_equal(out, np.zeros((3, 3)))
        rc, out = raw_gram(ctx, xs, xs[:2], 0, 0)
        assert rc == 0 and np.array_equal(out, np.zeros((3, 2)))
        with pytest.raises(RuntimeError):
            ctx.vec_gram(xs, [other])
    finally:
        free_all(ctx, xs + [other])


def test_ranged_copy(ctx):
    src = ctx.vec_from(np.arange(1000.0))
    dst = ctx.vec_from(np.full(300, POISON))
    try:
        ctx.vec_copy_range(dst, 7, src, 501, 290)
        want = np.full(300, POISON)
        want[7:297] = np.arange(501.0, 791.0)
        assert np.array_equal(ctx.vec_download(dst), want)
        ctx.vec_copy_range(dst, 0, src, 0, 0)
        ctx.vec_copy_range(src, 0, src, 500, 500)                        # disjoint ranges of one vector
        assert np.array_equal(ctx.vec_download(src)[:500], np.arange(500.0, 1000.0))
        for args in ((dst, 11, src, 0, 290), (dst, 0, src, 711, 290), (dst, -1, src, 0, 5), (dst, 0, src, 0, -1), (src, 0, src, 1, 10),
                     (dst, 0, 999999, 0, 1)):
            assert ctx.lib.pgd_vec_copy_range(ctx.h, *args) == -1
        assert np.array_equal(ctx.vec_download(dst), want)
    finally:
        free_all(ctx, [src, dst])
