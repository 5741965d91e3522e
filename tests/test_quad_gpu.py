"""pgd_quad_forms and pgd_vec_ratio on the MI355X, through the C-ABI: the f64-MFMA kernel and the plain fma kernel against the
restatement of tests/uq_reference.py - exact on integer data (fragment maps of both operands, the multiplier of every
accumulator entry, padded rows and modes, ragged tiles, several tiles per wave), inside the derived rounding bound on
floating-point data, bit-identical across grid sizes and whether a form is computed alone or among others, the extrema equal
to those of the stored fields - the clamp, forms without a field, the blocked binding above 64 forms, and every refusal."""
import ctypes as C

import numpy as np
import pytest

from pgdrome_amd import _lib
from tests.uq_reference import bound, quad_exact, scale

pytestmark = pytest.mark.gpu

VARIANTS = {"mfma": 1, "plain": 0}
POISON = -12345.678
PD = C.POINTER(C.c_double)


class Knobs:
    def __init__(self, ctx, variant=1, grid_max=0):
        self.ctx, self.values = ctx, (variant, grid_max)

    def __enter__(self):
        self.ctx.tune(_lib.TUNE_QUAD_VARIANT, self.values[0])
        self.ctx.tune(_lib.TUNE_QUAD_GRID_MAX, self.values[1])

    def __exit__(self, *exc):
        self.ctx.tune(_lib.TUNE_QUAD_VARIANT, 1)
        self.ctx.tune(_lib.TUNE_QUAD_GRID_MAX, 0)


def upload(ctx, F):
    return [ctx.vec_from(np.ascontiguousarray(F[:, k], dtype=np.float64)) for k in range(F.shape[1])]


def poisoned(ctx, n, count):
    return [ctx.vec_from(np.full(n, POISON)) for _ in range(count)]


def free_all(ctx, vs):
    for v in vs:
        ctx.vec_free(v)


def raw_quad(ctx, modes, Q, outs, flags=0, k=None, nq=None, extrema=True):
    """One call of the C entry point with a poisoned extrema buffer: (return code, extrema as (nq, 2))."""
    k = len(modes) if k is None else k
    nq = len(Q) if nq is None else nq
    ma = (_lib.H * max(len(modes), 1))(*[int(v) for v in modes]) if modes is not None else None
    oa = (_lib.H * max(len(outs), 1))(*[int(v) for v in outs]) if outs is not None else None
    qa = np.ascontiguousarray(Q, dtype=np.float64) if Q is not None else None
    ext = np.full((max(nq, 1), 2), POISON)
    rc = ctx.lib.pgd_quad_forms(ctx.h, ma, k, qa.ctypes.data_as(PD) if qa is not None else None, nq, flags, oa,
                                ext.ctypes.data_as(PD) if extrema else None)
    return rc, ext


# (n, k, nq, grid_max): every n of {1, 15, 16, 17, 63, 64, 65, 293, 70001}, every k of {1, 3, 4, 5, 16, 17, 48, 49, 128, 129, 256}
# (all six instances of the matrix-unit kernel, both sides of each of their limits), every nq of {1, 2, 5, 64}, every grid cap
SHAPES = [
    (1, 1, 1, 0), (15, 3, 2, 0), (16, 4, 1, 0), (17, 5, 5, 0), (63, 16, 2, 1), (64, 17, 1, 0), (65, 48, 5, 3), (293, 49, 2, 0),
    (70001, 3, 2, 0), (70001, 17, 5, 0), (293, 128, 2, 1), (65, 129, 1, 0), (64, 256, 2, 0), (17, 256, 64, 0), (1, 256, 1, 3),
    (15, 128, 5, 0), (16, 129, 2, 1), (293, 16, 64, 3), (63, 49, 1, 0), (70001, 48, 1, 3), (1, 17, 64, 0), (65, 1, 5, 1),
    (293, 4, 1, 0), (64, 5, 2, 3), (15, 49, 5, 1),
]
IDS = ["n%d-k%d-nq%d-g%d" % s for s in SHAPES]


@pytest.mark.parametrize("sign", ["mixed", "positive"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_exact_layout_on_integer_data(ctx, shape, sign):
    """Integers in [-3, 3]: every product and sum is an exact integer below 256^2 * 27 < 2^53, so both variants must EQUAL the
    int64 result whatever the order.  Q is not symmetric: a transposed fragment shows.  All-positive data turns a padded row or
    mode that entered an extremum into a wrong minimum; the poisoned outputs show a value that was never written.  With more
    than one form, form 1 has no field: its extrema come all the same."""
    n, k, nq, grid_max = shape
    rng = np.random.default_rng(100000 * k + 1000 * nq + n)
    lim = (-3, 4) if sign == "mixed" else (1, 4)
    F, Q = rng.integers(*lim, size=(n, k)), rng.integers(*lim, size=(nq, k, k))
    ref = quad_exact(F, Q).astype(np.float64)
    modes = upload(ctx, F)
    try:
        for name, variant in VARIANTS.items():
            outs = poisoned(ctx, n, nq)
            try:
                handles = [0 if (nq > 1 and f == 1) else outs[f] for f in range(nq)]
                with Knobs(ctx, variant=variant, grid_max=grid_max):
                    rc, ext = raw_quad(ctx, modes, Q, handles)
                assert rc == 0, (name, ctx.last_error() if hasattr(ctx, "last_error") else rc)
                for f in range(nq):
                    got = ctx.vec_download(outs[f])
                    if handles[f] == 0:
                        assert np.all(got == POISON), (name, f)
                    else:
                        assert np.array_equal(got, ref[f]), (name, f)
                assert np.array_equal(ext[:, 0], ref.min(axis=1)) and np.array_equal(ext[:, 1], ref.max(axis=1)), name
            finally:
                free_all(ctx, outs)
    finally:
        free_all(ctx, modes)


@pytest.fixture(scope="module", params=[(70001, 17, 3), (1541, 48, 5)], ids=["n70001-k17-nq3", "n1541-k48-nq5"])
def float_case(request):
    """Seeded normal data (Q indefinite and not symmetric: negative values for the clamp) with its references, computed once."""
    n, k, nq = request.param
    rng = np.random.default_rng(20250611 + n)
    F, Q = rng.standard_normal((n, k)), rng.standard_normal((nq, k, k))
    return {"n": n, "k": k, "nq": nq, "F": F, "Q": Q, "exact": quad_exact(F, Q), "B": scale(F, Q)}


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_floating_point_inside_the_bound_and_invariant(ctx, float_case, variant):
    """Against the longdouble values: the derived bound.  The grid changes which wave takes a tile, never a value's chain: not
    a bit moves.  A form computed alone has the bits it has among the others.  The extrema are those of the stored fields."""
    c = float_case
    n, nq = c["n"], c["nq"]
    modes = upload(ctx, c["F"])
    outs = poisoned(ctx, n, nq)
    try:
        base = None
        for grid_max in (0, 1, 3):
            with Knobs(ctx, variant=VARIANTS[variant], grid_max=grid_max):
                rc, ext = raw_quad(ctx, modes, c["Q"], outs)
            assert rc == 0
            got = np.stack([ctx.vec_download(o) for o in outs])
            if base is None:
                base = (got, ext)
                ratio = np.abs(got - c["exact"]) / bound(c["k"], c["B"])
                print("max error / bound: %.3g" % float(ratio.max()))
                assert ratio.max() <= 1.0
                assert np.array_equal(ext[:, 0], got.min(axis=1)) and np.array_equal(ext[:, 1], got.max(axis=1))
                assert got.min() < 0.0
            else:
                assert np.array_equal(got, base[0]) and np.array_equal(ext, base[1]), grid_max
        with Knobs(ctx, variant=VARIANTS[variant]):
            # alone
            for f in (0, nq - 1):
                rc, ext = raw_quad(ctx, modes, c["Q"][f:f + 1], [outs[0]])
                assert rc == 0 and np.array_equal(ctx.vec_download(outs[0]), base[0][f]) and np.array_equal(ext[0], base[1][f])
            # clamped: the same values, those below 0 stored and reduced as 0
            rc, ext = raw_quad(ctx, modes, c["Q"], outs, flags=_lib.QUAD_CLAMP)
            assert rc == 0
            got = np.stack([ctx.vec_download(o) for o in outs])
            want = np.where(base[0] < 0.0, 0.0, base[0])
            assert np.array_equal(got, want) and np.all(ext[:, 0] == 0.0) and np.array_equal(ext[:, 1], want.max(axis=1))
            # extrema only: no field is touched (with a null list and with a list of zeros)
            for o in outs:
                ctx.vec_fill(o, POISON)
            before = np.stack([ctx.vec_download(o) for o in outs])
            for handles in (None, [0] * nq):
                rc, ext = raw_quad(ctx, modes, c["Q"], handles)
                assert rc == 0 and np.array_equal(ext, base[1])
            assert np.array_equal(np.stack([ctx.vec_download(o) for o in outs]), before)
            # fields only
            rc, ext = raw_quad(ctx, modes, c["Q"], outs, extrema=False)
            assert rc == 0 and np.array_equal(np.stack([ctx.vec_download(o) for o in outs]), base[0])
    finally:
        free_all(ctx, modes + outs)


def test_binding_blocks_more_than_64_forms(ctx):
    n, k, nq = 293, 5, 70
    rng = np.random.default_rng(70)
    F, Q = rng.integers(-3, 4, size=(n, k)), rng.integers(-3, 4, size=(nq, k, k))
    ref = quad_exact(F, Q).astype(np.float64)
    modes, outs = upload(ctx, F), poisoned(ctx, n, nq)
    try:
        mn, mx = ctx.quad_forms(modes, Q, [None if f == 66 else outs[f] for f in range(nq)])
        assert np.array_equal(mn, ref.min(axis=1)) and np.array_equal(mx, ref.max(axis=1))
        for f in range(nq):
            assert np.array_equal(ctx.vec_download(outs[f]), np.full(n, POISON) if f == 66 else ref[f])
        mn, mx = ctx.quad_forms(modes, Q[2], clamp=True)
        assert mn.shape == (1,) and mn[0] == max(ref[2].min(), 0.0) and mx[0] == max(ref[2].max(), 0.0)
        with pytest.raises(ValueError):
            ctx.quad_forms(modes, Q[:, :4, :4])
        with pytest.raises(ValueError):
            ctx.quad_forms(modes, Q, outs[:3])
    finally:
        free_all(ctx, modes + outs)


def test_vec_ratio(ctx):
    n = 70001
    rng = np.random.default_rng(4)
    num, den = rng.standard_normal(n), rng.uniform(0.0, 1.0, n)
    den[::7] = 0.0
    den[3] = 0.25                                                  # exactly the floor: not above it
    hn, hd, ho = ctx.vec_from(num), ctx.vec_from(den), ctx.vec_from(np.full(n, POISON))
    short = ctx.vec_from(np.ones(n - 1))
    try:
        want = np.where(den > 0.25, num / np.where(den > 0.25, den, 1.0), 0.0)
        ctx.vec_ratio(ho, hn, hd, 0.25)
        assert np.array_equal(ctx.vec_download(ho), want) and want[3] == 0.0
        ctx.vec_ratio(ho, hn, hd)                                  # floor 0: the zeros of den give 0, no inf
        assert np.array_equal(ctx.vec_download(ho), np.where(den > 0.0, num / np.where(den > 0.0, den, 1.0), 0.0))
        for args in ((ho, hn, short, 0.0), (short, hn, hd, 0.0), (ho, short, hd, 0.0), (ho, 999999, hd, 0.0), (0, hn, hd, 0.0),
                     (ho, hn, hd, float("nan"))):
            assert ctx.lib.pgd_vec_ratio(ctx.h, *args[:3], C.c_double(args[3])) == -1
        assert np.array_equal(ctx.vec_download(hn), num) and np.array_equal(ctx.vec_download(hd), den)
        ctx.vec_ratio(hn, hn, hd, 0.25)                            # in place
        assert np.array_equal(ctx.vec_download(hn), want)
    finally:
        free_all(ctx, [hn, hd, ho, short])


def test_refusals_leave_the_outputs_untouched(ctx):
    """Everything the header names is PGD_ERR_INVALID before a launch: fields and extrema keep their poison."""
    n, k, nq = 40, 3, 2
    modes = upload(ctx, np.ones((n, k)))
    outs = poisoned(ctx, n, nq)
    other = ctx.vec_from(np.full(n + 1, POISON))
    Q = np.ones((nq, k, k))
    try:
        bad = [
            raw_quad(ctx, None, Q, outs, k=k),                               # null modes
            raw_quad(ctx, modes, None, outs, nq=nq),                         # null matrices
            raw_quad(ctx, modes, Q, outs, k=0),                              # k out of range
            raw_quad(ctx, modes * 86, np.ones((1, 258, 258)), outs[:1]),     # 258 modes
            raw_quad(ctx, modes, Q, outs, nq=0),                             # nq out of range
            raw_quad(ctx, modes, np.ones((65, k, k)), outs * 33, nq=65),
            raw_quad(ctx, [modes[0], 999999, modes[1]], Q, outs),            # invalid handles
            raw_quad(ctx, [modes[0], 0, modes[1]], Q, outs),
            raw_quad(ctx, modes, Q, [outs[0], 999999]),
            raw_quad(ctx, [modes[0], other, modes[1]], Q, outs),             # vectors of different lengths
            raw_quad(ctx, modes, Q, [outs[0], other]),
            raw_quad(ctx, modes, Q, [outs[0], modes[2]]),                    # an output that is a mode
            raw_quad(ctx, modes, Q, [outs[0], outs[0]]),                     # ... or another output
            raw_quad(ctx, modes, Q, None, extrema=False),                    # neither a field nor extrema
            raw_quad(ctx, modes, Q, [0, 0], extrema=False),
            raw_quad(ctx, modes, Q, outs, flags=2),                          # an unknown flag
        ]
        for i, (rc, ext) in enumerate(bad):
            assert rc == -1 and np.all(ext == POISON), i
        for o in outs + [other]:
            assert np.all(ctx.vec_download(o) == POISON)
        assert np.array_equal(ctx.vec_download(modes[2]), np.ones(n))
        with pytest.raises(RuntimeError):
            ctx.quad_forms(modes, Q, [outs[0], outs[0]])
        rc, ext = raw_quad(ctx, modes, Q, outs)                               # the context still works
        assert rc == 0 and np.array_equal(ext, np.full((nq, 2), 9.0)) and np.all(ctx.vec_download(outs[1]) == 9.0)
    finally:
        free_all(ctx, modes + outs + [other])
