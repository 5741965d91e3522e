"""Column blocks (pgd_block.hip): k columns in one allocation as fp32 or f64, all dots in one pass, the combination in one
pass; pgd_vec_lincomb in one launch; the spectral start of the spatial solves on a block.

Sizes: 1003 rows (one trip, ragged end) and 600 011 (> 2048 x 256: the tile loop of the dots kernel takes a second trip);
neither is a multiple of the 4 rows a lane takes at a time."""
import numpy as np
import pytest

from pgdrome_amd import _lib, fem

pytestmark = pytest.mark.gpu

SIZES = (1003, 600_011)
KMAX = 64
F32, F64 = _lib.BLOCK_F32, _lib.BLOCK_F64


@pytest.fixture(scope="module")
def data(ctx):
    """Per size: 64 random columns (host + device vectors) with exact zeros on some rows, r, a base vector.  Never modified."""
    out = {}
    rng = np.random.default_rng(54)
    for n in SIZES:
        Y = rng.standard_normal((KMAX, n)) * np.exp(rng.uniform(-3, 3, (KMAX, 1)))
        Y[:, :: 7] = 0.0                  # "Dirichlet rows"
        Y[:, -1] = 0.0
        r = rng.standard_normal(n)
        base = rng.standard_normal(n)
        out[n] = dict(Y=Y, Y32=Y.astype(np.float32).astype(np.float64), r=r, base=base,
                      vecs=[ctx.vec_from(Y[j]) for j in range(KMAX)], rv=ctx.vec_from(r), bv=ctx.vec_from(base))
    yield out
    for d in out.values():
        for v in d["vecs"] + [d["rv"], d["bv"]]:
            ctx.vec_free(v)


def _block(ctx, d, n, k, dtype, rounded=False):
    """A block of the first k columns; rounded: an f64 block that holds the fp32-rounded columns."""
    b = ctx.block_create(n, k, dtype)
    for j in range(k):
        if rounded:
            v = ctx.vec_from(d["Y32"][j])
            ctx.block_set_column(b, j, v)
            ctx.vec_free(v)
        else:
            ctx.block_set_column(b, j, d["vecs"][j])
    return b


@pytest.mark.parametrize("n", SIZES)
def test_column_round_trip(ctx, data, n):
    d = data[n]
    out = ctx.vec_alloc(n)
    for dtype, want in ((F64, d["Y"]), (F32, d["Y32"])):
        b = _block(ctx, d, n, 3, dtype)
        info = ctx.block_info(b)
        assert info["n"] == n and info["k"] == 3 and info["dtype"] == ("fp32", "f64")[dtype]
        assert info["bytes"] >= 3 * n * (4, 8)[dtype]
        for j in (0, 2):
            ctx.block_get_column(b, j, out)
            got = ctx.vec_download(out)
            assert np.array_equal(got, want[j])
            assert np.all(got[:: 7] == 0.0) and got[-1] == 0.0 and not np.any(np.signbit(got[:: 7]))
        with pytest.raises(_lib.PgdError):
            ctx.block_set_column(b, 3, d["vecs"][0])
        ctx.block_free(b)
    ctx.vec_free(out)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dtype", (F32, F64))
@pytest.mark.parametrize("k", (1, 17, 48, 64))
def test_dots(ctx, data, n, dtype, k):
    """Against numpy f64 on the columns as stored; |err_j| <= 1e-12 sum_i |Y_ij r_i| (a loose multiple of n eps); the same bits twice."""
    d = data[n]
    Y = (d["Y32"] if dtype == F32 else d["Y"])[:k]
    b = _block(ctx, d, n, k, dtype)
    for lo, hi in ((0, n), (5, n - 3)):
        got = ctx.block_dots(b, d["rv"], lo, hi)
        again = ctx.block_dots(b, d["rv"], lo, hi)
        prod = Y[:, lo:hi] * d["r"][lo:hi]
        ref, scale = prod.sum(axis=1), np.abs(prod).sum(axis=1)
        err = np.abs(got - ref) / scale
        print("dots n=%d k=%d %s [%d, %d): max |err| / sum |Y r| = %.2e" % (n, k, ("fp32", "f64")[dtype], lo, hi, err.max()))
        assert got.shape == (k,) and np.all(err <= 1e-12)
        assert np.array_equal(got, again)
    whole = ctx.block_dots(b, d["rv"])                 # hi = -1: all rows
    assert np.array_equal(whole, ctx.block_dots(b, d["rv"], 0, n))
    assert np.array_equal(ctx.block_dots(b, d["rv"], 9, 9), np.zeros(k))
    ctx.block_free(b)


def _lincomb_sequence(ctx, n, vecs, coefs, base):
    """Today's way: vec_zeros, one vec_lincomb over [base] + vecs, vec_copy into a fresh vector."""
    out, x = ctx.vec_alloc(n), ctx.vec_alloc(n)
    vs, cs = list(vecs), list(coefs)
    if base is not None:
        vs, cs = [base] + vs, [1.0] + cs
    ctx.vec_lincomb(out, vs, cs)
    ctx.vec_copy(x, out)
    got = ctx.vec_download(x)
    ctx.vec_free(out)
    ctx.vec_free(x)
    return got


def _against_numpy(got, Y, cs, base):
    """|got_i - (base_i + sum_j c_j Y_ij)| <= 2 (k + 2) eps (|base_i| + sum_j |c_j Y_ij|): a chain of k fmas and numpy's own sum of
    k + 1 rounded terms each stay within (k + 1) eps of the exact value relative to the sum of magnitudes."""
    c = np.asarray(cs)[:, None]
    ref = (c * Y).sum(axis=0) + (0.0 if base is None else base)
    mag = np.abs(c * Y).sum(axis=0) + (0.0 if base is None else np.abs(base))
    assert np.all(np.abs(got - ref) <= 2 * (len(cs) + 2) * np.finfo(float).eps * mag)


@pytest.mark.parametrize("dtype", (F32, F64))
def test_combine_second_trip(ctx, dtype):
    """2 100 003 rows: more than 2048 x 256 groups of 4 (fp32) or 2 (f64) rows, so the grid-stride loop of k_block_combine
    takes a second trip; two columns keep it quick.  Against numpy, and for f64 against the vec_lincomb sequence bit for bit."""
    n, k = 2_100_003, 2
    rng = np.random.default_rng(7)
    Y, base, cs = rng.standard_normal((k, n)), rng.standard_normal(n), [0.75, -1.5]
    vecs, bv, x = [ctx.vec_from(Y[j]) for j in range(k)], ctx.vec_from(base), ctx.vec_alloc(n)
    b = ctx.block_create(n, k, dtype)
    for j in range(k):
        ctx.block_set_column(b, j, vecs[j])
    ctx.block_combine(b, cs, bv, x)
    got = ctx.vec_download(x)
    _against_numpy(got, Y.astype(np.float32).astype(np.float64) if dtype == F32 else Y, cs, base)
    if dtype == F64:
        assert np.array_equal(got, _lincomb_sequence(ctx, n, vecs, cs, bv))
    ctx.block_free(b)
    for v in vecs + [bv, x]:
        ctx.vec_free(v)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("k", (1, 7, 8, 9, 48))
def test_combine(ctx, data, n, k):
    """f64 block: the bits of the vec_zeros / vec_lincomb / vec_copy sequence, without a base, with one, and in place;
    fp32 block: the bits of the f64 block that holds the rounded columns."""
    d = data[n]
    cs = list(np.random.default_rng(k).uniform(-2, 2, k))
    b64, b32, b64r = _block(ctx, d, n, k, F64), _block(ctx, d, n, k, F32), _block(ctx, d, n, k, F64, rounded=True)
    x = ctx.vec_alloc(n)
    for base in (None, d["bv"], "x"):
        want = _lincomb_sequence(ctx, n, d["vecs"][:k], cs, d["bv"] if base == "x" else base)
        res = {}
        for name, b in (("f64", b64), ("fp32", b32), ("f64 of rounded", b64r)):
            if base == "x":
                ctx.vec_copy(x, d["bv"])
                ctx.block_combine(b, cs, x, x)
            else:
                ctx.vec_fill(x, 123.0)
                ctx.block_combine(b, cs, base, x)
            res[name] = ctx.vec_download(x)
        assert np.array_equal(res["f64"], want), (k, base)
        assert np.array_equal(res["fp32"], res["f64 of rounded"]), (k, base)
        # ... and the values themselves, against numpy (both kernels above could share an error)
        _against_numpy(res["f64"], d["Y"][:k], cs, None if base is None else d["base"])
        _against_numpy(res["fp32"], d["Y32"][:k], cs, None if base is None else d["base"])
    assert np.array_equal(ctx.vec_download(d["bv"]), d["base"])          # a base that is not x is left alone
    with pytest.raises(ValueError):
        ctx.block_combine(b64, cs + [1.0], None, x)
    for h in (b64, b32, b64r):
        ctx.block_free(h)
    ctx.vec_free(x)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("k", (9, 16, 17, 64))
def test_lincomb_one_launch(ctx, data, n, k):
    """One launch for any k <= 64: the bits of 8-term combinations chained by hand, each accumulating onto the last through
    `base` (an f64 block of its eight columns)."""
    d = data[n]
    cs = list(np.random.default_rng(100 + k).uniform(-2, 2, k))
    y = ctx.vec_alloc(n)
    ctx.vec_fill(y, -7.0)
    ctx.vec_lincomb(y, d["vecs"][:k], cs)
    got = ctx.vec_download(y)
    acc = ctx.vec_alloc(n)
    for first in range(0, k, 8):
        m = min(8, k - first)
        b = ctx.block_create(n, m, F64)
        for j in range(m):
            ctx.block_set_column(b, j, d["vecs"][first + j])
        ctx.block_combine(b, cs[first:first + m], acc if first else None, acc)
        ctx.block_free(b)
    assert np.array_equal(got, ctx.vec_download(acc))
    _against_numpy(got, d["Y"][:k], cs, None)
    # ... and in place: the first term is y itself
    ctx.vec_copy(y, d["vecs"][0])
    ctx.vec_lincomb_inplace(y, [y] + d["vecs"][1:k], cs)
    assert np.array_equal(ctx.vec_download(y), got)
    with pytest.raises(_lib.PgdError):
        ctx.vec_lincomb_inplace(y, [d["vecs"][0], y], cs[:2])
    ctx.vec_free(y)
    ctx.vec_free(acc)


# ---- end to end: the 64^3 x 17 run of tests/test_spectral.py::test_spectral_start_on_gpu under the three storages

@pytest.fixture(scope="module")
def runs():
    from pgdrome_amd.hip_backend import HipBackend
    from tests.test_spectral import _run
    old = fem._backend
    be = fem.set_backend(HipBackend(0))
    out = {}
    try:
        for name, knob in (("vectors", 0), ("f64 block", 2), ("fp32 block", 1)):
            be.ctx.tune(_lib.TUNE_BLOCK_STORAGE, knob)
            p, modes, its, st, sp = _run((63, 63, 63), 12, nmax=5)
            assert st["harvests"] == 1 and len(sp) == 1
            out[name] = dict(p=p, modes=modes, its=its, info=dict(sp[0].info), k=sp[0].k, block=sp[0].block is not None)
            print("spectral start at 64^3, %s: %d Jacobi-PCG iterations, passes %s, %d vectors, %d bytes"
                  % (name, its, [int(v) for v in p.num_fp_it], sp[0].k, sp[0].info["bytes"]))
    finally:
        fem.set_backend(old)
        fem.clear_caches()
    return out


def test_storage_is_reported(runs):
    n, k = 64 ** 3, runs["vectors"]["k"]
    assert not runs["vectors"]["block"] and runs["vectors"]["info"]["storage"] == "f64 vectors" and runs["vectors"]["info"]["bytes"] == 8 * k * n
    assert runs["f64 block"]["block"] and runs["f64 block"]["info"]["storage"] == "f64 block"
    assert runs["fp32 block"]["block"] and runs["fp32 block"]["info"]["storage"] == "fp32 block"
    assert runs["f64 block"]["k"] == k and runs["fp32 block"]["k"] == k
    assert 4 * k * n <= runs["fp32 block"]["info"]["bytes"] < 1.01 * 4 * k * n
    assert 8 * k * n <= runs["f64 block"]["info"]["bytes"] < 1.01 * 8 * k * n


def test_f64_block_is_the_vector_path(runs):
    """Same stored numbers and the same combination bit for bit (test_combine), but the dots group their partial sums by
    256-row tiles of one wave where pgd_vec_multidot groups them by grid-stride threads, so Y'AY and Y'r differ in their last
    bits and with them the start vectors: the modes are NOT bit-identical.  Measured: iteration count (1211) and pass counts
    equal, worst relative difference of a mode 3.5e-10 (the solves stop at 1e-10).  Asserted: the counts equal (inside the +-2 foreseen for a count that moves)
    and the modes to 1e-9."""
    a, b = runs["f64 block"], runs["vectors"]
    worst = max(np.linalg.norm(a["modes"][d][m] - b["modes"][d][m]) / np.linalg.norm(b["modes"][d][m])
                for d in range(2) for m in range(b["p"].PGD_modes))
    print("f64 block against vectors: Jacobi-PCG iterations %d / %d, worst relative mode difference %.2e" % (a["its"], b["its"], worst))
    assert a["its"] == b["its"], (a["its"], b["its"])
    assert [int(v) for v in a["p"].num_fp_it] == [int(v) for v in b["p"].num_fp_it] and a["p"].PGD_modes == b["p"].PGD_modes
    assert worst <= 1e-9, worst


def test_fp32_block_is_the_same_run(runs):
    """Pass counts of the f64 block, modes within the bounds of tests/test_spectral.py, and at most 2 % more Jacobi-PCG
    iterations - the shift the project accepted for a regrouping of sums (301 -> 306 per pass at 256^3)."""
    from tests.test_spectral import _same_run
    a, b = runs["fp32 block"], runs["f64 block"]
    _same_run(a["p"], a["modes"], b["p"], b["modes"])
    print("Jacobi-PCG iterations: fp32 block %d, f64 block %d" % (a["its"], b["its"]))
    assert a["its"] <= 1.02 * b["its"], (a["its"], b["its"])
