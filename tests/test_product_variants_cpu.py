"""tests/product_variant_reference.py - the longdouble product from an operator's own CSR values and the two bars of
tests/test_product_variants_gpu.py - held to references that do not share its code, on the numpy oracle backend (no GPU):

* exact rational arithmetic (tests/exact_reference.py) on lattice_4x3x3: the helper's y_ref is within its own stated error of the exact
  product of the same double values, row by row, and its (|A||x|)_i is the exact one to a rounding per term;
* scipy's CSR product on 65 x 4 x 9, all five Dirichlet sets, which it must meet far inside the kernels' bar;
* the dot condition, with the oracle's product, on every shape, Dirichlet set, row range and weight vector the GPU module uses: the
  reference alone leaves at least 95 % of the rows of a range above the dot's bar, so a dot that drops or doubles a row cannot pass."""
import functools
import math
from fractions import Fraction

import numpy as np
import pytest
import scipy.sparse as sps

from oracle import fem_numpy as F
from oracle.backend_numpy import NumpyBackend
from tests import exact_reference as X
from tests import product_variant_reference as R


def oracle_operator(coords, cells, bc):
    """(rp, cols, vals, scipy matrix) of K + 0.37 M with the rows and columns of bc eliminated, through the oracle backend."""
    be = NumpyBackend()
    mh = be.mesh(coords, cells)
    ak, am = be.atom(mh, F.STIFF, 0, 0, 0), be.atom(mh, F.MASS, 0, 0, 0)
    op = be.combine(mh, [ak, am], list(R.COEFS), bc)
    rp, cols = be.mesh_pattern(mh)
    vals = be.atom_values(op, be.mesh_info(mh)["nnz"])
    A = sps.csr_matrix((vals, cols, rp), shape=(coords.shape[0],) * 2)
    return rp, cols, vals, A


@functools.lru_cache(maxsize=None)
def lattice(name):
    shape = R.SHAPES[name]
    coords, cells = F.box_mesh((0, 0, 0), R.BOX, shape[0] - 1, shape[1] - 1, shape[2] - 1)
    x, w = R.vectors(coords.shape[0])
    bcs = R.boundary_sets(coords, shape)
    ops = {name: oracle_operator(coords, cells, bcs[name]) for name in R.BOUNDARIES}
    return {"name": name, "shape": shape, "coords": coords, "x": x, "w": w, "bcs": bcs, "ops": ops}


@pytest.fixture(scope="module", params=sorted(R.SHAPES))
def oracle_lattice(request):
    return lattice(request.param)


def test_vectors_are_uniform_in_half_to_one_with_both_signs():
    x, w = R.vectors(4096)
    for v in (x, w):
        assert np.all((np.abs(v) >= 0.5) & (np.abs(v) <= 1.0))
        assert 0.4 < np.mean(v > 0) < 0.6
    assert not np.array_equal(x, w)


def test_reference_against_exact_rational_products():
    coords, cells = X.lattice_box(X.LATTICE_SHAPES["lattice_4x3x3"])
    lay = X.ExactLayout(coords, cells)
    shape = tuple(s + 1 for s in X.LATTICE_SHAPES["lattice_4x3x3"])
    assert coords.shape[0] == shape[0] * shape[1] * shape[2]
    lo = coords.min(axis=0)
    x, _ = R.vectors(lay.n, seed=3)
    for name, bc in (("natural", np.zeros(0, dtype=np.int32)), ("one face", np.where(coords[:, 2] <= lo[2])[0].astype(np.int32))):
        rp, cols, vals, _ = oracle_operator(coords, cells, bc)
        assert np.array_equal(rp, lay.rp) and np.array_equal(cols, lay.cols)
        y_ref, rowabs = R.csr_product(rp, cols, vals, x)
        fv = X.frac_vec(vals)
        exact = lay.matvec(fv, x)
        exact_abs = lay.matvec(np.array([abs(v) for v in fv], dtype=object), np.abs(x))
        bound = R.reference_error_bound(rp, rowabs)
        worst = 0.0
        for i in range(lay.n):
            err = abs(Fraction(*map(int, y_ref[i].as_integer_ratio())) - exact[i])
            assert err <= Fraction(float(bound[i])), (name, i, float(err), bound[i])
            assert abs(Fraction(float(rowabs[i])) - exact_abs[i]) <= 16 * 2.0 ** -53 * exact_abs[i], (name, i)
            worst = max(worst, float(err) / (R.ROW_TOL * rowabs[i]))
        print("lattice_4x3x3", name, "largest |y_ref - exact| / (4e-15 |A||x|) = %.3g" % worst)
        assert worst <= 1e-3                                              # the reference's error is nothing beside the kernels' bar
        assert R.row_excess(np.array([float(v) for v in exact]), y_ref, rowabs, 0, lay.n) <= 0.1     # the correctly rounded product passes
        # ... and what a kernel could get wrong does not: one coupling left out of one row, one row of the plane below
        k = int(np.argmax(np.abs(vals[rp[7]:rp[8]] * x[cols[rp[7]:rp[8]]]))) + int(rp[7])
        wrong = np.array([float(v) for v in exact])
        wrong[7] -= vals[k] * x[cols[k]]
        assert R.row_excess(wrong, y_ref, rowabs, 0, lay.n) > 1e10
        assert R.row_excess(wrong, y_ref, rowabs, 8, lay.n) <= 0.1


def test_reference_against_scipy():
    g = lattice("65x4x9")
    for name in R.BOUNDARIES:
        rp, cols, vals, A = g["ops"][name]
        y_ref, rowabs = R.csr_product(rp, cols, vals, g["x"])
        assert np.array_equal(rowabs > 0, np.ones(A.shape[0], dtype=bool))
        y = A @ g["x"]
        assert np.allclose(rowabs, abs(A) @ np.abs(g["x"]), rtol=1e-14, atol=0.0)
        worst = R.row_excess(y, y_ref, rowabs, 0, A.shape[0])
        print(g["name"], name, "scipy: largest error / bound = %.3g" % worst)
        assert worst <= 1.0
        bc = g["bcs"][name]
        assert np.array_equal(y_ref[bc].astype(np.float64), g["x"][bc])                 # identity rows


def test_dot_condition_holds_for_the_reference(oracle_lattice):
    g = oracle_lattice
    ranges = R.row_ranges(g["shape"])
    assert ranges["slab"][1] - ranges["slab"][0] == (g["shape"][2] - 2) * g["shape"][0] * g["shape"][1]
    for name in R.BOUNDARIES:
        rp, cols, vals, A = g["ops"][name]
        y = A @ g["x"]
        for rname in R.RANGES:
            r0, r1 = ranges[rname]
            for wname, w in (("w = x", g["x"]), ("third vector", g["w"])):
                share = R.dot_share(w, y, r0, r1)
                d, bar = R.dot_reference(w, y, r0, r1)
                print(g["name"], name, rname, wname, "share above the bar %.4f, dot %.6g, bar %.3g" % (share, d, bar))
                assert share >= R.DOT_SHARE, (g["name"], name, rname, wname, share)
                # a dropped and a doubled row are seen: both move the dot by more than the bar for at least that share of the rows
                t = np.abs(w[r0:r1] * y[r0:r1])
                assert np.count_nonzero(t > bar) >= R.DOT_SHARE * (r1 - r0)
                assert math.isclose(d, float(w[r0:r1] @ y[r0:r1]), rel_tol=0.0, abs_tol=bar)
