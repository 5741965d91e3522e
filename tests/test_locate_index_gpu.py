"""The bin index of pgd_points_locate on the MI355X, through the C-ABI: the indexed path gives the general kernel's cells and lam bit
for bit on every mesh, grid and class of points; the index itself equals the numpy restatement of
tests/locate_index_reference.py; when the path is taken, when the index is built, rebuilt and freed; and the ``index=`` argument of
the frontend on the hip backend.

The index is NOT refused on tiny meshes: one tetrahedron and one cube get their (one-bin or few-bin) grid like any other mesh, and
the tests below expect path 3 there too."""
import numpy as np
import pytest

from pgdrome_amd import _lib, fem
from tests import locate_index_reference as ixref
from tests import sensor_reference as ref

pytestmark = pytest.mark.gpu

NPTS = 700                   # three workgroups of 256 threads, the last one ragged
TARGETS = (0, 1, 10 ** 9)    # the rule; the finest grid (the cap coarsens it where needed); one bin per axis
TOL = 1e-10


def box(n, p1=(1.0, 1.0, 1.0)):
    m = fem.BoxMesh(fem.Point(0, 0, 0), fem.Point(*p1), *n)
    return m.coordinates(), m.cells()


def mesh_arrays(name):
    """(node coordinates, records, lattice path available): the meshes of tests/test_sensors_gpu.py, and a P2 layout in 2-D and 3-D."""
    if name == "triangles2":
        m = fem.RectangleMesh(fem.Point(0, 0), fem.Point(2, 1), 1, 1)
        return m.coordinates(), m.cells(), False
    if name in ("rectangle_jittered", "rectangle_jittered_p2"):
        m = fem.RectangleMesh(fem.Point(0, 0), fem.Point(1, 1), 5, 4)
        X, C = ref.jitter(m.coordinates(), 0.2, 3), m.cells()
        if name.endswith("_p2"):
            lay = fem.Mesh(X, C).layout(2)
            return np.asarray(lay.coords, dtype=np.float64).reshape(lay.n, -1), np.asarray(lay.cells), False
        return X, C, False
    if name == "tetrahedron1":
        return np.array([[0.0, 0, 0], [1.0, 0.1, 0], [0.2, 0.9, 0.1], [0.1, 0.2, 1.1]]), np.array([[0, 1, 2, 3]], dtype=np.int32), False
    if name == "cube1":
        return box((1, 1, 1)) + (False,)
    if name == "box345":
        return box((3, 4, 5)) + (True,)
    if name in ("box345_jittered", "box345_jittered_p2"):
        X, C = box((3, 4, 5))
        X = ref.jitter(X, 0.2, 4, amount=0.2)
        if name.endswith("_p2"):
            lay = fem.Mesh(X, C).layout(2)
            return np.asarray(lay.coords, dtype=np.float64).reshape(lay.n, -1), np.asarray(lay.cells), False
        return X, C, False
    if name == "box765":
        return box((7, 6, 5)) + (True,)
    raise KeyError(name)


MESHES = ["triangles2", "rectangle_jittered", "tetrahedron1", "cube1", "box345", "box345_jittered", "box765", "rectangle_jittered_p2",
          "box345_jittered_p2"]
LATTICES = ["box345", "box765"]


def strided(a, count):
    return a if len(a) <= count else a[np.linspace(0, len(a) - 1, count).astype(np.int64)]


def point_set(X, C, tol):
    """NPTS points: on the hull pushed outward along the barycentric direction of the facet's cell to minima of -tol / 2 (kept) and
    -2 tol (outside that cell), far outside the box, a NaN, +inf and -inf; vertices, edge midpoints and centroids (ties over many
    cells and across bin borders); interior points; the rest seeded in the box scaled by 1.3 about its centre."""
    D = X.shape[1]
    V = C[:, :D + 1]
    verts = X[np.unique(V)]
    lo, hi = verts.min(axis=0), verts.max(axis=0)
    mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    count = {}
    for e, rec in enumerate(V):
        for drop in range(D + 1):
            key = tuple(sorted(int(v) for j, v in enumerate(rec) if j != drop))
            count.setdefault(key, []).append(int(rec[drop]))
    hull = [(k, v[0]) for k, v in sorted(count.items()) if len(v) == 1]
    hull = [hull[i] for i in np.linspace(0, len(hull) - 1, min(len(hull), 40)).astype(np.int64)]
    pushed = []
    for facet, opposite in hull:
        centre = X[list(facet)].mean(axis=0)
        for s in (0.5 * tol, 2.0 * tol):
            pushed.append(centre + s * (centre - X[opposite]))
    nan, pinf, ninf = mid.copy(), mid.copy(), mid.copy()
    nan[0], pinf[-1], ninf[0] = np.nan, np.inf, -np.inf
    special = np.array(pushed + [mid + 1e6, mid - 1e6, lo - 3.0 * half, hi + 3.0 * half, nan, pinf, ninf])
    room = NPTS - len(special)
    ties = strided(ref.tie_points(X, V), room // 2)
    inner = strided(ref.interior_points(X, V, seed=5)[0], room // 3)
    rng = np.random.default_rng(17)
    wide = mid + 1.3 * half * rng.uniform(-1.0, 1.0, size=(NPTS - len(special) - len(ties) - len(inner), D))
    pts = np.concatenate([special, ties, inner, wide])
    assert pts.shape == (NPTS, D)
    return pts


def kept_on_the_hull(X, C, cells):
    """The points pushed out to a minimum of -tol / 2 come first in point_set, every other one: all of them must have a cell."""
    D = X.shape[1]
    facets = {}
    for rec in C[:, :D + 1]:
        for drop in range(D + 1):
            key = tuple(sorted(int(v) for j, v in enumerate(rec) if j != drop))
            facets[key] = facets.get(key, 0) + 1
    pushed = 2 * min(40, sum(1 for v in facets.values() if v == 1))
    return pushed >= 8 and bool(np.all(cells[0:pushed:2] >= 0))


class Knobs:
    def __init__(self, ctx, lattice=0, target=0):
        self.ctx, self.values = ctx, (lattice, target)

    def __enter__(self):
        self.ctx.tune(_lib.TUNE_LOCATE_LATTICE, self.values[0])
        self.ctx.tune(_lib.TUNE_LOCATE_INDEX_TARGET, self.values[1])

    def __exit__(self, *exc):
        self.ctx.tune(_lib.TUNE_LOCATE_LATTICE, 1)
        self.ctx.tune(_lib.TUNE_LOCATE_INDEX_TARGET, 0)


def locate(ctx, mh, pts, tol=TOL, index=False):
    """(cells, lam as int64 bit patterns, path) of one pgd_points_locate under knob 66 = index; the set is freed."""
    h = ctx.points_locate(mh, pts, tol, index=index)
    try:
        cells, lam = ctx.points_download(h)
        return cells, lam.view(np.int64), ctx.points_last_path()
    finally:
        ctx.points_free(h)


@pytest.fixture(scope="module")
def uploaded(ctx):
    """name -> (X, records, lattice, mesh handle, points, the general kernel's (cells, lam bits)): one reference per mesh for all tests."""
    out = {}
    for name in MESHES:
        X, C, lattice = mesh_arrays(name)
        mh = ctx.mesh_upload(X, C)
        pts = point_set(X, C, TOL)
        with Knobs(ctx, lattice=0):
            cells, lam, path = locate(ctx, mh, pts)
        assert path == _lib.LOCATE_PATH_GENERAL
        assert ctx.points_index_info(mh)["built"] == 0
        out[name] = (X, C, lattice, mh, pts, (cells, lam))
    yield out
    for v in out.values():
        ctx.mesh_free(v[3])      # (with an index alive)


def test_the_knob_is_off_by_default(ctx, uploaded):
    X, C, _, mh, pts, _ = uploaded["rectangle_jittered"]
    h = ctx.points_locate(mh, pts[:5], TOL, index=None)
    ctx.points_free(h)
    assert ctx.points_last_path() == _lib.LOCATE_PATH_GENERAL


def test_the_knob_itself_selects_the_index(ctx, uploaded):
    """PGD_TUNE_LOCATE_INDEX set through tune() - what a call with ``index=None`` runs under: 1 takes the bin index, with the cells and lam
    of the general kernel bit for bit, and 0 afterwards takes the general kernel again."""
    X, C, _, mh, pts, (cells0, lam0) = uploaded["rectangle_jittered"]
    try:
        with Knobs(ctx, lattice=0):
            ctx.tune(_lib.TUNE_LOCATE_INDEX, 1)
            cells, lam, path = locate(ctx, mh, pts, index=None)
            ctx.tune(_lib.TUNE_LOCATE_INDEX, 0)
            cells2, lam2, path2 = locate(ctx, mh, pts, index=None)
    finally:
        ctx.tune(_lib.TUNE_LOCATE_INDEX, 0)
    assert (path, path2) == (_lib.LOCATE_PATH_INDEX, _lib.LOCATE_PATH_GENERAL)
    for c, l in ((cells, lam), (cells2, lam2)):
        assert np.array_equal(c, cells0) and np.array_equal(l, lam0)


@pytest.mark.parametrize("target", TARGETS)
@pytest.mark.parametrize("name", MESHES)
def test_index_equals_the_general_kernel(ctx, uploaded, name, target):
    """Knob 66 = 0 and then 1: cells and lam are equal as bits, on every class of points (the reference has points inside and
    outside), for the grid of the rule, the finest grid and a single bin.  Path 3 on every mesh, the tiny ones included."""
    X, C, lattice, mh, pts, (cells0, lam0) = uploaded[name]
    nc = len(C)
    assert (cells0 >= 0).sum() >= min(nc, 10) and (cells0 < 0).sum() >= 7 and kept_on_the_hull(X, C, cells0)
    with Knobs(ctx, lattice=0, target=target):
        cells, lam, path = locate(ctx, mh, pts, index=True)
        info = ctx.points_index_info(mh)
    assert path == _lib.LOCATE_PATH_INDEX
    assert np.array_equal(cells, cells0) and np.array_equal(lam, lam0)
    assert info["built"] == 1 and nc <= info["entries"] <= ixref.CAP * nc
    if target == 10 ** 9:
        assert info["n"] == (1, 1, 1) and info["entries"] == nc == info["longest"]
    print("%s target %d: bins %s, %.2f entries per cell, longest list %d, %d bytes"
          % (name, target, info["n"], info["entries"] / nc, info["longest"], info["bytes"]))


@pytest.mark.parametrize("name", LATTICES)
def test_the_lattice_path_keeps_precedence(ctx, uploaded, name):
    X, C, _, mh, pts, (cells0, lam0) = uploaded[name]
    with Knobs(ctx, lattice=1):
        cells2, lam2, path2 = locate(ctx, mh, pts, index=True)
    with Knobs(ctx, lattice=0):
        cells3, lam3, path3 = locate(ctx, mh, pts, index=True)
    assert (path2, path3) == (_lib.LOCATE_PATH_LATTICE, _lib.LOCATE_PATH_INDEX)
    for cells, lam in ((cells2, lam2), (cells3, lam3)):
        assert np.array_equal(cells, cells0) and np.array_equal(lam, lam0)


@pytest.mark.parametrize("target", TARGETS)
@pytest.mark.parametrize("name", MESHES)
def test_downloaded_index_equals_the_restatement(ctx, uploaded, name, target):
    X, C, _, mh, pts, _ = uploaded[name]
    nc = len(C)
    want = ixref.build(X, C, target)
    with Knobs(ctx, lattice=0, target=target):
        locate(ctx, mh, pts[:3], index=True)
        info = ctx.points_index_info(mh)
        bin_ptr, bin_cells, o, inv, n = ctx.points_index_download(mh)
    assert np.array_equal(n, want["n"]) and np.array_equal(o, want["o"]) and np.array_equal(inv, want["inv"])
    assert np.array_equal(bin_ptr, want["bin_ptr"])
    for b, cells in enumerate(want["lists"]):
        assert np.array_equal(np.sort(bin_cells[bin_ptr[b]:bin_ptr[b + 1]]), cells), (name, target, b)
    assert info["entries"] == want["entries"] == len(bin_cells) and info["longest"] == want["longest"]
    assert info["n"] == tuple(int(k) for k in want["n"])
    assert info["bytes"] == 4 * (len(bin_ptr) + max(len(bin_cells), 1))
    assert np.array_equal(np.unique(bin_cells), np.arange(nc))      # every cell sits in >= 1 bin
    assert info["entries"] <= ixref.CAP * nc
    if target == 1 and nc > 16:
        fine, _ = ixref.grid(nc, want["o"][:X.shape[1]], X[np.unique(C[:, :X.shape[1] + 1])].max(axis=0), 1)
        print("%s: finest grid %s -> %s after the cap" % (name, [int(k) for k in fine], [int(k) for k in want["n"]]))


@pytest.mark.parametrize("name", ["rectangle_jittered", "box345_jittered", "box345_jittered_p2"])
def test_tolerances_the_index_serves(ctx, uploaded, name):
    """tol = 2^-10 takes the index and equals the general kernel - with the hull points pushed out by that tol; 2^-9 and 0.5 take the
    general kernel although the index was asked for."""
    X, C, _, mh, _, _ = uploaded[name]
    tol = 2.0 ** -10
    pts = point_set(X, C, tol)
    with Knobs(ctx, lattice=0):
        cells0, lam0, path0 = locate(ctx, mh, pts, tol=tol)
        cells1, lam1, path1 = locate(ctx, mh, pts, tol=tol, index=True)
        assert (path0, path1) == (_lib.LOCATE_PATH_GENERAL, _lib.LOCATE_PATH_INDEX)
        assert np.array_equal(cells0, cells1) and np.array_equal(lam0, lam1)
        assert kept_on_the_hull(X, C, cells0)      # (minima of -2^-11: inside the margin of the boxes, outside the cells)
        for wide in (2.0 ** -9, 0.5):
            assert locate(ctx, mh, pts[:40], tol=wide, index=True)[2] == _lib.LOCATE_PATH_GENERAL


def test_build_once_rebuild_on_a_new_target_drop_and_free(ctx):
    X, C, _ = mesh_arrays("box345_jittered")
    pts = point_set(X, C, TOL)[:64]
    zero = dict(built=0, builds=0, n=(0, 0, 0), entries=0, longest=0, bytes=0)
    mh = ctx.mesh_upload(X, C)
    blocked = ctx.mesh_blocked(mh, 3)
    try:
        assert ctx.points_index_info(mh) == zero
        ctx.points_index_drop(mh)                                     # nothing to drop: fine
        with pytest.raises(_lib.PgdError, match="no index"):
            ctx.points_index_download(mh)
        with Knobs(ctx, lattice=0):
            locate(ctx, mh, pts, index=False)
            assert ctx.points_index_info(mh) == zero                  # the general kernel builds nothing
            first = locate(ctx, mh, pts, index=True)
            one = ctx.points_index_info(mh)
            assert one["built"] == 1 and one["builds"] == 1 and one["bytes"] > 0
            assert locate(ctx, blocked, pts, index=True)[2] == _lib.LOCATE_PATH_INDEX      # the blocked layout uses its base's index
            locate(ctx, mh, pts[:7], index=True)
            assert ctx.points_index_info(mh) == one == ctx.points_index_info(blocked)
        with Knobs(ctx, lattice=0, target=5):
            second = locate(ctx, mh, pts, index=True)
            two = ctx.points_index_info(mh)
            assert two["builds"] == 2 and two["n"] != one["n"]
            locate(ctx, mh, pts, index=True)
            assert ctx.points_index_info(mh) == two
            ctx.points_index_drop(mh)
            assert ctx.points_index_info(mh) == zero
            third = locate(ctx, mh, pts, index=True)
            assert ctx.points_index_info(mh) == dict(two, builds=1)
        for got in (second, third):
            assert np.array_equal(got[0], first[0]) and np.array_equal(got[1], first[1]) and got[2] == _lib.LOCATE_PATH_INDEX
    finally:
        ctx.mesh_free(blocked)
        ctx.mesh_free(mh)                                             # with the index alive
    other = ctx.mesh_upload(X, C)                                     # the context goes on
    try:
        assert ctx.points_index_info(other) == zero
    finally:
        ctx.mesh_free(other)


def test_intervals_keep_the_general_kernel(ctx):
    m = fem.IntervalMesh(7, -1.0, 2.5)
    mh = ctx.mesh_upload(m.coordinates(), m.cells())
    try:
        assert locate(ctx, mh, np.linspace(-1.0, 2.5, 9).reshape(-1, 1), index=True)[2] == _lib.LOCATE_PATH_GENERAL
        assert ctx.points_index_info(mh)["built"] == 0
    finally:
        ctx.mesh_free(mh)


# ---- the frontend on the hip backend
@pytest.fixture(scope="module")
def hip_backend():
    from pgdrome_amd.hip_backend import HipBackend
    old = fem._backend
    be = HipBackend(0)
    fem.set_backend(be)
    fem.clear_caches()
    yield be
    fem.set_backend(old)
    fem.clear_caches()


def jittered_box():
    X, C = box((3, 4, 5))
    return fem.Mesh(ref.jitter(X, 0.2, 4, amount=0.2), C)


def test_frontend_locate_points(hip_backend):
    be = hip_backend
    mesh = jittered_box()
    pts = ref.interior_points(mesh.coordinates(), mesh.cells(), seed=21)[0]
    mh = mesh.layout(1).handle()
    a = fem.locate_points(mesh, pts, index=True)
    assert a.path == "index" and be.points_index_info(mh)["builds"] == 1
    assert fem.locate_points(mesh, pts, index=False) is a                 # one cache entry: the bits are the same
    mesh.__dict__.pop("_located")
    b = fem.locate_points(mesh, pts, index=False)
    assert b.path == "general" and b is not a
    assert np.array_equal(a.cells, b.cells) and np.array_equal(a.lam.view(np.int64), b.lam.view(np.int64))
    assert np.array_equal(a.cells, np.arange(mesh.num_cells()))
    mesh.__dict__.pop("_located")
    assert fem.LOCATE_INDEX_MIN_WORK > len(pts) * mesh.num_cells()
    c = fem.locate_points(mesh, pts[:50])                                 # auto: the mesh holds an index
    assert c.path == "index" and be.points_index_info(mh)["builds"] == 1
    with pytest.raises(NotImplementedError, match="index"):
        fem.locate_points(mesh, pts, index=True, device=False)
    fem.clear_caches()
    assert be.points_index_info(mh) == dict(built=0, builds=0, n=(0, 0, 0), entries=0, longest=0, bytes=0)
    d = fem.locate_points(mesh, pts[:50])                                 # auto, nothing built, below the threshold
    assert d.path == "general" and be.points_index_info(mh)["built"] == 0
    fem.clear_caches()


def test_frontend_sensor_response(hip_backend):
    """evaluate_sensor_response_many(index=True) on a jittered box: values and Jacobian equal those of index=False, bit for bit."""
    from pgdrome_amd.model import PGD
    be = hip_backend
    rng = np.random.default_rng(31)
    mesh = jittered_box()
    m1, m2 = fem.IntervalMesh(6, 0.0, 1.0), fem.IntervalMesh(4, 1.0, 3.0)
    spaces = (fem.VectorFunctionSpace(mesh, "CG", 2, dim=3), fem.FunctionSpace(m1, "CG", 1), fem.FunctionSpace(m2, "CG", 2))
    modes = []
    for W in spaces:
        row = []
        for _ in range(4):
            f = fem.Function(W)
            f.vector()._host = rng.uniform(-1.0, 1.0, W.dim())
            f.vector().touched_host()
            row.append(f)
        modes.append(row)
    sol = PGD(name="s", n_modes=4, fmeshes=[mesh, m1, m2], pgd_modes=modes, name_coord=["X", "p", "q"], modes_info=["U", "Node", "Vector"])
    pts = ref.interior_points(mesh.coordinates(), mesh.cells(), seed=22)[0][::2]
    samples = np.stack([rng.uniform(0.0, 1.0, 6), rng.uniform(1.0, 3.0, 6)], axis=1)
    mh = mesh.layout(1).handle()
    got = {}
    for index in (True, False):
        fem.clear_caches()
        res = sol.evaluate_sensor_response_many(0, [1, 2], samples, 0, pts, d_dim=[1, 2], index=index)
        assert be.points_last_path() == (_lib.LOCATE_PATH_INDEX if index else _lib.LOCATE_PATH_GENERAL)
        assert be.points_index_info(mh)["built"] == int(index)
        got[index] = (res.values.copy(), res.jacobian.copy())
    assert got[True][0].shape == (6, len(pts), 3) and got[True][1].shape == (6, len(pts), 3, 2)
    assert np.array_equal(got[True][0].view(np.int64), got[False][0].view(np.int64))
    assert np.array_equal(got[True][1].view(np.int64), got[False][1].view(np.int64))
    fem.clear_caches()
    assert be.points_index_info(mh)["built"] == 0
