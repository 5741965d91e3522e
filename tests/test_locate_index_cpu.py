"""The bin index of the point location without a GPU: the numpy restatement of the index (tests/locate_index_reference.py) never
misses a cell that the longdouble barycentric coordinates accept, and the ``index=`` argument of fem.locate_points - its checks and
the auto rule, the latter against a stub backend."""
import numpy as np
import pytest

from oracle.backend_numpy import NumpyBackend
from pgdrome_amd import _lib, fem
from tests import locate_index_reference as ixref
from tests import sensor_reference as ref


def base_meshes():
    rect = fem.RectangleMesh(fem.Point(0, 0), fem.Point(1, 1), 5, 4)
    box = fem.BoxMesh(fem.Point(0, 0, 0), fem.Point(1, 1, 1), 3, 4, 5)
    return {"rectangle_jittered": fem.Mesh(ref.jitter(rect.coordinates(), 0.2, 3), rect.cells()),
            "box345_jittered": fem.Mesh(ref.jitter(box.coordinates(), 0.2, 4, amount=0.2), box.cells())}


def arrays(name, degree):
    """(node coordinates, records) of the P1 mesh or of its P2 layout: the vertices are the first D + 1 record entries."""
    mesh = base_meshes()[name]
    if degree == 1:
        return mesh.coordinates(), mesh.cells()
    lay = mesh.layout(2)
    return np.asarray(lay.coords, dtype=np.float64).reshape(lay.n, -1), np.asarray(lay.cells)


def point_set(X, C):
    D = X.shape[1]
    verts = X[np.unique(C[:, :D + 1])]
    lo, hi = verts.min(axis=0), verts.max(axis=0)
    mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    rng = np.random.default_rng(11)
    wide = mid + 1.3 * half * rng.uniform(-1.0, 1.0, size=(400, D))
    return np.concatenate([ref.interior_points(X, C, seed=5)[0], ref.tie_points(X[:, :D], C), verts, wide])


def test_constants_are_the_librarys():
    assert ixref.INDEX_TOL == _lib.LOCATE_INDEX_TOL == 2.0 ** -10


@pytest.mark.parametrize("target", [0, 1, 10 ** 9])
@pytest.mark.parametrize("degree", [1, 2])
@pytest.mark.parametrize("name", ["rectangle_jittered", "box345_jittered"])
def test_no_accepted_cell_is_missing_from_the_bin(name, degree, target):
    """Every cell whose longdouble minimum is >= -t is among the candidates of the point's bin, t in {0, 1e-10, 2^-10}: parts (a)
    and (c) of the argument beside k_locate_index, on interior points, vertices, edge midpoints, centroids and 400 seeded points
    of the box scaled by 1.3 about its centre (clamped into the grid from outside).  The default grid, the finest one (target 1,
    which the cap on the entries coarsens) and a single bin."""
    X, C = arrays(name, degree)
    D = X.shape[1]
    nc = len(C)
    index = ixref.build(X, C, target)
    assert index["entries"] <= ixref.CAP * nc and index["bin_ptr"][-1] == index["entries"]
    assert np.array_equal(np.unique(np.concatenate(index["lists"])), np.arange(nc))      # every cell in >= 1 bin
    if target == 10 ** 9:
        assert tuple(index["n"]) == (1, 1, 1) and index["entries"] == nc
    pts = point_set(X, C)
    mins = np.asarray(ref.barycentric_all(X, C[:, :D + 1], pts).min(axis=2), dtype=np.longdouble)
    cand = ixref.candidates(index, pts)
    member = np.zeros((len(pts), nc), dtype=bool)
    for p, cells in enumerate(cand):
        member[p, cells] = True
    for t in (0.0, 1e-10, 2.0 ** -10):
        accepted = mins >= -np.longdouble(t)
        assert accepted.any(axis=1).sum() >= nc      # (the interior points at least)
        missed = accepted & ~member
        assert not missed.any(), (name, degree, target, t, np.argwhere(missed)[:5])


def test_bin_of_clamps_and_sends_nan_to_zero():
    x = np.array([-np.inf, -1.0, 0.0, 0.49, 0.5, 0.99, 1.0, 7.0, np.inf, np.nan])
    assert list(ixref.bin_of(x, 0.0, 2.0, 2)) == [0, 0, 0, 0, 1, 1, 1, 1, 1, 0]
    assert list(ixref.bin_of(x, 0.0, 0.0, 1)) == [0] * len(x)      # a flat axis: inf * 0 is a NaN


# ---- fem.locate_points(index=...)
@pytest.fixture
def numpy_backend():
    old = fem._backend
    fem.set_backend(NumpyBackend())
    fem.clear_caches()
    yield fem.get_backend()
    fem.set_backend(old)
    fem.clear_caches()


def test_argument_checks(numpy_backend):
    mesh = base_meshes()["rectangle_jittered"]
    pts = ref.interior_points(mesh.coordinates(), mesh.cells(), seed=1)[0][:3]
    for bad in ("x", 1, 0, "auto"):
        with pytest.raises(ValueError, match="index"):
            fem.locate_points(mesh, pts, index=bad)
    with pytest.raises(NotImplementedError, match="index"):
        fem.locate_points(mesh, pts, index=True)                     # the numpy backend has no index (and locates on the host)
    with pytest.raises(NotImplementedError, match="index"):
        fem.locate_points(mesh, pts, index=True, device=False)
    for ok in (None, False):
        got = fem.locate_points(mesh, pts, index=ok)
        assert got.path == "host" and got.cells.shape == (3,)


class StubBackend(NumpyBackend):
    """The numpy backend with the location entry points of the library, answered on the host: records what it was asked."""
    name = "stub"

    def __init__(self):
        super().__init__()
        self.built, self.asked, self.dropped, self.sets = set(), [], [], {}

    def points_locate(self, mesh, pts, tol=1e-10, index=False):
        self.asked.append(bool(index))
        if index:
            self.built.add(mesh)
        self.last = 3 if index else 1
        self.sets[len(self.sets) + 1] = self._fem_mesh
        self._pts = pts
        return len(self.sets)

    def points_download(self, handle):
        cells, lam, _ = fem._locate_host(self.sets[handle], self._pts)
        return cells.astype(np.int32), lam

    def points_last_path(self):
        return self.last

    def points_free(self, handle):
        self.sets.pop(handle, None)

    def points_index_info(self, mesh):
        return dict(built=int(mesh in self.built), builds=int(mesh in self.built), n=(0, 0, 0), entries=0, longest=0, bytes=0)

    def points_index_drop(self, mesh):
        self.dropped.append(mesh)
        self.built.discard(mesh)


def test_auto_rule_with_a_stub_backend(monkeypatch):
    """index=None: the index where points x cells reaches LOCATE_INDEX_MIN_WORK or the mesh holds one already, else the general
    kernel; True and False decide by themselves; clear_caches drops what was built."""
    old = fem._backend
    be = fem.set_backend(StubBackend())
    fem.clear_caches()
    try:
        mesh = base_meshes()["rectangle_jittered"]
        be._fem_mesh = mesh
        nc = mesh.num_cells()
        pts = ref.interior_points(mesh.coordinates(), mesh.cells(), seed=2)[0]
        monkeypatch.setattr(fem, "LOCATE_INDEX_MIN_WORK", 10 * nc)
        a = fem.locate_points(mesh, pts[:9])                        # 9 nc < 10 nc, no index yet
        assert be.asked == [False] and a.path == "general"
        b = fem.locate_points(mesh, pts[:10])                       # reaches the threshold: builds
        assert be.asked == [False, True] and b.path == "index"
        c = fem.locate_points(mesh, pts[:2])                        # small, but the mesh holds an index now
        assert be.asked == [False, True, True] and c.path == "index"
        d = fem.locate_points(mesh, pts[:3], index=False)           # forced off
        assert be.asked[-1] is False and d.path == "general"
        assert fem.locate_points(mesh, pts[:3], index=True) is d    # the cache does not tell them apart: the same cells and lam
        monkeypatch.setattr(fem, "LOCATE_INDEX_MIN_WORK", float("inf"))
        fem.clear_caches()
        assert be.dropped == [mesh.layout(1).handle()] and not be.built
        e = fem.locate_points(mesh, pts[:30])                       # never by itself at an infinite threshold
        assert be.asked[-1] is False and e.path == "general"
        f = fem.locate_points(mesh, pts[:4], index=True)
        assert be.asked[-1] is True and f.path == "index"
        assert np.array_equal(f.cells, np.arange(4))
    finally:
        fem.set_backend(old)
        fem.clear_caches()
