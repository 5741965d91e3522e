"""The three multigrid cycles of the PCG on the device against their numpy restatements, NODE BY NODE:

  (a) cut-off solves: pgd_pcg_solve with maxit = 1, 2, 3 under PGD_TUNE_PCG_PRECOND = 1 (pgdrome_amd/csrc/pgd_mg.hip), 2 and 3
      (csrc/pgd_vmg.hip) against the restatement's pcg(..., maxit = k) on the cases of tests/mg_cycle_cases.py.  The first iterate is
      alpha M b with alpha = r.z / p.Ap: it holds the whole cycle and the fused r . z of its last pass, the second holds beta.  A
      converged solve - what the other test files compare - hides a wrong preconditioner behind the Krylov method;
  (b) the z-slab pieces pgd_mg_slab_* / pgd_mg_coarse called directly in one process, ghost planes filled by hand, every stage
      against oracle/mg_numpy.py::Slab from the restatement's input of that stage;
  (c) the depth of the hierarchies the counters report.

Tolerances: tests/mg_cycle_cases.py::TAU (100 x the restatement's own 1-ulp noise, tests/test_mg_cycles_cpu.py).
"""
import contextlib
import functools
import math
import types

import numpy as np
import pytest

from oracle import fem_numpy as FN
from oracle import mg_numpy as MG
from pgdrome_amd import fem
from pgdrome_amd._lib import PgdError
from tests import mg_cycle_cases as T
from tests import vmg_reference as V

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
ERR_INVALID = -1
_WORST = {}                        # (cycle, k) -> largest deviation seen, printed as it grows (the figures of the commit message)


@pytest.fixture(scope="module")
def hip_backend():
    from pgdrome_amd.hip_backend import HipBackend
    old = fem._backend
    be = fem.set_backend(HipBackend(0))
    fem.clear_caches()
    yield be
    _CMG.clear()
    fem.set_backend(old)
    fem.clear_caches()


class _Device:
    """Meshes and atoms of the cases on the device, uploaded at first use and freed when the module is done."""

    def __init__(self, ctx):
        self.ctx, self.meshes, self.cases, self.extra = ctx, {}, {}, []

    def stencil_atoms(self, shape, origin_plane=0):
        """(mesh, stiffness, mass) of the box of `shape` nodes whose first plane is plane `origin_plane` of a taller lattice."""
        key = (shape, origin_plane)
        if key not in self.meshes:
            coords, cells = V.box(shape, origin=(0.0, 0.0, origin_plane / 16.0))
            h = self.ctx.mesh_upload(coords, cells.astype(np.int32))
            self.meshes[key] = (h, self.ctx.atom_assemble(h, FN.STIFF), self.ctx.atom_assemble(h, FN.MASS))
        return self.meshes[key]

    def vmg(self, name):
        """(mesh, atoms, coefficients, Dirichlet dofs) of a vmg case."""
        if name not in self.cases:
            case = T.VMG_CASES[name]
            coords, cells = T.vmg_mesh(case)
            h = self.ctx.mesh_upload(coords, cells.astype(np.int32))
            assert self.ctx.mesh_lattice(h)[0]
            atoms, coefs, bcf, _, extra = T.family(self.ctx, h, coords, cells, case["family"])
            self.extra += extra
            self.cases[name] = (h, atoms, coefs, T.vmg_dirichlet(case, coords, bcf))
        return self.cases[name]

    def free(self):
        for h, atoms, _, _ in self.cases.values():
            for a in atoms:
                self.ctx.atom_free(a)
            self.ctx.mesh_free(h)
        for v in self.extra:
            self.ctx.vec_free(v)
        for h, ak, am in self.meshes.values():
            self.ctx.atom_free(ak)
            self.ctx.atom_free(am)
            self.ctx.mesh_free(h)


@pytest.fixture(scope="module")
def device(ctx):
    d = _Device(ctx)
    yield d
    d.free()


def _hold(cycle, k, what, x, ref, idx=None):
    """max |x - ref| <= TAU max |ref| over the dofs idx (default: all); the figure is printed before it is judged."""
    d = T.deviation(x, ref, idx)
    tau = T.TAU[cycle][k] if k else T.TAU[cycle]
    if d > _WORST.get((cycle, k), -1.0):
        _WORST[(cycle, k)] = d
    print("deviation %s k=%d %s: %.2e (tau %.1e; largest so far %.2e)" % (cycle, k, what, d, tau, _WORST[(cycle, k)]))
    assert d <= tau, (cycle, k, what, d, tau)


def _cut_off_solves(ctx, cycle, case, make_op, kind, rhs, ref, bc, ncomp=1):
    """pgd_pcg_solve with maxit = 1, 2, 3 on a fresh operator against the restatement's iterates of the same cut-off."""
    b, x0 = rhs[kind]
    idx = T.delta_neighbourhood(case, kind, ncomp)
    op = make_op()
    bv = ctx.vec_from(b)
    try:
        for k in T.KS:
            xv = ctx.vec_from(np.zeros(b.size) if x0 is None else x0)
            try:
                it, rel = ctx.pcg_solve(op, bv, xv, T.RTOL, 0.0, k)
                x = ctx.vec_download(xv)
            finally:
                ctx.vec_free(xv)
            assert it == k and rel > T.RTOL
            assert np.array_equal(x[bc], b[bc])
            _hold(cycle, k, kind, x, ref[kind][k - 1])
            if idx is not None:                              # a delta: a wrong coupling at one offset cannot hide behind the peak
                _hold(cycle, k, kind + " (15-point neighbourhood)", x, ref[kind][k - 1], idx)
    finally:
        ctx.vec_free(bv)
        ctx.atom_free(op)


# ---- (a) vmg ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,kind", [(n, k) for n in sorted(T.VMG_CASES) for k in T.kinds(T.VMG_CASES[n])])
def test_vmg_cut_off_solves_walk_the_restatement(ctx, device, name, kind):
    """PGD_TUNE_PCG_PRECOND = 2.  The lattices that march run twice, level 0 in k_vmg_march (both epilogues, counted) and in the plain
    kernels: both are held to the SAME reference."""
    case = T.VMG_CASES[name]
    h, atoms, coefs, bc = device.vmg(name)
    rhs, ref = T.vmg_reference(name)
    try:
        for march_min in case["march"]:
            ctx.tune(40, 2)
            ctx.tune(42, march_min)
            v0, mg0 = ctx.vmg_stats(), ctx.mg_stats()
            _cut_off_solves(ctx, "vmg", case, lambda: ctx.op_combine(h, atoms, coefs, bc), kind, rhs, ref, bc)
            v1 = ctx.vmg_stats()
            assert v1["solves"] == v0["solves"] + len(T.KS) and v1["fallbacks"] == v0["fallbacks"] and ctx.mg_stats() == mg0
            assert v1["levels"] == case["levels"]                                                       # (c)
            if len(case["march"]) > 1:
                assert (v1["march_passes"] > v0["march_passes"]) == (march_min > 0), (march_min, v0, v1)
    finally:
        ctx.tune(40, 0)
        ctx.tune(42, 64)


# ---- (a) cmg ------------------------------------------------------------------------------------------------------------------------

_CMG = {}


def _cmg_device(name):
    """(fem.Matrix on the HIP backend, its operator read back, Dirichlet dofs, right-hand sides, the restatement's iterates)"""
    if name not in _CMG:
        case = T.CMG_CASES[name]
        A, M, bc = T.cmg_operator(case, T.cmg_space(case))
        _CMG[name] = (A, M, bc) + T.cmg_reference(case, M)
    return _CMG[name]


@pytest.mark.parametrize("name,kind", [(n, k) for n in sorted(T.CMG_CASES) for k in T.kinds(T.CMG_CASES[n])])
def test_cmg_cut_off_solves_walk_the_restatement(hip_backend, name, kind):
    """PGD_TUNE_PCG_PRECOND = 3 on operators built through the frontend and read back from the device for the restatement."""
    ctx, case = hip_backend.ctx, T.CMG_CASES[name]
    A, M, bc, rhs, ref = _cmg_device(name)
    try:
        ctx.tune(40, 3)
        c0, v0, mg0 = ctx.cmg_stats(), ctx.vmg_stats(), ctx.mg_stats()
        _cut_off_solves(ctx, "cmg", case, A.op, kind, rhs, ref, bc, case["ncomp"])
        c1 = ctx.cmg_stats()
        assert c1["solves"] == c0["solves"] + len(T.KS) and c1["fallbacks"] == c0["fallbacks"]
        assert ctx.vmg_stats() == v0 and ctx.mg_stats() == mg0
        assert c1["levels"] == case["levels"]                                                           # (c)
    finally:
        ctx.tune(40, 0)
        if kind == T.kinds(case)[-1]:
            _CMG.pop(name, None)


# ---- (a) mg -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,kind", [(n, k) for n in sorted(T.MG_CASES) for k in T.kinds(T.MG_CASES[n])])
def test_mg_cut_off_solves_walk_the_restatement(ctx, device, name, kind):
    """PGD_TUNE_PCG_PRECOND = 1 on stiffness + 3 mass with the hull eliminated.  67 x 19 x 9 runs level 0 in the stencil march of the
    product (PGD_TUNE_MG_MARCH_MIN = 16: two more march launches per cycle, counted) and in k_mg_pass, against the same reference.
    (pgd_mg_counts reports no depth: a 33 x 18 x 16 hierarchy that stopped at two levels would smooth 1 224 nodes 24 times where the
    restatement coarsens once more, and miss it by orders of magnitude more than the tolerance.)"""
    case = T.MG_CASES[name]
    h, ak, am = device.stencil_atoms(case["shape"])
    _, hull = T.mg_stencil(name)
    rhs, ref = T.mg_reference(name)
    launches = {}
    try:
        for march_min in case["march"]:
            ctx.tune(40, 1)
            ctx.tune(42, march_min)
            s0, v0, k0 = ctx.mg_stats(), ctx.vmg_stats(), ctx.kernel_counts()["stencil_march"]
            _cut_off_solves(ctx, "mg", case, lambda: ctx.op_combine(h, [ak, am], [1.0, 3.0], hull), kind, rhs, ref, hull)
            s1 = ctx.mg_stats()
            assert s1["solves"] == s0["solves"] + len(T.KS) and s1["fallbacks"] == s0["fallbacks"] and ctx.vmg_stats()["solves"] == v0["solves"]
            launches[march_min] = ctx.kernel_counts()["stencil_march"] - k0
        if len(case["march"]) > 1:
            # the three solves run at least 1 + 2 + 3 cycles, two level-0 passes each
            assert launches[16] >= launches[0] + 2 * 6, launches
    finally:
        ctx.tune(40, 0)
        ctx.tune(42, 64)


# ---- (b) the slab pieces ---------------------------------------------------------------------------------------------------------------

NX, NY, NZ = T.SLAB_SHAPE
PLANE = NX * NY
ZYX = (NZ, NY, NX)


def _hull_of_the_global_lattice(zoff, nzloc):
    x, y, z = V.node_coords((NX, NY, nzloc))
    z = z + zoff
    return (x == 0) | (y == 0) | (z == 0) | (x == NX - 1) | (y == NY - 1) | (z == NZ - 1)


@contextlib.contextmanager
def _slab(device, name, march_min=64, bc=None):
    """The local operator of a slab the way dist.sharded_box_mesh / TorchComm build it - a box of the local planes, op_combine with
    the global hull's nodes that lie in it - and pgd_mg_slab_setup on it."""
    ctx = device.ctx
    zoff, nzloc, lz0, lz1 = T.SLABS[name] if isinstance(name, str) else name
    h, ak, am = device.stencil_atoms((NX, NY, nzloc), zoff)
    hull = _hull_of_the_global_lattice(zoff, nzloc)
    op = ctx.op_combine(h, [ak, am], [1.0, 3.0], np.where(hull)[0].astype(np.int32) if bc is None else bc)
    vecs = []

    def vec(a):
        vecs.append(ctx.vec_from(a))
        return vecs[-1]
    try:
        ctx.tune(42, march_min)
        s = types.SimpleNamespace(op=op, zoff=zoff, nzloc=nzloc, lz0=lz0, lz1=lz1, own0=lz0 * PLANE, own1=lz1 * PLANE, n=nzloc * PLANE,
                                  hull=hull, vec=vec, planes=slice(zoff, zoff + nzloc))
        s.n1 = ctx.mg_slab_setup(op, NZ, zoff, s.own0, s.own1)
        s.owned = np.zeros((nzloc, NY, NX), dtype=bool)
        s.owned[lz0:lz1] = True
        yield s
    finally:
        ctx.tune(42, 64)
        for v in vecs:
            ctx.vec_free(v)
        ctx.atom_free(op)


@functools.lru_cache(maxsize=None)
def _slab_reference():
    """The whole lattice in the restatement: (stencil, Slab, r, t, b1, x1, z) - every stage's input for every slab."""
    c, _ = T.mg_stencil("slab")
    sl = MG.Slab(ZYX, c, 0, NZ, 0, NZ)
    r = np.random.default_rng(17).uniform(-1, 1, ZYX) * sl.levels[0].mask
    t = sl.down(r)
    b1 = sl.restrict(t)
    x1 = sl.coarse(b1)
    out = (c, sl, r, t, b1, x1, sl.up(r, x1)[0])
    for a in out[2:]:
        a.setflags(write=False)
    return out


def _dot_depth(marched):
    """Roundings on the longest path from a product r_i z_i to the sum (tests/test_slot_pieces_gpu.py::reduce_depth): the lane's own
    chain - one product in k_mg_pass; 4 rows x 3 planes of fmas in a three-plane march of k_spmv_stencil_march - then block_sum
    (6 + 2) and k_reduce_partials on under 2048 partials (1 + 3 + 6 + 16)."""
    return (12 if marched else 1) + 6 + 2 + 1 + 3 + 6 + 16


@pytest.mark.parametrize("name,march_min", T.SLAB_RUNS, ids=["%s-march_min_%d" % r for r in T.SLAB_RUNS])
def test_slab_pieces_stage_by_stage(ctx, device, name, march_min):
    """down, restrict, coarse, up of one slab, each from the restatement's input of that stage, so that one wrong stage fails alone."""
    c, whole, r_g, t_g, b1_g, x1_g, _ = _slab_reference()
    with _slab(device, name, march_min) as s:
        assert s.n1 == b1_g.size == whole.n_coarse
        sl = MG.Slab(ZYX, c, s.zoff, s.nzloc, s.lz0, s.lz1)
        L, C = sl.levels[0], sl.levels[1]
        assert len(sl.levels) == 3
        marched = march_min > 0 and min(NX, NY) >= march_min and s.lz1 - s.lz0 >= 3
        k0 = ctx.kernel_counts()["stencil_march"]
        r = np.ascontiguousarray(r_g[s.planes])                           # ghost planes filled by hand from the global vector
        rv = s.vec(r)
        # down: t = r - w A r on the owned planes, nothing written elsewhere
        tv = s.vec(np.zeros(s.n))
        ctx.mg_slab_down(rv, tv)
        t = ctx.vec_download(tv).reshape(r.shape)
        _hold("slab", 0, "%s down" % name, t, sl.down(r))
        assert np.all(t[~s.owned] == 0.0) and np.all(t[sl.mask == 0.0] == 0.0)
        # restrict: from the restatement's t (ghost planes current); the slab's coarse planes, exact zeros elsewhere
        b1v = s.vec(np.full(s.n1, 7.0))
        ctx.mg_slab_restrict(s.vec(t_g[s.planes]), b1v)
        b1 = ctx.vec_download(b1v).reshape(C.shape)
        ref = sl.restrict(np.ascontiguousarray(t_g[s.planes]))
        _hold("slab", 0, "%s restrict" % name, b1, ref)
        mine = np.zeros(C.shape, dtype=bool)
        mine[(s.zoff + s.lz0 + 1) // 2:(s.zoff + s.lz1 + 1) // 2] = True
        assert np.all(b1[~mine] == 0.0) and np.all(b1[C.mask == 0.0] == 0.0) and np.any(b1[mine] != 0.0)
        # the replicated levels (they honour the done flag)
        ctx.flags_reset()
        x1v = s.vec(np.full(s.n1, 7.0))
        ctx.mg_coarse(s.vec(b1_g), x1v)
        x1 = ctx.vec_download(x1v).reshape(C.shape)
        _hold("slab", 0, "%s coarse" % name, x1, sl.coarse(b1_g))
        assert np.all(x1[C.mask == 0.0] == 0.0)
        # up: t = w r + P x1 on ALL local planes, z = t + w (r - A t) on the owned ones, r . z over them
        t2v, zv = s.vec(np.full(s.n, 7.0)), s.vec(np.zeros(s.n))
        dot = ctx.mg_slab_up(rv, s.vec(x1_g), t2v, zv)
        z = ctx.vec_download(zv).reshape(r.shape)
        zref, dref = sl.up(r, x1_g)
        _hold("slab", 0, "%s up: t on all local planes" % name, ctx.vec_download(t2v).reshape(r.shape),
              (L.w * r + MG.prolong(x1_g, L.shape)[s.planes]) * sl.mask)
        _hold("slab", 0, "%s up: z" % name, z, zref)
        assert np.all(z[~s.owned] == 0.0) and np.all(z[sl.mask == 0.0] == 0.0)
        if name == "whole":
            _hold("slab", 0, "whole up: z against the V-cycle", z, MG.vcycle(sl.levels, 0, r_g))
        exact, mag = math.fsum((r * z).ravel()), math.fsum(np.abs(r * z).ravel())
        bar = _dot_depth(marched) * U * mag
        ctx.mg_slab_up(rv, s.vec(x1_g), t2v, zv, slot=40)
        in_slot = ctx.slots_download(40, 1)[0]
        print("%s r . z: host %.17g slot %.17g exact %.17g, off by %.2f and %.2f of the bound" %
              (name, dot, in_slot, exact, abs(dot - exact) / bar, abs(in_slot - exact) / bar))
        assert abs(dot - exact) <= bar and abs(in_slot - exact) <= bar
        assert np.array_equal(ctx.vec_download(zv).reshape(r.shape), z)
        assert abs(exact - dref) <= T.TAU["slab"] * mag
        # the march ran where the slab is wide and thick enough for it, and only there: down + two up passes
        assert ctx.kernel_counts()["stencil_march"] - k0 == (3 if marched else 0)


def test_slab_restrictions_of_a_partition_sum_to_the_whole_bit_for_bit(ctx, device):
    """Every entry of the level-1 right-hand side has ONE non-zero contribution, so the all-reduce over the ranks is exact."""
    _, _, _, t_g, _, _, _ = _slab_reference()
    got = {}
    for name in ("whole",) + T.SLAB_PARTITION:
        with _slab(device, name) as s:
            b1v = s.vec(np.full(s.n1, 7.0))
            ctx.mg_slab_restrict(s.vec(t_g[s.planes]), b1v)
            got[name] = ctx.vec_download(b1v)
    parts = [got[n] for n in T.SLAB_PARTITION]
    assert np.all(sum((p != 0.0).astype(int) for p in parts) <= 1)
    assert np.array_equal(sum(parts), got["whole"]) and np.any(got["whole"] != 0.0)


def test_slab_cycle_is_symmetric_and_positive_on_the_device(ctx, device):
    """The four pieces chained on the whole lattice are z = M r: u . M v = v . M u within the tolerance of the stages and v . M v > 0,
    for 6 seeded pairs that vanish on the hull - the premise of the PCG, checked on the device's own numbers."""
    c, whole, *_ = _slab_reference()
    mask = whole.levels[0].mask.ravel()
    rng = np.random.default_rng(41)
    with _slab(device, "whole") as s:
        rv, tv, zv = s.vec(np.zeros(s.n)), s.vec(np.zeros(s.n)), s.vec(np.zeros(s.n))
        b1v, x1v = s.vec(np.zeros(s.n1)), s.vec(np.zeros(s.n1))

        def M(v):
            ctx.vec_upload(rv, v)
            ctx.mg_slab_down(rv, tv)
            ctx.mg_slab_restrict(tv, b1v)
            ctx.flags_reset()
            ctx.mg_coarse(b1v, x1v)
            ctx.mg_slab_up(rv, x1v, tv, zv)
            return ctx.vec_download(zv)
        for pair in range(6):
            u, v = rng.uniform(-1, 1, s.n) * mask, rng.uniform(-1, 1, s.n) * mask
            Mu, Mv = M(u), M(v)
            lhs, rhs = math.fsum(u * Mv), math.fsum(v * Mu)
            bar = T.TAU["slab"] * np.linalg.norm(u) * np.linalg.norm(Mv)
            print("pair %d: u.Mv - v.Mu = %.2e (bound %.2e), v.Mv = %.3e" % (pair, lhs - rhs, bar, math.fsum(v * Mv)))
            assert abs(lhs - rhs) <= bar
            assert math.fsum(v * Mv) > 0.0 and math.fsum(u * Mu) > 0.0


@pytest.mark.parametrize("name", ["interior", "top"])
def test_slab_fix_start_touches_eliminated_owned_rows_only(ctx, device, name):
    rng = np.random.default_rng(43)
    with _slab(device, name) as s:
        b, x = rng.uniform(-1, 1, s.n), rng.uniform(-1, 1, s.n)
        xv = s.vec(x)
        ctx.mg_slab_fix_start(s.op, s.vec(b), xv, s.own0, s.own1)
        hit = s.hull & s.owned.ravel()
        assert hit.any() and (s.hull & ~s.owned.ravel()).any()
        assert np.array_equal(ctx.vec_download(xv), np.where(hit, b, x))


def test_slab_setup_refuses_what_the_cycle_is_not_built_for(ctx, device):
    """applies = 0 (the caller keeps Jacobi), never a crash: an owned plane without its ghost, eliminated nodes that are not the hull,
    an axis under 8 nodes.  PGD_ERR_INVALID: owned rows that are not whole planes, and r == t."""
    with _slab(device, (7, 6, 0, 6)) as s:                         # global planes [7, 13) all owned: the first and the last lack a ghost
        assert s.n1 == 0
    with _slab(device, (6, 8, 1, 8)) as s:                         # ... the last one only
        assert s.n1 == 0
    x, y, z = V.node_coords((NX, NY, NZ))
    with _slab(device, "whole", bc=np.where(z == 0)[0].astype(np.int32)) as s:
        assert s.n1 == 0
    for shape in ((7, 9, 9), (9, 7, 9), (9, 9, 7)):
        h, ak, am = device.stencil_atoms(shape)
        coords, _ = V.box(shape)
        op = ctx.op_combine(h, [ak, am], [1.0, 3.0], V.dirichlet_sets(coords)["hull"].astype(np.int32))
        try:
            assert ctx.mg_slab_setup(op, shape[2], 0, 0, int(np.prod(shape))) == 0
        finally:
            ctx.atom_free(op)
    with _slab(device, "interior") as s:
        assert s.n1 > 0
        for own0, own1 in ((s.own0 + 5, s.own1), (s.own0, s.own1 - 1)):
            with pytest.raises(PgdError) as e:
                ctx.mg_slab_setup(s.op, NZ, s.zoff, own0, own1)
            assert e.value.code == ERR_INVALID
        assert ctx.mg_slab_setup(s.op, NZ, s.zoff, s.own0, s.own1) == s.n1
        rv = s.vec(np.zeros(s.n))
        with pytest.raises(PgdError) as e:
            ctx.mg_slab_down(rv, rv)
        assert e.value.code == ERR_INVALID
