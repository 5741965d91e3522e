"""The case table of tests/test_mg_cycles_cpu.py and tests/test_mg_cycles_gpu.py: lattices, operator families, Dirichlet sets, seeds
and right-hand sides on which the three multigrid cycles of the PCG - the constant-stencil cycle (pgdrome_amd/csrc/pgd_mg.hip,
restated in oracle/mg_numpy.py), the variable-coefficient cycle (csrc/pgd_vmg.hip, tests/vmg_reference.py) and the component-wise
cycle (tests/cmg_reference.py) - are held to their restatements node by node, on the FIRST THREE iterates of a cut-off solve instead
of the converged one (a Krylov method repairs a wrong preconditioner: the converged solve cannot see it), and the tolerance table TAU
of that comparison.

Every lattice is as small as its purpose allows; the comment beside it says what it reaches that the others do not.
"""
import contextlib
import functools

import numpy as np
import scipy.sparse as sps

from oracle import fem_numpy as FN
from oracle import mg_numpy as MG
from tests import cmg_reference as CM
from tests import robin_reference as R
from tests import vmg_reference as V

KS = (1, 2, 3)
RTOL = 1e-14                      # never reached in three iterations from the right-hand sides below: a cut-off solve runs k iterations

# ---- the tolerance --------------------------------------------------------------------------------------------------------------
# max |x_dev - x_ref| <= TAU[cycle][k] * max |x_ref| for the k-th iterate.  TAU = 100 N_k, N_k the rounding noise of the RESTATEMENT:
# the largest relative max-norm change of x_k over the cases of the table (all three kinds of right-hand side) when every operator
# entry moves by up to 1 ulp, symmetrically, 3 seeds (tests/test_mg_cycles_cpu.py measures it and asserts N_k <= TAU / 32).  The
# factor 100 stands for what the ulp perturbation does not sample: the device groups its 15-term rows, its levels, its 24 sweeps and
# its dot trees differently and contracts to fma.  Hard cap 1e-10: the smallest effect of a mutant on x_1 is 4e-6.
# NOISE: the measured N_k, rounded up.  DEVICE: the largest deviations of an MI355X from the restatement over the same cases, as
# tests/test_mg_cycles_gpu.py printed them when the table was set (data, not a bound: 16 to 170 times under TAU).  A deviation above
# TAU is a finding, to be settled by reading the kernel against the restatement, not by widening.
TAU_CAP = 1e-10
NOISE = {"vmg": {1: 1.5e-15, 2: 3.5e-15, 3: 7.5e-15},       # largest on 33x25x20-mixed; 17x17x17-weighted stays under 9e-16
         "cmg": {1: 1.4e-15, 2: 1.5e-15, 3: 1.5e-15},
         "mg": {1: 1.1e-14, 2: 1.4e-14, 3: 1.3e-14},        # (8 stencil values move ALL rows the same way: 33x18x16 is the largest)
         "slab": 1.6e-14}                                   # the four stages of one cycle on 20x17x24, each from the stage before
TAU = {c: ({k: min(100.0 * n, TAU_CAP) for k, n in v.items()} if isinstance(v, dict) else min(100.0 * v, TAU_CAP)) for c, v in NOISE.items()}
DEVICE = {"vmg": {1: 4.2e-15, 2: 1.4e-14, 3: 4.6e-14}, "cmg": {1: 1.5e-15, 2: 1.5e-15, 3: 1.4e-15},
          "mg": {1: 6.3e-15, 2: 6.9e-15, 3: 6.6e-15}, "slab": 1.0e-14}

# ---- the lattices ---------------------------------------------------------------------------------------------------------------
# vmg: (shape (nx, ny, nz), steps, family, Dirichlet set (None: the family's own), levels, values of PGD_TUNE_MG_MARCH_MIN, deltas)
VMG_CASES = {
    # two levels, the hull eliminated (every kernel's range logic rests on zeros there), a weight that varies along every axis
    "17x17x17-weighted": dict(shape=(17, 17, 17), step=1.0 / 16, family="weighted", dirichlet=None, levels=2, march=(64,),
                              deltas={"centre": (8, 8, 8)}),
    # even node counts along y and z: far faces without a coarse counterpart; robin eliminates NO node, so hull, edge and corner
    # nodes are live on both levels - the far corner interpolates from no coarse node of its own on any axis
    "33x25x20-robin": dict(shape=(33, 25, 20), step=1.0 / 16, family="robin", dirichlet=None, levels=2, march=(64,),
                           deltas={"far_corner": (32, 24, 19), "inward": (31, 23, 18)}),
    # the same lattice with two eliminated faces that meet in an edge: live far faces next to eliminated ones
    "33x25x20-mixed": dict(shape=(33, 25, 20), step=1.0 / 16, family="mixed", dirichlet=None, levels=2, march=(64,),
                           deltas={"far_y_face": (16, 24, 9)}),
    # three levels (41 535 -> 5 940 -> 918 nodes), an odd ny (the last thread pair of a march patch has a live lower and a dead upper
    # row, in both epilogues and in the dot), a second x tile one node wide, marches of three planes; under PGD_TUNE_MG_MARCH_MIN = 64
    # level 0 runs in k_vmg_march, under 0 in k_vmg_pass / k_vmg_wmul.  Only the face z = 0 is eliminated, so the seam and the last
    # row pair carry live nodes
    "65x71x9-weighted": dict(shape=(65, 71, 9), step=1.0 / 64, family="weighted", dirichlet="face", levels=3, march=(64, 0),
                             deltas={"seam_63": (63, 35, 4), "seam_64": (64, 35, 4), "last_row": (30, 70, 4)}),
}

# cmg: 17^3 base lattice (two levels per component).  (ncomp, family, Dirichlet case, delta dof = (node, component))
CMG_CASES = {
    # only u_x fixed on x = 0 and only u_z on z = 0: three different eliminated sets, one of them empty
    "17x17x17-roller": dict(shape=(17, 17, 17), ncomp=3, family="elastic", dirichlet="roller", levels=2, deltas={"centre_uy": ((8, 8, 8), 1)}),
    # all components share one eliminated set
    "17x17x17-clamped": dict(shape=(17, 17, 17), ncomp=3, family="elastic", dirichlet="clamped", levels=2, deltas={"far_corner_uz": ((16, 16, 16), 2)}),
    # two components on the 3-D lattice (the stride of k_cmg_split / k_cmg_merge is ncomp, not the dimension)
    "17x17x17-pair": dict(shape=(17, 17, 17), ncomp=2, family="pair", dirichlet="clamped", levels=2, deltas={"centre_u1": ((8, 8, 8), 1)}),
}

# mg through pgd_pcg_solve: stiffness + 3 mass, the hull eliminated.  (shape (nx, ny, nz), levels, march minima)
MG_CASES = {
    # two levels, an even node count along x and z: far faces without a coarse counterpart
    "20x17x12": dict(shape=(20, 17, 12), levels=2, march=(64,), deltas={"next_to_far_x": (18, 8, 6)}),
    # three levels (33x18x16 -> 17x9x8 -> 9x5x4): the only mg lattice on which k_mg_restrict / k_mg_prolong run between coarse levels
    "33x18x16": dict(shape=(33, 18, 16), levels=3, march=(64,), deltas={"centre": (16, 9, 8)}),
    # wide enough for the stencil march under PGD_TUNE_MG_MARCH_MIN = 16: two x tiles, the second three nodes wide, a second y tile
    # three rows high, marches of three planes; the same lattice under 0 in k_mg_pass
    "67x19x9": dict(shape=(67, 19, 9), levels=2, march=(16, 0), deltas={"seam": (64, 16, 4)}),
}

# the slab pieces: global lattice (x, y, z), stencil stiffness + 3 mass; name -> (first local plane, local planes, owned local planes)
SLAB_SHAPE = (20, 17, 24)          # levels 20x17x24 -> 10x9x12 -> 5x5x6: pgd_mg_coarse runs a restriction and a prolongation of its own
SLABS = {
    "whole": (0, 24, 0, 24),        # no ghosts: mg_slab_up returns z = M r itself
    "bottom": (0, 8, 0, 7),         # global planes [0, 7): one ghost above
    "interior": (6, 8, 1, 7),       # global planes [7, 13), starts at an ODD plane: coarse planes (7 + 1) // 2 = 4 .. 6; two ghosts
    "top": (12, 12, 1, 12),         # global planes [13, 24): ends at the far face (even nz: no coarse counterpart)
    "three": (6, 5, 1, 4),          # global planes [7, 10): exactly three owned planes, the least mg_slab_march takes
}
SLAB_PARTITION = ("bottom", "interior", "top")
SLAB_RUNS = [("whole", 64), ("whole", 16), ("bottom", 64), ("interior", 64), ("top", 64), ("three", 16), ("three", 0)]


def node_index(shape, xyz):
    nx, ny, _ = shape
    return xyz[0] + nx * (xyz[1] + ny * xyz[2])


def neighbourhood(shape, xyz):
    """Node indices of the 15-point neighbourhood of a node, inside the lattice."""
    out = []
    for dx, dy, dz in V.PATTERN:
        p = (xyz[0] + dx, xyz[1] + dy, xyz[2] + dz)
        if all(0 <= q < s for q, s in zip(p, shape)):
            out.append(node_index(shape, p))
    return np.array(out)


def kinds(case):
    return ["zero", "start"] + ["delta:" + d for d in sorted(case["deltas"])]


def right_hand_side(n, kind, delta_index=None):
    """(b, x0) of one kind: a zero start with a random b; a random start (it violates the Dirichlet values, which are b) with another
    random b; b = e_j from a zero start."""
    if kind == "zero":
        return np.random.default_rng(11).uniform(-1, 1, n), None
    if kind == "start":
        rng = np.random.default_rng(29)
        return rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    b = np.zeros(n)
    b[delta_index] = 1.0
    return b, None


# ---- the operator families (moved here from tests/test_vmg_gpu.py, which imports it) ----------------------------------------------

def far_facets(coords, cells):
    on = coords[:, 0] >= coords[:, 0].max()
    return np.array([c[on[c]] for c in cells[on[cells].sum(axis=1) == 3]], dtype=np.int32)


def family(ctx, h, coords, cells, name):
    """(device atoms, coefficients, Dirichlet dofs, the same operator from the numpy oracle's assembly, handles to free).  ctx None: no
    device, the atoms are an empty list."""
    n = coords.shape[0]
    sets = V.dirichlet_sets(coords)
    dev = ctx is not None
    if name == "weighted":
        w = 1.0 + coords[:, 0] + 4.0 * coords[:, 1] * coords[:, 2]
        wv = ctx.vec_from(w) if dev else 0
        atoms = [ctx.atom_assemble(h, FN.WSTIFF, 0, 0, wv)] if dev else []
        A = FN.assemble_atom(coords, cells, FN.WSTIFF, 0, 0, w)
        return atoms, [1.0], sets["hull"], A, [wv] if dev else []
    if name == "two_material":
        mask = V.inclusion_mask(coords, cells)
        assert 0 < mask.sum() < mask.size
        atoms = [ctx.atom_assemble_cells(h, FN.STIFF, 0, 0, 0, 1 - mask), ctx.atom_assemble_cells(h, FN.STIFF, 0, 0, 0, mask)] if dev else []
        A = FN.assemble_atom(coords, cells[mask == 0], FN.STIFF) + 25.0 * FN.assemble_atom(coords, cells[mask != 0], FN.STIFF)
        return atoms, [1.0, 25.0], sets["face"], A, []
    if name == "robin":
        facets = far_facets(coords, cells)
        atoms = [ctx.atom_assemble(h, FN.STIFF), ctx.atom_assemble_facets(h, facets)] if dev else []
        A = 2.0 * FN.assemble_atom(coords, cells, FN.STIFF) + 3.0 * sps.csr_matrix(R.facet_mass_matrix(coords, facets, n))
        return atoms, [2.0, 3.0], sets["none"], A, []
    if name == "constant":
        # one stencil with the hull eliminated - what PGD_TUNE_PCG_PRECOND = 1 is made for: under 2 it takes the new cycle as well
        atoms = [ctx.atom_assemble(h, FN.STIFF), ctx.atom_assemble(h, FN.MASS)] if dev else []
        A = FN.assemble_atom(coords, cells, FN.STIFF) + 3.0 * FN.assemble_atom(coords, cells, FN.MASS)
        return atoms, [1.0, 3.0], sets["hull"], A, []
    # stiffness + mass, eliminated: the face x = min and the face z = max (two faces that meet in an edge, nothing else)
    lo, hi = coords.min(axis=0), coords.max(axis=0)
    bc = np.where((coords[:, 0] <= lo[0]) | (coords[:, 2] >= hi[2]))[0]
    atoms = [ctx.atom_assemble(h, FN.STIFF), ctx.atom_assemble(h, FN.MASS)] if dev else []
    A = FN.assemble_atom(coords, cells, FN.STIFF) + 0.5 * FN.assemble_atom(coords, cells, FN.MASS)
    return atoms, [1.0, 0.5], bc, A, []


def vmg_mesh(case):
    return V.box(case["shape"], steps=(case["step"],) * 3)


def vmg_dirichlet(case, coords, bc_family):
    return np.asarray(bc_family if case["dirichlet"] is None else V.dirichlet_sets(coords)[case["dirichlet"]], dtype=np.int32)


@functools.lru_cache(maxsize=None)
def vmg_operator(name):
    """(A with the identity on the Dirichlet rows and columns, Dirichlet dofs) of a vmg case, from the numpy oracle's assembly."""
    case = VMG_CASES[name]
    coords, cells = vmg_mesh(case)
    _, _, bc, A, _ = family(None, 0, coords, cells, case["family"])
    bc = vmg_dirichlet(case, coords, bc)
    return V.apply_dirichlet_exact(sps.csr_matrix(A), bc), bc


@functools.lru_cache(maxsize=None)
def mg_stencil(name):
    """(the 8 couplings of stiffness + 3 mass on the case's mesh, slot s = dx + 2 dy + 4 dz, from a row in the middle; hull dofs)."""
    shape = (MG_CASES[name]["shape"] if name in MG_CASES else SLAB_SHAPE)
    coords, cells = V.box(shape)
    nx, ny, nz = shape
    A = (FN.assemble_atom(coords, cells, FN.STIFF) + 3.0 * FN.assemble_atom(coords, cells, FN.MASS)).tocsr()
    mid = node_index(shape, (nx // 2, ny // 2, nz // 2))
    c = np.array([A[mid, mid + dx + nx * dy + nx * ny * dz] for dx, dy, dz in MG.OFFS])
    return c, V.dirichlet_sets(coords)["hull"].astype(np.int32)


def cmg_space(case):
    from pgdrome_amd import fem
    shape = case["shape"]
    if case["ncomp"] == 3:
        return CM.vector_space(shape)
    cells = tuple(s - 1 for s in shape)
    mesh = fem.BoxMesh(fem.Point(0.0, 0.0, 0.0), fem.Point(*(c / 16.0 for c in cells)), *cells)
    return fem.VectorFunctionSpace(mesh, "P", 1, dim=case["ncomp"])


def cmg_operator(case, Vh):
    """(fem.Matrix, the combined operator read back from the backend in use, Dirichlet dofs) of a cmg case, through the frontend."""
    from pgdrome_amd import fem
    bc = CM.dirichlet_dofs(case["shape"], case["ncomp"], case["dirichlet"])
    if case["family"] == "elastic":
        A, M = CM.frontend_operator(Vh, "elastic", bc, k_found=2.0)
        return A, M, bc
    # "pair": two fields on the box, each with its own Laplacian, coupled through u_0,x v_1,y + u_1,y v_0,x (symmetric; positive with
    # the foundation term: |2 a b| <= a^2 + b^2)
    u, v = fem.TrialFunction(Vh), fem.TestFunction(Vh)
    a = sum(u[i].dx(k) * v[i].dx(k) * fem.dx for i in range(2) for k in range(3))
    a = a + fem.Constant(0.5) * (u[0].dx(0) * v[1].dx(1) + u[1].dx(1) * v[0].dx(0)) * fem.dx + fem.Constant(2.0) * fem.inner(u, v) * fem.dx
    A = fem.assemble(a)
    A.bc_vertices = np.unique(np.asarray(bc, dtype=np.int32))       # (as CM.frontend_operator does, and for its reasons)
    A._op = 0
    return A, CM.read_back(A), bc


# ---- the restatements' iterates ----------------------------------------------------------------------------------------------------

@contextlib.contextmanager
def built_once(module, attr):
    """Inside: module.attr is computed at the first call and handed out again at the later ones - the cut-off solves of one operator
    for k = 1, 2, 3 and several right-hand sides share the restatement's hierarchy instead of rebuilding it.  The arguments must be
    the same at every call (they are: one operator per block)."""
    real, box = getattr(module, attr), []

    def once(*a, **kw):
        if not box:
            box.append(real(*a, **kw))
        return box[0]
    setattr(module, attr, once)
    try:
        yield
    finally:
        setattr(module, attr, real)


def vmg_iterates(A, shape, rhs):
    """{kind: [x_1, x_2, x_3]} of V.pcg on one operator; rhs = {kind: (b, x0)}."""
    out = {}
    with built_once(V, "scale_unit"), built_once(V, "build"):
        for kind, (b, x0) in rhs.items():
            out[kind] = []
            for k in KS:
                x, it, _ = V.pcg(A, b, shape, x0=x0, rtol=RTOL, maxit=k)
                assert it == k
                out[kind].append(x)
    return out


def cmg_iterates(M, shape, ncomp, rhs):
    out = {}
    with built_once(CM, "build"):
        for kind, (b, x0) in rhs.items():
            out[kind] = []
            for k in KS:
                x, it, _ = CM.pcg(M, b, shape, ncomp, rtol=RTOL, maxit=k, x0=x0)
                assert it == k
                out[kind].append(x)
    return out


def mg_iterates(shape, c, rhs):
    """shape = (nx, ny, nz); vectors flat in node order (the restatement's arrays are [z, y, x]: the same memory)."""
    zyx = shape[::-1]
    out = {}
    with built_once(MG, "build_levels"):
        for kind, (b, x0) in rhs.items():
            out[kind] = []
            for k in KS:
                x, it, _ = MG.pcg(zyx, c, b.reshape(zyx), x0=None if x0 is None else x0.reshape(zyx), rtol=RTOL, maxit=k)
                assert it == k
                out[kind].append(x.ravel())
    return out


def case_rhs(case, n, index_of):
    """{kind: (b, x0)} of a case; index_of maps a delta's entry of the table to its dof."""
    return {kind: right_hand_side(n, kind, index_of(case["deltas"][kind[6:]]) if kind.startswith("delta:") else None) for kind in kinds(case)}


@functools.lru_cache(maxsize=None)
def vmg_reference(name):
    case = VMG_CASES[name]
    A, bc = vmg_operator(name)
    rhs = case_rhs(case, A.shape[0], lambda xyz: node_index(case["shape"], xyz))
    return rhs, vmg_iterates(A, case["shape"], rhs)


@functools.lru_cache(maxsize=None)
def mg_reference(name):
    case = MG_CASES[name]
    c, hull = mg_stencil(name)
    rhs = case_rhs(case, int(np.prod(case["shape"])), lambda xyz: node_index(case["shape"], xyz))
    return rhs, mg_iterates(case["shape"], c, rhs)


def cmg_reference(case, M):
    rhs = case_rhs(case, M.shape[0], lambda nc: case["ncomp"] * node_index(case["shape"], nc[0]) + nc[1])
    return rhs, cmg_iterates(M, case["shape"], case["ncomp"], rhs)


def deviation(x, ref, idx=None):
    """max |x - ref| / max |ref| over the dofs idx (default: all)."""
    if idx is not None:
        x, ref = x[idx], ref[idx]
    return float(np.abs(x - ref).max() / np.abs(ref).max())


def delta_neighbourhood(case, kind, ncomp=1):
    """The dofs of the 15-point neighbourhood of a delta's node (all components), None for the other kinds."""
    if not kind.startswith("delta:"):
        return None
    d = case["deltas"][kind[6:]]
    nodes = neighbourhood(case["shape"], d if ncomp == 1 else d[0])
    return nodes if ncomp == 1 else (nodes[:, None] * ncomp + np.arange(ncomp)[None, :]).ravel()


# ---- 1-ulp perturbations (the noise the tolerance is set from) ------------------------------------------------------------------------

def ulp_perturbed(A, seed):
    """A with every stored entry of a row that has couplings multiplied by 1 + e 2^-52, e in {-1, 0, 1} seeded, symmetrically (the
    upper triangle decides); identity rows stay exact."""
    A = sps.csr_matrix(A).tocoo()
    rng = np.random.default_rng(seed)
    e = rng.integers(-1, 2, A.nnz).astype(np.float64)
    lo, hi = np.minimum(A.row, A.col), np.maximum(A.row, A.col)
    _, first, inv = np.unique(lo.astype(np.int64) * A.shape[0] + hi, return_index=True, return_inverse=True)
    e = e[first][inv]                                        # (i, j) and (j, i) share one draw
    e[V.eliminated_rows(A)[A.row]] = 0.0                     # identity rows
    return sps.csr_matrix((A.data * (1.0 + e * 2.0 ** -52), (A.row, A.col)), shape=A.shape)


def ulp_perturbed_stencil(c, seed):
    return np.asarray(c) * (1.0 + np.random.default_rng(seed).integers(-1, 2, 8) * 2.0 ** -52)
