"""Robin boundary terms on the MI355X: (1) the facet atom (pgd_atom_assemble_facets) on the n^3 BoxMesh with all six faces against
k_assemble_p1_regular on the same mesh, and its memory; (2) robin_heat, the parametric Robin heat problem, on an m^3 box x 128
values of h: setup, then the fixed-point iterations of its first enrichment (seconds per iteration) and the product kernels that ran.

    python tools/bench_robin.py [n=256] [m=128]

One JSON line per part.  (The pass builds its facet set through the frontend - Mesh.facets() on the host, 4 x cells sorted keys -
which is what bounds m here, not the device.)"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pgdrome_amd import _lib, fem, problems               # noqa: E402


def box_boundary_triangles(cells, n):
    """The boundary triangles of the n^3-vertex box mesh: faces of a tetrahedron whose three vertices share a lattice index 0 or
    n - 1 along one axis (no interior face does), vertices ascending."""
    P = n * n
    out = []
    for c0 in range(0, cells.shape[0], 1 << 23):
        c = cells[c0:c0 + (1 << 23)].astype(np.int64)
        idx = np.stack([c % n, (c // n) % n, c // P], axis=2)                      # (cells, 4, 3)
        for j in range(4):
            keep = [k for k in range(4) if k != j]
            f = idx[:, keep, :]
            on = np.zeros(c.shape[0], dtype=bool)
            for a in range(3):
                for side in (0, n - 1):
                    on |= np.all(f[:, :, a] == side, axis=1)
            if on.any():
                out.append(np.sort(c[on][:, keep], axis=1))
    return np.concatenate(out).astype(np.int32)


def timed(ctx, fn, reps=3):
    a = fn()                                     # warm: allocations
    ctx.atom_free(a)
    ts = []
    for _ in range(reps):
        ctx.sync()
        ctx.timer_start()
        a = fn()
        ts.append(ctx.timer_stop())
        if _ < reps - 1:
            ctx.atom_free(a)
    return min(ts), a


def atom_part(n):
    ctx = _lib.Context(0)
    coords, cells = fem.box_mesh_arrays((0, 0, 0), (1, 1, 1), n - 1, n - 1, n - 1)
    t0 = time.perf_counter()
    tri = box_boundary_triangles(cells, n)
    t_host = time.perf_counter() - t0
    mesh = ctx.mesh_upload(coords, cells)
    info = ctx.mesh_info(mesh)
    slots = ctx.mesh_sym_info(mesh)["slots"]
    del coords, cells
    t_k, K = timed(ctx, lambda: ctx.atom_assemble(mesh, fem.STIFF))
    t_r, R = timed(ctx, lambda: ctx.atom_assemble_facets(mesh, tri))
    # the atom's diagonal form is built when it first goes into an operator on this structured grid
    op = ctx.op_combine(mesh, [K, R], [1.0, 2.0])
    form = ctx.atom_product_form(R)
    ctx.atom_free(op)
    out = {"part": "facet_atom", "n": n, "rows": info["nv"], "nnz": info["nnz"], "facets": int(tri.shape[0]),
           "facet_atom_seconds": t_r, "k_assemble_p1_regular_stiffness_seconds": t_k, "facet_list_host_seconds": t_host,
           "atom_csr_bytes": 8 * info["nnz"], "diagonal_form_bytes": 8 * slots * info["nv"], "diagonal_form_slots": slots,
           "atom_product_form_after_combine": form}
    print(json.dumps(out), flush=True)
    for a in (K, R):
        ctx.atom_free(a)
    ctx.mesh_free(mesh)
    ctx.close()


def pass_part(m, n_h=128):
    from pgdrome_amd.hip_backend import HipBackend
    from pgdrome_amd.solver import PGDProblem
    be = fem.set_backend(HipBackend(0))
    t0 = time.perf_counter()
    spec = problems.robin_heat(fem.BoxMesh(fem.Point(0, 0, 0), fem.Point(1, 1, 1), m - 1, m - 1, m - 1), n_h=n_h, PGD_nmax=1,
                               PGD_tol=1e-8)
    t_spec = time.perf_counter() - t0
    p = PGDProblem(**spec)
    k0, st0 = be.ctx.kernel_counts(), dict(fem.STATS)
    be.ctx.sync()
    t1 = time.perf_counter()
    p.solve_PGD(_problem="linear")
    be.ctx.sync()
    t_solve = time.perf_counter() - t1
    k1 = be.ctx.kernel_counts()
    kern = {k: k1[k] - k0[k] for k in k1 if k1[k] != k0[k]}
    out = {"part": "robin_heat_pass", "space": "%d^3" % m, "n_h": n_h, "setup_seconds": t_spec, "solve_seconds": t_solve,
           "fixed_point_iterations": p.num_fp_it, "seconds_per_fixed_point_iteration": t_solve / max(1, sum(p.num_fp_it)),
           "pcg_iterations": fem.STATS["pcg_iterations"] - st0.get("pcg_iterations", 0),
           "linear_solves": fem.STATS["linear_solves"] - st0.get("linear_solves", 0),
           "product_kernels": kern, "product_kernel": max(kern, key=kern.get) if kern else None}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    args = [int(a) for a in sys.argv[1:]]
    atom_part(args[0] if args else 256)
    pass_part(args[1] if len(args) > 1 else 128)
