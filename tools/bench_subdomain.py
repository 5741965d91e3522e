"""Cell-subdomain integrals dx(id) on the MI355X: (1) a masked stiffness atom (pgd_atom_assemble_cells) on the n^3 BoxMesh with a
seeded random half of the cells marked, against the unmasked atom (k_assemble_p1_regular) in the same run, and the upload of a
mask's bytes timed on its own; (2) inclusion_heat on an m^3 box x 128
values of kappa: setup, the fixed-point iterations of its first enrichment, PCG iterations, the product kernels and the product
form of its space operator; (3) the host time of a repeated dx(id) lookup with unchanged markers at each of the sizes given.

    python tools/bench_subdomain.py [n=256] [m=128]

One JSON line per part.  Which kernel ran is not visible here: run the atom part under rocprofv3 --kernel-trace --stats."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pgdrome_amd import _lib, fem, problems               # noqa: E402


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
    nc = cells.shape[0]
    mask = np.zeros(nc, dtype=np.uint8)
    mask[np.random.default_rng(0).permutation(nc)[:nc // 2]] = 1
    mesh = ctx.mesh_upload(coords, cells)
    info = ctx.mesh_info(mesh)
    del coords, cells
    t_k, K = timed(ctx, lambda: ctx.atom_assemble(mesh, fem.STIFF))
    t_m, Km = timed(ctx, lambda: ctx.atom_assemble_cells(mesh, fem.STIFF, 0, 0, 0, mask))
    # the mask upload on its own: a vector of nc / 8 doubles carries the same bytes through the same host-to-device copy
    buf = ctx.vec_alloc(max(1, nc // 8))
    host = np.zeros(max(1, nc // 8))
    ts = []
    for _ in range(3):
        ctx.sync()
        t0 = time.perf_counter()
        ctx.vec_upload(buf, host)
        ctx.sync()
        ts.append(time.perf_counter() - t0)
    ctx.vec_free(buf)
    out = {"part": "masked_atom", "n": n, "rows": info["nv"], "cells": nc, "marked_cells": int(mask.sum()), "nnz": info["nnz"],
           "masked_stiffness_seconds": t_m, "unmasked_stiffness_seconds": t_k, "mask_upload_seconds": min(ts),
           "mask_bytes": nc, "atom_csr_bytes": 8 * info["nnz"]}
    print(json.dumps(out), flush=True)
    for a in (K, Km):
        ctx.atom_free(a)
    ctx.mesh_free(mesh)
    ctx.close()


def pass_part(m, n_k=128):
    from pgdrome_amd.hip_backend import HipBackend
    from pgdrome_amd.solver import PGDProblem
    be = fem.set_backend(HipBackend(0))
    t0 = time.perf_counter()
    spec = problems.inclusion_heat(fem.BoxMesh(fem.Point(0, 0, 0), fem.Point(1, 1, 1), m - 1, m - 1, m - 1), n_k=n_k, PGD_nmax=1,
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
    # the product form of a space operator of the problem: K_out + kappa K_in with the boundary rows eliminated
    V = spec["Vs"][0]
    u, v = fem.TrialFunction(V), fem.TestFunction(V)
    dxs = fem.Measure("dx", domain=V.mesh(), subdomain_data=spec["param"]["markers"])
    A = fem.assemble(fem.inner(fem.grad(u), fem.grad(v)) * dxs(problems.OUTSIDE)
                     + 3.0 * fem.inner(fem.grad(u), fem.grad(v)) * dxs(problems.INCLUSION))
    spec["bc_fct"](spec["Vs"], None, spec["param"])[0].apply(A)
    op = A.op()
    x, y = fem.Vector(V, np.ones(V.dim())), fem.Vector(V)
    be.spmv(op, x.dev(), y.dev_for_write())
    form = be.ctx.atom_product_form(op)
    be.atom_free(op)
    out = {"part": "inclusion_heat_pass", "space": "%d^3" % m, "n_kappa": n_k, "setup_seconds": t_spec, "solve_seconds": t_solve,
           "fixed_point_iterations": p.num_fp_it, "seconds_per_fixed_point_iteration": t_solve / max(1, sum(p.num_fp_it)),
           "pcg_iterations": fem.STATS["pcg_iterations"] - st0.get("pcg_iterations", 0),
           "linear_solves": fem.STATS["linear_solves"] - st0.get("linear_solves", 0),
           "product_kernels": kern, "product_kernel": max(kern, key=kern.get) if kern else None,
           "space_operator_product_form": form}
    print(json.dumps(out), flush=True)


def lookup_part(m, reps=5):
    """Host time of dx(id) with unchanged markers: the comparison against the snapshot, nothing assembled or uploaded."""
    mesh = fem.BoxMesh(fem.Point(0, 0, 0), fem.Point(1, 1, 1), m - 1, m - 1, m - 1)
    cf = fem.MeshFunction("size_t", mesh, 3, 1)
    cf.array()[::2] = 2
    fem._CellSet(cf, 1)                           # first sight: the snapshot
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fem._CellSet(cf, 1)
        ts.append(time.perf_counter() - t0)
    print(json.dumps({"part": "dx_id_lookup", "space": "%d^3" % m, "cells": mesh.num_cells(), "marker_bytes": cf.array().nbytes,
                      "best_seconds": min(ts), "median_seconds": float(np.median(ts))}), flush=True)


if __name__ == "__main__":
    args = [int(a) for a in sys.argv[1:]]
    n, m = (args[0] if args else 256), (args[1] if len(args) > 1 else 128)
    atom_part(n)
    pass_part(m)
    for size in sorted({m, n}):
        lookup_part(size)
