"""Jacobi-PCG against the variable-coefficient multigrid PCG (PGD_TUNE_PCG_PRECOND = 2, settings["preconditioner"] = "vmg",
pgdrome_amd/csrc/pgd_vmg.hip) on the spatial operators of three problems on an n^3-node box, in one process on the same operator:

    inclusion_heat   K_out + kappa K_in (kappa = 10 inside the ball), hull eliminated           - problems.inclusion_heat
    robin_heat       K + h R (h = 10 on every face but x = min), the face x = min eliminated    - problems.robin_heat
    weighted         int w grad u . grad v, w = 1 + x + y z, hull eliminated

    python tools/bench_vmg.py [n ...]        (default 128 256)

One JSON line per problem and size: iterations per solve, seconds per solve (best of three, operator combine not included), the
device time of the Galerkin setup per solve (it is part of the solve's seconds) and passes/s = 1 / seconds per solve - the rate a
fixed-point pass would have if the spatial solve were all of it.  Right-hand side 1 on the free nodes, zero start, rtol 1e-10.
Kernel times (a level-0 pass of the cycle against the product): run it under rocprofv3 --kernel-trace --stats."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pgdrome_amd import _lib, fem               # noqa: E402


def boundary_facets(coords, cells, skip_x_min=True):
    """Node triples of the boundary triangles (those in the face x = min left out)."""
    lo, hi = coords.min(axis=0), coords.max(axis=0)
    onb = np.any((coords <= lo) | (coords >= hi), axis=1)
    cand = cells[onb[cells].sum(axis=1) >= 3]
    out = []
    for ax in range(3):
        for val, is_min in ((lo[ax], True), (hi[ax], False)):
            if skip_x_min and ax == 0 and is_min:
                continue
            on = coords[:, ax] == val
            sel = cand[on[cand].sum(axis=1) == 3]
            out.append(np.sort(np.where(on[sel], sel, -1), axis=1)[:, 1:])
    return np.concatenate(out).astype(np.int32)


def problems_on(ctx, h, coords, cells):
    """name -> (atoms, coefficients, Dirichlet dofs); the handles to free afterwards."""
    lo, hi = coords.min(axis=0), coords.max(axis=0)
    hull = np.where(np.any((coords <= lo) | (coords >= hi), axis=1))[0].astype(np.int32)
    c, r = 0.5 * (lo + hi), 0.25 * float((hi - lo).min())
    inside = ((coords - c) ** 2).sum(axis=1) <= r * r * (1.0 + 1e-12)
    mask = inside[cells].all(axis=1).astype(np.uint8)          # (a ball is convex: the midpoint of such a cell is inside too)
    k_out, k_in = ctx.atom_assemble_cells(h, fem.STIFF, 0, 0, 0, 1 - mask), ctx.atom_assemble_cells(h, fem.STIFF, 0, 0, 0, mask)
    k = ctx.atom_assemble(h, fem.STIFF)
    rb = ctx.atom_assemble_facets(h, boundary_facets(coords, cells))
    wv = ctx.vec_from(1.0 + coords[:, 0] + coords[:, 1] * coords[:, 2])
    kw = ctx.atom_assemble(h, fem.WSTIFF, 0, 0, wv)
    face = np.where(coords[:, 0] <= lo[0])[0].astype(np.int32)
    out = {"inclusion_heat": ([k_out, k_in], [1.0, 10.0], hull), "robin_heat": ([k, rb], [1.0, 10.0], face),
           "weighted": ([kw], [1.0], hull)}
    return out, [k_out, k_in, k, rb, kw], [wv]


def main():
    sizes = [int(a) for a in sys.argv[1:]] or [128, 256]
    ctx = _lib.Context(0)
    for npts in sizes:
        coords, cells = fem.box_mesh_arrays((0, 0, 0), (1, 1, 1), npts - 1, npts - 1, npts - 1)
        n = coords.shape[0]
        h = ctx.mesh_upload(coords, cells)
        probs, atoms, vecs = problems_on(ctx, h, coords, cells)
        del cells
        for name, (ats, coefs, bc) in probs.items():
            b = np.ones(n)
            b[bc] = 0.0
            bv = ctx.vec_from(b)
            res = {}
            for prec in (0, 2):
                ctx.tune(40, prec)
                best, st0 = None, ctx.vmg_stats()
                for rep in range(3):
                    op = ctx.op_combine(h, ats, coefs, bc)
                    xv = ctx.vec_alloc(n)
                    ctx.sync()
                    t = time.perf_counter()
                    it, rel = ctx.pcg_solve(op, bv, xv, 1e-10, 0.0, 20000)
                    dt = time.perf_counter() - t
                    best = dt if best is None else min(best, dt)
                    ctx.vec_free(xv)
                    ctx.atom_free(op)
                st1 = ctx.vmg_stats()
                res[prec] = {"iterations": it, "relres": rel, "seconds_per_solve": best, "passes_per_s": 1.0 / best}
                if prec == 2:
                    ran = st1["solves"] - st0["solves"]
                    res[prec].update(vmg_solves=ran, fallbacks=st1["fallbacks"] - st0["fallbacks"], levels=st1["levels"],
                                     galerkin_setup_seconds_per_solve=1e-3 * (st1["setup_ms"] - st0["setup_ms"]) / max(ran, 1))
                    res[prec]["galerkin_setup_share"] = res[prec]["galerkin_setup_seconds_per_solve"] / best
            ctx.tune(40, 0)
            print(json.dumps({"bench": "vmg", "problem": name, "n": npts, "rows": n, "rtol": 1e-10, "jacobi_pcg": res[0], "vmg_pcg": res[2],
                              "speedup": res[0]["seconds_per_solve"] / res[2]["seconds_per_solve"]}), flush=True)
            ctx.vec_free(bv)
        for a in atoms:
            ctx.atom_free(a)
        for v in vecs:
            ctx.vec_free(v)
        ctx.mesh_free(h)
    ctx.close()


if __name__ == "__main__":
    main()
