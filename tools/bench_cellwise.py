"""Cell-wise constant (DG0) coefficients on the MI355X, on the n^3 BoxMesh for every n given: (1) a cell-weighted stiffness atom
(pgd_atom_assemble_cellwise) through the regular-lattice instance and through the general kernel (PGD_TUNE_ASM_LATTICE = 3), with
the unmasked atom, one masked atom and the nodal WSTIFF atom beside them, and the upload of the field; (2) an 8-material
operator built as 8 dx(id) atoms against one cell-weighted atom: seconds and bytes of HBM held by the atoms; (3) one "vmg" and
one Jacobi-PCG solve of K[kappa], kappa a seeded random 8-level field in {0.5 ... 64}, one face eliminated.

    python tools/bench_cellwise.py [n=128 256 ...] > profiles/cellwise_bench_n1.jsonl

One JSON line per part and size.  Which kernel ran is not visible here: run under rocprofv3 --kernel-trace --stats.

    PGD_BENCH_PACKAGE_ROOT=<built checkout of another commit> python tools/bench_cellwise.py --baseline [n ...]

times the nodal WSTIFF atom and the unweighted atom alone, through entry points every commit since the weighted atoms has, with
the package of that checkout: the figures of the parent commit in profiles/cellwise_parent_atoms.jsonl were taken this way, in the
same session as the main run."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.environ.get("PGD_BENCH_PACKAGE_ROOT") or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pgdrome_amd import _lib, fem               # noqa: E402


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


def wall(ctx, fn, reps=3):
    ts, out = [], None
    for _ in range(reps):
        ctx.sync()
        t0 = time.perf_counter()
        out = fn()
        ctx.sync()
        ts.append(time.perf_counter() - t0)
    return min(ts), out


def run(n):
    ctx = _lib.Context(0)
    coords, cells = fem.box_mesh_arrays((0, 0, 0), (1, 1, 1), n - 1, n - 1, n - 1)
    nc, nv = cells.shape[0], coords.shape[0]
    rng = np.random.default_rng(0)
    level = rng.integers(0, 8, nc)
    kappa = 2.0 ** (level - 1.0)
    mask = (level < 4).astype(np.uint8)
    w = 1.0 + coords[:, 0] + coords[:, 1] * coords[:, 2]
    face = np.where(coords[:, 0] <= 0.0)[0].astype(np.int32)
    mesh = ctx.mesh_upload(coords, cells)
    info = ctx.mesh_info(mesh)
    del coords, cells
    wv = ctx.vec_from(w)
    cv = ctx.vec_alloc(nc)
    t_up, _ = wall(ctx, lambda: ctx.vec_upload(cv, kappa))

    # (1) the atoms
    t_plain, a = timed(ctx, lambda: ctx.atom_assemble(mesh, fem.STIFF))
    ctx.atom_free(a)
    t_mask, a = timed(ctx, lambda: ctx.atom_assemble_cells(mesh, fem.STIFF, 0, 0, 0, mask))
    ctx.atom_free(a)
    t_ws, a = timed(ctx, lambda: ctx.atom_assemble(mesh, fem.WSTIFF, 0, 0, wv))
    ctx.atom_free(a)
    t_cw, K = timed(ctx, lambda: ctx.atom_assemble_cellwise(mesh, fem.STIFF, 0, 0, 0, cv, None, nc))
    ctx.tune(20, 3)
    t_cw_gen, a = timed(ctx, lambda: ctx.atom_assemble_cellwise(mesh, fem.STIFF, 0, 0, 0, cv, None, nc))
    ctx.atom_free(a)
    ctx.tune(20, 1)
    print(json.dumps({"part": "cellwise_atom", "n": n, "rows": nv, "cells": nc, "nnz": info["nnz"],
                      "cellwise_stiffness_regular_seconds": t_cw, "cellwise_stiffness_general_seconds": t_cw_gen,
                      "unmasked_stiffness_seconds": t_plain, "masked_stiffness_seconds": t_mask, "nodal_wstiff_seconds": t_ws,
                      "field_upload_seconds": t_up, "field_bytes": 8 * nc, "atom_csr_bytes": 8 * info["nnz"],
                      "regular_bytes_read": 8 * nc + 4 * nv, "regular_bytes_written": 8 * info["nnz"]}), flush=True)

    # (2) eight materials: 8 dx(id) atoms and their combination against one cell-weighted atom.  Both sides start from host
    # arrays that exist before the clock runs (the eight masks; the field) and pay for their upload, assembly and combination;
    # each is built twice and the faster build counts (the first pays for fresh device allocations).
    masks = [(level == l).astype(np.uint8) for l in range(8)]

    def by_masks():
        atoms = [ctx.atom_assemble_cells(mesh, fem.STIFF, 0, 0, 0, masks[l]) for l in range(8)]
        op = ctx.op_combine(mesh, atoms, [2.0 ** (l - 1.0) for l in range(8)], face)
        return atoms, op

    def by_field():
        ctx.vec_upload(cv, kappa)
        atom = ctx.atom_assemble_cellwise(mesh, fem.STIFF, 0, 0, 0, cv, None, nc)
        return [atom], ctx.op_combine(mesh, [atom], [1.0], face)
    res = {}
    for name, build in (("dx_id", by_masks), ("cellwise", by_field)):
        ts = []
        for _ in range(2):
            ctx.sync()
            t0 = time.perf_counter()
            atoms, op = build()
            ctx.sync()
            ts.append(time.perf_counter() - t0)
            for a in atoms + [op]:
                ctx.atom_free(a)
        res[name + "_seconds"], res[name + "_first_build_seconds"] = min(ts), ts[0]
        res[name + "_atoms"] = len(atoms)
        res[name + "_atom_bytes"] = 8 * info["nnz"] * len(atoms)
    del masks
    print(json.dumps(dict({"part": "eight_materials", "n": n, "field_bytes": 8 * nc, "mask_bytes_each": nc}, **res)), flush=True)

    # (3) the solves
    b = np.random.default_rng(11).uniform(-1, 1, nv)
    bv = ctx.vec_from(b)
    out = {"part": "solves", "n": n, "rtol": 1e-8, "dirichlet": "face x = 0", "levels": "2^(l-1), l = 0 ... 7"}
    for name, prec in (("vmg", 2), ("jacobi", 0)):
        ctx.tune(40, prec)
        v0 = ctx.vmg_stats()
        op = ctx.op_combine(mesh, [K], [1.0], face)
        xv = ctx.vec_alloc(nv)
        ctx.sync()
        t0 = time.perf_counter()
        it, rel = ctx.pcg_solve(op, bv, xv, 1e-8, 0.0, 20000)
        ctx.sync()
        out[name + "_seconds"] = time.perf_counter() - t0
        out[name + "_iterations"], out[name + "_relres"] = int(it), float(rel)
        v1 = ctx.vmg_stats()
        out[name + "_vcycle_solves"] = v1["solves"] - v0["solves"]
        if prec == 2:
            out["vmg_setup_ms"] = v1["setup_ms"] - v0["setup_ms"]
        ctx.vec_free(xv)
        ctx.atom_free(op)
    ctx.tune(40, 0)
    print(json.dumps(out), flush=True)
    ctx.atom_free(K)
    for v in (wv, cv, bv):
        ctx.vec_free(v)
    ctx.mesh_free(mesh)
    ctx.close()


def baseline(n):
    """The nodal WSTIFF atom and the unweighted atom alone, with the same mesh, weight and timing loop as run()."""
    ctx = _lib.Context(0)
    coords, cells = fem.box_mesh_arrays((0, 0, 0), (1, 1, 1), n - 1, n - 1, n - 1)
    w = 1.0 + coords[:, 0] + coords[:, 1] * coords[:, 2]
    mesh = ctx.mesh_upload(coords, cells)
    del coords, cells
    wv = ctx.vec_from(w)
    t_ws, a = timed(ctx, lambda: ctx.atom_assemble(mesh, fem.WSTIFF, 0, 0, wv))
    ctx.atom_free(a)
    t_plain, a = timed(ctx, lambda: ctx.atom_assemble(mesh, fem.STIFF))
    ctx.atom_free(a)
    print(json.dumps({"part": "baseline_atoms", "n": n, "nodal_wstiff_seconds": t_ws, "unmasked_stiffness_seconds": t_plain}),
          flush=True)
    ctx.vec_free(wv)
    ctx.mesh_free(mesh)
    ctx.close()


if __name__ == "__main__":
    args = sys.argv[1:]
    part = baseline if "--baseline" in args else run
    for size in [int(a) for a in args if a != "--baseline"] or [128, 256]:
        part(size)
