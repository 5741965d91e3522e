"""Weighted derivative atoms on the MI355X: (1) every new kind (WDUDV, WCONV, WCONVT) on the n^3 P1 BoxMesh against its
unweighted kind and against WSTIFF - the unweighted kinds of a regular lattice take k_assemble_p1_regular, the weighted ones
k_assemble_p1<3> with index steps; (2) the operator build of weighted vector-P1 elasticity E inner(C eps(u), eps(v)) (9 WDUDV
atoms + their embedding into the blocks, then pgd_op_combine, timed apart) on an m^3 box against the unweighted one.

    python tools/bench_weighted.py [n=256] [m=96] [out.jsonl]

Times are HIP-event intervals on the library's stream (pgd_timer_start / pgd_timer_stop), best of `reps` after one warm-up
run.  One JSON line per measurement, also appended to out.jsonl when given."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pgdrome_amd import _lib, fem, problems               # noqa: E402

OUT = []


def emit(rec):
    print(json.dumps(rec), flush=True)
    OUT.append(rec)


def timed_atom(ctx, mesh, kind, da, db, w, reps=5):
    a = ctx.atom_assemble(mesh, kind, da, db, w)                 # warm-up
    ctx.atom_free(a)
    ts = []
    for _ in range(reps):
        ctx.sync()
        ctx.timer_start()
        a = ctx.atom_assemble(mesh, kind, da, db, w)
        ts.append(ctx.timer_stop())
        ctx.atom_free(a)
    return min(ts), float(np.median(ts))


def atom_part(n):
    ctx = _lib.Context(0)
    coords, cells = fem.box_mesh_arrays((0, 0, 0), (1, 1, 1), n - 1, n - 1, n - 1)
    mesh = ctx.mesh_upload(coords, cells)
    w = ctx.vec_from(1.0 + coords[:, 0] + 0.5 * coords[:, 1] * coords[:, 2])
    info = ctx.mesh_info(mesh)
    del coords, cells
    cases = [("WSTIFF", fem.WSTIFF, 0, 0, w), ("DUDV", fem.DUDV, 0, 1, 0), ("WDUDV", fem.WDUDV, 0, 1, w),
             ("CONV", fem.CONV, 0, 0, 0), ("WCONV", fem.WCONV, 0, 0, w), ("CONVT", fem.CONVT, 0, 0, 0),
             ("WCONVT", fem.WCONVT, 0, 0, w)]
    res = {}
    for name, kind, da, db, wv in cases:
        best, med = timed_atom(ctx, mesh, kind, da, db, wv)
        res[name] = best
        emit({"part": "atom", "n": n, "rows": info["nv"], "nnz": info["nnz"], "kind": name, "da": da, "db": db,
              "kernel": "k_assemble_p1<3>" if wv else "k_assemble_p1_regular", "best_seconds": best, "median_seconds": med})
    emit({"part": "atom_ratios", "n": n, **{"%s_over_%s" % (a, b): res[a] / res[b] for a, b in
                                           (("WDUDV", "DUDV"), ("WCONV", "CONV"), ("WCONVT", "CONVT"),
                                            ("WDUDV", "WSTIFF"), ("WCONV", "WSTIFF"), ("WCONVT", "WSTIFF"))}})
    ctx.vec_free(w)
    ctx.mesh_free(mesh)
    ctx.close()


def elasticity_part(m, reps=3):
    from pgdrome_amd.hip_backend import HipBackend
    be = fem.set_backend(HipBackend(0))
    C = problems._voigt_C(0.3)

    def build(weighted):
        mesh = fem.BoxMesh(fem.Point(0, 0, 0), fem.Point(1, 1, 1), m - 1, m - 1, m - 1)
        V = fem.VectorFunctionSpace(mesh, "CG", 1)
        u, v = fem.TrialFunction(V), fem.TestFunction(V)
        energy = fem.inner(C * problems._strain(u), problems._strain(v))
        if weighted:
            E = fem.interpolate(fem.Expression("1 + x[0] + 0.5*x[1]*x[2]", degree=1), fem.FunctionSpace(mesh, "CG", 1))
            energy = E * energy
            E.vector().dev()                                   # the weight is on the device before the clock starts
        form = energy * fem.dx
        A = fem.assemble(form)
        V._lay.handle()
        be.ctx.sync()
        be.ctx.timer_start()
        handles, coefs = A.merged()                            # the scalar atoms and their embedding into the blocks
        t_atoms = be.ctx.timer_stop()
        be.ctx.timer_start()
        op = be.combine(V._lay.handle(), handles, coefs, A.bc_vertices, 0)
        t_combine = be.ctx.timer_stop()
        be.atom_free(op)
        nref = len(A.refs)
        del A, V, mesh
        fem.clear_caches()
        return t_atoms, t_combine, nref

    for weighted in (False, True):
        build(weighted)                                        # warm-up
        ts = [build(weighted) for _ in range(reps)]
        emit({"part": "vector_elasticity_operator_build", "space": "%d^3" % m, "dofs": 3 * m ** 3, "weighted": weighted,
              "block_terms": ts[0][2], "scalar_atoms": 9,
              "atoms_and_embedding_best_seconds": min(t[0] for t in ts), "combine_best_seconds": min(t[1] for t in ts),
              "total_best_seconds": min(t[0] + t[1] for t in ts)})


if __name__ == "__main__":
    args = sys.argv[1:]
    n = int(args[0]) if args else 256
    m = int(args[1]) if len(args) > 1 else 96
    atom_part(n)
    elasticity_part(m)
    if len(args) > 2:
        with open(args[2], "a") as f:
            for rec in OUT:
                f.write(json.dumps(rec) + "\n")
