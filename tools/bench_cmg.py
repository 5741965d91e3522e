"""Jacobi-PCG against the component-wise multigrid PCG (PGD_TUNE_PCG_PRECOND = 3, settings["preconditioner"] = "cmg",
pgdrome_amd/csrc/pgd_vmg.hip) on the spatial operators of the two vector-valued problems on an n^3-node box, built through the
frontend, in one process on the same operator:

    elastic_block    eps(v) : C(0.3) eps(u) + 2 v . u, clamped at x = 0                          - problems.elastic_block
    graded_block     (1 + g) eps(v) : C(0.3) eps(u) + 2 v . u, g = x + 4 y z (theta = 1), clamped - problems.graded_block

    python tools/bench_cmg.py [n ...] [--reps R] [--only jacobi|cmg] [--problem NAME]      (default sizes 65 129, R = 3)

One JSON line per problem and size: iterations, ms per solve (median and best of R after one warm-up solve per preconditioner, the
two preconditioners alternating; operator combine not included), the device time of the hierarchy setup per solve (part of the
solve's ms), ms per iteration.  Right-hand side: the body load g = (0, 0, -1), zero start, rtol 1e-10.

The split of an iteration into product / cycle / vector work comes from a separate run under the profiler:

    rocprofv3 --kernel-trace --output-format csv -d <dir> -- python tools/bench_cmg.py 129 --reps 1 --only cmg --problem elastic_block
    python tools/bench_cmg.py --stages <dir>

which sums the trace's kernel times by stage and prints one JSON line (ms and share per stage)."""
import csv
import glob
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

STAGES = (("product", ("k_spmv",)), ("cycle", ("k_vmg_march", "k_vmg_pass", "k_vmg_wmul", "k_vmg_restrict", "k_vmg_prolong", "k_vmg_bottom",
                                               "k_cmg_split", "k_cmg_merge")),
          ("setup", ("k_cmg_extract", "k_vmg_rowsum", "k_vmg_galerkin", "k_cmg_fix_start", "k_diag_inv")),
          ("vector", ("k_pcg_", "k_reduce_")))


def stages(path):
    files = glob.glob(path + "/**/*kernel_trace.csv", recursive=True)
    if not files:
        raise SystemExit("no *_kernel_trace.csv under %s" % path)
    ms, calls, per_kernel = {}, {}, {}
    for f in files:
        with open(f) as fh:
            for row in csv.DictReader(fh):
                name = row["Kernel_Name"]
                d = (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e6
                stage = next((s for s, keys in STAGES if any(k in name for k in keys)), "other")
                ms[stage] = ms.get(stage, 0.0) + d
                calls[stage] = calls.get(stage, 0) + 1
                short = name.split("(")[0].replace("void ", "").replace("pgd::", "")
                per_kernel[short] = per_kernel.get(short, 0.0) + d
    total = sum(ms.values())
    top = sorted(per_kernel.items(), key=lambda kv: -kv[1])[:12]
    print(json.dumps({"bench": "cmg_stages", "kernel_ms_total": total,
                      "stages": {s: {"ms": ms[s], "share": ms[s] / total, "dispatches": calls[s]} for s in ms},
                      "top_kernels_ms": {k: round(v, 3) for k, v in top}}))


def operator(fem, problems, Vh, name):
    u, v = fem.TrialFunction(Vh), fem.TestFunction(Vh)
    energy = fem.inner(problems._voigt_C(0.3) * problems._strain(u), problems._strain(v))
    a = energy * fem.dx + fem.Constant(2.0) * fem.inner(u, v) * fem.dx
    if name == "graded_block":
        g = fem.interpolate(fem.Expression("x[0] + 4*x[1]*x[2]", degree=1), fem.FunctionSpace(Vh.mesh(), "P", 1))
        a = a + g * energy * fem.dx
    A = fem.assemble(a)
    bc = fem.DirichletBC(Vh, fem.Constant((0.0, 0.0, 0.0)), problems._clamped)
    bc.apply(A)
    b = fem.assemble(fem.dot(fem.Constant((0.0, 0.0, -1.0)), v) * fem.dx)
    bc.apply(b)
    return A, b


def main():
    argv = sys.argv[1:]
    if "--stages" in argv:
        return stages(argv[argv.index("--stages") + 1])

    def opt(flag, default):
        if flag in argv:
            i = argv.index(flag)
            val = argv[i + 1]
            del argv[i:i + 2]
            return val
        return default
    reps, only, which = int(opt("--reps", 3)), opt("--only", None), opt("--problem", None)
    sizes = [int(a) for a in argv] or [65, 129]
    from pgdrome_amd import fem, problems
    from pgdrome_amd.hip_backend import HipBackend
    be = fem.set_backend(HipBackend(0))
    ctx = be.ctx
    precs = [(n, p) for n, p in (("jacobi", 0), ("cmg", 3)) if only in (None, n)]
    for npts in sizes:
        fem.clear_caches()
        mesh = fem.BoxMesh(fem.Point(0, 0, 0), fem.Point(1, 1, 1), npts - 1, npts - 1, npts - 1)
        Vh = fem.VectorFunctionSpace(mesh, "P", 1)
        for name in ("elastic_block", "graded_block"):
            if which not in (None, name):
                continue
            A, b = operator(fem, problems, Vh, name)
            n, bv = A.lay.n, b.dev()
            times = {p: [] for _, p in precs}
            res = {}
            c0 = ctx.cmg_stats()
            for rep in range(reps + 1):                      # (rep 0: warm-up, not timed)
                for pname, prec in precs:
                    op = A.op()
                    xv = ctx.vec_alloc(n)
                    ctx.tune(40, prec)
                    ctx.sync()
                    t = time.perf_counter()
                    it, rel = ctx.pcg_solve(op, bv, xv, 1e-10, 0.0, 50000)
                    dt = time.perf_counter() - t             # (the solve returns synchronised)
                    ctx.tune(40, 0)
                    ctx.vec_free(xv)
                    ctx.atom_free(op)
                    if rep > 0:
                        times[prec].append(1e3 * dt)
                    res[pname] = {"iterations": it, "relres": rel}
            c1 = ctx.cmg_stats()
            for pname, prec in precs:
                t = times[prec]
                res[pname].update(ms_per_solve_median=statistics.median(t), ms_per_solve_best=min(t), ms_per_solve_all=[round(v, 3) for v in t])
                res[pname]["ms_per_iteration"] = statistics.median(t) / max(res[pname]["iterations"], 1)
            line = {"bench": "cmg", "problem": name, "n": npts, "rows": n, "rtol": 1e-10, "reps": reps}
            if "cmg" in res:
                ran = c1["solves"] - c0["solves"]
                setup = (c1["setup_ms"] - c0["setup_ms"]) / max(ran, 1)
                res["cmg"].update(cmg_solves=ran, fallbacks=c1["fallbacks"] - c0["fallbacks"], levels=c1["levels"], setup_ms_per_solve=setup,
                                  march_passes=c1["march_passes"] - c0["march_passes"])
                res["cmg"]["ms_per_iteration_without_setup"] = (res["cmg"]["ms_per_solve_median"] - setup) / max(res["cmg"]["iterations"], 1)
            line.update({"%s_pcg" % k: v for k, v in res.items()})
            if len(res) == 2:
                line["speedup"] = res["jacobi"]["ms_per_solve_median"] / res["cmg"]["ms_per_solve_median"]
            print(json.dumps(line), flush=True)
            del A, b
    ctx.tune(40, 0)


if __name__ == "__main__":
    main()
