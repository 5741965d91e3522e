"""Jacobi-PCG against the p-multigrid PCG (PGD_TUNE_PCG_PRECOND = 4, settings["preconditioner"] = "pmg",
pgdrome_amd/csrc/pgd_pmg.hip) on P2 operators over an n^3-VERTEX box ((2 n - 1)^3 P2 nodes), built through the frontend, in one
process on the same operator:

    elastic_block    eps(v) : C(0.3) eps(u) + 2 v . u, clamped at x = 0, body load (0, 0, -1)   - problems.elastic_block, degree 2
    stiffness        grad(v) . grad(u), the hull eliminated, body load 1                         - a scalar P2 space

    python tools/bench_pmg.py [n ...] [--reps R] [--problem NAME] [--out FILE] [--limit SECONDS]      (default sizes 33 65, R = 3)

Every (problem, size) runs in a child process of its own under `timeout` (--limit, default 900 s); the first child that does not
end cleanly ends the run.  One JSON line per problem and size, printed and appended to --out (default
profiles/pmg_bench_n1.jsonl): iterations, ms per solve (median and best of R after one warm-up solve per preconditioner, the two
alternating; operator combine not included), the device time of the setup per solve (eliminated bytes, Galerkin blocks and chains:
part of the solve's ms), levels, and the us of one CSR product of the operator (mean of 20 after 3, synchronised)."""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PROBLEMS = ("elastic_block", "stiffness")


def operator(fem, problems, mesh, name):
    if name == "elastic_block":
        Vh = fem.VectorFunctionSpace(mesh, "P", 2)
        u, v = fem.TrialFunction(Vh), fem.TestFunction(Vh)
        a = (fem.inner(problems._voigt_C(0.3) * problems._strain(u), problems._strain(v)) + fem.Constant(2.0) * fem.inner(u, v)) * fem.dx
        bc = fem.DirichletBC(Vh, fem.Constant((0.0, 0.0, 0.0)), problems._clamped)
        L = fem.dot(fem.Constant((0.0, 0.0, -1.0)), v) * fem.dx
    else:
        Vh = fem.FunctionSpace(mesh, "P", 2)
        u, v = fem.TrialFunction(Vh), fem.TestFunction(Vh)
        a = fem.inner(fem.grad(u), fem.grad(v)) * fem.dx
        bc = fem.DirichletBC(Vh, 0.0, lambda x, on_boundary: on_boundary)
        L = fem.Constant(1.0) * v * fem.dx
    A, b = fem.assemble(a), fem.assemble(L)
    bc.apply(A)
    bc.apply(b)
    return A, b


def one(name, npts, reps):
    from pgdrome_amd import fem, problems
    from pgdrome_amd.hip_backend import HipBackend
    be = fem.set_backend(HipBackend(0))
    ctx = be.ctx
    mesh = fem.BoxMesh(fem.Point(0, 0, 0), fem.Point(1, 1, 1), npts - 1, npts - 1, npts - 1)
    A, b = operator(fem, problems, mesh, name)
    bound = A.lay.bind_p2_lattice(be)
    n, bv = A.lay.n, b.dev()
    precs = (("jacobi", 0), ("pmg", 4))
    times, res = {p: [] for _, p in precs}, {}
    c0 = ctx.pmg_stats()
    for rep in range(reps + 1):                              # (rep 0: warm-up, not timed)
        for pname, prec in precs:
            op = A.op()
            xv = ctx.vec_alloc(n)
            ctx.tune(40, prec)
            ctx.sync()
            t = time.perf_counter()
            it, rel = ctx.pcg_solve(op, bv, xv, 1e-10, 0.0, 50000)
            dt = time.perf_counter() - t                     # (the solve returns synchronised)
            ctx.tune(40, 0)
            ctx.vec_free(xv)
            ctx.atom_free(op)
            if rep > 0:
                times[prec].append(1e3 * dt)
            res[pname] = {"iterations": it, "relres": rel}
    c1 = ctx.pmg_stats()
    for pname, prec in precs:
        t = times[prec]
        res[pname].update(ms_per_solve_median=statistics.median(t), ms_per_solve_best=min(t), ms_per_solve_all=[round(v, 3) for v in t])
        res[pname]["ms_per_iteration"] = statistics.median(t) / max(res[pname]["iterations"], 1)
    ran = c1["solves"] - c0["solves"]
    setup = (c1["setup_ms"] - c0["setup_ms"]) / max(ran, 1)
    res["pmg"].update(pmg_solves=ran, fallbacks=c1["fallbacks"] - c0["fallbacks"], levels=c1["levels"], setup_ms_per_solve=setup,
                      march_passes=c1["march_passes"] - c0["march_passes"])
    res["pmg"]["ms_per_iteration_without_setup"] = (res["pmg"]["ms_per_solve_median"] - setup) / max(res["pmg"]["iterations"], 1)
    # one CSR product of the operator
    op = A.op()
    yv = ctx.vec_alloc(n)
    for _ in range(3):
        ctx.spmv(op, bv, yv)
    ctx.sync()
    t = time.perf_counter()
    for _ in range(20):
        ctx.spmv(op, bv, yv)
    ctx.sync()
    product_us = 1e6 * (time.perf_counter() - t) / 20
    ctx.vec_free(yv)
    ctx.atom_free(op)
    line = {"bench": "pmg", "problem": name, "n_vertices": npts, "rows": n, "bound": bool(bound), "rtol": 1e-10, "reps": reps,
            "csr_product_us": product_us, "nnz": int(ctx.mesh_info(A.lay.handle())["nnz"])}
    line.update({"%s_pcg" % k: v for k, v in res.items()})
    line["speedup"] = res["jacobi"]["ms_per_solve_median"] / res["pmg"]["ms_per_solve_median"]
    print(json.dumps(line), flush=True)


def main():
    argv = sys.argv[1:]

    def opt(flag, default):
        if flag in argv:
            i = argv.index(flag)
            val = argv[i + 1]
            del argv[i:i + 2]
            return val
        return default
    reps, which, limit = int(opt("--reps", 3)), opt("--problem", None), int(opt("--limit", 900))
    out = opt("--out", os.path.join(ROOT, "profiles", "pmg_bench_n1.jsonl"))
    child = opt("--one", None)
    sizes = [int(a) for a in argv] or [33, 65]
    if child is not None:
        return one(child, sizes[0], reps)
    for npts in sizes:
        for name in PROBLEMS:
            if which not in (None, name):
                continue
            cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), str(npts), "--one", name, "--reps", str(reps)]
            run = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
            sys.stdout.write(run.stdout)
            sys.stdout.flush()
            if run.returncode != 0:
                raise SystemExit("bench_pmg: %s at %d^3 vertices ended with status %d; nothing more is started" % (name, npts, run.returncode))
            with open(out, "a") as fh:
                fh.write("".join(l + "\n" for l in run.stdout.splitlines() if l.startswith("{")))


if __name__ == "__main__":
    main()
