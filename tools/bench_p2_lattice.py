"""The CSR product against the row-class product (PGD_TUNE_SPMV_P2_LATTICE = 59, settings["p2_product"] = "lattice",
pgdrome_amd/csrc/pgd_p2lat.hip) on P2 operators over an n^3-VERTEX box ((2 n - 1)^3 P2 nodes), built through the frontend, both
products alternating in one process on the same operator (the operators of tools/bench_pmg.py):

    elastic_block    eps(v) : C(0.3) eps(u) + 2 v . u, clamped at x = 0, body load (0, 0, -1)   - problems.elastic_block, degree 2
    stiffness        grad(v) . grad(u), the hull eliminated, body load 1                         - a scalar P2 space

    python tools/bench_p2_lattice.py [n ...] [--reps R] [--jacobi-reps J] [--products K] [--problem NAME] [--out FILE] [--limit SECONDS]
                                                                                              (default sizes 33 65, R = 3, K = 20)

Every (problem, size) runs in a child process of its own under `timeout`; the first child that does not end cleanly ends the run.
--limit defaults to 240 s below 65 vertices per axis and to 480 s from there on: one Jacobi solve of elastic_block on the CSR
product takes 91.5 s at 65^3 (README), the child runs one per product there, and the rest - assembly, the products, the "pmg"
solves - stays below two minutes.  One JSON line per problem and size, printed and appended to --out (default
profiles/p2_lattice_bench_n1.jsonl):
  * us per product: K launches of pgd_spmv (y = A x) and of pgd_spmv_dot_slot (the PCG instance: y = A x with x . y) between two HIP
    events, median and all of R rounds after a warm-up round per product, knob 0 and knob 1 alternating; whether the slowest round
    of the form is faster than the fastest round of the CSR product (the gain exceeds the spread);
  * the bytes a product must move, from the shapes - CSR: 12 nnz + 20 rows; the form: 8 per slot of its arrays + 16 rows - and the
    TB/s that makes;
  * ms per solve and iterations under "pmg" (PGD_TUNE_PCG_PRECOND = 4) and under the Jacobi-PCG, rtol 1e-10, zero start, operator
    combine not included, the form's extraction included: median of R (Jacobi: J, default R below 65 vertices per axis and 1 from
    there on) after one warm-up solve per product under "pmg"; whether iterations and solutions of the two products are equal;
  * the share of a "pmg" iteration (setup and extraction taken off) that one product is, for both products;
  * the extraction's device time per form (pgd_p2lat_times) and the form's bytes against the CSR value array's.
The reference of every time is the CSR product (knob 0) in the same run."""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_pmg import PROBLEMS, operator      # noqa: E402  (the same two operators)

KNOB = 59
PRODUCTS = (("csr", 0), ("p2_lattice", 1))


def one(name, npts, reps, jreps, nprod):
    import numpy as np
    from pgdrome_amd import fem, problems
    from pgdrome_amd.hip_backend import HipBackend
    be = fem.set_backend(HipBackend(0))
    ctx = be.ctx
    mesh = fem.BoxMesh(fem.Point(0, 0, 0), fem.Point(1, 1, 1), npts - 1, npts - 1, npts - 1)
    A, b = operator(fem, problems, mesh, name)
    bound = A.lay.bind_p2_lattice(be)
    n, bv = A.lay.n, b.dev()
    nc = getattr(A.lay, "ncomp", 1)
    nnz = int(ctx.mesh_info(A.lay.handle())["nnz"])
    nvr = nc * npts ** 3
    pad = lambda rows: (rows + 63) // 64 * 64
    form_bytes = 8 * nc * (65 * pad(nvr) + 27 * pad(n - nvr))
    moved = {"csr": 12 * nnz + 20 * n, "p2_lattice": 8 * nc * (65 * nvr + 27 * (n - nvr)) + 16 * n}
    s0 = ctx.p2lat_stats()
    line = {"bench": "p2_lattice", "problem": name, "n_vertices": npts, "rows": n, "nnz": nnz, "bound": bool(bound), "rtol": 1e-10,
            "reps": reps, "jacobi_reps": jreps, "products_per_round": nprod}
    # ---- the product alone
    op = A.op()
    xv, yv = ctx.vec_from(np.random.default_rng(1).uniform(-1, 1, n)), ctx.vec_alloc(n)
    us = {(p, kind): [] for p, _ in PRODUCTS for kind in ("store", "dot_store")}
    for rnd in range(reps + 1):                      # (round 0: warm-up - it holds the extraction - not timed)
        for pname, knob in PRODUCTS:
            ctx.tune(KNOB, knob)
            for kind in ("store", "dot_store"):
                ctx.flags_reset()
                ctx.sync()
                ctx.timer_start()
                for _ in range(nprod):
                    if kind == "store":
                        ctx.spmv(op, xv, yv)
                    else:
                        ctx.spmv_dot_slot(op, xv, yv, xv, 0, -1, 60)
                dt = ctx.timer_stop()
                if rnd > 0:
                    us[(pname, kind)].append(1e6 * dt / nprod)
    ctx.tune(KNOB, 0)
    for v in (xv, yv):
        ctx.vec_free(v)
    ctx.atom_free(op)
    for pname, _ in PRODUCTS:
        d = {"us_%s_median" % kind: statistics.median(us[(pname, kind)]) for kind in ("store", "dot_store")}
        d.update({"us_%s_all" % kind: [round(v, 1) for v in us[(pname, kind)]] for kind in ("store", "dot_store")})
        d["bytes_moved"] = moved[pname]
        d["tb_per_s"] = moved[pname] / d["us_store_median"] * 1e-6
        line["%s_product" % pname] = d
    line["product_speedup"] = {kind: line["csr_product"]["us_%s_median" % kind] / line["p2_lattice_product"]["us_%s_median" % kind]
                               for kind in ("store", "dot_store")}
    line["gain_exceeds_spread"] = {kind: max(us[("p2_lattice", kind)]) < min(us[("csr", kind)]) for kind in ("store", "dot_store")}
    print("products done", file=sys.stderr, flush=True)
    # ---- whole solves
    for prec_name, prec, nrep in (("pmg", 4, reps), ("jacobi", 0, jreps)):
        times = {p: [] for p, _ in PRODUCTS}
        res, sol = {}, {}
        c0, e0 = ctx.pmg_stats(), ctx.p2lat_stats()
        for rep in range(nrep + (1 if prec == 4 else 0)):      # (under "pmg" rep 0 is the warm-up of both products' kernels)
            for pname, knob in PRODUCTS:
                op = A.op()
                xv = ctx.vec_alloc(n)
                ctx.tune(40, prec)
                ctx.tune(KNOB, knob)
                ctx.sync()
                t = time.perf_counter()
                it, rel = ctx.pcg_solve(op, bv, xv, 1e-10, 0.0, 50000)
                dt = time.perf_counter() - t             # (the solve returns synchronised)
                ctx.tune(40, 0)
                ctx.tune(KNOB, 0)
                sol[pname] = ctx.vec_download(xv)
                ctx.vec_free(xv)
                ctx.atom_free(op)
                if prec != 4 or rep > 0:
                    times[pname].append(1e3 * dt)
                res[pname] = {"iterations": it, "relres": rel}
                print("%s solve on %s: %d iterations, %.1f ms" % (prec_name, pname, it, 1e3 * dt), file=sys.stderr, flush=True)
        c1, e1 = ctx.pmg_stats(), ctx.p2lat_stats()
        for pname, _ in PRODUCTS:
            t = times[pname]
            res[pname].update(ms_per_solve_median=statistics.median(t), ms_per_solve_all=[round(v, 3) for v in t],
                              ms_per_iteration=statistics.median(t) / max(res[pname]["iterations"], 1))
        if prec == 4:
            setup = (c1["setup_ms"] - c0["setup_ms"]) / max(c1["solves"] - c0["solves"], 1)
            extract = (e1["extract_ms"] - e0["extract_ms"]) / max(e1["forms_built"] - e0["forms_built"], 1)
            for pname, _ in PRODUCTS:
                rest = res[pname]["ms_per_solve_median"] - setup - (extract if pname == "p2_lattice" else 0.0)
                per_it = rest / max(res[pname]["iterations"], 1)
                res[pname].update(pmg_solves=c1["solves"] - c0["solves"], setup_ms_per_solve=setup, ms_per_iteration_without_setup=per_it,
                                  product_share_of_iteration=1e-3 * line["%s_product" % pname]["us_dot_store_median"] / per_it)
        line["%s_pcg" % prec_name] = dict(res, solve_speedup=res["csr"]["ms_per_solve_median"] / res["p2_lattice"]["ms_per_solve_median"],
                                          same_iterations=res["csr"]["iterations"] == res["p2_lattice"]["iterations"],
                                          same_solution_bits=bool(np.array_equal(sol["csr"], sol["p2_lattice"])))
    s1 = ctx.p2lat_stats()
    forms = s1["forms_built"] - s0["forms_built"]
    line["forms_built"], line["fallbacks"] = forms, s1["fallbacks"] - s0["fallbacks"]
    line["extract_ms_per_form"] = (s1["extract_ms"] - s0["extract_ms"]) / max(forms, 1)
    line["form_bytes"], line["csr_value_bytes"], line["csr_column_bytes"] = form_bytes, 8 * nnz, 4 * nnz
    line["form_over_csr_values"] = form_bytes / (8 * nnz)
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
    reps, jreps, nprod, which = int(opt("--reps", 3)), opt("--jacobi-reps", None), int(opt("--products", 20)), opt("--problem", None)
    limit = opt("--limit", None)
    out = opt("--out", os.path.join(ROOT, "profiles", "p2_lattice_bench_n1.jsonl"))
    child = opt("--one", None)
    sizes = [int(a) for a in argv] or [33, 65]
    if child is not None:
        return one(child, sizes[0], reps, int(jreps), nprod)
    for npts in sizes:
        jr = int(jreps) if jreps is not None else (reps if npts < 65 else 1)
        lim = int(limit) if limit is not None else (240 if npts < 65 else 480)
        for name in PROBLEMS:
            if which not in (None, name):
                continue
            cmd = ["timeout", "-k", "10", str(lim), sys.executable, os.path.abspath(__file__), str(npts), "--one", name,
                   "--reps", str(reps), "--jacobi-reps", str(jr), "--products", str(nprod)]
            run = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
            sys.stdout.write(run.stdout)
            sys.stdout.flush()
            if run.returncode != 0:
                raise SystemExit("bench_p2_lattice: %s at %d^3 vertices ended with status %d; nothing more is started" % (name, npts, run.returncode))
            with open(out, "a") as fh:
                fh.write("".join(l + "\n" for l in run.stdout.splitlines() if l.startswith("{")))


if __name__ == "__main__":
    main()
