"""The CSR product against the row-diagonal product (PGD_TUNE_SPMV_BLOCK_DIA = 58, settings["block_product"] = "diagonal",
pgdrome_amd/csrc/pgd_bdia.hip) on the spatial operators of the two vector-valued problems on an n^3-node box, built through the
frontend, both products alternating in one process on the same operator:

    elastic_block    eps(v) : C(0.3) eps(u) + 2 v . u, clamped at x = 0                          - problems.elastic_block
    graded_block     (1 + g) eps(v) : C(0.3) eps(u) + 2 v . u, g = x + 4 y z (theta = 1), clamped - problems.graded_block

    python tools/bench_block_dia.py [n ...] [--reps R] [--jacobi-reps J] [--products K] [--problem NAME]   (default sizes 65 129, R = 3, K = 20)

One JSON line per problem and size:
  * us per product: K launches of pgd_spmv (y = A x) and of pgd_spmv_dot_slot (the PCG instance: y = A x with x . y) between two HIP
    events, median of R rounds after a warm-up round, knob 0 and knob 1 alternating;
  * ms per solve and iterations under the Jacobi-PCG and under "cmg" (PGD_TUNE_PCG_PRECOND = 3), rtol 1e-10, body load, zero start,
    operator combine not included, the form's extraction included: median of R (Jacobi: J, default 3 below 100 nodes per axis and 1
    from there on, where one Jacobi solve on the CSR product takes 17 - 23 s) after one warm-up solve per product under "cmg";
  * whether iterations and solutions of the two products are equal (they must be: the same fma chains);
  * the extraction's device time per form (pgd_bdia_times) and the form's bytes.
The reference of every time is the CSR product (knob 0) in the same run."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.bench_cmg import operator      # noqa: E402  (the same two operators)

KNOB = 58
PRODUCTS = (("csr", 0), ("block_dia", 1))


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
    sizes = [int(a) for a in argv] or [65, 129]
    import numpy as np
    from pgdrome_amd import fem, problems
    from pgdrome_amd.hip_backend import HipBackend
    be = fem.set_backend(HipBackend(0))
    ctx = be.ctx
    for npts in sizes:
        fem.clear_caches()
        mesh = fem.BoxMesh(fem.Point(0, 0, 0), fem.Point(1, 1, 1), npts - 1, npts - 1, npts - 1)
        Vh = fem.VectorFunctionSpace(mesh, "P", 1)
        jr = int(jreps) if jreps is not None else (reps if npts < 100 else 1)
        for name in ("elastic_block", "graded_block"):
            if which not in (None, name):
                continue
            A, b = operator(fem, problems, Vh, name)
            n, bv = A.lay.n, b.dev()
            s0 = ctx.bdia_stats()
            line = {"bench": "block_dia", "problem": name, "n": npts, "rows": n, "rtol": 1e-10, "reps": reps, "jacobi_reps": jr,
                    "products_per_round": nprod}
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
                line["%s_product" % pname] = {"us_%s_median" % kind: statistics.median(us[(pname, kind)]) for kind in ("store", "dot_store")}
                line["%s_product" % pname].update({"us_%s_all" % kind: [round(v, 1) for v in us[(pname, kind)]] for kind in ("store", "dot_store")})
            line["product_speedup"] = {kind: line["csr_product"]["us_%s_median" % kind] / line["block_dia_product"]["us_%s_median" % kind]
                                       for kind in ("store", "dot_store")}
            # ---- whole solves
            for prec_name, prec, nrep in (("cmg", 3, reps), ("jacobi", 0, jr)):
                times = {p: [] for p, _ in PRODUCTS}
                res, sol = {}, {}
                for rep in range(nrep + (1 if prec == 3 else 0)):      # (under "cmg" rep 0 is the warm-up of both products' kernels)
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
                        if prec != 3 or rep > 0:
                            times[pname].append(1e3 * dt)
                        res[pname] = {"iterations": it, "relres": rel}
                for pname, _ in PRODUCTS:
                    t = times[pname]
                    res[pname].update(ms_per_solve_median=statistics.median(t), ms_per_solve_all=[round(v, 3) for v in t],
                                      ms_per_iteration=statistics.median(t) / max(res[pname]["iterations"], 1))
                line["%s_pcg" % prec_name] = dict(res, solve_speedup=res["csr"]["ms_per_solve_median"] / res["block_dia"]["ms_per_solve_median"],
                                                  same_iterations=res["csr"]["iterations"] == res["block_dia"]["iterations"],
                                                  same_solution_bits=bool(np.array_equal(sol["csr"], sol["block_dia"])))
            s1 = ctx.bdia_stats()
            forms = s1["forms_built"] - s0["forms_built"]
            line["forms_built"], line["fallbacks"] = forms, s1["fallbacks"] - s0["fallbacks"]
            line["extract_ms_per_form"] = (s1["extract_ms"] - s0["extract_ms"]) / max(forms, 1)
            line["form_bytes"] = 15 * 3 * ((n + 63) // 64 * 64) * 8
            line["csr_value_bytes"], line["csr_column_bytes"] = 8 * A_nnz(be, A), 4 * A_nnz(be, A)
            print(json.dumps(line), flush=True)
            del A, b


def A_nnz(be, A):
    return int(be.mesh_info(A.lay.handle())["nnz"])


if __name__ == "__main__":
    main()
