"""The stress quantities of PGD.evaluate_gradient_many ("max_principal", "min_principal", "tresca", "stress_component") on the
MI355X beside von Mises of the same run: what the eigenvalue epilogue (one acos, a cos, five roots per value) costs against the
norm epilogue (one root) on the same planes, stored (pgd_eval_batch_quantity) and fused (pgd_eval_batch_grad_quantity /
pgd_eval_batch_grad_p2_quantity).

    p1            problems.elastic_block on a 65^3-vertex box, P1
    p2_midpoint   problems.elastic_block(degree=2) on a 33^3-vertex box, at="midpoint"
    p2_vertices   the same, at="vertices"

    python tools/bench_eval_gradient_tensor.py [p1=65] [p2=33] [--case NAME] [--out FILE] [--limit SECONDS]

Every case runs in a child process of its own under `timeout` (--limit, default 900 s); the first child that does not end cleanly
ends the run.  One JSON line per case, quantity, `planes` and S in {64, 256, 1024}, printed and written to --out (default
profiles/eval_gradient_tensor_bench_n1.jsonl), where a run replaces the rows of the cases it runs and keeps those of the others.
Seconds are host-clock times around calls that end in the download of the statistics (a device synchronisation; statistics and
envelopes are asked for): the smallest of five calls after a warm-up call of the same shape, with the spread (largest -
smallest) / smallest of the five beside it; `over_von_mises` is the ratio to the von Mises call of the same case, `planes` and S.
E is a two-valued DG0 Function, nu = 0.3."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CASES = {"p1": ("p1", 1, None), "p2_midpoint": ("p2", 2, "midpoint"), "p2_vertices": ("p2", 2, "vertices")}
SAMPLES = (64, 256, 1024)
QUANTITIES = (("von_mises", {}), ("max_principal", {"nu": 0.3}), ("min_principal", {"nu": 0.3}), ("tresca", {"nu": 0.3}),
              ("stress_component", {"nu": 0.3, "component": (0, 0)}))


def timed(fn, reps=5):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return min(out), (max(out) - min(out)) / min(out)


def one(case, n_side):
    import numpy as np
    from pgdrome_amd import fem, model, problems
    from pgdrome_amd.hip_backend import HipBackend
    from pgdrome_amd.solver import PGDProblem
    _, degree, at = CASES[case]
    be = fem.set_backend(HipBackend(0))
    mesh = fem.BoxMesh(fem.Point(0, 0, 0), fem.Point(1, 1, 1), n_side - 1, n_side - 1, n_side - 1)
    p = PGDProblem(**problems.elastic_block(mesh, 9, PGD_nmax=3, degree=degree))
    p.solve_PGD(_problem="linear", settings={"preconditioner": "cmg" if degree == 1 else "pmg"})
    print("%s %d^3 vertices: solved" % (case, n_side), file=sys.stderr, flush=True)
    sol = p.return_PGD()
    scale = fem.Function(fem.FunctionSpace(mesh, "DG", 0))
    mid = mesh.coordinates()[mesh.cells()].mean(axis=1)[:, 0]
    scale.vector()[:] = np.where(mid < 0.5, 70.0, 210.0)
    X = sol.mesh[1].dataX
    npt = 4 if at == "vertices" else 1
    common = {"bench": "eval_gradient_tensor", "case": case, "n_vertices": n_side, "cells": mesh.num_cells(), "entries": npt * mesh.num_cells(),
              "K": sol.used_numModes, "at": at, "outputs": "stats+envelope"}
    model.DEVICE_EVAL_MIN_DOFS = 0
    for S in SAMPLES:
        coords = np.random.default_rng(S).uniform(X.min(), X.max(), size=(S, 1))
        for planes in ("stored", "fused"):
            base = None
            for quantity, kw in QUANTITIES:
                call = lambda: sol.evaluate_gradient_many(0, [1], coords, 0, quantity=quantity, scale=scale, stats=True, envelope=True,
                                                          planes=planes, at=at, **kw)
                res = call()                                     # warm-up; stored: builds the planes of this quantity
                t, spread = timed(call)
                base = t if base is None else base
                rec = dict(common, S=S, planes=planes, quantity=quantity, seconds=t, spread=spread, over_von_mises=t / base,
                           eval_norm_shape=list(be.ctx.eval_norm_last_shape()), max_of_max=float(res.max.max()), min_of_min=float(res.min.min()))
                print(json.dumps(rec), flush=True)
            sol.mesh[0].attributes[0]._gradient_modes = None


def main():
    argv = sys.argv[1:]

    def opt(flag, default):
        if flag in argv:
            i = argv.index(flag)
            val = argv[i + 1]
            del argv[i:i + 2]
            return val
        return default
    which, limit = opt("--case", None), int(opt("--limit", 900))
    out = opt("--out", os.path.join(ROOT, "profiles", "eval_gradient_tensor_bench_n1.jsonl"))
    child = opt("--one", None)
    sizes = {"p1": 65, "p2": 33}
    for a in argv:
        k, v = a.split("=")
        sizes[k] = int(v)
    if child is not None:
        return one(child, sizes[CASES[child][0]])
    todo = [case for case in CASES if which in (None, case)]
    if os.path.exists(out):                                  # a run replaces the rows of the cases it runs: one set of rows per case
        kept = [l for l in open(out) if l.strip() and json.loads(l).get("case") not in todo]
        with open(out, "w") as fh:
            fh.writelines(kept)
    for case in todo:
        key = CASES[case][0]
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "%s=%d" % (key, sizes[key]), "--one", case]
        run = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(run.stdout)
        sys.stdout.flush()
        if run.returncode != 0:
            raise SystemExit("bench_eval_gradient_tensor: %s ended with status %d; nothing more is started" % (case, run.returncode))
        with open(out, "a") as fh:
            fh.write("".join(l + "\n" for l in run.stdout.splitlines() if l.startswith("{")))


if __name__ == "__main__":
    main()
