"""PGD.evaluate_gradient_many on P2 modes on the MI355X: at="midpoint" and at="vertices", the stored stages
(pgd_cell_gradient_p2, then pgd_eval_batch_norm) and the fused call (pgd_eval_batch_grad_p2), beside two baselines taken in the
same process on the same mesh - the numpy host path of the same request, and the P1 kernels on the vertex values of the same modes
(equal cell count, a quarter of the entries of "vertices").

    elastic_block        von Mises stress of problems.elastic_block(degree=2), a two-valued DG0 scale, on an n^3-VERTEX box
    reaction_diffusion   |grad u| of problems.reaction_diffusion(degree=2)

    python tools/bench_eval_gradient_p2.py [elastic=33] [scalar=65] [--problem NAME] [--out FILE] [--limit SECONDS]

Every problem runs in a child process of its own under `timeout` (--limit, default 900 s); the first child that does not end
cleanly ends the run.  One JSON line per problem, `at` and S in {64, 256, 1024}, printed and appended to --out (default
profiles/eval_gradient_p2_bench_n1.jsonl), and one line per problem for the P1 kernels.  Seconds are host-clock times around calls
that end in the download of the statistics (a device synchronisation): the smallest of five calls after a warm-up call of the same
shape, with the spread (largest - smallest) / smallest of the five beside it.  Stage 1 is timed by dropping the cache of the
derived modes and subtracting a cached call of the same shape.  The `stats_only_*` figures are the same calls without the
envelopes: at="vertices" downloads its two envelope vectors of 4 x cells entries and reduces them on the host, which is most of such
a call on a large mesh.  The host path is timed once, at S = 64 (its (entries x samples)
blocks at 16 samples a time), statistics and envelopes as on the device."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PROBLEMS = {"elastic_block": "elastic", "reaction_diffusion": "scalar"}
SAMPLES = (64, 256, 1024)


def timed(fn, reps=5):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return min(out), (max(out) - min(out)) / min(out)


def one(name, n_side):
    import numpy as np
    from pgdrome_amd import fem, model, problems
    from pgdrome_amd.hip_backend import HipBackend
    from pgdrome_amd.model import PGD
    from pgdrome_amd.solver import PGDProblem
    be = fem.set_backend(HipBackend(0))
    mesh = fem.BoxMesh(fem.Point(0, 0, 0), fem.Point(1, 1, 1), n_side - 1, n_side - 1, n_side - 1)
    if name == "elastic_block":
        p = PGDProblem(**problems.elastic_block(mesh, 9, PGD_nmax=3, degree=2))
        p.solve_PGD(_problem="linear", settings={"preconditioner": "pmg"})
        quantity = "von_mises"
        scale = fem.Function(fem.FunctionSpace(mesh, "DG", 0))
        mid = mesh.coordinates()[mesh.cells()].mean(axis=1)[:, 0]
        scale.vector()[:] = np.where(mid < 0.5, 1.0 / 1.3, 3.0 / 1.3)
    else:
        p = PGDProblem(**problems.reaction_diffusion(mesh, 33, PGD_nmax=4, degree=2))
        p.solve_PGD(_problem="linear")
        quantity, scale = "gradient_norm", None
    print("%s %d^3 vertices: solved" % (name, n_side), file=sys.stderr, flush=True)
    sol = p.return_PGD()
    att = sol.mesh[0].attributes[0]
    V = att.interpolationfct[0].function_space()
    K, nc, ncomp = sol.used_numModes, mesh.num_cells(), V._ncomp
    q = fem.gradient_quantity(quantity, 3, ncomp).shape[0]
    X = sol.mesh[1].dataX
    common = {"bench": "eval_gradient_p2", "problem": name, "n_vertices": n_side, "nodes": V.dim() // ncomp, "cells": nc, "K": K, "q": q,
              "quantity": quantity, "outputs": "stats+envelope"}

    def measure(s, S, at):
        """stored stage 1 per mode, stored stage 2, fused of the solution ``s`` (seconds, spreads, row blocks)."""
        a = s.mesh[0].attributes[0]
        coords = np.random.default_rng(S).uniform(X.min(), X.max(), size=(S, 1))
        call = lambda planes="stored", envelope=True: s.evaluate_gradient_many(0, [1], coords, 0, quantity=quantity, scale=scale,
                                                                               stats=True, envelope=envelope, planes=planes, at=at)

        def drop_and_call():
            a._gradient_modes = None
            return call()
        stored = drop_and_call()                                  # warm-up of both stages
        cached, cached_spread = timed(call)
        stats_stored, _ = timed(lambda: call(envelope=False))
        first, _ = timed(drop_and_call)
        shape_stored = list(be.ctx.eval_norm_last_shape())
        a._gradient_modes = None                                  # (the fused call runs without the planes on the device)
        fused = call("fused")
        t_fused, fused_spread = timed(lambda: call("fused"))
        stats_fused, _ = timed(lambda: call("fused", False))
        return {"S": S, "stored_stage1_seconds_per_mode": max(first - cached, 0.0) / K, "stored_stage2_seconds": cached,
                "stored_stage2_spread": cached_spread, "fused_seconds": t_fused, "fused_spread": fused_spread,
                "fused_over_stored_stage2": t_fused / cached, "stats_only_stored_stage2_seconds": stats_stored,
                "stats_only_fused_seconds": stats_fused, "eval_norm_shape_stored": shape_stored,
                "eval_norm_shape_fused": list(be.ctx.eval_norm_last_shape()),
                "fused_vs_stored_max_rel_diff": float(np.abs(fused.max - stored.max).max() / np.abs(stored.max).max())}, coords, stored

    model.DEVICE_EVAL_MIN_DOFS = 0
    for at in ("midpoint", "vertices"):
        npt = 1 if at == "midpoint" else 4
        for S in SAMPLES:
            rec, coords, dev = measure(sol, S, at)
            rec.update(common, at=at, entries=npt * nc, stored_plane_bytes=K * q * npt * nc * 8)
            if S == SAMPLES[0]:                                   # the numpy host path of the same request, once
                model.DEVICE_EVAL_MIN_DOFS = 1 << 60
                att._gradient_modes = None
                host_call = lambda: sol.evaluate_gradient_many(0, [1], coords, 0, quantity=quantity, scale=scale, stats=True,
                                                               envelope=True, at=at, sample_chunk=16)
                t0 = time.perf_counter()
                host = host_call()
                t1 = time.perf_counter()
                host_call()
                t2 = time.perf_counter()
                model.DEVICE_EVAL_MIN_DOFS = 0
                att._gradient_modes = None
                rec.update(host_stage1_seconds_per_mode=max((t1 - t0) - (t2 - t1), 0.0) / K, host_stage2_seconds=t2 - t1,
                           host_vs_device_max_rel_diff=float(np.abs(host.max - dev.max).max() / np.abs(dev.max).max()))
            print(json.dumps(rec), flush=True)
    # the P1 kernels on the same mesh: the vertex values of the same modes
    V1 = fem.VectorFunctionSpace(mesh, "CG", 1) if ncomp > 1 else fem.FunctionSpace(mesh, "CG", 1)
    fs = []
    for k in range(K):
        f = fem.Function(V1)
        f.vector().set_local(np.asarray(att.data[k], dtype=np.float64).reshape(-1))
        fs.append(f)
    sol1 = PGD(name="p1", n_modes=K, fmeshes=[mesh, sol.mesh[1].fenics_mesh],
               pgd_modes=[fs, list(sol.mesh[1].attributes[0].interpolationfct)[:K]], name_coord=["x", "p"])
    for S in SAMPLES:
        rec = measure(sol1, S, None)[0]
        rec.update(common, bench="eval_gradient_p2_baseline_p1", at=None, entries=nc, nodes=V1.dim() // ncomp, stored_plane_bytes=K * q * nc * 8)
        print(json.dumps(rec), flush=True)


def main():
    argv = sys.argv[1:]

    def opt(flag, default):
        if flag in argv:
            i = argv.index(flag)
            val = argv[i + 1]
            del argv[i:i + 2]
            return val
        return default
    which, limit = opt("--problem", None), int(opt("--limit", 900))
    out = opt("--out", os.path.join(ROOT, "profiles", "eval_gradient_p2_bench_n1.jsonl"))
    child = opt("--one", None)
    sizes = {"elastic": 33, "scalar": 65}
    for a in argv:
        k, v = a.split("=")
        sizes[k] = int(v)
    if child is not None:
        return one(child, sizes[PROBLEMS[child]])
    for name, key in PROBLEMS.items():
        if which not in (None, name):
            continue
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "%s=%d" % (key, sizes[key]), "--one", name]
        run = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(run.stdout)
        sys.stdout.flush()
        if run.returncode != 0:
            raise SystemExit("bench_eval_gradient_p2: %s ended with status %d; nothing more is started" % (name, run.returncode))
        with open(out, "a") as fh:
            fh.write("".join(l + "\n" for l in run.stdout.splitlines() if l.startswith("{")))


if __name__ == "__main__":
    main()
