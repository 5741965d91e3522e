"""Sensor responses for many samples (pgdrome_amd/csrc/pgd_locate.hip, PGD.evaluate_sensor_response_many) beside the host path
(fem.point_basis per point, PGD.eval_fixed_modes, a loop over PGD.evaluate_sensor_response) on the same inputs in the same process:

    locate      P points on BoxMesh at n^3 vertices: the general kernel (PGD_TUNE_LOCATE_LATTICE = 0), the lattice path, the general
                kernel on a jittered (non-lattice) copy of the mesh, and fem.point_basis for the first --host-points points
    sample      48 scalar P1 modes at the located points: pgd_points_sample per mode against PGD.eval_fixed_modes (its point_basis
                calls on --host-points points, and its gather loop)
    response    PGD.evaluate_sensor_response_many at S = 1024 samples of two parameters with the Jacobian for both, against
                eval_fixed_modes + a loop over evaluate_sensor_response (--host-samples samples) on the same model

    python tools/bench_sensors.py [n ...] [--points P ...] [--reps R] [--out FILE] [--limit SECONDS] [--host-points H] [--host-samples HS]
                                                                        (defaults: n = 65 129, P = 100 10000, R = 3, H = 8, HS = 32)

Every configuration runs in a child process of its own under `timeout` (--limit, default 600 s); the first child that does not end
cleanly ends the run.  One JSON line per configuration, printed and appended to --out (default profiles/sensor_bench_n1.jsonl).
Times are wall-clock seconds around calls that end synchronised (median of R after one warm-up); the host path is timed once."""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
K_MODES = 48


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def setup(n):
    import numpy as np
    from pgdrome_amd import fem
    from pgdrome_amd.hip_backend import HipBackend
    be = fem.set_backend(HipBackend(0))
    mesh = fem.BoxMesh(fem.Point(0, 0, 0), fem.Point(1, 1, 1), n - 1, n - 1, n - 1)
    return np, fem, be, mesh


def points_in(np, mesh, count, seed):
    X, C = mesh.coordinates(), mesh.cells()
    rng = np.random.default_rng(seed)
    cells = rng.integers(0, len(C), count)
    lam = 0.05 + 0.8 * rng.dirichlet(np.ones(4), size=count)
    return np.einsum("pa,pad->pd", lam, X[C[cells]])


def host_point_basis(fem, mesh, pts):
    """seconds per point of fem.point_basis (the first call, which builds the mesh's inverse maps, apart)"""
    lay = mesh.layout(1)
    t0 = time.perf_counter()
    fem.point_basis(lay, pts[0])
    first = time.perf_counter() - t0
    t0 = time.perf_counter()
    for x in pts[1:]:
        fem.point_basis(lay, x)
    return first, (time.perf_counter() - t0) / max(1, len(pts) - 1)


def one_locate(n, P, reps, host_points):
    from pgdrome_amd import _lib
    np, fem, be, mesh = setup(n)
    ctx = be.ctx
    X, C = mesh.coordinates(), mesh.cells()
    pts = points_in(np, mesh, P, 1)
    mh = mesh.layout(1).handle()
    line = {"bench": "locate", "n": n, "cells": int(len(C)), "points": P}

    def run(handle, knob):
        ctx.tune(_lib.TUNE_LOCATE_LATTICE, knob)
        ctx.points_free(ctx.points_locate(handle, pts, 1e-10))
    line["lattice_s"] = timed(lambda: run(mh, 1), reps)
    assert ctx.points_last_path() == _lib.LOCATE_PATH_LATTICE
    line["general_s"] = timed(lambda: run(mh, 0), reps)
    assert ctx.points_last_path() == _lib.LOCATE_PATH_GENERAL
    line["general_cell_tests_per_s"] = P * len(C) / line["general_s"]
    h = 1.0 / (n - 1)
    Xj = X + 0.2 * h * np.random.default_rng(2).uniform(-1, 1, X.shape)
    jh = ctx.mesh_upload(Xj, C)
    lam = 0.05 + 0.8 * np.random.default_rng(1).dirichlet(np.ones(4), size=P)
    cells = np.random.default_rng(3).integers(0, len(C), P)
    ptsj = np.einsum("pa,pad->pd", lam, Xj[C[cells]])

    def runj():
        ctx.points_free(ctx.points_locate(jh, ptsj, 1e-10))
    ctx.tune(_lib.TUNE_LOCATE_LATTICE, 1)
    line["jittered_general_s"] = timed(runj, reps)
    assert ctx.points_last_path() == _lib.LOCATE_PATH_GENERAL
    got = ctx.points_locate(jh, ptsj, 1e-10)
    assert np.array_equal(ctx.points_download(got)[0], cells)
    ctx.points_free(got)
    line["jittered_cell_tests_per_s"] = P * len(C) / line["jittered_general_s"]
    first, per = host_point_basis(fem, mesh, pts[:host_points])
    line.update(host_point_basis_first_s=first, host_point_basis_per_point_s=per, host_points_timed=min(P, host_points),
                host_extrapolated_s=first + per * (P - 1))
    print(json.dumps(line), flush=True)


def model(np, fem, mesh, K, seed):
    from pgdrome_amd.model import PGD
    rng = np.random.default_rng(seed)
    V = fem.FunctionSpace(mesh, "CG", 1)
    m1, m2 = fem.IntervalMesh(64, 0.0, 1.0), fem.IntervalMesh(32, 1.0, 3.0)
    spaces = (V, fem.FunctionSpace(m1, "CG", 1), fem.FunctionSpace(m2, "CG", 2))
    modes = []
    for W in spaces:
        fs = []
        for _ in range(K):
            f = fem.Function(W)
            f.vector()._host = rng.uniform(-1.0, 1.0, W.dim())
            f.vector().touched_host()
            fs.append(f)
        modes.append(fs)
    return PGD(name="bench", n_modes=K, fmeshes=[mesh, m1, m2], pgd_modes=modes, name_coord=["X", "p", "q"], modes_info=["U", "Node", "Scalar"])


def one_sample(n, P, reps, host_points):
    np, fem, be, mesh = setup(n)
    ctx = be.ctx
    sol = model(np, fem, mesh, K_MODES, 5)
    pts = points_in(np, mesh, P, 1)
    modes = sol.mesh[0].attributes[0].interpolationfct
    handles = [m.vector().dev() for m in modes]
    loc = fem.locate_points(mesh, pts)
    mh = mesh.layout(1).handle()
    outs = [ctx.vec_alloc(P) for _ in range(K_MODES)]

    def run():
        for h, o in zip(handles, outs):
            ctx.points_sample(loc.handle, mh, h, o)
        ctx.sync()
    line = {"bench": "sample", "n": n, "points": P, "modes": K_MODES, "device_sample_s": timed(run, reps)}
    t0 = time.perf_counter()
    sol.sensor_modes(pts, 0, 0).host()
    line["sensor_modes_first_call_s"] = time.perf_counter() - t0
    hp = pts[:host_points]
    t0 = time.perf_counter()
    sol.eval_fixed_modes(hp, 0, 0)
    t = time.perf_counter() - t0
    line.update(host_eval_fixed_modes_s=t, host_points_timed=len(hp), host_extrapolated_s=t * P / len(hp))
    print(json.dumps(line), flush=True)


def one_response(n, P, reps, host_samples, S=1024):
    np, fem, be, mesh = setup(n)
    sol = model(np, fem, mesh, K_MODES, 6)
    pts = points_in(np, mesh, P, 1)
    rng = np.random.default_rng(7)
    samples = np.stack([rng.uniform(0.0, 1.0, S), rng.uniform(1.0, 3.0, S)], axis=1)
    t0 = time.perf_counter()
    res = sol.evaluate_sensor_response_many(0, [1, 2], samples, 0, pts, d_dim=[1, 2])
    first = time.perf_counter() - t0
    again = timed(lambda: sol.evaluate_sensor_response_many(0, [1, 2], samples, 0, pts, d_dim=[1, 2]), reps)
    line = {"bench": "response", "n": n, "points": P, "modes": K_MODES, "samples": S, "many_first_call_s": first, "many_cached_s": again}
    t0 = time.perf_counter()
    sol.eval_fixed_modes(pts, 0, 0)
    line["host_eval_fixed_modes_s"] = time.perf_counter() - t0
    sol.create_derivation_fct([1, 2], 0)
    t0 = time.perf_counter()
    loop = np.array([sol.evaluate_sensor_response(0, [1, 2], list(c), 0, pts) for c in samples[:host_samples]])
    for d in (1, 2):
        for c in samples[:host_samples]:
            sol.evaluate_derivative_sensor_response(0, [1, 2], list(c), 0, d, pts)
    t = time.perf_counter() - t0
    line.update(host_loop_s=t, host_samples_timed=host_samples, host_loop_extrapolated_s=t * S / host_samples,
                max_difference=float(np.abs(loop - res.values[:host_samples]).max()))
    print(json.dumps(line), flush=True)


def main():
    argv = sys.argv[1:]

    def opt(flag, default, many=False):
        if flag not in argv:
            return default
        i = argv.index(flag)
        j = i + 1
        while many and j + 1 < len(argv) and not argv[j + 1].startswith("--"):
            j += 1
        vals = argv[i + 1:j + 1]
        del argv[i:j + 1]
        return vals if many else vals[0]
    reps, limit = int(opt("--reps", 3)), int(opt("--limit", 600))
    host_points, host_samples = int(opt("--host-points", 8)), int(opt("--host-samples", 32))
    out = opt("--out", os.path.join(ROOT, "profiles", "sensor_bench_n1.jsonl"))
    child = opt("--one", None)
    counts = [int(p) for p in opt("--points", ["100", "10000"], many=True)]
    sizes = [int(a) for a in argv] or [65, 129]
    if child is not None:
        fn = {"locate": lambda: one_locate(sizes[0], counts[0], reps, host_points), "sample": lambda: one_sample(sizes[0], counts[0], reps, host_points),
              "response": lambda: one_response(sizes[0], counts[0], reps, host_samples)}[child]
        return fn()
    configs = [(kind, n, P) for n in sizes for P in counts for kind in ("locate", "sample")] + [("response", sizes[0], counts[0])]
    for kind, n, P in configs:
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), str(n), "--one", kind, "--points", str(P),
               "--reps", str(reps), "--host-points", str(host_points), "--host-samples", str(host_samples)]
        run = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(run.stdout)
        sys.stdout.flush()
        if run.returncode != 0:
            raise SystemExit("bench_sensors: %s at %d^3 vertices, %d points ended with status %d; nothing more is started" % (kind, n, P, run.returncode))
        with open(out, "a") as fh:
            fh.write("".join(l + "\n" for l in run.stdout.splitlines() if l.startswith("{")))


if __name__ == "__main__":
    main()
