"""PGD.evaluate_gradient_many(planes="fused") on the MI355X - the planes formed inside the batch evaluation (pgd_eval_batch_grad),
none stored - beside the stored path where both run, and alone where the stored planes do not fit.

  both:   problems.elastic_block on the 65^3 box (von Mises stress, a two-valued DG0 scale, 3 modes) and
          problems.reaction_diffusion on the 129^3 box (|grad u|, 4 modes), each solved once, S in {64, 256, 1024}:
          stored stage 1 (modes -> planes) per mode, stored stage 2 per call, fused per call.  What "auto" should prefer is
          decided by fused_seconds against stored_stage2_seconds: the stored figure is the yardstick.
  large:  a synthetic solution of 48 seeded random nodal modes on the 256^3 box (6.4 GB of modes; the stored planes of
          "gradient_norm" would take 115 GB and are refused), S in {64, 256, 1024}, statistics and envelopes: seconds per call and
          the matrix-unit work 2 q K cells S over them - to be read beside pgd_eval_batch's FLOP/s on the same lattice
          (profiles/eval_batch_bench_n1.jsonl) - and the refusal of planes="stored".

    python tools/bench_eval_gradient_fused.py [both] [large] [elastic=65] [scalar=129] [box=256] > profiles/eval_gradient_fused_bench_n1.jsonl

One JSON line per problem and S.  Seconds are host-clock times around calls that end in the download of the statistics (a device
synchronisation), the smallest of three calls after a warm-up call of the same shape.  Stage 1 is timed by dropping the cache of
the derived modes and subtracting a cached call of the same shape."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pgdrome_amd import fem, model, problems                # noqa: E402
from pgdrome_amd.hip_backend import HipBackend              # noqa: E402
from pgdrome_amd.model import PGD                           # noqa: E402
from pgdrome_amd.solver import PGDProblem                   # noqa: E402

SAMPLES = (64, 256, 1024)


def best_of(fn, reps=3):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return min(out)


def note(text):
    print(text, file=sys.stderr, flush=True)


def run_both(name, n_side, be):
    mesh = fem.BoxMesh(fem.Point(0, 0, 0), fem.Point(1, 1, 1), n_side - 1, n_side - 1, n_side - 1)
    if name == "elastic_block":
        p = PGDProblem(**problems.elastic_block(mesh, 9, PGD_nmax=3))
        p.solve_PGD(_problem="linear", settings={"preconditioner": "cmg"})
        quantity = "von_mises"
        scale = fem.Function(fem.FunctionSpace(mesh, "DG", 0))
        mid = mesh.coordinates()[mesh.cells()].mean(axis=1)[:, 0]
        scale.vector()[:] = np.where(mid < 0.5, 1.0 / 1.3, 3.0 / 1.3)
    else:
        p = PGDProblem(**problems.reaction_diffusion(mesh, 33, PGD_nmax=4))
        p.solve_PGD(_problem="linear")
        quantity, scale = "gradient_norm", None
    note("%s %d^3: solved" % (name, n_side))
    sol = p.return_PGD()
    att = sol.mesh[0].attributes[0]
    K, nc = sol.used_numModes, mesh.num_cells()
    q = fem.gradient_quantity(quantity, 3, att.interpolationfct[0].function_space()._ncomp).shape[0]
    X = sol.mesh[1].dataX
    for S in SAMPLES:
        coords = np.random.default_rng(S).uniform(X.min(), X.max(), size=(S, 1))
        call = lambda planes="stored": sol.evaluate_gradient_many(0, [1], coords, 0, quantity=quantity, scale=scale, stats=True,
                                                                  envelope=True, planes=planes)

        def drop_and_call():
            att._gradient_modes = None
            return call()
        stored = drop_and_call()                                  # warm-up of both stages
        cached = best_of(call)
        stage1 = max(best_of(drop_and_call) - cached, 0.0) / K
        shape_stored = list(be.ctx.eval_norm_last_shape())
        att._gradient_modes = None                               # (the fused call runs without the planes on the device)
        fused = call("fused")
        t_fused = best_of(lambda: call("fused"))
        rec = {"part": "eval_gradient_fused", "problem": name, "n": n_side, "cells": nc, "K": K, "q": q, "S": S, "quantity": quantity,
               "stored_stage1_seconds_per_mode": stage1, "stored_stage2_seconds": cached, "fused_seconds": t_fused,
               "fused_over_stored_stage2": t_fused / cached, "stored_first_call_seconds": cached + K * stage1,
               "eval_norm_shape_stored": shape_stored, "eval_norm_shape_fused": list(be.ctx.eval_norm_last_shape()),
               "stored_plane_bytes": K * q * nc * 8,
               "fused_vs_stored_max_rel_diff": float(np.abs(fused.max - stored.max).max() / np.abs(stored.max).max())}
        print(json.dumps(rec), flush=True)


def run_large(n_side, be, K=48):
    mesh = fem.BoxMesh(fem.Point(0, 0, 0), fem.Point(1, 1, 1), n_side - 1, n_side - 1, n_side - 1)
    pm = fem.IntervalMesh(32, 0.0, 1.0)
    V, Vp = fem.FunctionSpace(mesh, "CG", 1), fem.FunctionSpace(pm, "CG", 1)
    note("box %d^3: mesh and space built" % n_side)
    rng = np.random.default_rng(n_side)
    fs, gs = [], []
    for _ in range(K):
        f, g = fem.Function(V), fem.Function(Vp)
        f.vector().set_local(rng.standard_normal(V.dim()))
        f.vector().dev()                                         # on the device now; the host copy may go
        g.vector().set_local(rng.standard_normal(Vp.dim()))
        fs.append(f)
        gs.append(g)
    note("box %d^3: %d modes on the device" % (n_side, K))
    sol = PGD(name="synthetic", n_modes=K, fmeshes=[mesh, pm], pgd_modes=[fs, gs], name_coord=["x", "p"])
    nc, q = mesh.num_cells(), 3
    for S in SAMPLES:
        coords = np.random.default_rng(S).uniform(0.0, 1.0, size=(S, 1))
        call = lambda planes: sol.evaluate_gradient_many(0, [1], coords, 0, quantity="gradient_norm", stats=True, envelope=True,
                                                         planes=planes)
        res = call("fused")
        t = best_of(lambda: call("fused"))
        try:
            call("stored")
            refusal = None
        except ValueError as exc:
            refusal = str(exc)
        flop = 2.0 * q * K * nc * S
        rec = {"part": "eval_gradient_fused_large", "n": n_side, "nodes": V.dim(), "cells": nc, "K": K, "q": q, "S": S,
               "quantity": "gradient_norm", "outputs": "stats+envelope", "mode_bytes": K * V.dim() * 8, "stored_plane_bytes": K * q * nc * 8,
               "fused_seconds": t, "flop": flop, "fused_flops": flop / t, "eval_norm_shape_fused": list(be.ctx.eval_norm_last_shape()),
               "max_of_max": float(res.max.max()), "stored_refusal": refusal}
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    sizes = {"elastic": 65, "scalar": 129, "box": 256}
    parts = []
    for a in sys.argv[1:]:
        if "=" in a:
            k, v = a.split("=")
            sizes[k] = int(v)
        else:
            parts.append(a)
    parts = parts or ["both", "large"]
    backend = HipBackend(0)
    fem.set_backend(backend)
    model.DEVICE_EVAL_MIN_DOFS = 0
    if "both" in parts:
        run_both("elastic_block", sizes["elastic"], backend)
        fem.clear_caches()
        run_both("reaction_diffusion", sizes["scalar"], backend)
        fem.clear_caches()
    if "large" in parts:
        run_large(sizes["box"], backend)
