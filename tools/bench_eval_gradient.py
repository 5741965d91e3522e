"""Batched evaluation of gradient quantities (PGD.evaluate_gradient_many) on the MI355X, against its numpy host path:
problems.elastic_block on the 65^3 box (von Mises stress, a two-valued DG0 scale) and problems.reaction_diffusion on the 129^3
box (|grad u|), each solved once with a few modes, then for S in {64, 256} samples

  stage 1: the modes -> cell-wise planes (pgd_cell_gradient), seconds per mode, device and numpy;
  stage 2: the product on the planes with the square root and the reductions (pgd_eval_batch_norm, statistics + envelopes),
           seconds per sample, for the MFMA kernel, the plain fma kernel (PGD_TUNE_EVAL_VARIANT) and numpy.

    python tools/bench_eval_gradient.py [elastic=65] [scalar=129] > profiles/eval_gradient_bench_n1.jsonl

One JSON line per problem and S.  Seconds are host-clock times around calls that end in a device synchronisation (stage 2 returns
the statistics, so it does); device times are the smallest of three calls after a warm-up of the same shape, numpy times one call.
Stage 1 is timed by dropping the cache of the derived modes and subtracting a cached call of the same shape; numpy is timed at the
smallest S only (its time per sample does not depend on S)."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pgdrome_amd import _lib, fem, model, problems          # noqa: E402
from pgdrome_amd.hip_backend import HipBackend              # noqa: E402
from pgdrome_amd.solver import PGDProblem                   # noqa: E402

SAMPLES = (64, 256)


def best_of(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return min(out)


def run(name, n_side, be):
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
    sol = p.return_PGD()
    att = sol.mesh[0].attributes[0]
    K, nc = sol.used_numModes, mesh.num_cells()
    X = sol.mesh[1].dataX
    for S in SAMPLES:
        coords = np.random.default_rng(S).uniform(X.min(), X.max(), size=(S, 1))
        call = lambda: sol.evaluate_gradient_many(0, [1], coords, 0, quantity=quantity, scale=scale, stats=True, envelope=True,
                                                  sample_chunk=16)       # (the numpy path: 16 columns of cells x 8 bytes at a time)
        rec = {"part": "eval_gradient", "problem": name, "n": n_side, "cells": nc, "K": K, "S": S, "quantity": quantity}

        def drop_and_call():
            att._gradient_modes = None
            return call()
        results = {}
        model.DEVICE_EVAL_MIN_DOFS = 0
        for vname, variant in (("mfma", 1), ("plain", 0)):
            be.ctx.tune(_lib.TUNE_EVAL_VARIANT, variant)
            drop_and_call()                                  # warm-up of both stages
            results[vname] = call()
            cached = best_of(call, 3)
            rec[vname + "_stage2_seconds_per_sample"] = cached / S
            if variant:
                rec["device_stage1_seconds_per_mode"] = max(best_of(drop_and_call, 3) - cached, 0.0) / K
                rec["eval_norm_shape"] = list(be.ctx.eval_norm_last_shape())
        be.ctx.tune(_lib.TUNE_EVAL_VARIANT, 1)
        if S != SAMPLES[0]:                                   # numpy is timed at the smallest S only: it scales with S
            print(json.dumps(rec), flush=True)
            continue
        model.DEVICE_EVAL_MIN_DOFS = 1 << 60                  # the numpy path
        t_all = best_of(drop_and_call, 1)
        t0 = time.perf_counter()
        results["numpy"] = call()
        t_cached = time.perf_counter() - t0
        rec["numpy_stage1_seconds_per_mode"] = max(t_all - t_cached, 0.0) / K
        rec["numpy_stage2_seconds_per_sample"] = t_cached / S
        att._gradient_modes = None
        big = np.abs(results["numpy"].max).max()
        rec["mfma_vs_numpy_max_rel_diff"] = float(np.abs(results["mfma"].max - results["numpy"].max).max() / big)
        rec["plain_vs_numpy_max_rel_diff"] = float(np.abs(results["plain"].max - results["numpy"].max).max() / big)
        rec["numpy_over_mfma_stage2"] = rec["numpy_stage2_seconds_per_sample"] / rec["mfma_stage2_seconds_per_sample"]
        rec["numpy_over_device_stage1"] = rec["numpy_stage1_seconds_per_mode"] / max(rec["device_stage1_seconds_per_mode"], 1e-12)
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    sizes = {"elastic": 65, "scalar": 129}
    for a in sys.argv[1:]:
        k, v = a.split("=")
        sizes[k] = int(v)
    backend = HipBackend(0)
    fem.set_backend(backend)
    run("elastic_block", sizes["elastic"], backend)
    fem.clear_caches()
    run("reaction_diffusion", sizes["scalar"], backend)
