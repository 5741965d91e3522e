"""Gram blocks (pgd_vec_gram) on the MI355X: K in {16, 48, 128} vectors on the n^3 space for n in {128, 256}, the symmetric block
X^T X and a cross block X^T Y, three ways in one process, alternating: the MFMA kernel, the plain fma kernel
(PGD_TUNE_GRAM_VARIANT) and K calls of pgd_vec_multidot - the only way to the same matrix without the entry point.  Then
PGD.compress end to end on 48 synthetic modes of true rank 12 at n^3 x 128, with what evaluate_many at S = 1024 costs before
and after.

    python tools/bench_gram.py [n=128 256 ...] [compress=256]      # writes profiles/gram_bench_n1.jsonl

Every size runs in a child process of its own under a time limit; a size that fails or runs out of time leaves a line that
says so and the next size still runs.  Seconds are host-clock times around calls that end in a device synchronisation: the
median of 3 rounds after a warm-up round, the three ways taking turns inside a round; "spread" is (max - min) / median of the
rounds.  TB/s counts 8 n (kx + ky) bytes (8 n kx in the symmetric case) - what the data requires - and TFLOP/s 2 n kx ky (the
symmetric case computes the 16 x 16 tiles on and above the diagonal only; the rate is quoted on the full 2 n K^2 all the
same)."""
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "gram_bench_n1.jsonl")
KS = (16, 48, 128)
CHILD_LIMIT = 420           # seconds per child process


def rounds(ctx, ways, nrounds=3):
    """{name: (median seconds, spread)} of the callables in `ways`, taking turns: one warm-up round, then `nrounds` timed ones."""
    for fn in ways.values():
        fn()
    ctx.sync()
    t = {name: [] for name in ways}
    for _ in range(nrounds):
        for name, fn in ways.items():
            ctx.sync()
            t0 = time.perf_counter()
            fn()
            ctx.sync()
            t[name].append(time.perf_counter() - t0)
    return {name: (statistics.median(v), (max(v) - min(v)) / statistics.median(v)) for name, v in t.items()}


def run_kernel(n_side):
    from pgdrome_amd import _lib
    ctx = _lib.Context(0)
    n = n_side ** 3
    kmax = max(KS)
    base = np.random.default_rng(n_side).standard_normal(n + 16 * 2 * kmax)
    vecs = [ctx.vec_from(base[16 * k:16 * k + n]) for k in range(2 * kmax)]          # shifted windows: distinct, cheap to make
    del base
    for K in KS:
        xs, ys = vecs[:K], vecs[kmax:kmax + K]
        for case in ("symmetric", "cross"):
            yarg = None if case == "symmetric" else ys
            res = {}

            def gram(variant, key):
                ctx.tune(_lib.TUNE_GRAM_VARIANT, variant)
                res[key] = ctx.vec_gram(xs, yarg)
                ctx.tune(_lib.TUNE_GRAM_VARIANT, 1)

            def multidot():
                res["multidot"] = np.array([ctx.vec_multidot(x, xs if yarg is None else ys) for x in xs])

            t = rounds(ctx, {"mfma": lambda: gram(1, "mfma"), "plain": lambda: gram(0, "plain"), "multidot": multidot})
            nbytes = 8.0 * n * (K if case == "symmetric" else 2 * K)
            flop = 2.0 * n * K * K
            rec = {"part": "gram", "n": n_side, "rows": n, "K": K, "case": case, "bytes": nbytes, "flop": flop,
                   "multidot_vector_reads": (-(-K // 17) + K) * K, "gram_vector_reads": K if case == "symmetric" else 2 * K}
            for name, (sec, spread) in t.items():
                rec[name + "_us"] = 1e6 * sec
                rec[name + "_spread"] = spread
                rec[name + "_TBps"] = nbytes / sec / 1e12
                rec[name + "_TFLOPs"] = flop / sec / 1e12
            rec["plain_over_mfma"] = t["plain"][0] / t["mfma"][0]
            rec["multidot_over_mfma"] = t["multidot"][0] / t["mfma"][0]
            scale = np.abs(res["multidot"]).max()
            rec["mfma_vs_plain_max_rel_diff"] = float(np.abs(res["mfma"] - res["plain"]).max() / scale)
            rec["mfma_vs_multidot_max_rel_diff"] = float(np.abs(res["mfma"] - res["multidot"]).max() / scale)
            print(json.dumps(rec), flush=True)
    for v in vecs:
        ctx.vec_free(v)
    ctx.close()


def run_compress(n_side, n_mu=128, K=48, rank=12, S=1024):
    from pgdrome_amd import fem, model
    from pgdrome_amd.hip_backend import HipBackend
    be = fem.set_backend(HipBackend(0))
    t0 = time.perf_counter()
    V = fem.FunctionSpace(fem.BoxMesh(fem.Point(0, 0, 0), fem.Point(1, 1, 1), n_side - 1, n_side - 1, n_side - 1), "CG", 1)
    Vp = fem.FunctionSpace(fem.IntervalMesh(n_mu - 1, 0.0, 1.0), "CG", 1)
    t_mesh = time.perf_counter() - t0
    rng = np.random.default_rng(n_side)
    n = V.dim()
    # fixed dimension: `rank` seeded vectors on the device, the K modes are their combinations (pgd_vec_lincomb)
    basis = [be.vec_zeros(n) for _ in range(rank)]
    for h in basis:
        be.vec_upload(h, rng.standard_normal(n))
    A = rng.standard_normal((rank, K))
    big = []
    for k in range(K):
        f = fem.Function(V)
        be.vec_lincomb(f.vector().dev_for_write(), basis, A[:, k])
        f.vector().touched_dev()
        big.append(f)
    for h in basis:
        be.vec_free(h)
    small = []
    P = np.linalg.qr(rng.standard_normal((n_mu, rank)))[0] @ rng.standard_normal((rank, K))
    for k in range(K):
        f = fem.Function(Vp)
        f.vector()._host = np.ascontiguousarray(P[:, k])
        f.vector().touched_host()
        small.append(f)
    # (the constructor would pull every mode's vertex values to the host: the attributes are filled by hand)
    sol = model.PGD(name="bench", n_modes=0, fmeshes=[V.mesh(), Vp.mesh()], pgd_modes=[[], []], name_coord=["x", "mu"])
    sol.numModes = sol.used_numModes = K
    for pm, modes in zip(sol.mesh, (big, small)):
        pm.attributes[0].interpolationfct, pm.attributes[0].n_modes = modes, K
    be.ctx.sync()

    def clock(fn):
        be.ctx.sync()
        t0 = time.perf_counter()
        out = fn()
        be.ctx.sync()
        return out, time.perf_counter() - t0

    sol.mode_gram(0)                                                      # warm-up: workspace, code objects
    Gs, t_gram = clock(lambda: [sol.mode_gram(d) for d in range(2)])
    plan, t_host = clock(lambda: model.compress_grams(Gs, 1e-6))
    _, t_comb = clock(lambda: [sol._combine_modes(W, m, Wd) for W, m, Wd in zip((V, Vp), (big, small), plan["W"])])
    res, t_all = clock(lambda: sol.compress(tol=1e-6))
    coords = rng.uniform(0.0, 1.0, size=(S, 1))
    sol.evaluate_many(0, [1], coords[:64], 0)
    res.evaluate_many(0, [1], coords[:64], 0)
    full, t_full = clock(lambda: sol.evaluate_many(0, [1], coords, 0))
    comp, t_comp = clock(lambda: res.evaluate_many(0, [1], coords, 0))
    rec = {"part": "compress", "n": n_side, "rows": n, "n_mu": n_mu, "modes_in": K, "true_rank": rank, "compression": res.compression,
           "mesh_seconds": t_mesh, "gram_seconds": t_gram, "host_algorithm_seconds": t_host, "recombination_seconds": t_comb,
           "compress_seconds_end_to_end": t_all, "S": S, "evaluate_many_seconds_modes_in": t_full,
           "evaluate_many_seconds_modes_out": t_comp, "evaluate_many_speedup": t_full / t_comp,
           "max_abs_rel_diff": float(np.abs(full.max_abs - comp.max_abs).max() / np.abs(full.max_abs).max()),
           "distance": sol.distance(res)}
    print(json.dumps(rec), flush=True)


def main(argv):
    sizes = [int(a) for a in argv if a.isdigit()] or [128, 256]
    comp = [int(a.split("=")[1]) for a in argv if a.startswith("compress=")] or [256]
    jobs = [("kernel", s) for s in sizes] + [("compress", s) for s in comp if s > 0]
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as out:
        for what, size in jobs:
            cmd = ["timeout", "-k", "10", str(CHILD_LIMIT), sys.executable, os.path.abspath(__file__), "--child", what, str(size)]
            p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
            out.write(p.stdout)
            if p.returncode != 0:
                out.write(json.dumps({"part": what, "n": size, "failed": True, "returncode": p.returncode}) + "\n")
            out.flush()
            sys.stdout.write(p.stdout)
            sys.stdout.flush()
            if p.returncode != 0:          # nothing more is started on a device that a child left in doubt
                return p.returncode
    return 0


if __name__ == "__main__":
    if len(sys.argv) >= 4 and sys.argv[1] == "--child":
        (run_kernel if sys.argv[2] == "kernel" else run_compress)(int(sys.argv[3]))
    else:
        sys.exit(main(sys.argv[1:]))
