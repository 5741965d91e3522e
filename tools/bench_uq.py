"""Quadratic forms of the modes (pgd_quad_forms) on the MI355X: K in {16, 48, 128} seeded normal mode vectors on the n^3 space for
n in {65, 129, 256}, nq in {1, 5, 9} seeded positive semidefinite forms (9 = what variance_decomposition asks for with three
random parameters and order 2, plus the total), fields stored and clamped as the frontend does, three ways in one process,
alternating: the MFMA kernel, the plain fma kernel (PGD_TUNE_QUAD_VARIANT) and pgd_eval_batch (statistics only) on the same
modes at S = nq 16 ceil(K / 16) samples - the same product F Q with nothing done to it.  At 65^3 also the numpy route of
PGD.quadratic_forms on the same data.

    python tools/bench_uq.py [65 129 256]      # writes profiles/uq_bench_n1.jsonl

Every size runs in a child process of its own under a time limit; a size that fails or runs out of time leaves a line that
says so and nothing more is started.  Seconds are host-clock times around whole calls, their device synchronisation and the
layout and upload of the matrices included: the median of 3 rounds after a warm-up round, the ways taking turns inside a round;
"spread" is (max - min) / median of the rounds.  TFLOP/s counts 2 n K^2 nq (the product F Q alone; the nq n K multiplications of
the epilogue are not counted), TB/s counts 8 n (K + nq) bytes - every mode read once, every field written once."""
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "uq_bench_n1.jsonl")
KS = (16, 48, 128)
NQS = (1, 5, 9)
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


def numpy_route(F, Q, row_chunk=8192):
    """What PGD.quadratic_forms does below DEVICE_EVAL_MIN_DOFS (model.py), on arrays."""
    out = np.empty((Q.shape[0], F.shape[0]))
    for r0 in range(0, F.shape[0], row_chunk):
        Fc = F[r0:r0 + row_chunk]
        for q in range(Q.shape[0]):
            out[q, r0:r0 + Fc.shape[0]] = np.maximum(np.einsum("ik,ik->i", Fc @ Q[q].T, Fc), 0.0)
    return out


def run_size(n_side):
    from pgdrome_amd import _lib
    ctx = _lib.Context(0)
    n = n_side ** 3
    kmax, qmax = max(KS), max(NQS)
    rng = np.random.default_rng(n_side)
    base = rng.standard_normal(n + 16 * kmax)
    vecs = [ctx.vec_from(base[16 * k:16 * k + n]) for k in range(kmax)]             # shifted windows: distinct, cheap to make
    outs = [ctx.vec_from(np.zeros(n)) for _ in range(qmax)]
    for K in KS:
        modes = vecs[:K]
        for nq in NQS:
            A = rng.standard_normal((nq, K, K))
            Q = A @ A.transpose(0, 2, 1) / K
            S = nq * 16 * ((K + 15) // 16)
            Cs = rng.standard_normal((K, S))
            res = {}

            def quad(variant, key):
                ctx.tune(_lib.TUNE_QUAD_VARIANT, variant)
                res[key] = ctx.quad_forms(modes, Q, outs[:nq], clamp=True)
                ctx.tune(_lib.TUNE_QUAD_VARIANT, 1)

            ways = {"mfma": lambda: quad(1, "mfma"), "plain": lambda: quad(0, "plain"),
                    "eval_batch": lambda: ctx.eval_batch(modes, Cs, stats=True)}
            if n_side <= 65:
                F = np.stack([base[16 * k:16 * k + n] for k in range(K)], axis=1)
                ways["numpy"] = lambda: res.__setitem__("numpy", numpy_route(F, Q))
            t = rounds(ctx, ways)
            flop, nbytes = 2.0 * n * K * K * nq, 8.0 * n * (K + nq)
            rec = {"part": "quad_forms", "n": n_side, "rows": n, "K": K, "nq": nq, "flop": flop, "bytes": nbytes, "eval_batch_S": S,
                   "eval_batch_flop": 2.0 * n * K * S}
            for name, (sec, spread) in t.items():
                rec[name + "_ms"] = 1e3 * sec
                rec[name + "_spread"] = spread
                rec[name + "_TFLOPs"] = (rec["eval_batch_flop"] if name == "eval_batch" else flop) / sec / 1e12
                if name != "eval_batch":
                    rec[name + "_TBps"] = nbytes / sec / 1e12
            rec["plain_over_mfma"] = t["plain"][0] / t["mfma"][0]
            rec["eval_batch_over_mfma"] = t["eval_batch"][0] / t["mfma"][0]
            if "numpy" in t:
                rec["numpy_over_mfma"] = t["numpy"][0] / t["mfma"][0]
            scale = max(np.abs(res["plain"][1]).max(), 1e-300)
            rec["mfma_vs_plain_max_rel_diff_of_extrema"] = float(max(np.abs(res["mfma"][i] - res["plain"][i]).max() for i in (0, 1)) / scale)
            if "numpy" in res:
                rec["mfma_vs_numpy_max_rel_diff_of_maxima"] = float(np.abs(res["mfma"][1] - res["numpy"].max(axis=1)).max() / scale)
            print(json.dumps(rec), flush=True)
    for v in vecs + outs:
        ctx.vec_free(v)
    ctx.close()


def main(argv):
    sizes = [int(a) for a in argv if a.isdigit()] or [65, 129, 256]
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as out:
        for size in sizes:
            cmd = ["timeout", "-k", "10", str(CHILD_LIMIT), sys.executable, os.path.abspath(__file__), "--child", str(size)]
            p = subprocess.Popen(cmd, stdout=subprocess.PIPE, text=True)
            for line in p.stdout:          # a record as soon as its shape is measured
                out.write(line)
                out.flush()
                sys.stdout.write(line)
                sys.stdout.flush()
            if p.wait() != 0:              # nothing more is started on a device that a child left in doubt
                out.write(json.dumps({"part": "quad_forms", "n": size, "failed": True, "returncode": p.returncode}) + "\n")
                return p.returncode
    return 0


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "--child":
        run_size(int(sys.argv[2]))
    else:
        sys.exit(main(sys.argv[1:]))
