"""Posteriors for a stream of data sets (pgd_grid_posterior_many) on the MI355X: K = 48 seeded synthetic modes, 100 sensor entries
(reduced to 48 rows by the thin QR, as PGD.sensor_posterior_many does), three parameter dimensions on grids of 64^3 and 128^3
samples, N = 64, 1024 and 4096 data sets (the same state, fresh noise per data set).  Four ways in one process, alternating:

  * mfma:        the call with the chained matrix-unit kernel, PGD_POST_THETA, skip of underflowed tiles on (the defaults);
  * mfma_noskip: the same with PGD_TUNE_POSTMANY_SKIP = 0;
  * plain:       the same call with PGD_TUNE_POSTMANY_VARIANT = 0.  Above ``PLAIN_WORK`` = N S it is timed on the first
                 ``PLAIN_SUBSET`` data sets and extrapolated linearly in N ("plain_extrapolated": true);
  * parent:      what the parent commit offers: one pgd_grid_misfit + pgd_grid_posterior(PGD_POST_THETA) per data set on a fresh
                 vector, the device calls of sensor_posterior(outputs=("theta",)).  It is timed on the first min(N, 32) data sets and
                 EXTRAPOLATED linearly to N ("parent_extrapolated": true; "parent_ms" is the extrapolation, "parent_subset_ms" what
                 was measured).

    python tools/bench_posterior_many.py [64 128] [--n 64 1024 4096]      # writes profiles/posterior_many_bench_n1.jsonl

Every case runs in a child process of its own under a time limit; a case that fails or runs out of time leaves a line that says so
and nothing more is started.  Seconds are host-clock times around whole calls, the layout and upload of the tables and data and the
device synchronisations included: the median of 3 rounds after a warm-up round, the ways taking turns inside a round; "spread" is
(max - min) / median of the rounds.  TFLOP/s counts 2 m N S (the second product alone, m = 48 rows), per pass of which there are
two; "exp_per_s" is N S / seconds, the exponentials a call without skipping evaluates."""
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "posterior_many_bench_n1.jsonl")
K, SENSORS = 48, 100
PARENT_SUBSET = 32
PLAIN_WORK = 1 << 31
PLAIN_SUBSET = 256
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


def run_case(grid, N):
    from pgdrome_amd import _lib
    ctx = _lib.Context(0)
    rng = np.random.default_rng(48)
    phi = rng.standard_normal((SENSORS, K)) / np.sqrt(K)
    n = [grid] * 3
    tables = [1.0 + 0.3 * rng.standard_normal((K, v)) for v in n]
    absc = [np.linspace(0.0, 1.0, v) for v in n]
    weights = [np.full(v, 1.0 / v) for v in n]
    S = int(np.prod(n, dtype=np.int64))
    c = np.ones(K)
    for t in tables:
        c = c * t[:, t.shape[1] // 3]
    Y = (phi @ c)[None, :] + 0.1 * rng.standard_normal((N, SENSORS))
    Q, Rm = np.linalg.qr(phi)
    a, Z = np.ascontiguousarray(Rm), np.ascontiguousarray(Y @ Q)
    alpha, beta = np.ones(N), np.einsum("np,np->n", Z, Z)
    res = {}

    def many(key, variant, skip, rows):
        ctx.tune(_lib.TUNE_POSTMANY_VARIANT, variant)
        ctx.tune(_lib.TUNE_POSTMANY_SKIP, skip)
        res[key] = ctx.grid_posterior_many(a, Z[:rows], alpha[:rows], beta[:rows], tables, weights, abscissae=absc, want=_lib.POST_THETA)
        ctx.tune(_lib.TUNE_POSTMANY_VARIANT, 1)
        ctx.tune(_lib.TUNE_POSTMANY_SKIP, 1)

    def parent(rows):
        out = []
        for j in range(rows):
            h = ctx.vec_alloc(S)
            cmin, arg = ctx.grid_misfit(a, Z[j], tables, h)
            out.append((cmin, arg, ctx.grid_posterior(h, cmin, n, weights, abscissae=absc, want=_lib.POST_THETA)))
            ctx.vec_free(h)
        res["parent"] = out

    nplain = N if N * S <= PLAIN_WORK else min(N, PLAIN_SUBSET)
    npar = min(N, PARENT_SUBSET)
    ways = {"mfma": lambda: many("mfma", 1, 1, N), "mfma_noskip": lambda: many("mfma_noskip", 1, 0, N),
            "plain_subset": lambda: many("plain", 0, 1, nplain), "parent_subset": lambda: parent(npar)}
    t = rounds(ctx, ways)
    rec = {"part": "posterior_many", "grid": grid, "n": n, "S": S, "N": N, "K": K, "sensor_entries": SENSORS, "rows": a.shape[0],
           "product_flop": 2.0 * a.shape[0] * N * S, "plain_subset": nplain, "plain_extrapolated": nplain < N, "parent_subset": npar,
           "parent_extrapolated": npar < N}
    for key, (sec, spread) in t.items():
        rec[key + "_ms"] = 1e3 * sec
        rec[key + "_spread"] = spread
    rec["plain_ms"] = rec["plain_subset_ms"] * N / nplain
    rec["parent_ms"] = rec["parent_subset_ms"] * N / npar
    for v in ("mfma", "mfma_noskip", "plain"):
        rec[v + "_TFLOPs"] = rec["product_flop"] / (rec[v + "_ms"] * 1e-3) / 1e12
    rec["exp_per_s_noskip"] = N * S / (rec["mfma_noskip_ms"] * 1e-3)
    rec["noskip_over_skip"] = rec["mfma_noskip_ms"] / rec["mfma_ms"]
    rec["plain_over_mfma"] = rec["plain_ms"] / rec["mfma_ms"]
    rec["parent_over_mfma"] = rec["parent_ms"] / rec["mfma_ms"]
    rec["mfma_ms_per_data_set"] = rec["mfma_ms"] / N
    rec["skip_changes_no_bit"] = all(np.array_equal(res["mfma"][key], res["mfma_noskip"][key]) for key in res["mfma"])
    rec["argmin_equal_to_plain"] = bool(np.array_equal(res["mfma"]["argmin"][:nplain], res["plain"]["argmin"]))
    rec["mfma_vs_plain_max_rel_diff_of_Z"] = float(np.abs(res["mfma"]["Z"][:nplain] / res["plain"]["Z"] - 1.0).max())
    # the parent's numbers are relative to the minimum of the difference form: compare what does not depend on the shift
    zm = np.array([p[2]["theta1"] / p[2]["Z"] for p in res["parent"]])
    rec["mean_vs_parent_max_abs_diff"] = float(np.abs(res["mfma"]["theta1"][:npar] / res["mfma"]["Z"][:npar, None] - zm).max())
    rec["argmin_equal_to_parent"] = all(int(res["mfma"]["argmin"][j]) == p[1] for j, p in enumerate(res["parent"]))
    print(json.dumps(rec), flush=True)
    ctx.close()


def main(argv):
    grids = [a for a in argv[:argv.index("--n")] if a.isdigit()] if "--n" in argv else [a for a in argv if a.isdigit()]
    counts = [a for a in argv[argv.index("--n") + 1:] if a.isdigit()] if "--n" in argv else []
    grids, counts = grids or ["64", "128"], counts or ["64", "1024", "4096"]
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "a" if "--append" in argv else "w") as out:
        for grid in grids:
            for N in counts:
                cmd = ["timeout", "-k", "10", str(CHILD_LIMIT), sys.executable, os.path.abspath(__file__), "--child", grid, N]
                p = subprocess.Popen(cmd, stdout=subprocess.PIPE, text=True)
                for line in p.stdout:
                    out.write(line)
                    out.flush()
                    sys.stdout.write(line)
                    sys.stdout.flush()
                if p.wait() != 0:              # nothing more is started on a device that a child left in doubt
                    out.write(json.dumps({"part": "posterior_many", "grid": int(grid), "N": int(N), "failed": True, "returncode": p.returncode}) + "\n")
                    return p.returncode
    return 0


if __name__ == "__main__":
    if len(sys.argv) >= 4 and sys.argv[1] == "--child":
        run_case(int(sys.argv[2]), int(sys.argv[3]))
    else:
        sys.exit(main(sys.argv[1:]))
