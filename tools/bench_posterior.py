"""Grid posterior from sensor data (pgd_grid_misfit + pgd_grid_posterior) on the MI355X: K = 48 seeded synthetic modes, 100 sensor
entries (reduced to 48 rows by the thin QR, as PGD.sensor_posterior does), three parameter dimensions on grids of 64^3, 128^3 and
256^3 samples, and one scattered case of S = 2^20 samples (one dimension whose table is the 48 x S coefficient matrix).  Three ways
in one process, alternating:

  * mfma:   both calls with the matrix-unit kernels (all outputs: marginals, parameter moments, coefficient moments);
  * plain:  the same calls with PGD_TUNE_MISFIT_VARIANT = PGD_TUNE_POST_VARIANT = 0;
  * parent: the route that exists without these calls - the arithmetic of evaluate_sensor_response_many in chunks of 4096 samples
    (mode_factors_many's gather and product of the 1-D tables, the contraction with the sampled modes: numpy below
    DEVICE_EVAL_MIN_DOFS entries per sample) plus the misfit, the weights and the same sums in numpy.  It is timed on the FIRST
    ``PARENT_SUBSET`` samples only and extrapolated linearly to S ("parent_extrapolated": true; "parent_ms" is the extrapolation,
    "parent_subset_ms" what was measured).  The 1-D interpolation of the modes at the abscissae is left out of it: it works on the
    same tables as the other two.

    python tools/bench_posterior.py [64 128 256 scattered]      # writes profiles/posterior_bench_n1.jsonl

Every case runs in a child process of its own under a time limit; a case that fails or runs out of time leaves a line that says so
and nothing more is started.  Seconds are host-clock times around whole calls, the layout and upload of the tables and the
device synchronisation included: the median of 3 rounds after a warm-up round, the ways taking turns inside a round; "spread" is
(max - min) / median of the rounds.  TFLOP/s counts 2 m k S with the m = 48 rows the kernel sees, for the misfit call and (2 k k S)
for the coefficient moments; the two calls are also timed apart."""
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "posterior_bench_n1.jsonl")
K, SENSORS = 48, 100
PARENT_SUBSET = 1 << 16
PARENT_CHUNK = 4096
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


def parent_route(phi, y, tables, weights, absc, nsub):
    """The sums of the posterior over the first nsub samples the way the parent commit allows: coefficients, sensor values and
    misfits in numpy, PARENT_CHUNK samples at a time (two passes: the minimum first, as the shift)."""
    n = [t.shape[1] for t in tables]
    chi2 = np.empty(nsub)
    for s0 in range(0, nsub, PARENT_CHUNK):
        idx = np.unravel_index(np.arange(s0, min(nsub, s0 + PARENT_CHUNK)), n)
        C = np.ones((tables[0].shape[0], idx[0].size))
        for d, t in enumerate(tables):
            C *= t[:, idx[d]]
        U = C.T @ phi.T                                     # SensorModes.contract: (S, m) values
        r = U - y[None, :]
        chi2[s0:s0 + idx[0].size] = np.einsum("sp,sp->s", r, r)
    shift = chi2.min()
    Z, M = 0.0, np.zeros((tables[0].shape[0],) * 2)
    marg = [np.zeros(v) for v in n]
    for s0 in range(0, nsub, PARENT_CHUNK):
        idx = np.unravel_index(np.arange(s0, min(nsub, s0 + PARENT_CHUNK)), n)
        C = np.ones((tables[0].shape[0], idx[0].size))
        w = np.ones(idx[0].size)
        for d, t in enumerate(tables):
            C *= t[:, idx[d]]
            w *= weights[d][idx[d]]
        e = w * np.exp(-0.5 * (chi2[s0:s0 + idx[0].size] - shift))
        Z += e.sum()
        M += (C * e) @ C.T
        for d in range(len(n)):
            marg[d] += np.bincount(idx[d], weights=e, minlength=n[d])
    return Z, M, marg


def run_case(name):
    from pgdrome_amd import _lib
    ctx = _lib.Context(0)
    rng = np.random.default_rng(48)
    phi = rng.standard_normal((SENSORS, K)) / np.sqrt(K)
    if name == "scattered":
        n = [1 << 20]
        tables = [1.0 + 0.3 * rng.standard_normal((K, n[0]))]
        weights, absc, want = [np.full(n[0], 1.0 / n[0])], None, _lib.POST_COEF
    else:
        n = [int(name)] * 3
        tables = [1.0 + 0.3 * rng.standard_normal((K, v)) for v in n]
        absc = [np.linspace(0.0, 1.0, v) for v in n]
        weights = [np.full(v, 1.0 / v) for v in n]
        want = _lib.POST_MARGINALS | _lib.POST_THETA | _lib.POST_COEF
    S = int(np.prod(n, dtype=np.int64))
    c = np.ones(K)
    for t in tables:
        c = c * t[:, t.shape[1] // 3]
    y = phi @ c + 0.1 * rng.standard_normal(SENSORS)
    Q, Rm = np.linalg.qr(phi)
    a, z = np.ascontiguousarray(Rm), Q.T @ y
    h = ctx.vec_alloc(S)
    res = {}

    def device(variant, key, part="both"):
        ctx.tune(_lib.TUNE_MISFIT_VARIANT, variant)
        ctx.tune(_lib.TUNE_POST_VARIANT, variant)
        if part != "posterior":
            res[key + "_min"] = ctx.grid_misfit(a, z, tables, h)
        if part != "misfit":
            res[key] = ctx.grid_posterior(h, res[key + "_min"][0], n, weights, tables=tables, abscissae=absc, want=want)
        ctx.tune(_lib.TUNE_MISFIT_VARIANT, 1)
        ctx.tune(_lib.TUNE_POST_VARIANT, 1)

    nsub = min(S, PARENT_SUBSET)
    ways = {"mfma": lambda: device(1, "mfma"), "plain": lambda: device(0, "plain"),
            "mfma_misfit": lambda: device(1, "mfma", "misfit"), "plain_misfit": lambda: device(0, "plain", "misfit"),
            "mfma_posterior": lambda: device(1, "mfma", "posterior"), "plain_posterior": lambda: device(0, "plain", "posterior"),
            "parent_subset": lambda: res.__setitem__("parent", parent_route(phi, y, tables, weights, absc, nsub))}
    t = rounds(ctx, ways)
    rec = {"part": "posterior", "case": name, "n": n, "S": S, "K": K, "sensor_entries": SENSORS, "rows": a.shape[0], "want": want,
           "misfit_flop": 2.0 * a.shape[0] * K * S, "coef_flop": 2.0 * K * K * S, "parent_subset": nsub, "parent_extrapolated": nsub < S}
    for key, (sec, spread) in t.items():
        rec[key + "_ms"] = 1e3 * sec
        rec[key + "_spread"] = spread
    for v in ("mfma", "plain"):
        rec[v + "_misfit_TFLOPs"] = rec["misfit_flop"] / t[v + "_misfit"][0] / 1e12
        rec[v + "_posterior_TFLOPs"] = rec["coef_flop"] / t[v + "_posterior"][0] / 1e12
    rec["parent_ms"] = rec["parent_subset_ms"] * S / nsub
    rec["plain_over_mfma"] = t["plain"][0] / t["mfma"][0]
    rec["plain_over_mfma_misfit"] = t["plain_misfit"][0] / t["mfma_misfit"][0]
    rec["plain_over_mfma_posterior"] = t["plain_posterior"][0] / t["mfma_posterior"][0]
    rec["parent_over_mfma"] = rec["parent_ms"] / rec["mfma_ms"]
    rec["mfma_vs_plain_rel_diff_of_Z"] = abs(res["mfma"]["Z"] - res["plain"]["Z"]) / res["plain"]["Z"]
    rec["mfma_vs_plain_max_rel_diff_of_coef2"] = float(np.abs(res["mfma"]["coef2"] - res["plain"]["coef2"]).max() / np.abs(res["plain"]["coef2"]).max())
    rec["argmin_equal"] = res["mfma_min"][1] == res["plain_min"][1]
    print(json.dumps(rec), flush=True)
    ctx.vec_free(h)
    ctx.close()


def main(argv):
    cases = [a for a in argv if a.isdigit() or a == "scattered"] or ["64", "128", "256", "scattered"]
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as out:
        for case in cases:
            cmd = ["timeout", "-k", "10", str(CHILD_LIMIT), sys.executable, os.path.abspath(__file__), "--child", case]
            p = subprocess.Popen(cmd, stdout=subprocess.PIPE, text=True)
            for line in p.stdout:
                out.write(line)
                out.flush()
                sys.stdout.write(line)
                sys.stdout.flush()
            if p.wait() != 0:              # nothing more is started on a device that a child left in doubt
                out.write(json.dumps({"part": "posterior", "case": case, "failed": True, "returncode": p.returncode}) + "\n")
                return p.returncode
    return 0


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "--child":
        run_case(sys.argv[2])
    else:
        sys.exit(main(sys.argv[1:]))
