"""Greedy sensor placement (pgd_design_update + pgd_design_gains) on the MI355X: K = 48 seeded synthetic modes, three parameter
dimensions on grids of 64^3 and 128^3 samples, M = 10^3, 10^4 and 10^5 candidates of R = 1 and R = 3 rows, n_select = 8 greedy steps
(a reset, then per step the gains of all candidates, the argmax and the update with the chosen rows - what PGD.sensor_placement does
on the device).  Three ways, alternating in one process:

  * mfma:  the whole greedy call with the matrix-unit kernel (the default);
  * plain: the same with PGD_TUNE_DESIGN_VARIANT = 0.  Above ``PLAIN_WORK`` = M R S it is timed on the first ``plain_subset`` candidates
           and extrapolated linearly in M ("plain_extrapolated": true);
  * numpy: the numpy route (model.design_update_numpy / design_gains_numpy), the only route of the parent commit, ONE greedy step on the
           first ``numpy_candidates`` candidates and the first ``numpy_samples`` samples (the first abscissae of the slowest dimension),
           one round, EXTRAPOLATED linearly in both to M candidates, S samples and 8 steps ("numpy_extrapolated": true).

    python tools/bench_placement.py [64 128] [--m 1000 10000 100000] [--r 1 3]      # writes profiles/placement_bench_n1.jsonl
    python tools/bench_placement.py --crossover                                     # writes profiles/placement_crossover_n1.jsonl:
                                                  # grids of 4^3 .. 32^3 samples, M = 16 / 128 / 1024: both routes in full, for the threshold

Every case runs in a child process of its own under a time limit; a case that fails or runs out of time leaves a line that says so
and nothing more is started.  Seconds are host-clock times around whole calls, the layout and upload of the tables and rows, the
downloads and the device synchronisations included: the median of 3 rounds after a warm-up round, the ways taking turns inside a
round; "spread" is (max - min) / median of the rounds.  Per step: milliseconds = the call / 8; TFLOP/s counts 2 M R K S ndim per step
against the time inside pgd_design_gains alone ("gains_ms_per_step") and against the whole step."""
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "placement_bench_n1.jsonl")
K, NDIM, N_SELECT = 48, 3, 8
PLAIN_WORK = 1 << 32
NUMPY_CANDIDATES = 1000
CHILD_LIMIT = 560           # seconds per child process


def greedy(update, gains_of, a, M, R, h0, n_select, clock=None):
    """The loop of PGD.sensor_placement on the callables of a route; ``clock``: accumulates the seconds inside gains_of."""
    taken = np.zeros(M, dtype=bool)
    sel, gs, lds = [], [], [update(h0=h0)[0]]
    for _ in range(n_select):
        t0 = time.perf_counter()
        g = gains_of(a)
        if clock is not None:
            clock[0] += time.perf_counter() - t0
        j = int(np.argmax(np.where(taken[:g.size], -np.inf, g)))
        taken[j] = True
        sel.append(j), gs.append(g[j])
        lds.append(update(rows=a[j * R:(j + 1) * R])[0])
    return sel, np.array(gs), np.array(lds)


def run_case(grid, M, R):
    from pgdrome_amd import _lib, model
    ctx = _lib.Context(0)
    rng = np.random.default_rng(48)
    n = [grid] * NDIM
    S = int(np.prod(n, dtype=np.int64))
    tables = [1.0 + 0.3 * rng.standard_normal((K, v)) for v in n]
    dtables = [rng.standard_normal((K, v)) for v in n]
    weights = [np.full(v, 1.0 / v) for v in n]
    a = np.ascontiguousarray(rng.standard_normal((M * R, K)) / np.sqrt(K) * np.repeat(rng.uniform(0.3, 3.0, M), R)[:, None])
    h0 = 3.0 * np.eye(NDIM)
    res, inside = {}, {"mfma": [0.0], "plain": [0.0]}

    def device(key, variant, rows):
        ctx.tune(_lib.TUNE_DESIGN_VARIANT, variant)
        state = ctx.design_state(n)
        try:
            inside[key][0] = 0.0
            res[key] = greedy(lambda **kw: ctx.design_update(state, tables, dtables, weights, **kw),
                              lambda x: ctx.design_gains(x[:rows * R], R, state, tables, dtables, weights), a, M, R, h0, N_SELECT, inside[key])
        finally:
            ctx.vec_free(state)
            ctx.tune(_lib.TUNE_DESIGN_VARIANT, 1)

    nplain = M if M * R * S <= PLAIN_WORK else max(min(M, PLAIN_WORK // (R * S)) // 256 * 256, 256)
    ways = {"mfma": lambda: device("mfma", 1, M), "plain_subset": lambda: device("plain", 0, nplain)}
    for fn in ways.values():
        fn()
    ctx.sync()
    t = {name: [] for name in ways}
    tin = {name: [] for name in ways}
    for _ in range(3):
        for name, fn in ways.items():
            ctx.sync()
            t0 = time.perf_counter()
            fn()
            ctx.sync()
            t[name].append(time.perf_counter() - t0)
            tin[name].append(inside["mfma" if name == "mfma" else "plain"][0])
    flop = 2.0 * M * R * K * S * NDIM
    rec = {"part": "placement", "grid": grid, "n": n, "S": S, "M": M, "R": R, "K": K, "ndim": NDIM, "n_select": N_SELECT, "flop_per_step": flop,
           "plain_subset": nplain, "plain_extrapolated": nplain < M}
    for name in ways:
        med = statistics.median(t[name])
        rec[name + "_call_ms"] = 1e3 * med
        rec[name + "_spread"] = (max(t[name]) - min(t[name])) / med
        rec[name + "_gains_ms_per_step"] = 1e3 * statistics.median(tin[name]) / N_SELECT
    rec["mfma_ms_per_step"] = rec["mfma_call_ms"] / N_SELECT
    rec["mfma_TFLOPs_step"] = flop / (rec["mfma_ms_per_step"] * 1e-3) / 1e12
    rec["mfma_TFLOPs_gains"] = flop / (rec["mfma_gains_ms_per_step"] * 1e-3) / 1e12
    rec["plain_gains_ms_per_step"] = rec["plain_subset_gains_ms_per_step"] * M / nplain
    rec["plain_over_mfma_gains"] = rec["plain_gains_ms_per_step"] / rec["mfma_gains_ms_per_step"]
    rec["update_ms_per_step"] = (rec["mfma_call_ms"] - N_SELECT * rec["mfma_gains_ms_per_step"]) / (N_SELECT + 1)
    if nplain == M:
        rec["same_selection_as_plain"] = res["mfma"][0] == res["plain"][0]
        rec["mfma_vs_plain_max_rel_diff_of_gains"] = float(np.abs(res["mfma"][1] / res["plain"][1] - 1.0).max())
    # ---- the numpy route on a stated subset, one step, one round
    nm, n0 = min(M, NUMPY_CANDIDATES), 2
    sub_t, sub_d, sub_w = [tables[0][:, :n0]] + tables[1:], [dtables[0][:, :n0]] + dtables[1:], [weights[0][:n0]] + weights[1:]
    st = model.design_state_numpy([n0] + n[1:])
    t0 = time.perf_counter()
    model.design_update_numpy(st, sub_t, sub_d, sub_w, h0=h0)
    g = model.design_gains_numpy(a[:nm * R], R, st, sub_t, sub_d, sub_w)
    model.design_update_numpy(st, sub_t, sub_d, sub_w, rows=a[:R])
    sec = time.perf_counter() - t0
    rec.update(numpy_candidates=nm, numpy_samples=n0 * n[1] * n[2], numpy_extrapolated=True, numpy_subset_step_ms=1e3 * sec,
               numpy_ms_per_step=1e3 * sec * (M / nm) * (n[0] / n0))
    rec["numpy_over_mfma_step"] = rec["numpy_ms_per_step"] / rec["mfma_ms_per_step"]
    rec["selected"] = res["mfma"][0]
    print(json.dumps(rec), flush=True)
    ctx.close()


def run_crossover():
    """Small problems, whole 8-step greedy calls on both routes in full: where the device call overtakes the numpy route."""
    from pgdrome_amd import _lib, model
    ctx = _lib.Context(0)
    rng = np.random.default_rng(3)
    h0 = 3.0 * np.eye(NDIM)
    for grid in (4, 8, 16, 32):
        for M in (16, 128, 1024):
            for R in (1, 3):
                n, S = [grid] * NDIM, grid ** NDIM
                tables = [1.0 + 0.3 * rng.standard_normal((K, v)) for v in n]
                dtables = [rng.standard_normal((K, v)) for v in n]
                weights = [np.full(v, 1.0 / v) for v in n]
                a = np.ascontiguousarray(rng.standard_normal((M * R, K)) / np.sqrt(K))

                def dev():
                    state = ctx.design_state(n)
                    try:
                        return greedy(lambda **kw: ctx.design_update(state, tables, dtables, weights, **kw),
                                      lambda x: ctx.design_gains(x, R, state, tables, dtables, weights), a, M, R, h0, N_SELECT)
                    finally:
                        ctx.vec_free(state)

                def host():
                    st = model.design_state_numpy(n)
                    return greedy(lambda **kw: model.design_update_numpy(st, tables, dtables, weights, **kw),
                                  lambda x: model.design_gains_numpy(x, R, st, tables, dtables, weights), a, M, R, h0, N_SELECT)

                rec = {"part": "placement_crossover", "grid": grid, "S": S, "M": M, "R": R, "MS": M * S}
                sel = {}
                for name, fn in (("device", dev), ("numpy", host)):
                    if name == "numpy" and M * S * R > 3e7:          # (seconds per call: far beyond any crossover)
                        continue
                    fn()
                    ts = []
                    for _ in range(3):
                        t0 = time.perf_counter()
                        sel[name] = fn()[0]
                        ts.append(time.perf_counter() - t0)
                    rec[name + "_call_ms"] = 1e3 * statistics.median(ts)
                if "numpy" in sel:
                    rec["same_selection"] = sel["device"] == sel["numpy"]
                print(json.dumps(rec), flush=True)
    ctx.close()


def main(argv):
    if "--crossover" in argv:
        cmd = ["timeout", "-k", "10", str(CHILD_LIMIT), sys.executable, os.path.abspath(__file__), "--child-crossover"]
        with open(os.path.join(ROOT, "profiles", "placement_crossover_n1.jsonl"), "w") as out:
            p = subprocess.Popen(cmd, stdout=subprocess.PIPE, text=True)
            for line in p.stdout:
                out.write(line)
                sys.stdout.write(line)
            return p.wait()

    def take(flag):
        if flag not in argv:
            return []
        out = []
        for v in argv[argv.index(flag) + 1:]:
            if not v.isdigit():
                break
            out.append(v)
        return out
    first = min([argv.index(f) for f in ("--m", "--r") if f in argv] + [len(argv)])
    grids = [v for v in argv[:first] if v.isdigit()] or ["64", "128"]
    counts, rs = take("--m") or ["1000", "10000", "100000"], take("--r") or ["1", "3"]
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "a" if "--append" in argv else "w") as out:
        for grid in grids:
            for M in counts:
                for R in rs:
                    cmd = ["timeout", "-k", "10", str(CHILD_LIMIT), sys.executable, os.path.abspath(__file__), "--child", grid, M, R]
                    p = subprocess.Popen(cmd, stdout=subprocess.PIPE, text=True)
                    for line in p.stdout:
                        out.write(line)
                        out.flush()
                        sys.stdout.write(line)
                        sys.stdout.flush()
                    if p.wait() != 0:              # nothing more is started on a device that a child left in doubt
                        out.write(json.dumps({"part": "placement", "grid": int(grid), "M": int(M), "R": int(R), "failed": True,
                                              "returncode": p.returncode}) + "\n")
                        return p.returncode
    return 0


if __name__ == "__main__":
    if len(sys.argv) >= 5 and sys.argv[1] == "--child":
        run_case(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]))
    elif len(sys.argv) >= 2 and sys.argv[1] == "--child-crossover":
        run_crossover()
    else:
        sys.exit(main(sys.argv[1:]))
