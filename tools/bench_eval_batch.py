"""Batched online evaluation (pgd_eval_batch) on the MI355X: K = 48 seeded random mode vectors on the n^3 P1 space for every n
given, S in {64, 256, 1024} samples, (a) per-sample statistics + envelopes and (b) statistics only, for the MFMA kernel and the
plain fma kernel (PGD_TUNE_EVAL_VARIANT), and - in the same run, on the same modes - S calls of pgd_vec_lincomb: the per-sample
kernel PGD.evaluate uses, which forms no statistic at all.

    python tools/bench_eval_batch.py [n=128 256 ...] > profiles/eval_batch_bench_n1.jsonl

One JSON line per n, S and output set.  Seconds are host-clock times around calls that end in a device synchronisation, the
smallest of the repetitions after a warm-up call of the same shape (windows of at least 0.25 s: short calls are repeated inside
the window); FLOP/s = 2 n K S over those seconds - the whole call (upload of the coefficients, kernel, final pass, download of
the statistics), not the kernel alone."""
import json
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pgdrome_amd import _lib               # noqa: E402

K = 48
SAMPLES = (64, 256, 1024)


def timed(ctx, fn, reps):
    """Smallest seconds per call over `reps` windows of at least 0.25 s each, after one warm-up call."""
    fn()
    ctx.sync()
    t0 = time.perf_counter()
    fn()
    ctx.sync()
    t1 = time.perf_counter() - t0
    inner = max(1, min(50, int(math.ceil(0.25 / max(t1, 1e-6)))))
    best = t1
    for _ in range(reps):
        ctx.sync()
        t0 = time.perf_counter()
        for _i in range(inner):
            fn()
        ctx.sync()
        best = min(best, (time.perf_counter() - t0) / inner)
    return best


def run(n_side):
    ctx = _lib.Context(0)
    n = n_side ** 3
    rng = np.random.default_rng(n_side)
    modes = [ctx.vec_from(rng.standard_normal(n)) for _ in range(K)]
    emn, emx, y = ctx.vec_alloc(n), ctx.vec_alloc(n), ctx.vec_alloc(n)
    for S in SAMPLES:
        Cm = np.random.default_rng(S).standard_normal((K, S))
        flop = 2.0 * n * K * S
        # the parent's way: one lincomb per sample (8 (K + ceil(K / 8)) n bytes each, no statistics)
        cols = [np.ascontiguousarray(Cm[:, j]) for j in range(S)]
        for j in range(2):
            ctx.vec_lincomb(y, modes, cols[j])
        ctx.sync()
        t0 = time.perf_counter()
        for j in range(S):
            ctx.vec_lincomb(y, modes, cols[j])
        ctx.sync()
        t_lin = time.perf_counter() - t0
        for outputs in ("stats+envelope", "stats"):
            kw = {"env_min": emn, "env_max": emx} if outputs == "stats+envelope" else {}
            rec = {"part": "eval_batch", "n": n_side, "rows": n, "K": K, "S": S, "outputs": outputs, "flop": flop,
                   "lincomb_S_calls_seconds": t_lin, "lincomb_seconds_per_sample": t_lin / S}
            stats = {}
            for name, variant in (("mfma", 1), ("plain", 0)):
                ctx.tune(_lib.TUNE_EVAL_VARIANT, variant)
                t = timed(ctx, lambda: stats.__setitem__(name, ctx.eval_batch(modes, Cm, stats=True, **kw)),
                          reps=3 if flop < 5e11 else 2)
                rec[name + "_seconds"] = t
                rec[name + "_flops"] = flop / t
            ctx.tune(_lib.TUNE_EVAL_VARIANT, 1)
            # the two variants differ by rounding only: largest difference of a statistic over the largest statistic
            rec["variants_max_rel_diff"] = float(np.abs(stats["mfma"] - stats["plain"]).max() / np.abs(stats["plain"]).max())
            rec["mfma_over_plain"] = rec["plain_seconds"] / rec["mfma_seconds"]
            rec["lincomb_over_mfma"] = t_lin / rec["mfma_seconds"]
            print(json.dumps(rec), flush=True)
    for v in modes + [emn, emx, y]:
        ctx.vec_free(v)
    ctx.close()


if __name__ == "__main__":
    for size in [int(a) for a in sys.argv[1:]] or [128, 256]:
        run(size)
