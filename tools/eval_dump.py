"""Run pgd_eval_batch and pgd_eval_batch_norm through the C ABI on fixed seeded cases and dump every output, for comparing two
builds of the library bit by bit:

    python tools/eval_dump.py run OUT.npz [--tree DIR]      # DIR: the checkout whose pgdrome_amd is loaded (default: this one)
    python tools/eval_dump.py compare A.npz B.npz

The cases: the floating-point cases of tests/test_eval_many_gpu.py (n = 1541, K = 50, S = 100, threshold 0.25) and of
tests/test_eval_gradient_gpu.py (m = 1541, q = 6, K = 50, S = 100, threshold 7.0), and for the norms shapes of that file's SHAPES
that make the launcher take each of its five choices (64, 32, 16 rows staged, 16 rows in more than 64 KiB, 16 rows from global
memory), with normal data.  Every case runs with both variants (PGD_TUNE_EVAL_VARIANT), sample chunks 0 (the default), 16, 48
and grid caps 0 (none), 2, and asks for all four outputs; statistics, envelopes, counts, fields and - for the norms - the
launcher's choice are stored.  Needs a GPU."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (m, q, K, S) of tests/test_eval_gradient_gpu.py::SHAPES and the (rows, staged) the matrix-unit launcher chooses at the default chunk
NORM_SHAPES = [((293, 4, 5, 17), (64, 1)), ((1541, 1, 1, 65), (64, 1)), ((1541, 2, 49, 17), (32, 1)), ((293, 6, 49, 65), (16, 1)),
               ((1541, 6, 129, 17), (16, 2)), ((293, 9, 256, 1), (16, 0)), ((17, 6, 256, 1025), (16, 0))]
POISON = -12345.678


def cases():
    """(name, q or 0, modes as (K, q or 1, m), coefficients (K, S), threshold, expected launcher choice or None)"""
    rng = np.random.default_rng(20240517)
    F, Cm = rng.standard_normal((1541, 50)), rng.standard_normal((50, 100))
    yield "signed-float", 0, np.ascontiguousarray(F.T)[:, None, :], Cm, 0.25, None
    rng = np.random.default_rng(20250911)
    P, Cm = rng.standard_normal((50, 6, 1541)), rng.standard_normal((50, 100))
    yield "norm-float", 6, P, Cm, 7.0, None
    for (m, q, K, S), choice in NORM_SHAPES:
        rng = np.random.default_rng(100000 * q + 1000 * m + 10 * K + S)
        yield "norm-m%d-q%d-K%d-S%d" % (m, q, K, S), q, rng.standard_normal((K, q, m)), rng.standard_normal((K, S)), float(np.sqrt(q * K)), choice


def run(out, tree):
    sys.path.insert(0, os.path.abspath(tree))
    from pgdrome_amd import _lib
    ctx = _lib.Context(0)
    knobs = (_lib.TUNE_EVAL_VARIANT, _lib.TUNE_EVAL_SAMPLE_CHUNK, _lib.TUNE_EVAL_GRID_MAX)
    arrays = {}
    for name, q, P, Cm, threshold, choice in cases():
        m, S = P.shape[2], Cm.shape[1]
        modes = [ctx.vec_from(np.ascontiguousarray(P[k]).reshape(-1)) for k in range(P.shape[0])]
        outs = [ctx.vec_alloc(m), ctx.vec_alloc(m), ctx.vec_alloc(m), ctx.vec_alloc(m * S)]
        try:
            for variant in (1, 0):
                for chunk in (0, 16, 48):
                    for grid_max in (0, 2):
                        for knob, v in zip(knobs, (variant, chunk, grid_max)):
                            ctx.tune(knob, v)
                        for v in outs:
                            ctx.vec_fill(v, POISON)
                        kw = dict(stats=True, env_min=outs[0], env_max=outs[1], exceed=outs[2], threshold=threshold, fields=outs[3])
                        st = ctx.eval_batch_norm(modes, q, Cm, **kw) if q else ctx.eval_batch(modes, Cm, **kw)
                        key = "%s/%s/chunk%d/grid%d/" % (name, "mfma" if variant else "plain", chunk, grid_max)
                        arrays[key + "stats"] = st
                        for what, v in zip(("env_min", "env_max", "exceed", "fields"), outs):
                            arrays[key + what] = ctx.vec_download(v)
                        if q:
                            arrays[key + "shape"] = np.array(ctx.eval_norm_last_shape(), dtype=np.int64)
                            if choice and variant and chunk == 0 and tuple(arrays[key + "shape"]) != choice:
                                raise SystemExit("%s: the launcher chose %s, the case is here for %s" % (name, arrays[key + "shape"], choice))
            print("%-28s %d calls" % (name, 12), flush=True)
        finally:
            for knob, v in zip(knobs, (1, 0, 0)):
                ctx.tune(knob, v)
            for v in modes + outs:
                ctx.vec_free(v)
    ctx.close()
    np.savez(out, **arrays)
    print("%d arrays stored" % len(arrays))


def compare(a, b):
    A, B = np.load(a), np.load(b)
    keys = sorted(set(A.files) | set(B.files))
    differ = [k for k in keys if k not in A.files or k not in B.files or A[k].shape != B[k].shape or A[k].tobytes() != B[k].tobytes()]
    print("%d arrays compared, %d differ%s" % (len(keys), len(differ), ": " + ", ".join(differ[:10]) if differ else ""))
    return 1 if differ else 0


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "run":
        run(sys.argv[2], sys.argv[4] if len(sys.argv) >= 5 and sys.argv[3] == "--tree" else ROOT)
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        raise SystemExit(compare(sys.argv[2], sys.argv[3]))
    else:
        raise SystemExit(__doc__)
