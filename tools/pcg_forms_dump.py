"""Run the case table of tests/pcg_form_cases.py - one case per recurrence and preconditioner pgd_pcg_solve can pick - and dump
what every solve returned, for comparing two builds of the library bit by bit:

    python tools/pcg_forms_dump.py run OUT.npz [--tree DIR]      # DIR: the checkout whose pgdrome_amd is loaded (default: this one)
    python tools/pcg_forms_dump.py compare A.npz B.npz

Per case: iteration count, reported residual and x of the solve cut at 37 iterations and of the solve to convergence
(rtol 1e-10).  The case table is always this checkout's, so an older tree is driven through exactly the same solves; nothing the
older tree lacks (pgd_pcg_last_form) is required - where it exists the names are stored too.  Needs a GPU."""
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(out, tree):
    sys.path.insert(0, os.path.abspath(tree))
    spec = importlib.util.spec_from_file_location("pcg_form_cases", os.path.join(ROOT, "tests", "pcg_form_cases.py"))
    PC = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(PC)
    from pgdrome_amd import fem
    from pgdrome_amd.hip_backend import HipBackend
    ctx = fem.set_backend(HipBackend(0)).ctx
    systems, arrays = {}, {}
    for name, system, bc, knobs, form, precond, _ in PC.CASES:
        if system not in systems:
            systems[system] = PC.build_system(ctx, system)
        try:
            PC.set_knobs(ctx, knobs)
            for key, maxit, rtol in (("cut", PC.CUT, 0.0), ("full", 10000, 1e-10)):
                it, rel, x, _ = PC.solve(ctx, systems[system], bc, maxit, rtol)
                arrays["%s/%s/iterations" % (name, key)] = np.array([it], dtype=np.int64)
                arrays["%s/%s/relres" % (name, key)] = np.array([rel])
                arrays["%s/%s/x" % (name, key)] = x
            chosen = ctx.pcg_last_form() if hasattr(ctx, "pcg_last_form") else None
        finally:
            PC.set_knobs(ctx, {})
        print("%-32s expected %s/%s, reported %s, cut %d, converged in %d (%.3g)" % (
            name, form, precond, chosen, arrays[name + "/cut/iterations"][0], arrays[name + "/full/iterations"][0], arrays[name + "/full/relres"][0]), flush=True)
    np.savez(out, **arrays)


def compare(a, b):
    A, B = np.load(a), np.load(b)
    keys = sorted(set(A.files) | set(B.files))
    differ = [k for k in keys if k not in A.files or k not in B.files or A[k].shape != B[k].shape or A[k].tobytes() != B[k].tobytes()]
    print("%d arrays compared (%d cases x 2 solves x iterations, residual, x), %d differ%s" % (
        len(keys), len(keys) // 6, len(differ), ": " + ", ".join(differ[:10]) if differ else ""))
    return 1 if differ else 0


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "run":
        run(sys.argv[2], sys.argv[4] if len(sys.argv) >= 5 and sys.argv[3] == "--tree" else ROOT)
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        raise SystemExit(compare(sys.argv[2], sys.argv[3]))
    else:
        raise SystemExit(__doc__)
