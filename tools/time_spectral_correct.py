"""Where the per-solve cost of the spectral start goes, for every storage of the Ritz vectors (PGD_TUNE_BLOCK_STORAGE):
python tools/time_spectral_correct.py [n] [k] [out.jsonl]

One harvest (f64 vectors); the fp32 and the f64 column block are filled from the same vectors.  Per storage: correct() whole,
Y'r and x += Y c on their own in ms, and the TB/s of those two on the bytes they must move (Y once, r or x)."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pgdrome_amd import _lib, fem, problems, spectral
from pgdrome_amd.hip_backend import HipBackend
from pgdrome_amd.solver import PGDProblem
import bench

n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
k = int(sys.argv[2]) if len(sys.argv) > 2 else 16
out_path = sys.argv[3] if len(sys.argv) > 3 else None
be = fem.set_backend(HipBackend(0))
P = fem.Point
mesh = fem.BoxMesh(P(0, 0, 0), P(1, 1, 1), n - 1, n - 1, n - 1)
spec = problems.reaction_diffusion(mesh, 128, PGD_nmax=50, PGD_tol=1e-12)
prob = PGDProblem(**spec)
A, b = bench._first_spatial_system(prob)
be.tune(_lib.TUNE_BLOCK_STORAGE, 0)
sp_vec = spectral.get(fem, A, b, k, fem._Params())
print("harvest", sp_vec.info["seconds"], "k", sp_vec.k)
op = A.op()
lay = A.lay
lo, hi = lay.owned_range()


def t(label, fn, reps=5):
    be.sync()
    fn()
    be.sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    be.sync()
    ms = 1e3 * (time.perf_counter() - t0) / reps
    print("%-40s %.3f ms" % (label, ms))
    return ms


r = fem.Vector(b.V)
be.spmv(op, b.dev(), r.dev_for_write(), lo, hi)
r.touched_dev()
for knob in (1, 2, 0):
    be.tune(_lib.TUNE_BLOCK_STORAGE, knob)
    sp = sp_vec if knob == 0 else spectral.SpectralStart(lay, list(sp_vec.Y), sp_vec.theta, sp_vec.residuals, dict(sp_vec.info), be)
    print("---- storage: %s, %.3f GB" % (sp.info["storage"], sp.info["bytes"] / 1e9))
    x = b.copy()
    x.scale(0.5)
    rec = {"n": n, "k": sp.k, "storage": sp.info["storage"], "bytes": sp.info["bytes"]}
    rec["correct_ms"] = t("correct() whole", lambda: sp.correct(fem, A, op, b, x))
    t("A.merged + gram (cached)", lambda: sp.gram(fem, *A.merged()))
    rec["dots_ms"] = t("Y'r (one host synchronisation)", lambda: sp.dots(fem, lay, r))
    cs = [0.1] * sp.k
    if sp.block is not None:
        rec["combine_ms"] = t("x += Y c", lambda: be.block_combine(sp.block, cs, x.dev(), x.dev()))
    else:
        def old():
            out = be.vec_zeros(lay.n)
            be.vec_lincomb(out, [x.dev()] + [y.dev() for y in sp.Y], [1.0] + cs)
            be.vec_copy(x.dev_for_write(), out)
            be.vec_free(out)
        rec["combine_ms"] = t("x += Y c (zeros, lincomb, copy)", old)
    own = sp.info["bytes"] if sp.block is not None else 8.0 * sp.k * lay.n
    rec["dots_TBps"] = (own + 8.0 * lay.n) / rec["dots_ms"] * 1e-9
    rec["combine_TBps"] = (own + 16.0 * lay.n) / rec["combine_ms"] * 1e-9
    print("TB/s on own bytes: dots %.2f, combine %.2f" % (rec["dots_TBps"], rec["combine_TBps"]))
    if out_path:
        with open(out_path, "a") as f:
            f.write(json.dumps({"time_spectral_correct": rec}) + "\n")
    del sp
t("rescale_start (k=1)", lambda: fem._rescale_start(lay, op, b, x))
