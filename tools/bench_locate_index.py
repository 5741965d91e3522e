"""The bin index of pgd_points_locate (pgdrome_amd/csrc/pgd_locate.hip, PGD_TUNE_LOCATE_INDEX) beside the general kernel on jittered
(non-lattice) copies of BoxMesh at n^3 vertices, in the same process on the same points:

    build_s        a call with ONE point on a mesh without an index (pgd_points_index_drop before it): the build and next to nothing
    first_index_s  the first indexed call with all P points on a mesh without an index: what a caller pays who has no index yet
    index_s        an indexed call on the mesh that holds its index
    general_s      the general kernel (PGD_TUNE_LOCATE_INDEX = 0)

    python tools/bench_locate_index.py [n ...] [--points P ...] [--reps R] [--out FILE] [--limit SECONDS]
                                       [--general-max-work W] [--general-once-work W1] [--target T]
                                           (defaults: n = 65 129 257, P = 100 10000 100000, R = 3, W = 2e11, W1 = 2e13, T = 0)

--target: PGD_TUNE_LOCATE_INDEX_TARGET, cells per bin (0: the library's rule); the line carries it.

Every mesh size runs in a child process of its own under `timeout` (--limit, default 900 s); the first child that does not end
cleanly ends the run.  One JSON line per (n, P), printed and appended to --out (default profiles/locate_index_bench_n1.jsonl).
Times are whole calls on the host clock - upload of the points, the kernels, the download of the cells and the synchronisation that
ends pgd_points_locate.  After one warm-up of either path the paths ALTERNATE for R rounds; a figure is the median of the rounds and
`*_spread` is (max - min) / median of them.  The general kernel takes part in every round while P x cells <= W, in ONE round (no
warm-up, no spread) while P x cells <= W1, and is "not measured" beyond that.  Where both ran, cells and lam are compared as bits.
candidate_tests_per_s: the lengths of the lists of the points' bins, summed, over index_s.  index_sorted_s: the indexed call on the same
points ordered by their bins on the host beforehand (the ordering is not timed)."""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def clock(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def spread(ts):
    return (max(ts) - min(ts)) / statistics.median(ts) if len(ts) > 1 else None


def one_size(n, counts, reps, general_max_work, general_once_work, target):
    import numpy as np
    from pgdrome_amd import _lib, fem
    ctx = _lib.Context(0)
    mesh = fem.BoxMesh(fem.Point(0, 0, 0), fem.Point(1, 1, 1), n - 1, n - 1, n - 1)
    X, C = mesh.coordinates(), mesh.cells()
    X = X + 0.2 / (n - 1) * np.random.default_rng(2).uniform(-1, 1, X.shape)
    nc = int(len(C))
    mh = ctx.mesh_upload(X, C)
    ctx.tune(_lib.TUNE_LOCATE_LATTICE, 1)
    ctx.tune(_lib.TUNE_LOCATE_INDEX_TARGET, target)
    one_point = X[C[0]].mean(axis=0).reshape(1, 3)

    def locate(pts, index, keep=False):
        h = ctx.points_locate(mh, pts, 1e-10, index=index)
        if keep:
            return h
        ctx.points_free(h)

    def build_only():
        ctx.points_index_drop(mh)
        return clock(lambda: locate(one_point, True))
    build_only()
    builds = [build_only() for _ in range(reps)]
    info = ctx.points_index_info(mh)
    bin_ptr, _, o, inv, nb = ctx.points_index_download(mh)
    lengths = np.diff(bin_ptr.astype(np.int64))
    for P in counts:
        rng = np.random.default_rng(1)
        cells = rng.integers(0, nc, P)
        lam = 0.05 + 0.8 * rng.dirichlet(np.ones(4), size=P)
        pts = np.ascontiguousarray(np.einsum("pa,pad->pd", lam, X[C[cells]]))
        q = np.clip(np.floor((pts - o) * inv), 0, nb - 1).astype(np.int64)
        walked = int(lengths[q[:, 0] + nb[0] * (q[:, 1] + nb[1] * q[:, 2])].sum())
        work = float(P) * nc
        rounds_general = reps if work <= general_max_work else 1 if work <= general_once_work else 0
        line = {"bench": "locate_index", "n": n, "cells": nc, "points": P, "work": work, "target": target, "bins": list(info["n"]), "index_bytes": info["bytes"],
                "entries_per_cell": info["entries"] / nc, "mean_list": info["entries"] / float(np.prod(info["n"])), "longest_list": info["longest"],
                "build_s": statistics.median(builds), "build_spread": spread(builds), "mean_walk_per_point": walked / P}
        firsts = []
        for _ in range(reps):
            ctx.points_index_drop(mh)
            firsts.append(clock(lambda: locate(pts, True)))
        line.update(first_index_s=statistics.median(firsts), first_index_spread=spread(firsts))
        locate(pts, True)                                            # warm-up (the index is there)
        if rounds_general == reps:
            locate(pts, False)
        ti, tg = [], []
        for r in range(reps):
            ti.append(clock(lambda: locate(pts, True)))
            assert ctx.points_last_path() == _lib.LOCATE_PATH_INDEX
            if r < rounds_general:
                tg.append(clock(lambda: locate(pts, False)))
                assert ctx.points_last_path() == _lib.LOCATE_PATH_GENERAL
        line.update(index_s=statistics.median(ti), index_spread=spread(ti), candidate_tests_per_s=walked / statistics.median(ti))
        # the same points in the order of their bins (a raster comes like that; the seeded points above do not): lanes of a wave walk
        # the same or neighbouring lists
        by_bin = np.ascontiguousarray(pts[np.argsort(q[:, 0] + nb[0] * (q[:, 1] + nb[1] * q[:, 2]), kind="stable")])
        locate(by_bin, True)
        ts = [clock(lambda: locate(by_bin, True)) for _ in range(reps)]
        line.update(index_sorted_s=statistics.median(ts), index_sorted_spread=spread(ts))
        hi = locate(pts, True, keep=True)
        ci, li = ctx.points_download(hi)
        ctx.points_free(hi)
        assert np.array_equal(ci, cells)
        if tg:
            hg = locate(pts, False, keep=True)
            cg, lg = ctx.points_download(hg)
            ctx.points_free(hg)
            line.update(general_s=statistics.median(tg), general_spread=spread(tg), general_rounds=len(tg),
                        general_cell_tests_per_s=work / statistics.median(tg), same_bits=bool(np.array_equal(ci, cg) and np.array_equal(li.view(np.int64), lg.view(np.int64))),
                        speedup_warm=statistics.median(tg) / line["index_s"], speedup_first_call=statistics.median(tg) / line["first_index_s"])
            assert line["same_bits"]
        else:
            line.update(general_s="not measured", general_rounds=0)
        print(json.dumps(line), flush=True)
    ctx.mesh_free(mh)
    ctx.close()


def main():
    argv = sys.argv[1:]

    def opt(flag, default, many=False):
        if flag not in argv:
            return default
        i = argv.index(flag)
        j = i + 1
        while many and j + 1 < len(argv) and not argv[j + 1].startswith("--"):
            j += 1
        vals = argv[i + 1:j + 1]
        del argv[i:j + 1]
        return vals if many else vals[0]
    reps, limit = int(opt("--reps", 3)), int(opt("--limit", 900))
    general_max_work, general_once_work = float(opt("--general-max-work", 2e11)), float(opt("--general-once-work", 2e13))
    out = opt("--out", os.path.join(ROOT, "profiles", "locate_index_bench_n1.jsonl"))
    target = int(opt("--target", 0))
    child = opt("--one", None)
    counts = [int(p) for p in opt("--points", ["100", "10000", "100000"], many=True)]
    sizes = [int(a) for a in argv] or [65, 129, 257]
    if child is not None:
        return one_size(sizes[0], counts, reps, general_max_work, general_once_work, target)
    for n in sizes:
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), str(n), "--one", "size", "--points"] + [str(p) for p in counts] + \
              ["--reps", str(reps), "--general-max-work", repr(general_max_work), "--general-once-work", repr(general_once_work), "--target", str(target)]
        run = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(run.stdout)
        sys.stdout.flush()
        with open(out, "a") as fh:
            fh.write("".join(l + "\n" for l in run.stdout.splitlines() if l.startswith("{")))
        if run.returncode != 0:
            raise SystemExit("bench_locate_index: %d^3 vertices ended with status %d; nothing more is started" % (n, run.returncode))


if __name__ == "__main__":
    main()
