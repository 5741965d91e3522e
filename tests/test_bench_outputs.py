"""bench.py --dump-outputs and --steps on a machine without a GPU: the argument checks, the sample of a long dimension, and the
written outputs of one process and of two row-sharded ranks gathered onto rank 0 - through tests/helpers/bench_rehearsal.py,
which wraps bench's own record_last_pass / dump_outputs around the timed passes of the oracle backend."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REHEARSAL = os.path.join(ROOT, "tests", "helpers", "bench_rehearsal.py")
NAMES = {"mu_iterate.npy", "solution.npy", "space_iterate.npy"}


@pytest.mark.parametrize("argv", [["--steps", "0"], ["--steps", "-3"], ["--warmup", "-1"]])
def test_steps_below_one_are_refused(argv):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + argv, capture_output=True, timeout=120,
                       cwd=ROOT)
    assert r.returncode == 2 and b"--steps must be at least 1" in r.stderr and r.stdout == b""


def test_dump_sample_rows_are_seeded_sorted_and_nested():
    import bench
    a, b = bench.dump_sample_rows(10 ** 6, 5000), bench.dump_sample_rows(10 ** 6, 5000)
    assert np.array_equal(a, b) and len(np.unique(a)) == 5000 and np.all(np.diff(a) > 0) and 0 <= a[0] and a[-1] < 10 ** 6
    assert set(bench.dump_sample_rows(10 ** 6, 2500)) <= set(a)          # a smaller sample is a subset of a larger one
    assert np.array_equal(bench.dump_sample_rows(700, 5000), np.arange(700))


def _rehearse(tmp_path, name, gpus, rows, steps=3, warmup=1):
    out = tmp_path / name
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "PGD_BENCH_LAUNCHER")}
    env["PGD_REHEARSAL_DUMP_ROWS"] = str(rows)
    r = subprocess.run([sys.executable, REHEARSAL, "--gpus", str(gpus), "--n", "12", "--n-mu", "9", "--steps", str(steps),
                        "--warmup", str(warmup), "--dump-outputs", str(out)], capture_output=True, env=env, timeout=600,
                       cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    assert json.loads(r.stdout.decode())["steps"] == steps
    assert set(os.listdir(out)) == NAMES | {".gitignore"}
    return {n[:-4]: np.load(out / n) for n in NAMES}


def test_rehearsal_dumps_the_last_timed_pass_on_one_and_two_ranks(tmp_path):
    import bench
    full = _rehearse(tmp_path, "full", 1, 10 ** 6)           # 12^3 rows: all of them
    one = _rehearse(tmp_path, "one", 1, 1000)
    again = _rehearse(tmp_path, "again", 1, 1000)
    two = _rehearse(tmp_path, "two", 2, 1000)
    assert one["space_iterate"].shape == (1000,) and one["mu_iterate"].shape == (9,) and one["solution"].shape == (500, 9)
    assert full["space_iterate"].shape == (12 ** 3,) and full["solution"].shape == (12 ** 3, 9)
    for name, a in one.items():
        assert a.dtype == np.float64 and np.all(np.isfinite(a)) and np.abs(a).max() > 0, name
        assert np.array_equal(a, again[name]), name                        # same arguments, same outputs
    # the samples are the seeded rows of the whole vectors
    assert np.array_equal(one["space_iterate"], full["space_iterate"][bench.dump_sample_rows(12 ** 3, 1000)])
    assert np.array_equal(one["solution"], full["solution"][bench.dump_sample_rows(12 ** 3, 500)])
    assert np.array_equal(one["mu_iterate"], full["mu_iterate"])
    # two row-sharded ranks, gathered onto rank 0: the same outputs up to the solves' tolerance
    for name, a in one.items():
        assert two[name].shape == a.shape, name
        assert np.abs(two[name] - a).max() <= 1e-6 * np.abs(a).max(), name


def test_dumped_shapes_do_not_depend_on_the_window(tmp_path):
    """However many modes the timed window has stored - none after the first pass, none again right after the enrichment starts
    over - every array has the problem's shape and is not empty; after one pass the solution is the rank-one term in progress."""
    first = _rehearse(tmp_path, "first", 1, 10 ** 6, steps=1, warmup=0)
    later = _rehearse(tmp_path, "later", 1, 10 ** 6, steps=7, warmup=2)
    for name in first:
        assert first[name].shape == later[name].shape and first[name].size > 0 and np.abs(first[name]).max() > 0, name
    assert np.array_equal(first["solution"], np.outer(first["space_iterate"], first["mu_iterate"]))
    assert not np.array_equal(later["solution"], np.outer(later["space_iterate"], later["mu_iterate"]))    # stored modes count
