"""bench.py command line: the result line, --steps, --dump-outputs, --full.

Runs the benchmark on the CPU path (devices hidden from the child) at a toy
size, so the two runs compared here are bit-reproducible."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
SMALL = ["--gpus", "1", "--rows", "20000", "--features", "10",
         "--num-leaves", "7"]
DUMP_BUDGET = 64 * 1000 * 1000


def _run(extra):
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, BENCH] + SMALL + extra,
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.fixture(scope="module")
def two_runs(tmp_path_factory):
    out = []
    for name in ("a", "b"):
        d = str(tmp_path_factory.mktemp(name))
        res = _run(["--steps", "3", "--warmup", "1", "--dump-outputs", d])
        out.append((res, d))
    return out


def test_result_line_fields(two_runs):
    res, _ = two_runs[0]
    assert res["metric"] == "lightgbm_train_rows_per_sec"
    assert res["unit"] == "rows/s" and res["higher_is_better"] is True
    assert res["dtype"] == "fp32"
    assert res["steps"] == 3 and res["warmup"] == 1
    assert res["ms_per_step"] > 0
    # value and ms_per_step describe the same timed interval
    rows = res["config"]["rows_per_gpu"]
    assert res["value"] == pytest.approx(rows / (res["ms_per_step"] * 1e-3),
                                         rel=1e-9)


def test_dump_outputs_files(two_runs):
    _, d = two_runs[0]
    names = sorted(os.listdir(d))
    assert "raw_scores.npy" in names and "last_tree0_value.npy" in names
    assert all(n.endswith(".npy") for n in names)
    total = 0
    for n in names:
        a = np.load(os.path.join(d, n))
        assert a.dtype in (np.float32, np.float64), (n, a.dtype)
        total += a.nbytes
    assert total <= DUMP_BUDGET
    scores = np.load(os.path.join(d, "raw_scores.npy"))
    assert scores.shape == (20000, 1) and np.isfinite(scores).all()
    # 3 timed + 1 warmup iterations moved the scores off the constant init
    assert np.unique(scores).size > 1


def test_dump_outputs_reproducible(two_runs):
    (_, da), (_, db) = two_runs
    assert sorted(os.listdir(da)) == sorted(os.listdir(db))
    for n in os.listdir(da):
        np.testing.assert_array_equal(np.load(os.path.join(da, n)),
                                      np.load(os.path.join(db, n)), err_msg=n)


def test_steps_sets_timed_iterations(two_runs, tmp_path):
    """--steps is the number of timed iterations: fewer of them leave other
    scores behind than the 3-step run, and the line reports the count.
    --full is accepted alongside and changes nothing about the line."""
    res = _run(["--steps", "1", "--warmup", "1", "--full",
                "--dump-outputs", str(tmp_path)])
    assert res["steps"] == 1 and res["ms_per_step"] > 0
    assert set(res) == set(two_runs[0][0])
    scores = np.load(os.path.join(str(tmp_path), "raw_scores.npy"))
    ref = np.load(os.path.join(two_runs[0][1], "raw_scores.npy"))
    assert scores.shape == ref.shape
    assert np.abs(scores - ref).max() > 0


def test_dump_sample_is_bounded():
    """Outputs past the budget are cut to a fixed seeded row sample."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("_bench_under_test", BENCH)
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    assert bench.DUMP_MAX_SCORE_ELEMS * 4 < DUMP_BUDGET
    rows = bench.sample_rows(bench.DUMP_MAX_SCORE_ELEMS * 3, 1)
    assert rows is not None and rows.size == bench.DUMP_MAX_SCORE_ELEMS
    assert rows.min() >= 0 and rows.max() < bench.DUMP_MAX_SCORE_ELEMS * 3
    np.testing.assert_array_equal(
        rows, bench.sample_rows(bench.DUMP_MAX_SCORE_ELEMS * 3, 1))
    assert bench.sample_rows(1000, 1) is None
