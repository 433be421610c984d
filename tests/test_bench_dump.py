"""bench.py --dump-outputs: what the last timed step computed, as .npy files, and the plain / --full split.

The row selection and the file layout are checked on the CPU with a stand-in engine; the GPU test runs the
benchmark itself (two replicas, one step) and compares its files with an engine replaying the same seeds."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import ksim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RESULT_DT = np.dtype([("node", "<i4"), ("gpu_mask", "<i4"), ("score", "<i8"), ("n_feasible", "<i4"), ("status", "<i4")])


class FakeEngine:
    """results_array / report_arrays of a deterministic make-believe run."""

    def __init__(self, n_events):
        self.n_events = list(n_events)

    def results_array(self, r):
        n = self.n_events[r]
        a = np.zeros(n, dtype=RESULT_DT)
        a["node"] = np.arange(n) + 1000 * r
        a["gpu_mask"] = np.arange(n) % 255
        a["score"] = (np.arange(n, dtype=np.int64) + 1) * 7919
        a["n_feasible"] = n - np.arange(n)
        a["status"] = np.arange(n) % 3
        return a

    def report_arrays(self, r):
        import bench
        n = self.n_events[r]
        d = {c: np.arange(n, dtype=np.int64) * (i + 2) + r for i, c in enumerate(bench.REPORT_COLS)}
        d["frag_bins"] = np.arange(n * 7, dtype=np.float64).reshape(n, 7) / 3.0 + r
        return d


def test_dump_rows_keeps_everything_within_the_budget():
    import bench
    rows = bench.dump_rows([5, 0, 3], 56)
    assert [list(r) for r in rows] == [[0, 1, 2, 3, 4], [], [0, 1, 2]]


def test_dump_rows_samples_a_fixed_set_over_the_budget():
    import bench
    n_events = [1000, 0, 17, 5000]
    rows = bench.dump_rows(n_events, 56, budget=56 * 600)
    again = bench.dump_rows(n_events, 56, budget=56 * 600)
    assert sum(len(r) for r in rows) == 600
    for r, n, r2 in zip(rows, n_events, again):
        assert list(r) == list(r2)  # the same rows every run
        assert len(set(r)) == len(r) and list(r) == sorted(r) and (not len(r) or (0 <= r[0] and r[-1] < n))
    # an unbiased draw over all rows: the long replica holds about 5000/6017 of the sample
    assert 450 < len(rows[3]) < 550 and len(rows[1]) == 0


def test_dump_outputs_files(tmp_path):
    import bench
    eng = FakeEngine([4, 0, 6])
    shapes = bench.dump_outputs(eng, str(tmp_path / "out"), report=True)
    assert shapes == {"results.npy": [10, 7], "reports.npy": [10, 16]}
    res = np.load(tmp_path / "out" / "results.npy")
    rep = np.load(tmp_path / "out" / "reports.npy")
    assert res.dtype == np.float64 and rep.dtype == np.float64
    assert list(res[:, 0]) == [0] * 4 + [2] * 6 and list(res[:, 1]) == [0, 1, 2, 3, 0, 1, 2, 3, 4, 5]
    a = eng.results_array(2)
    for j, c in enumerate(bench.RESULT_COLS):
        assert list(res[4:, 2 + j]) == list(a[c])
    d = eng.report_arrays(2)
    assert (rep[4:, 2:9] == d["frag_bins"]).all() and (rep[:, :2] == res[:, :2]).all()
    for j, c in enumerate(bench.REPORT_COLS):
        assert list(rep[4:, 9 + j]) == list(d[c])
    # without the report: the results only
    assert bench.dump_outputs(eng, str(tmp_path / "out2")) == {"results.npy": [10, 7]}
    assert sorted(os.listdir(tmp_path / "out2")) == ["results.npy"]


def test_dump_budget_is_under_64_mb():
    import bench
    assert bench.DUMP_BUDGET_BYTES <= 64 * 10**6
    rows = sum(len(r) for r in bench.dump_rows([9_000_000], 56 + 128))
    assert rows * (56 + 128) <= bench.DUMP_BUDGET_BYTES < (rows + 1) * (56 + 128)


@pytest.mark.gpu
def test_plain_bench_run_dumps_the_last_steps_results(tmp_path):
    out = tmp_path / "dump"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--replicas", "2", "--dump-outputs", str(out)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    line = json.loads(p.stdout.strip().splitlines()[-1])
    assert line["steps"] == 2 and line["ms_per_step"] > 0 and line["unit"] == "pods/s"
    assert abs(line["value"] - line["config"]["events_per_gpu"] / (line["ms_per_step"] / 1e3)) <= 1e-6 * line["value"]
    assert "cpu_baseline" not in line  # a plain run: the headline figure only (--full adds the baselines)
    assert sorted(os.listdir(out)) == ["results.npy"] and line["dumped_outputs"]["results.npy"][1] == 7
    res = np.load(out / "results.npy")
    assert res.dtype == np.float64 and res.nbytes <= 64 * 10**6
    # the same two seeds on an engine of our own
    import bench
    trace = ksim.Trace.openb("default")
    eng = bench._engine_on(0, trace, bench.seeds_for_rank(0, 2), 0)
    eng.run()
    want = []
    for r in range(2):
        a = eng.results_array(r)
        want.append(np.stack([np.full(len(a), r, dtype=np.float64), np.arange(len(a), dtype=np.float64)]
                             + [a[c].astype(np.float64) for c in bench.RESULT_COLS], axis=1))
    eng.close()
    want = np.concatenate(want)
    assert res.shape == want.shape and (res == want).all()
