"""k_wsum's LDS layout and the run plan with KSIM_POLICY_WEIGHTED replicas, on the host (no GPU).

tests/native_host/wsum_plan_check.cpp compiles ksim_plan.hpp for the host and checks wsum_layout / wsum_lds /
wsum_fits (regions in order and aligned, strictly monotone in N, every plugin mask, openb's 1213 nodes fit with every
plugin on and the report's record, the refusal bound in closed form) and make_run_plan: the nine inputs of
tests/test_gpu_run_plan.py give exactly today's plans, and with WEIGHTED replicas appended the plan gains one k_wsum
group (K = 1, S = N, the union mask's LDS) after the policies' groups and before Go's Random, on a side stream
whenever the run is concurrent, the other groups unchanged.  It aborts on the first broken expectation.
"""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "native_wsum")
EXE = os.path.join(ROOT, "tests", "native_host", "wsum_plan_check")


def test_wsum_plan_check():
    subprocess.run(["make", "-s", "-C", HERE, "../native_host/wsum_plan_check"], check=True)
    p = subprocess.run([EXE], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=120)
    print(p.stdout, p.stderr)
    assert p.returncode == 0, p.stderr
    lines = p.stdout.strip().splitlines()
    assert lines[-1] == "ok"
    out = dict(l.split(": ", 1) for l in lines[:-1])
    m = re.match(r"cases=(\d+) lds_1213_all_report=(\d+) max_all_report=(\d+) max_lean=(\d+)$", out["layout"])
    assert m and int(m.group(1)) == 64 * 2 * 4200
    assert int(m.group(2)) <= 160 * 1024 and int(m.group(3)) >= 1213 and int(m.group(4)) > int(m.group(3))
    assert out["run_plan"] == "unchanged=9 with_weighted=9 on_side_stream=8"
