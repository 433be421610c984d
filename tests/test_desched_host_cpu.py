"""The host arithmetic of a descheduling plan (csrc/ksim_desched_host.hpp): no GPU.

The stand-alone program tests/native_desched_host (the header under the address and undefined-behaviour sanitizers)
checks by itself the per-replica event offsets against a plain prefix sum over ragged streams, the budget at
ratio = +inf (0 without a bound pod, every pod otherwise: tests/desched_ref.py raises there, so the two values are
the contract) and 0 <= budget <= n for n up to INT32_MAX.  For every n in 0..300 and the ratios below it writes the
budget out, and this test compares each with the formula of tests/desched_ref.py.
"""
import math
import os
import subprocess

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native_desched_host")
RATIOS = [0.0, 1e-9, 0.05, 0.3, 0.5, 1.0, 1.0 + 1e-12, 7.0, 1e300]
N_MAX = 300


def ref_budget(ratio, n):
    return min(int(math.ceil(ratio * float(n))), n)  # tests/desched_ref.py plan()


def test_native_program_under_sanitizers(tmp_path):
    subprocess.run(["make", "-s", "-C", HERE], check=True)
    dst = str(tmp_path / "budgets.txt")
    p = subprocess.run([os.path.join(HERE, "desched_host_check"), dst] + [q.hex() for q in RATIOS],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=120)
    print(p.stdout, p.stderr)
    assert p.returncode == 0, p.stderr
    lines = p.stdout.strip().splitlines()
    assert lines[-1] == "ok" and lines[0].endswith("lines=%d" % (len(RATIOS) * (N_MAX + 1)))
    got = [tuple(int(x) for x in line.split()) for line in open(dst)]
    want = [(i, n, ref_budget(q, n)) for i, q in enumerate(RATIOS) for n in range(N_MAX + 1)]
    assert got == want
    # the reference's formula has no value at +inf: int(ceil(inf)) raises, and inf * 0 is a NaN
    assert math.isnan(math.inf * 0.0)
