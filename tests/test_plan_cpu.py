"""The planners of ksim_plan.hpp (memo_plan, hmemo_plan, the event tables, the slice geometry, the kernel-form tables,
the run plan and the node-sharded runs' slices), compiled for the host and run without a GPU
(tests/native_host/plan_check.cpp).

The program checks the plans' invariants over seeded random inputs, plans the bench's C2 job from its trace and compares
with what the engine printed on the GPU (K=25 Cw=9 nfw=16, 250 workgroups for k_memo; K=1 S=1213 Cmax=151 Gmax=91
Smax=15 for k_hmemo; K=63 S=1600 for C5's 100 000 nodes), compares the slice function with the formulas its call sites
had over world 1..16 x nmax 64..200000, and memo_form / hmemo_form over every input with the conditionals they
replaced.  The run plan (make_run_plan): the nine cases of tests/test_gpu_run_plan.py as inputs with their plans written
out, invariants over 3000 seeded random inputs, and choose_wgs / replay_fit / replay_narrow / the shard slices against
the formulas the engine had.  It aborts on the first broken expectation; here its exit status and printed tallies are
checked.
"""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "native_host")
OPENB = os.path.join(ROOT, "data", "openb")


def test_plan_check():
    subprocess.run(["make", "-s", "-C", HERE, "plan_check"], check=True)
    p = subprocess.run([os.path.join(HERE, "plan_check"), os.path.join(OPENB, "openb_node_list_gpu_node.csv"),
                        os.path.join(OPENB, "openb_pod_list_default.csv")],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=120)
    print(p.stdout, p.stderr)
    assert p.returncode == 0, p.stderr
    lines = p.stdout.strip().splitlines()
    assert lines[-1] == "ok"
    out = dict(l.split(": ", 1) for l in lines[:-1])
    assert set(out) == {"memo_plan", "hmemo_plan", "recorded", "slices", "forms", "run_plan", "shard_slices"}
    m = re.match(r"cases=(\d+) planned=(\d+) refused=(\d+) hkeys=(\d+) decider=(\d+) residency_refusals=(\d+)$",
                 out["memo_plan"])
    assert m and int(m.group(1)) >= 300 and all(int(g) > 0 for g in m.groups())
    m = re.match(r"cases=(\d+) planned=(\d+) refused=\d+ wide=(\d+) per_model_tables=(\d+) whole_table_fallbacks=(\d+)$",
                 out["hmemo_plan"])
    assert m and int(m.group(1)) >= 300 and all(int(g) > 0 for g in m.groups())
    assert out["recorded"] == ("C2 k_memo K=25 Cw=9 nfw=16 workgroups=250 LDS=163124; "
                               "k_hmemo K=1 S=1213 Cmax=151 Gmax=91 Smax=15 LDS=92576; C5 slices K=63 S=1600")
    assert out["forms"] == "memo_inputs=384 memo_forms=8 hmemo_inputs=9216 hmemo_forms=12"
    assert re.match(r"compared=\d+$", out["slices"])
    m = re.match(r"cases=9 fuzz=(\d+) concurrent=(\d+) back_to_back=(\d+) split=(\d+) mix=(\d+) kernels=6 formulas=(\d+)$",
                 out["run_plan"])
    assert m and int(m.group(1)) >= 2000 and all(int(g) > 0 for g in m.groups())
    assert int(m.group(2)) + int(m.group(3)) == int(m.group(1))
    m = re.match(r"compared=(\d+)$", out["shard_slices"])
    assert m and int(m.group(1)) >= 16 * (200000 - 63) * 3
