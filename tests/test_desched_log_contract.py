"""The log contract of a descheduling run: the stage blocks the reference logs after InitSchedule.

tests/golden/desched_log_golden.json holds what the reference's scripts/analysis.py (log_to_csv) produced
from the oracle's log of tests/log_case.py's cluster followed by a descheduling stage (cosSim at the
reference's bars, fragOnePod; tests/desched_log_case.py, tests/golden/make_desched_log_golden.py): the
analysis.csv row with its *_init_schedule, *_post_eviction and *_post_deschedule columns.  Here the log is
rebuilt from the oracle (byte-identical: same sha256) and read back by ksim.analysis' restatement of that
parser, which must give the reference script's row.  The GPU side (tests/test_gpu_desched_log_contract.py)
writes the same bytes from the device's plan and reports.
"""
import hashlib
import json
import os

import pytest

import desched_log_case as case
import ksim.analysis as A
import log_case

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "desched_log_golden.json")) as f:
    GOLD = json.load(f)
with open(os.path.join(HERE, "golden", "log_golden.json")) as f:
    INIT = json.load(f)["policies"]["FGD"]


@pytest.mark.parametrize("policy", case.POLICIES)
def test_oracle_log_read_like_the_reference_harness(policy, tmp_path):
    log = tmp_path / "run.log"
    victims, budget = case.oracle_log(log, policy)
    want = GOLD["policies"][policy]
    assert ([v["event"] for v in victims], budget) == (want["victims"], want["budget"])
    assert hashlib.sha256(log.read_bytes()).hexdigest() == want["log_sha256"]
    with open(log) as f:
        lines = f.readlines()
    assert len(lines) == want["log_lines"]
    got = A.parse_log_full(lines)
    assert {k: float(v) for k, v in got["row"].items()} == want["row"]
    # the stage is not empty, and all three blocks are there with every column of the InitSchedule one
    assert len(victims) >= 4 and budget == 181
    init = sorted(k for k in want["row"] if k.endswith("_init_schedule"))
    for tag in ("_post_eviction", "_post_deschedule"):
        assert sorted(k[:-len(tag)] + "_init_schedule" for k in want["row"] if k.endswith(tag)) == init
    # the InitSchedule part is the plain run's: the same columns as the log without a descheduling stage
    assert {k: v for k, v in want["row"].items() if k.endswith("_init_schedule")} == \
        {k: v for k, v in INIT["row"].items() if k.endswith("_init_schedule")}
    # evicting frees GPU milli, rescheduling takes them back
    assert want["row"]["milli_gpu_amount_post_eviction"] < want["row"]["milli_gpu_amount_init_schedule"]
    assert want["row"]["milli_gpu_amount_post_eviction"] < want["row"]["milli_gpu_amount_post_deschedule"]


def test_stage_lines_in_the_reference_order(tmp_path):
    log = tmp_path / "run.log"
    victims, budget = case.oracle_log(log, "cosSim")
    with open(log) as f:
        msgs = [ln.split(A.INFOMSG)[1][1:-2] if A.INFOMSG in ln else "" for ln in f.readlines()]
    nv = len(victims)
    at = lambda text: [i for i, m in enumerate(msgs) if text in m]
    blocks = [at("Cluster Analysis Results (%s)" % t) for t in ("InitSchedule", "PostEviction", "PostDeschedule")]
    assert [len(b) for b in blocks] == [1, 1, 1]
    init, evicted, done = (b[0] for b in blocks)
    (cap,) = at("maximum number of pods that can be descheduled: %d, deschedule policy: cosSim" % budget)
    (n_desched,) = at("[DescheduleCluster] Num of Descheduled Pods: %d" % nv)
    (n_failed,) = at("[DescheduleCluster] Num of Failed Pods: ")
    (last,) = at("unscheduled pods")
    assert init < cap < evicted < n_desched < n_failed < done < last == len(msgs) - 1
    # the evictions are silent: no attempt-to-delete line for a victim; the re-creations count from 0
    assert not [i for i in at("attempt to delete") if i > init]
    stage = [m for m in msgs[n_desched:n_failed] if "attempt to create" in m]
    names = log_case.pod_lines(*log_case.inputs()[:2], log_case.N_EVENTS)[0]
    assert stage == ["[%d] attempt to create pod(%s)\\n" % (k, names[v["event"]]) for k, v in enumerate(victims)]
    # the arrived counters restart with the stage (simulator.go:384-385): the first re-creation's is its own
    alloc = [m for m in msgs[n_desched:n_failed] if m.startswith("[Alloc]")]
    ev = log_case.pod_lines(*log_case.inputs()[:2], log_case.N_EVENTS)[1][victims[0]["event"]]
    assert alloc[0].endswith("Arrived GPU Milli: %d\\n" % (ev[1] * ev[2]))
    # core.go:218: one more cluster report after the PostDeschedule block, without a [Power] line
    tail = msgs[done:last]
    assert [m.split(";")[0] for m in tail if m.startswith("[")] == ["[Report]", "[Alloc]", "[AllocCPU]"]


def test_write_desched_log_without_a_victim(tmp_path):
    rep = dict(frag_bins=[0.0] * 7, used_nodes=1, used_gpus=1, used_gpu_milli=500, total_gpus=1, arrived_gpu_milli=500,
               used_cpu_milli=1000, arrived_cpu_milli=1000)
    node = [dict(cpu_alloc=4000, cpu_used=1000, mem_alloc_mib=10, mem_used_mib=0, gpu_count=1, gpu_used=[500] + [0] * 7)]
    log = tmp_path / "none.log"
    A.write_desched_log(log, [rep], [], "fragMultiPod", 1, dict(InitSchedule=node, PostEviction=node,
                                                                 PostDeschedule=node))
    with open(log) as f:
        lines = f.readlines()
    row = A.parse_log_full(lines)["row"]
    assert row["milli_gpu_amount_post_eviction"] == row["milli_gpu_amount_post_deschedule"] == 500.0
    assert "Num of Descheduled Pods: 0" in "".join(lines) and "Num of Failed Pods: 0" in "".join(lines)
    # nothing was descheduled: the last report's arrived counters are the empty stage's
    assert lines[-2].endswith('Arrived GPU Milli: 0\\n"\n') and lines[-1].endswith('Arrived CPU Milli: 0\\n"\n')
    with pytest.raises(ValueError):
        A.write_desched_log(log, [], [], "cosSim", 0, dict(InitSchedule=node, PostEviction=node, PostDeschedule=node))
