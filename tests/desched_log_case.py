"""The descheduling log-contract case: tests/log_case.py's cluster (243 nodes, 3000 events, FGD) with a
descheduling stage, written as `simon apply`'s log from the oracle or from the GPU -- TEST INFRASTRUCTURE.

Two stages: cosSim at the reference's bars and fragOnePod, both at ratio 0.1.  The oracle's log is built from
the restatements of the plan (tests/desched_cos_ref.py, tests/desched_ref.py) and three oracle replays: the
original stream (InitSchedule), the extended stream cut after the last delete (PostEviction) and the whole
extended stream (PostDeschedule).  tests/golden/make_desched_log_golden.py passes it through the reference's
own scripts/analysis.py and commits what that produced; tests/test_desched_log_contract.py (CPU) and
tests/test_gpu_desched_log_contract.py (GPU) rebuild the log and compare.
"""
import ksim
import ksim.analysis as A
import ksim.desched

import desched_cos_ref as cos
import desched_ref as ref
import helpers
import log_case

SCHED, RATIO = "FGD", 0.1
POLICIES = ["cosSim", "fragOnePod"]


def oracle_final(nodes, state):
    return [dict(cpu_alloc=nd["cpu"], cpu_used=nd["cpu"] - st[0], mem_alloc_mib=nd["mem"],
                 mem_used_mib=nd["mem"] - st[1], gpu_count=nd["gpu"],
                 gpu_used=[1000 - g if j < nd["gpu"] else 0 for j, g in enumerate(st[3])])
            for nd, st in zip(nodes, state)]


def oracle_plan(policy):
    """(nodes, typical, events, results, state, victims, budget, info) of the case under `policy`."""
    import pyoracle as O
    t, rp, keep = log_case.inputs()
    nodes = helpers.oracle_subset(t, rp, keep)
    typ = helpers.oracle_typical(t)
    ev = helpers.oracle_events(t, rp, log_case.N_EVENTS)
    res, state, _ = O.run_events(nodes, typ, ev, policy=O.POL_FGD, gpu_sel=O.SEL_FGD)
    if policy == "cosSim":
        victims, budget, info = cos.plan(nodes, ev, res, state, RATIO)
    else:
        victims, budget, info = ref.plan(nodes, typ, ev, res, state, policy, RATIO)
    return nodes, typ, ev, res, state, victims, budget, info


def oracle_log(path, policy):
    """The log of the oracle's run and descheduling stage.  Returns (victims, budget)."""
    import pyoracle as O
    t, rp, _ = log_case.inputs()
    nodes, typ, ev, _, state0, victims, budget, _ = oracle_plan(policy)
    n, nv = len(ev), len(victims)
    ext = ref.extend_events(ev, victims)
    run = lambda events: O.run_events(nodes, typ, events, policy=O.POL_FGD, gpu_sel=O.SEL_FGD, with_report=True)
    _, state1, _ = run(ext[:n + nv])
    res, state2, reps = run(ext)
    reports = [dict(r, frag_bins=r["frag_bins_exact"]) for r in reps]
    power = [dict(cpu_w=r["power_cpu"], gpu_w=r["power_gpu"]) for r in reps]
    assert all(r["power_invalid"] == 0 for r in reps)
    names, reprs, n_orig = log_case.pod_lines(t, rp, n)
    stage_nodes = dict(InitSchedule=oracle_final(nodes, state0), PostEviction=oracle_final(nodes, state1),
                       PostDeschedule=oracle_final(nodes, state2))
    A.write_desched_log(path, reports, [v["event"] for v in victims], policy, budget, stage_nodes, pod_names=names,
                        power=power, pods=reprs, results=[r[4] for r in res], n_original=n_orig)
    return victims, budget


def node_dicts(recs):
    return [dict(cpu_alloc=n.cpu_alloc_milli, cpu_used=n.cpu_used_milli, mem_alloc_mib=n.mem_alloc_mib,
                 mem_used_mib=n.mem_used_mib, gpu_count=n.gpu_count, gpu_used=list(n.gpu_used_milli)) for n in recs]


def engine_log(path, policy):
    """The same log from the GPU engine: ksim.desched.run(..., stages=True), the device's reports and power
    reports of the extended stream.  Returns the victims' events and the budget."""
    t, rp, keep = log_case.inputs()
    nodes = helpers.subset_nodes(rp, keep)
    arr, n = t.typical()
    eng = ksim.Engine(len(keep), 1)
    try:
        eng.set_report(True)
        eng.set_nodes(0, nodes)
        eng.set_typical(0, arr, n)
        eng.set_policy(0, SCHED)
        eng.set_power_model(0, t.power_model())
        eng.load_events(0, rp.events, log_case.N_EVENTS)
        eng.run()
        o = ksim.desched.run(eng, policy, RATIO, stages=True)[0]
        reports, power = eng.reports(0), eng.power_reports(0)
        assert all(p["invalid_nodes"] == 0 for p in power)
        names, reprs, n_orig = log_case.pod_lines(t, rp, log_case.N_EVENTS)
        stage_nodes = {k: node_dicts(v) for k, v in o["stage_nodes"].items()}
        victims = [v.event for v in o["victims"]]
        A.write_desched_log(path, reports, victims, policy, o["budget"], stage_nodes, pod_names=names, power=power,
                            pods=reprs, results=[r[4] for r in eng.results(0)], n_original=n_orig)
        return victims, o["budget"]
    finally:
        eng.close()
