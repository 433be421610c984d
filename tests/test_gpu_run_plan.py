"""What a run decides, pinned through the last_run_* getters: which kernels a set of replicas is replayed
on, in how many launches on how many side streams, at which width, behind which gate.

Every case is the openb default cluster with at most 300 events per replica (ragged: the mixed launch
orders its replicas longest stream first) at wgs_per_replica=1 unless the case says otherwise.  The expected
tuples are literals, observed on the engine as it stood before its run path was split into a plan and
per-kernel launchers; the side-stream counts follow GPU_MAX_HW_QUEUES (no more side streams than hardware
queues).  Each replica's decisions and final state are also compared with the oracle, so a wrong replica
order or rep_list offset shows up as well.  The plan itself is host-only code (make_run_plan, ksim_plan.hpp):
tests/native_host/plan_check.cpp holds these nine cases as planner inputs with their plans written out, and
must be kept in step with CASES.
"""
import os

import pytest

import helpers
import ksim
import pyoracle as O

pytestmark = pytest.mark.gpu

SEED = 5
N_EV = 300
ORACLE = {"FGD": (O.POL_FGD, O.SEL_FGD), "BestFit": (O.POL_BESTFIT, O.SEL_BEST), "DotProd": (O.POL_DOTPROD, O.SEL_BEST),
          "GpuPacking": (O.POL_PACKING, O.SEL_BEST), "GpuClustering": (O.POL_CLUSTERING, O.SEL_BEST),
          "Random": (O.POL_RANDOM, O.SEL_RANDOM), "PWR 500 FGD 500": (O.POL_PWR_FGD, O.SEL_FGD)}


def side_streams(groups):
    """Side streams `groups` concurrent groups take: one each up to the process's hardware queues."""
    q = int(os.environ.get("GPU_MAX_HW_QUEUES", "0") or 0)
    return min(groups, max(1, min(q if q > 0 else 4, 6)))


def rep(policy, n_ev=N_EV, **kw):
    return dict(policy=policy, n_ev=n_ev, **kw)


# replicas; engine arguments; environment; expected (kernels, (launches, side streams), wgs, path, gate, overlap)
CASES = {
    "a-fgd-beside-mix": dict(
        reps=[rep("FGD"), rep("FGD", 260), rep("BestFit", 280), rep("GpuPacking")],
        want=(["k_hmemo", "k_scan1_mix"], (2, side_streams(2)), 1, "memo+k_replay", 1, 0)),
    "b-overlapped-report": dict(
        reps=[rep("FGD"), rep("FGD", 260), rep("BestFit", 280), rep("GpuPacking")],
        report=True, env={"KSIM_TEST": "report_overlap=1"},
        want=(["k_hmemo", "k_scan1_mix"], (2, side_streams(2)), 1, "memo+k_replay", 1, 2)),
    "c-memo-back-to-back": dict(
        reps=[rep("FGD"), rep("BestFit")], engine=dict(wgs_per_replica=0),
        want=(["k_memo", "k_replay"], (2, 0), 64, "memo+k_replay", 0, 0)),
    "d-split-fgd": dict(
        reps=[rep("FGD", wgs=6), rep("FGD", 260), rep("BestFit", 280), rep("GpuPacking")],
        want=(["k_memo", "k_hmemo", "k_scan1_mix"], (3, side_streams(2)), 1, "memo+k_replay", 1, 0)),
    "e-deletes-general-replay": dict(
        reps=[rep("GpuPacking", deletes=True), rep("BestFit")],
        want=(["k_replay"], (2, side_streams(2)), 1, "k_replay", 0, 0)),
    "f-random-go-last": dict(
        reps=[rep("Random", go=True), rep("BestFit", 280), rep("GpuPacking")],
        want=(["k_scan1_mix", "k_random_go"], (2, side_streams(2)), 1, "k_replay", 0, 0)),
    "g-round-robin-1": dict(
        reps=[rep("BestFit"), rep("DotProd", 260), rep("GpuPacking", 280), rep("GpuClustering", 240), rep("Random")],
        env={"KSIM_VARIANT": "scan1_mix=0", "KSIM_SIDE_STREAMS": "1"},
        want=(["k_scan1"], (5, 1), 1, "k_scan1", 0, 0)),
    "g-round-robin-2": dict(
        reps=[rep("BestFit"), rep("DotProd", 260), rep("GpuPacking", 280), rep("GpuClustering", 240), rep("Random")],
        env={"KSIM_VARIANT": "scan1_mix=0", "KSIM_SIDE_STREAMS": "2"},
        want=(["k_scan1"], (5, 2), 1, "k_scan1", 0, 0)),
    "h-pwr-fgd-replay": dict(
        reps=[rep("PWR 500 FGD 500")], engine=dict(run_mode=2, wgs_per_replica=1),
        want=(["k_replay"], (1, 0), 1, "k_replay", 0, 0)),
}


@pytest.fixture(scope="module")
def world():
    trace = ksim.Trace.openb("default")
    rp = trace.replay(seed=44)
    return dict(trace=trace, rp=rp, typical=trace.typical(), go=trace.go_state(seed=44),
                deletes=helpers.delete_stream(trace, rp, 230, p_delete=0.3, seed=3),
                onodes=helpers.oracle_nodes(trace, rp), otyp=helpers.oracle_typical(trace), oracle={})


def oracle(w, spec):
    """The oracle's (results, final state) of one replica; computed once per distinct replica, never changed."""
    key = (spec["policy"], spec["n_ev"], bool(spec.get("deletes")), bool(spec.get("go")))
    if key not in w["oracle"]:
        pol, sel = ORACLE[spec["policy"]]
        name, weights = ksim.parse_policy(spec["policy"])
        w_pwr, w_fgd = weights if weights else (0, 0)
        oev = w["deletes"][1] if spec.get("deletes") else helpers.oracle_events(w["trace"], w["rp"], spec["n_ev"])
        want, state, _ = O.run_events(w["onodes"], w["otyp"], oev, policy=pol, gpu_sel=sel, seed=SEED, threads=16,
                                      w_pwr=w_pwr, w_fgd=w_fgd, go_stream=w["go"][:3] if spec.get("go") else None)
        w["oracle"][key] = (want, state)
    return w["oracle"][key]


@pytest.mark.parametrize("case", sorted(CASES))
def test_run_plan(world, case, monkeypatch):
    c = CASES[case]
    for var in ("KSIM_VARIANT", "KSIM_TEST", "KSIM_SIDE_STREAMS", "KSIM_PROFILE", "KSIM_GROUP_TIMES"):
        monkeypatch.delenv(var, raising=False)
    for var, val in c.get("env", {}).items():
        monkeypatch.setenv(var, val)
    trace, rp = world["trace"], world["rp"]
    arr, n = world["typical"]
    reps = c["reps"]
    eng = ksim.Engine(trace.num_nodes, len(reps), **c.get("engine", dict(wgs_per_replica=1)))
    try:
        if c.get("report"):
            eng.set_report(True)
        for r, spec in enumerate(reps):
            eng.set_nodes(r, rp.nodes)
            eng.set_typical(r, arr, n)
            eng.set_policy(r, spec["policy"], seed=SEED)
            if spec["policy"].startswith("PWR"):
                eng.set_power_model(r, trace.power_model())
            if spec.get("go"):
                eng.set_go_stream(r, world["go"])
            if spec.get("wgs"):
                eng.set_replica_wgs(r, spec["wgs"])
            if spec.get("deletes"):
                evs = world["deletes"][0]
                eng.load_events(r, evs, len(evs))
            else:
                eng.load_events(r, rp.events, spec["n_ev"])
        eng.run()
        seen = (eng.last_run_kernels(), eng.last_run_launches(), eng.last_run_wgs(), eng.last_run_path(),
                eng.last_run_gate()[0], eng.last_run_report_overlap())
        got = [(eng.results(r), eng.nodes(r)) for r in range(len(reps))]
    finally:
        eng.close()
    print("run plan %s: %r" % (case, seen))
    assert seen == c["want"]
    for r, spec in enumerate(reps):
        want, want_state = oracle(world, spec)
        res, state = got[r]
        bad = [i for i, (a, b) in enumerate(zip(res, want)) if a != b]
        assert len(res) == len(want) and not bad, (r, spec["policy"], bad[:1])
        for i, (cpu_left, _, pods, gl) in enumerate(want_state):
            s = state[i]
            assert s.cpu_alloc_milli - s.cpu_used_milli == cpu_left and s.pods_used == pods, (r, i)
            assert [1000 - s.gpu_used_milli[g] if g < s.gpu_count else 0 for g in range(8)] == gl, (r, i)


# Two of CASES with the same replica count and engine arguments, one after the other on the same engine.  (CASES has
# no k_random_go-only case, so no pair ends on one after a memo case: "f-random-go-last" runs k_scan1_mix beside it and
# is the only case of three replicas.)
PAIRS = [("a-fgd-beside-mix", "d-split-fgd"), ("d-split-fgd", "a-fgd-beside-mix"), ("g-round-robin-1", "g-round-robin-2")]


def set_case(eng, world, c, monkeypatch):
    """Case c's environment, policies, hints and events on an engine that may have run another case before."""
    for var in ("KSIM_VARIANT", "KSIM_TEST", "KSIM_SIDE_STREAMS", "KSIM_PROFILE", "KSIM_GROUP_TIMES"):
        monkeypatch.delenv(var, raising=False)
    for var, val in c.get("env", {}).items():
        monkeypatch.setenv(var, val)
    for r, spec in enumerate(c["reps"]):
        assert not (spec.get("go") or spec.get("deletes") or spec["policy"].startswith("PWR"))  # (none of PAIRS)
        eng.set_policy(r, spec["policy"], seed=SEED)
        eng.set_replica_wgs(r, spec.get("wgs", 0))
        eng.load_events(r, world["rp"].events, spec["n_ev"])


@pytest.mark.parametrize("first,second", PAIRS, ids=["%s-then-%s" % (a[0], b[0]) for a, b in PAIRS])
def test_two_runs_report_each_run_alone(world, first, second, monkeypatch):
    assert len(CASES[first]["reps"]) == len(CASES[second]["reps"])
    assert CASES[first].get("engine") == CASES[second].get("engine") and not CASES[first].get("report")
    trace, rp = world["trace"], world["rp"]
    arr, n = world["typical"]
    R = len(CASES[first]["reps"])
    eng = ksim.Engine(trace.num_nodes, R, **CASES[first].get("engine", dict(wgs_per_replica=1)))
    seen, got = {}, {}
    try:
        for r in range(R):
            eng.set_nodes(r, rp.nodes)
            eng.set_typical(r, arr, n)
        for case in (first, second):
            set_case(eng, world, CASES[case], monkeypatch)
            eng.run()
            seen[case] = (eng.last_run_kernels(), eng.last_run_launches(), eng.last_run_wgs(), eng.last_run_path(),
                          eng.last_run_gate()[0], eng.last_run_report_overlap())
            got[case] = [eng.results(r) for r in range(R)]
    finally:
        eng.close()
    print("two runs %s, %s: %r" % (first, second, seen))
    for case in (first, second):
        assert seen[case] == CASES[case]["want"], case
        for r, spec in enumerate(CASES[case]["reps"]):
            want, _ = oracle(world, spec)
            bad = [i for i, (a, b) in enumerate(zip(got[case][r], want)) if a != b]
            assert len(got[case][r]) == len(want) and not bad, (case, r, spec["policy"], bad[:1])
