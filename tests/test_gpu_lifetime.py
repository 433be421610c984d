"""The engine's device resources over its life: event and report buffers replaced under a live engine, the
report switched on and off between runs, engines created and closed over and over in one process, and the
temporaries of time_steps.

Every case is the openb default cluster (1213 nodes) with at most 300 events per replica.  After every run the
results, the final node records and (where the report is on) every event's report row equal the oracle's for
the stream that was loaded, so a replica left pointing at a replaced buffer, or a buffer of the wrong size,
shows up as a wrong row.
"""
import pytest

import helpers
import ksim
import pyoracle as O
import test_gpu_run_plan as RP
from test_gpu_report import assert_reports

pytestmark = pytest.mark.gpu

POLICIES = ["FGD", "FGD", "BestFit", "GpuPacking"]
ENV = ("KSIM_VARIANT", "KSIM_TEST", "KSIM_SIDE_STREAMS", "KSIM_PROFILE", "KSIM_GROUP_TIMES")


@pytest.fixture(scope="module")
def world():
    trace = ksim.Trace.openb("default")
    rp = trace.replay(seed=44)
    return dict(trace=trace, rp=rp, typical=trace.typical(), onodes=helpers.oracle_nodes(trace, rp),
                otyp=helpers.oracle_typical(trace), oracle={})


@pytest.fixture(autouse=True)
def plain_env(monkeypatch):
    for var in ENV:
        monkeypatch.delenv(var, raising=False)


def oracle(w, policy, n_ev):
    """The oracle's (results, final state, reports) of one policy over the first n_ev events; computed once."""
    key = (policy, n_ev)
    if key not in w["oracle"]:
        pol, sel = RP.ORACLE[policy]
        w["oracle"][key] = O.run_events(w["onodes"], w["otyp"], helpers.oracle_events(w["trace"], w["rp"], n_ev),
                                        policy=pol, gpu_sel=sel, seed=RP.SEED, threads=16, with_report=True)
    return w["oracle"][key]


def make_engine(w, specs, report=False, **engine):
    """An engine of the replicas `specs` (test_gpu_run_plan.rep dicts), their events loaded."""
    trace, rp = w["trace"], w["rp"]
    arr, n = w["typical"]
    eng = ksim.Engine(trace.num_nodes, len(specs), **(engine or dict(wgs_per_replica=1)))
    try:
        if report:
            eng.set_report(True)
        for r, spec in enumerate(specs):
            eng.set_nodes(r, rp.nodes)
            eng.set_typical(r, arr, n)
            eng.set_policy(r, spec["policy"], seed=RP.SEED)
            if spec.get("wgs"):
                eng.set_replica_wgs(r, spec["wgs"])
            eng.load_events(r, rp.events, spec["n_ev"])
    except Exception:
        eng.close()
        raise
    return eng


def check(w, eng, specs, report):
    """The last run of `eng` against the oracle: results, final node records, report rows."""
    for r, spec in enumerate(specs):
        want, want_state, want_rep = oracle(w, spec["policy"], spec["n_ev"])
        res, state = eng.results(r), eng.nodes(r)
        bad = [i for i, (a, b) in enumerate(zip(res, want)) if a != b]
        assert len(res) == len(want) == spec["n_ev"] and not bad, (r, spec["policy"], bad[:1])
        for i, (cpu_left, _, pods, gl) in enumerate(want_state):
            s = state[i]
            assert s.cpu_alloc_milli - s.cpu_used_milli == cpu_left and s.pods_used == pods, (r, i)
            assert [1000 - s.gpu_used_milli[g] if g < s.gpu_count else 0 for g in range(8)] == gl, (r, i)
        if report:
            assert_reports(eng.reports(r), want_rep)


def test_reload_events(world):
    # the per-replica event, result and report buffers replaced by larger and then smaller ones while the
    # replicas point at them
    specs = [RP.rep(p, 100) for p in POLICIES]
    eng = make_engine(world, specs, report=True)
    try:
        for n_ev in (100, 300, 60):
            specs = [RP.rep(p, n_ev) for p in POLICIES]
            for r in range(len(specs)):
                eng.load_events(r, world["rp"].events, n_ev)
            eng.run()
            check(world, eng, specs, report=True)
    finally:
        eng.close()


def test_report_on_off_on(world):
    specs = [RP.rep(p) for p in POLICIES]
    eng = make_engine(world, specs)
    try:
        for report in (None, True, False, True):
            if report is not None:
                eng.set_report(report)
            eng.run()
            check(world, eng, specs, report=bool(report))
    finally:
        eng.close()


def test_create_run_close_twelve_times(world, monkeypatch):
    # side streams, the residency gate's flags, the overlapped report's queue and both memoised plans, made and
    # released a dozen times over
    monkeypatch.setenv("KSIM_TEST", "report_overlap=1")
    specs = RP.CASES["d-split-fgd"]["reps"]
    kernels = []
    for _ in range(12):
        eng = make_engine(world, specs, report=True)
        try:
            eng.run()
            kernels.append(eng.last_run_kernels())
            check(world, eng, specs, report=True)
        finally:
            eng.close()
    print("kernels", kernels[0])
    assert kernels[0] == RP.CASES["d-split-fgd"]["want"][0]
    assert all(k == kernels[0] for k in kernels)


def test_time_steps_then_run(world):
    specs = [RP.rep(p) for p in POLICIES]
    eng = make_engine(world, specs)
    try:
        assert eng.time_steps(8) > 0
        eng.run()
        check(world, eng, specs, report=False)
    finally:
        eng.close()
