"""GPU parity of the descheduling plan (ksim_engine_deschedule) and of the rescheduling replay.

Bar: the victims (event, node, devices, score, frag_before, frag_after, in eviction order) and the
budget equal tests/desched_ref.py's exactly -- `==` on the doubles -- for every replica, policy and
ratio; the replay of the extended stream equals the oracle's event for event.  The shapes are the
smallest at which the kernels can go wrong: the hand-made clusters of tests/test_desched_ref.py, a
64-node openb subset with deleted and failed pods and three replicas of different score policies, one
node holding more pods than a workgroup has threads, a cluster without a bound pod, and a cluster
whose per-node tables do not fit in LDS.  All of these have an untyped typical table and equal streams in every
replica; typed tables, ragged replicas, the stride edges of k_desched_select, both sides of its LDS / HBM switch
and a plan on an extended stream are in tests/test_gpu_desched_fuzz.py.  Every test needs a gfx950 device.
"""
import ctypes as C

import pytest

import desched_cases as cases
import desched_ref as ref
import ksim
import ksim.desched
import pyoracle as O
from test_gpu_report import assert_reports

pytestmark = pytest.mark.gpu

POLICIES = [ref.ONE_POD, ref.MULTI_POD]


def make_engine(case, scheds=("FGD",), report=False, run_mode=0):
    eng = ksim.Engine(len(case["nodes"]), len(scheds), run_mode=run_mode)
    for r, sched in enumerate(scheds):
        eng.set_nodes(r, case["nodes"])
        eng.set_typical(r, *case["typ"])
        eng.set_policy(r, sched)
    if report:
        eng.set_report(True)
    for r in range(len(scheds)):
        eng.load_events(r, case["events"], case["n"])
    return eng


_ORACLE = {}


def oracle_run(case, key, sched):
    """The oracle's replay of a case's stream, once per (case, score policy)."""
    if (key, sched) not in _ORACLE:
        pol, sel = cases.oracle_policy(sched)
        _ORACLE[key, sched] = O.run_events(case["onodes"], case["otyp"], case["oev"], policy=pol, gpu_sel=sel)[:2]
    return _ORACLE[key, sched]


def want_plan(case, key, sched, policy, ratio):
    res, state = oracle_run(case, key, sched)
    victims, budget, _ = ref.plan(case["onodes"], case["otyp"], case["oev"], res, state, policy, ratio)
    return ref.as_tuples(victims), budget


def got_plan(eng, r):
    victims, budget = eng.victims(r)
    return [(v.event, v.node, v.gpu_mask, v.score, v.frag_before, v.frag_after) for v in victims], budget


@pytest.fixture(scope="module")
def openb():
    return cases.openb64()


@pytest.mark.parametrize("run_mode,path", [(0, None), (1, "k_step"), (2, "k_replay"), (3, "k_memo"), (5, "k_hmemo")],
                         ids=["auto", "k_step", "k_replay", "k_memo", "k_hmemo"])
def test_hand_made_cluster(run_mode, path):
    # the plan reads only results and final node records: the same after every run path
    case = cases.hand()
    eng = make_engine(case, run_mode=run_mode)
    eng.run()
    assert path is None or eng.last_run_path() == path
    assert eng.results(0) == oracle_run(case, "hand", "FGD")[0]
    for policy in POLICIES:
        for ratio in (1.0, 0.1, 0.0):
            eng.deschedule(policy, ratio)
            assert got_plan(eng, 0) == want_plan(case, "hand", "FGD", policy, ratio), (policy, ratio)
    # the known answer itself (tests/test_desched_ref.py works it out)
    eng.deschedule(ref.MULTI_POD, 1.0)
    assert got_plan(eng, 0) == ([(5, 3, 1, 400, 800.0, 400.0), (3, 2, 1, 400, 800.0, 400.0)], 7)
    eng.close()


def test_openb_three_replicas_every_ratio(openb):
    eng = make_engine(openb, cases.OPENB_POLICIES)
    eng.run()
    for r, sched in enumerate(cases.OPENB_POLICIES):
        assert eng.results(r) == oracle_run(openb, "openb", sched)[0], sched
    n_victims = 0
    for policy in POLICIES:
        for ratio in (0.0, 0.05, 0.3, 1.0):
            assert eng.deschedule(policy, ratio) >= 0.0
            for r, sched in enumerate(cases.OPENB_POLICIES):
                got, want = got_plan(eng, r), want_plan(openb, "openb", sched, policy, ratio)
                assert got == want, (policy, ratio, sched)
                n_victims += len(got[0])
    assert n_victims > 0
    eng.close()


def test_planning_changes_no_state_and_can_be_repeated(openb):
    eng = make_engine(openb)
    eng.run()
    before = bytes(eng.nodes(0)), eng.results(0)
    eng.deschedule(ref.ONE_POD, 0.3)
    one = got_plan(eng, 0)
    eng.deschedule(ref.MULTI_POD, 1.0)
    assert got_plan(eng, 0) == want_plan(openb, "openb", "FGD", ref.MULTI_POD, 1.0)
    eng.deschedule(ref.ONE_POD, 0.3)
    assert got_plan(eng, 0) == one == want_plan(openb, "openb", "FGD", ref.ONE_POD, 0.3)
    assert (bytes(eng.nodes(0)), eng.results(0)) == before
    eng.close()


def test_more_pods_on_a_node_than_a_workgroup():
    case = cases.crowded()
    eng = make_engine(case)
    eng.run()
    assert eng.results(0) == oracle_run(case, "crowded", "FGD")[0]
    for policy in POLICIES:
        for ratio in (0.01, 1.0):
            eng.deschedule(policy, ratio)
            assert got_plan(eng, 0) == want_plan(case, "crowded", "FGD", policy, ratio)
    assert got_plan(eng, 0)[0] == [(293, 0, 0, 750, 1800.0, 1050.0)]
    eng.close()


def test_no_bound_pod():
    case = cases.empty()
    eng = make_engine(case)
    eng.run()
    for policy in POLICIES:
        eng.deschedule(policy, 1.0)
        assert got_plan(eng, 0) == ([], 0)
    eng.close()


def test_tables_beyond_lds(openb):
    # 3200 nodes: the per-node tables (20 B a node) pass the 60 KiB kept in LDS and sit in HBM.  The first 64
    # nodes are the openb subset, the others too small for any pod, so the answer is the subset's.
    n_big = 3200
    nodes = (ksim.Node * n_big)()
    C.memmove(nodes, openb["nodes"], C.sizeof(ksim.Node) * 64)
    onodes = list(openb["onodes"])
    for i in range(64, n_big):
        nodes[i].cpu_alloc_milli, nodes[i].mem_alloc_mib, nodes[i].pods_alloc, nodes[i].name_rank = 1, 1, 1001, i
        onodes.append(dict(name="~%05d" % i, cpu=1, mem=1, pods=1001, gpu=0, model=""))
    case = dict(openb, nodes=nodes, onodes=onodes)
    eng = make_engine(case)
    eng.run()
    res, state = O.run_events(onodes, case["otyp"], case["oev"])[:2]
    assert eng.results(0) == res
    for policy in POLICIES:
        eng.deschedule(policy, 0.3)
        victims, budget, _ = ref.plan(onodes, case["otyp"], case["oev"], res, state, policy, 0.3)
        assert got_plan(eng, 0) == (ref.as_tuples(victims), budget) and victims
    eng.close()


def test_error_returns(openb):
    eng = make_engine(openb)
    L = ksim.lib()
    n, b = C.c_int(-1), C.c_int(-1)
    assert L.ksim_engine_deschedule(eng.h, 0, 0.1) == ksim.KSIM_ESTATE          # before any run
    assert L.ksim_engine_get_victims(eng.h, 0, None, 0, C.byref(n), C.byref(b)) == ksim.KSIM_ESTATE
    eng.run()
    assert L.ksim_engine_get_victims(eng.h, 0, None, 0, C.byref(n), C.byref(b)) == ksim.KSIM_ESTATE  # before a plan
    for policy, ratio in ((2, 0.1), (-1, 0.1), (0, -0.5), (1, float("nan"))):
        assert L.ksim_engine_deschedule(eng.h, policy, ratio) == ksim.KSIM_EINVAL, (policy, ratio)
    assert L.ksim_engine_deschedule(eng.h, 0, 0.3) == ksim.KSIM_OK
    want, budget = want_plan(openb, "openb", "FGD", ref.ONE_POD, 0.3)
    assert len(want) >= 2
    short = (ksim.Victim * 1)()
    assert L.ksim_engine_get_victims(eng.h, 0, short, 1, C.byref(n), C.byref(b)) == ksim.KSIM_ERANGE
    assert (n.value, b.value) == (len(want), budget)                              # n_out is still set
    assert L.ksim_engine_get_victims(eng.h, 1, short, 1, C.byref(n), None) == ksim.KSIM_EINVAL
    # a new stream invalidates the run and its plan
    eng.load_events(0, openb["events"], 10)
    assert L.ksim_engine_deschedule(eng.h, 0, 0.3) == ksim.KSIM_ESTATE
    eng.close()


@pytest.mark.parametrize("policy", POLICIES)
def test_reschedule_end_to_end(openb, policy):
    scheds = cases.OPENB_POLICIES
    eng = make_engine(openb, scheds, report=True)
    eng.run()
    out = ksim.desched.run(eng, policy, 0.3)
    for r, sched in enumerate(scheds):
        victims, budget = want_plan(openb, "openb", sched, policy, 0.3)
        o = out[r]
        assert [v.event for v in o["victims"]] == [v[0] for v in victims] and o["budget"] == budget and victims
        n0, nv = openb["n"], len(victims)
        assert (o["n"], o["post_eviction"], o["post_deschedule"]) == (n0 + 2 * nv, n0 + nv - 1, n0 + 2 * nv - 1)
        oev = ref.extend_events(openb["oev"], [dict(event=v[0]) for v in victims])
        pol, sel = cases.oracle_policy(sched)
        want_res, want_state, want_rep = O.run_events(openb["onodes"], openb["otyp"], oev, policy=pol, gpu_sel=sel,
                                                      with_report=True)
        assert eng.results(r) == want_res, sched
        state = eng.nodes(r)
        for i, (cpu_left, mem_left, pods, gl) in enumerate(want_state):
            s = state[i]
            assert (s.cpu_alloc_milli - s.cpu_used_milli, s.mem_alloc_mib - s.mem_used_mib, s.pods_used) == \
                (cpu_left, mem_left, pods), (sched, i)
            assert [1000 - s.gpu_used_milli[g] if g < s.gpu_count else 0 for g in range(8)] == gl, (sched, i)
        got_rep = eng.reports(r)
        rows = [o["post_eviction"], o["post_deschedule"]]
        assert_reports([got_rep[i] for i in rows], [want_rep[i] for i in rows])
        # the evictions took effect and every victim came back through the ordinary cycle
        assert all(want_res[n0 + k][4] == ksim.DELETED and want_res[n0 + k][0] == victims[k][1] for k in range(nv))
    eng.close()
