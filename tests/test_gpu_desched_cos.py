"""GPU parity of the cosSim descheduling plan (ksim_engine_deschedule_cossim) and of its rescheduling replay.

Bar: the victims (event, node, devices, milli-GPU left, similarity, in eviction order) and the budget equal
tests/desched_cos_ref.py's exactly -- `==` on the doubles -- for every replica, pair of bars and ratio; the
replay of the extended stream equals the oracle's event for event.  The shapes are the smallest at which the
kernels can go wrong: the hand-made cluster of tests/test_desched_cos_ref.py, a 64-node openb subset with
deleted and failed pods and three replicas of different score policies, one node holding more pods than a
workgroup has threads, a cluster without a bound pod, 600 flat nodes whose order needs both sort keys over
more nodes than a workgroup has threads (at ratio 0.5 and, for the upper half of the sorted order, 1.0), and a
cluster whose per-node tables do not fit in LDS.  Typed typical tables, ragged replicas, the stride edges of
k_cos_select, both sides of its LDS / HBM switch and a plan on an extended stream are in
tests/test_gpu_desched_fuzz.py.  Every test needs a gfx950 device.
"""
import ctypes as C

import pytest

import desched_cases as cases
import desched_cos_cases as cos_cases
import desched_cos_ref as cos
import desched_ref as ref
import ksim
import ksim.desched
import pyoracle as O
from test_desched_cos_ref import SIM_6, SIM_22
from test_gpu_desched import make_engine, oracle_run
from test_gpu_report import assert_reports

pytestmark = pytest.mark.gpu

BARS = [(2000, 500), (32000, 300), (2 ** 30, 0)]
WIDE = (2 ** 30, 0)


def want_plan(case, key, sched, ratio, bars=(cos.CPU_BAR, cos.GPU_BAR)):
    res, state = oracle_run(case, key, sched)
    victims, budget, _ = cos.plan(case["onodes"], case["oev"], res, state, ratio, *bars)
    return cos.as_tuples(victims), budget


def got_plan(eng, r):
    victims, budget = eng.cos_victims(r)
    return [(v.event, v.node, v.gpu_mask, v.gpu_left_milli, v.similarity) for v in victims], budget


@pytest.fixture(scope="module")
def openb():
    return cases.openb64()


@pytest.mark.parametrize("run_mode,path", [(0, None), (1, "k_step"), (2, "k_replay"), (3, "k_memo"), (5, "k_hmemo")],
                         ids=["auto", "k_step", "k_replay", "k_memo", "k_hmemo"])
def test_hand_made_cluster(run_mode, path):
    # the plan reads only results and final node records: the same after every run path
    case = cos_cases.hand()
    eng = make_engine(case, run_mode=run_mode)
    eng.run()
    assert path is None or eng.last_run_path() == path
    assert eng.results(0) == oracle_run(case, "cos_hand", "FGD")[0]
    for bars in BARS + [(2001, 500), (2000, 499)]:
        for ratio in (1.0, 0.2, 0.0):
            eng.deschedule_cossim(ratio, *bars)
            assert got_plan(eng, 0) == want_plan(case, "cos_hand", "FGD", ratio, bars), (bars, ratio)
    # the known answer itself (tests/test_desched_cos_ref.py works it out)
    eng.deschedule_cossim(1.0)
    assert got_plan(eng, 0) == ([(4, 3, 1, 1200, SIM_22), (2, 2, 1, 1200, SIM_22), (8, 6, 1, 800, SIM_6)], 9)
    eng.deschedule_cossim(0.2)
    assert got_plan(eng, 0) == ([(4, 3, 1, 1200, SIM_22), (2, 2, 1, 1200, SIM_22)], 2)
    eng.close()


def test_openb_three_replicas_every_bar_and_ratio(openb):
    eng = make_engine(openb, cases.OPENB_POLICIES)
    eng.run()
    for r, sched in enumerate(cases.OPENB_POLICIES):
        assert eng.results(r) == oracle_run(openb, "openb", sched)[0], sched
    n_victims = 0
    for bars in BARS:
        for ratio in (0.0, 0.05, 0.3, 1.0):
            assert eng.deschedule_cossim(ratio, *bars) >= 0.0
            for r, sched in enumerate(cases.OPENB_POLICIES):
                got, want = got_plan(eng, r), want_plan(openb, "openb", sched, ratio, bars)
                assert got == want, (bars, ratio, sched)
                n_victims += len(got[0])
                if bars == WIDE and ratio == 0.05:  # the budget cuts the nodes with a victim
                    assert len(got[0]) == got[1] == 20
    assert n_victims > 0
    eng.close()


def test_more_pods_on_a_node_than_a_workgroup():
    case = cases.crowded()
    eng = make_engine(case)
    eng.run()
    assert eng.results(0) == oracle_run(case, "crowded", "FGD")[0]
    for ratio in (0.01, 1.0):
        eng.deschedule_cossim(ratio)
        assert got_plan(eng, 0) == want_plan(case, "crowded", "FGD", ratio)
    # 299 pods tie at the least similarity: the first of them
    assert [v[:4] for v in got_plan(eng, 0)[0]] == [(3, 0, 0, 1800)]
    eng.close()


def test_no_bound_pod():
    case = cases.empty()
    eng = make_engine(case)
    eng.run()
    eng.deschedule_cossim(1.0, *WIDE)
    assert got_plan(eng, 0) == ([], 0)
    eng.close()


def test_flat_cluster_order_needs_both_keys():
    case = cos_cases.flat()
    eng = make_engine(case)
    eng.run()
    assert eng.results(0) == oracle_run(case, "flat", "FGD")[0]
    eng.deschedule_cossim(0.5)
    got, want = got_plan(eng, 0), want_plan(case, "flat", "FGD", 0.5)
    assert got == want and len(got[0]) == got[1] == 300
    # the whole sorted order, its upper half included
    eng.deschedule_cossim(1.0)
    got, want = got_plan(eng, 0), want_plan(case, "flat", "FGD", 1.0)
    assert got == want and len(got[0]) == got[1] == 600
    eng.close()


def test_tables_beyond_lds(openb):
    # 3200 nodes: the per-node tables (24 B a node) pass the 60 KiB kept in LDS and sit in HBM.  The first 64
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
    for ratio in (0.05, 0.3):
        eng.deschedule_cossim(ratio, *WIDE)
        victims, budget, _ = cos.plan(onodes, case["oev"], res, state, ratio, *WIDE)
        assert got_plan(eng, 0) == (cos.as_tuples(victims), budget) and victims
    eng.close()


def test_error_returns_and_plan_exclusivity(openb):
    eng = make_engine(openb)
    L = ksim.lib()
    n, b = C.c_int(-1), C.c_int(-1)
    assert L.ksim_engine_deschedule_cossim(eng.h, 0.1, 2000, 500) == ksim.KSIM_ESTATE     # before any run
    assert L.ksim_engine_get_cos_victims(eng.h, 0, None, 0, C.byref(n), C.byref(b)) == ksim.KSIM_ESTATE
    eng.run()
    assert L.ksim_engine_get_cos_victims(eng.h, 0, None, 0, C.byref(n), C.byref(b)) == ksim.KSIM_ESTATE  # no plan
    for ratio, cpu_bar, gpu_bar in ((-0.5, 2000, 500), (float("nan"), 2000, 500), (0.1, -1, 500), (0.1, 2000, -1)):
        assert L.ksim_engine_deschedule_cossim(eng.h, ratio, cpu_bar, gpu_bar) == ksim.KSIM_EINVAL
    assert L.ksim_engine_deschedule_cossim(eng.h, 0.3, *WIDE) == ksim.KSIM_OK
    want, budget = want_plan(openb, "openb", "FGD", 0.3, WIDE)
    assert len(want) >= 2
    short = (ksim.CosVictim * 1)()
    assert L.ksim_engine_get_cos_victims(eng.h, 0, short, 1, C.byref(n), C.byref(b)) == ksim.KSIM_ERANGE
    assert (n.value, b.value) == (len(want), budget)                                      # n_out is still set
    assert L.ksim_engine_get_cos_victims(eng.h, 1, short, 1, C.byref(n), None) == ksim.KSIM_EINVAL
    # an engine holds one plan
    assert L.ksim_engine_get_victims(eng.h, 0, None, 0, C.byref(n), C.byref(b)) == ksim.KSIM_ESTATE
    assert L.ksim_engine_deschedule(eng.h, 0, 0.3) == ksim.KSIM_OK
    assert L.ksim_engine_get_cos_victims(eng.h, 0, None, 0, C.byref(n), C.byref(b)) == ksim.KSIM_ESTATE
    assert L.ksim_engine_get_victims(eng.h, 0, None, 0, C.byref(n), C.byref(b)) in (ksim.KSIM_OK, ksim.KSIM_ERANGE)
    # a new stream invalidates the run and its plan
    assert L.ksim_engine_deschedule_cossim(eng.h, 0.3, *WIDE) == ksim.KSIM_OK
    eng.load_events(0, openb["events"], 10)
    assert L.ksim_engine_get_cos_victims(eng.h, 0, None, 0, C.byref(n), C.byref(b)) == ksim.KSIM_ESTATE
    assert L.ksim_engine_deschedule_cossim(eng.h, 0.3, *WIDE) == ksim.KSIM_ESTATE
    eng.close()


def test_planning_changes_no_state_and_interleaves_with_frag_plans(openb):
    eng = make_engine(openb)
    eng.run()
    before = bytes(eng.nodes(0)), eng.results(0)
    eng.deschedule_cossim(0.3, *WIDE)
    one = got_plan(eng, 0)
    assert eng.last_deschedule_ms() >= 0.0
    eng.deschedule(ref.MULTI_POD, 1.0)
    res, state = oracle_run(openb, "openb", "FGD")
    victims, budget, _ = ref.plan(openb["onodes"], openb["otyp"], openb["oev"], res, state, ref.MULTI_POD, 1.0)
    frag = eng.victims(0)
    assert ([(v.event, v.node, v.gpu_mask, v.score, v.frag_before, v.frag_after) for v in frag[0]], frag[1]) == \
        (ref.as_tuples(victims), budget)
    eng.deschedule_cossim(0.05, *WIDE)
    assert got_plan(eng, 0) == want_plan(openb, "openb", "FGD", 0.05, WIDE)
    eng.deschedule_cossim(0.3, *WIDE)
    assert got_plan(eng, 0) == one == want_plan(openb, "openb", "FGD", 0.3, WIDE)
    assert (bytes(eng.nodes(0)), eng.results(0)) == before
    eng.close()


def test_reschedule_end_to_end(openb):
    scheds = cases.OPENB_POLICIES
    eng = make_engine(openb, scheds, report=True)
    eng.run()
    out = ksim.desched.run(eng, "cosSim", 0.3, cpu_bar=2 ** 30, gpu_bar=0)
    for r, sched in enumerate(scheds):
        victims, budget = want_plan(openb, "openb", sched, 0.3, WIDE)
        o = out[r]
        assert [v.event for v in o["victims"]] == [v[0] for v in victims] and o["budget"] == budget and victims
        n0, nv = openb["n"], len(victims)
        assert (o["n"], o["n_original"], o["post_eviction"], o["post_deschedule"]) == \
            (n0 + 2 * nv, n0, n0 + nv - 1, n0 + 2 * nv - 1)
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
        # every victim was deleted from its node and came back through the ordinary cycle
        assert all(want_res[n0 + k][4] == ksim.DELETED and want_res[n0 + k][0] == victims[k][1] for k in range(nv))
    eng.close()
