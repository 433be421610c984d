"""GPU parity of the three descheduling plans on adversarial clusters and at the size edges of the select kernels.

Bar: as tests/test_gpu_desched.py and tests/test_gpu_desched_cos.py -- `==` on every field of every victim, doubles
included, in eviction order, and the budget, against tests/desched_ref.py / tests/desched_cos_ref.py run on the
oracle's own replay; the engine's results equal the oracle's first, so a planning mismatch is not a replay mismatch
in disguise.  The cases (tests/desched_fuzz_cases.py; tests/test_desched_fuzz_cases.py asserts on the CPU that each
reaches its target):
- the fuzz generator's clusters: typed typical tables (frag_F<true> in k_desched_eval), 0 to 8 GPUs a node, tight
  pod limits, zero-CPU pods, multi-GPU victims, specs naming a model no node has;
- five ragged replicas of one engine, an empty one and a one-event one among them, and plans repeated in a row;
- flat clusters at the 64 / 256-thread stride edges of k_cos_select and k_desched_select, at ratio 1.0 so that the
  whole sorted order is written out and compared;
- both sides of the LDS / HBM switch of the two select kernels (2560 / 2561 and 3072 / 3073 nodes), with every
  node queued or sorted;
- a second plan on the ragged streams that ksim.desched.run extended;
- one engine of 3073 nodes planning fragMultiPod, cosSim and fragOnePod in turn: the three share one buffer for
  the tables in HBM, which cosSim needs larger (24 B a node) than the frag policies (20 B);
- ratio = +inf with an empty replica: the budget is defined (0 there, every bound pod elsewhere).
Every test needs a gfx950 device.
"""
import ctypes as C

import pytest

import desched_cases as cases
import desched_cos_ref as cos
import desched_fuzz_cases as fz
import desched_ref as ref
import ksim
import ksim.desched
import pyoracle as O
import test_gpu_desched as frag
import test_gpu_desched_cos as cosm
from test_gpu_desched import make_engine, oracle_run

pytestmark = pytest.mark.gpu

POLICIES = frag.POLICIES
BARS = cosm.BARS
WIDE = cosm.WIDE


def engine_of(replicas):
    """One engine, a case and a score policy of its own per replica: [(case, sched)]."""
    eng = ksim.Engine(len(replicas[0][0]["nodes"]), len(replicas))
    for r, (case, sched) in enumerate(replicas):
        eng.set_nodes(r, case["nodes"])
        eng.set_typical(r, *case["typ"])
        eng.set_policy(r, sched)
    for r, (case, _) in enumerate(replicas):
        eng.load_events(r, case["events"], case["n"])
    return eng


@pytest.mark.parametrize("spec", fz.FUZZ, ids=["s%d-n%d-e%d-d%g" % c for c in fz.FUZZ])
def test_adversarial_cluster(spec):
    case, key = fz.from_fuzz(*spec), ("fuzz",) + spec
    scheds = fz.FUZZ_POLICIES
    eng = make_engine(case, scheds)
    eng.run()
    for r, sched in enumerate(scheds):
        assert eng.results(r) == oracle_run(case, key, sched)[0], sched
    n_victims = 0
    for policy in POLICIES:
        for ratio in (0.0, 0.1, 1.0):
            eng.deschedule(policy, ratio)
            for r, sched in enumerate(scheds):
                got = frag.got_plan(eng, r)
                assert got == frag.want_plan(case, key, sched, policy, ratio), (policy, ratio, sched)
                n_victims += len(got[0])
    for bars in BARS:
        for ratio in (0.3, 1.0):
            eng.deschedule_cossim(ratio, *bars)
            for r, sched in enumerate(scheds):
                assert cosm.got_plan(eng, r) == cosm.want_plan(case, key, sched, ratio, bars), (bars, ratio, sched)
    assert n_victims > 0 or spec[1] == 1
    eng.close()


RAGGED_N = [0, 256, 257, None, 1]   # stream lengths (None: the whole stream, about 700 events)
RAGGED_SCHEDS = ["FGD", "FGD", "GpuPacking", "FGD", "FGD"]


def test_ragged_replicas():
    reps = [(fz.from_fuzz(20 + r, 150, 580, 0.2, n_events=n), RAGGED_SCHEDS[r]) for r, n in enumerate(RAGGED_N)]
    assert [c["n"] for c, _ in reps][:3] == [0, 256, 257] and reps[3][0]["n"] > 600 and reps[4][0]["n"] == 1
    eng = engine_of(reps)
    eng.run()
    L = ksim.lib()
    for r, (case, sched) in enumerate(reps):
        assert eng.results(r) == oracle_run(case, ("ragged", r), sched)[0], r
    n_victims = [0] * len(reps)
    # the second and third plan of each kind follow another ratio's: they must not see its marks or counts
    for policy, ratio in [(p, q) for p in POLICIES for q in (1.0, 0.1, 0.3)]:
        eng.deschedule(policy, ratio)
        for r, (case, sched) in enumerate(reps):
            got, want = frag.got_plan(eng, r), frag.want_plan(case, ("ragged", r), sched, policy, ratio)
            assert got == want, (policy, ratio, r)
            n, b = C.c_int(-1), C.c_int(-1)
            rc = L.ksim_engine_get_victims(eng.h, r, None, 0, C.byref(n), C.byref(b))
            assert rc == (ksim.KSIM_ERANGE if want[0] else ksim.KSIM_OK)
            assert (n.value, b.value) == (len(want[0]), want[1]), (policy, ratio, r)
            n_victims[r] += len(got[0])
    assert frag.got_plan(eng, 0) == ([], 0)
    assert n_victims[1] and n_victims[2] and n_victims[3]
    n_cos = [0] * len(reps)
    for bars, ratio in [(WIDE, 1.0), (WIDE, 0.05), (BARS[0], 1.0), (BARS[1], 0.3)]:
        eng.deschedule_cossim(ratio, *bars)
        for r, (case, sched) in enumerate(reps):
            got, want = cosm.got_plan(eng, r), cosm.want_plan(case, ("ragged", r), sched, ratio, bars)
            assert got == want, (bars, ratio, r)
            n, b = C.c_int(-1), C.c_int(-1)
            rc = L.ksim_engine_get_cos_victims(eng.h, r, None, 0, C.byref(n), C.byref(b))
            assert rc == (ksim.KSIM_ERANGE if want[0] else ksim.KSIM_OK)
            assert (n.value, b.value) == (len(want[0]), want[1]), (bars, ratio, r)
            n_cos[r] += len(got[0])
    assert cosm.got_plan(eng, 0) == ([], 0)
    assert n_cos[1] and n_cos[2] and n_cos[3]
    eng.close()


def check_flat_cos(n):
    case, key = fz.flat_cos(n), ("flat_cos", n)
    eng = make_engine(case)
    eng.run()
    assert eng.results(0) == oracle_run(case, key, "FGD")[0]
    for ratio in (1.0, 0.5):
        eng.deschedule_cossim(ratio)
        got = cosm.got_plan(eng, 0)
        assert got == cosm.want_plan(case, key, "FGD", ratio), ratio
        assert len(got[0]) == got[1] == (n if ratio == 1.0 else (n + 1) // 2)
    eng.close()


def check_flat_frag(n):
    case, key = fz.flat_frag(n), ("flat_frag", n)
    eng = make_engine(case)
    eng.run()
    assert eng.results(0) == oracle_run(case, key, "FGD")[0]
    for policy in POLICIES:
        for ratio in (0.5, 1.0):
            eng.deschedule(policy, ratio)
            got = frag.got_plan(eng, 0)
            assert got == frag.want_plan(case, key, "FGD", policy, ratio), (policy, ratio)
            assert len(got[0]) == got[1] == (n if ratio == 1.0 else (n + 1) // 2)
    eng.close()


@pytest.mark.parametrize("n", fz.COS_STRIDE_N)
def test_cos_select_stride_edges(n):
    check_flat_cos(n)


@pytest.mark.parametrize("n", fz.FRAG_STRIDE_N)
def test_desched_select_stride_edges(n):
    check_flat_frag(n)


@pytest.mark.parametrize("n", fz.COS_SWITCH_N)
def test_cos_select_lds_hbm_switch(n):
    # 2560 nodes: the largest in-LDS launch (60 KiB of dynamic LDS); 2561: the tables and the sort in HBM
    assert (n * 24 <= 60 * 1024) == (n == 2560)
    check_flat_cos(n)


@pytest.mark.parametrize("n", fz.FRAG_SWITCH_N)
def test_desched_select_lds_hbm_switch(n):
    # 3072 nodes: the largest in-LDS launch; 3073: every node queued and popped over tables in HBM
    assert (n * 20 <= 60 * 1024) == (n == 3072)
    check_flat_frag(n)


def test_every_policy_in_turn_over_one_table_buffer():
    n, m = fz.SHARED_TAB_N, fz.SHARED_TAB_PODS
    assert n * 24 > n * 20 > 60 * 1024
    case, key = fz.flat_frag(n, m), ("shared_tab", n, m)
    eng = make_engine(case)
    eng.run()
    assert eng.results(0) == oracle_run(case, key, "FGD")[0]
    # the table buffer is first made for 20 B a node, grows for cosSim, and is then used again at 20 B a node
    eng.deschedule(ref.MULTI_POD, 1.0)
    got = frag.got_plan(eng, 0)
    assert got == frag.want_plan(case, key, "FGD", ref.MULTI_POD, 1.0) and len(got[0]) == got[1] == m
    for ratio in (1.0, 0.3):
        eng.deschedule_cossim(ratio, *WIDE)
        got = cosm.got_plan(eng, 0)
        assert got == cosm.want_plan(case, key, "FGD", ratio, WIDE) and len(got[0]) == got[1] > 0
    for ratio in (1.0, 0.3):
        eng.deschedule(ref.ONE_POD, ratio)
        got = frag.got_plan(eng, 0)
        assert got == frag.want_plan(case, key, "FGD", ref.ONE_POD, ratio) and len(got[0]) == got[1] > 0
    eng.close()


def test_infinite_ratio_with_an_empty_replica():
    # inf * 0 bound pods is a NaN: the budget must not be made from it (the reference's formula raises at inf)
    reps = [(fz.from_fuzz(20 + r, 150, 580, 0.2, n_events=n), "FGD") for r, n in enumerate([257, 0])]
    eng = engine_of(reps)
    eng.run()
    L = ksim.lib()
    inf = float("inf")
    full = frag.want_plan(reps[0][0], ("ragged", 0, 257), "FGD", ref.MULTI_POD, 1.0)
    assert full[1] > 0
    for policy in POLICIES:
        assert L.ksim_engine_deschedule(eng.h, ksim.DESCHED_POLICY[policy], inf) == ksim.KSIM_OK
        assert frag.got_plan(eng, 1) == ([], 0)
        n, b = C.c_int(-1), C.c_int(-1)
        assert L.ksim_engine_get_victims(eng.h, 1, None, 0, C.byref(n), C.byref(b)) == ksim.KSIM_OK
        assert (n.value, b.value) == (0, 0)
        # every bound pod of the other replica: the plan of ratio 1
        assert frag.got_plan(eng, 0) == frag.want_plan(reps[0][0], ("ragged", 0, 257), "FGD", policy, 1.0)
    assert L.ksim_engine_deschedule_cossim(eng.h, inf, *WIDE) == ksim.KSIM_OK
    assert cosm.got_plan(eng, 1) == ([], 0)
    assert cosm.got_plan(eng, 0) == cosm.want_plan(reps[0][0], ("ragged", 0, 257), "FGD", 1.0, WIDE)
    eng.close()


def test_second_round_on_extended_streams():
    spec = (2, 97, 900, 0.25)
    case = fz.from_fuzz(*spec)
    scheds = cases.OPENB_POLICIES
    eng = make_engine(case, scheds)
    eng.run()
    out = ksim.desched.run(eng, ref.MULTI_POD, 0.3)
    n0 = case["n"]
    ext = []
    for r, sched in enumerate(scheds):
        first = [v.event for v in out[r]["victims"]]
        assert first and out[r]["n"] == n0 + 2 * len(first)
        oev = ref.extend_events(case["oev"], [dict(event=e) for e in first])
        pol, sel = cases.oracle_policy(sched)
        res, state = O.run_events(case["onodes"], case["otyp"], oev, policy=pol, gpu_sel=sel)[:2]
        assert eng.results(r) == res, sched
        ext.append((oev, res, state, first))
    assert len({len(x[0]) for x in ext}) > 1  # the streams are ragged now
    eng.deschedule(ref.ONE_POD, 1.0)
    recreated = 0
    for r, (oev, res, state, first) in enumerate(ext):
        victims, budget, _ = ref.plan(case["onodes"], case["otyp"], oev, res, state, ref.ONE_POD, 1.0)
        assert frag.got_plan(eng, r) == (ref.as_tuples(victims), budget) and victims, scheds[r]
        # the first round's victims are gone (their trailing deletes mark them); their copies are bound pods
        assert not {v["event"] for v in victims} & set(first)
        bound = ref.bound_pods(oev, res)
        assert not set(bound) & set(first)
        recreated += sum(1 for e in bound if e >= n0 + len(first))
    assert recreated > 0
    eng.deschedule_cossim(1.0, *WIDE)
    cos_recreated = 0
    for r, (oev, res, state, first) in enumerate(ext):
        victims, budget, _ = cos.plan(case["onodes"], oev, res, state, 1.0, *WIDE)
        assert cosm.got_plan(eng, r) == (cos.as_tuples(victims), budget) and victims, scheds[r]
        assert not {v["event"] for v in victims} & set(first)
        cos_recreated += sum(1 for v in victims if v["event"] >= n0 + len(first))
    print("re-created pods bound:", recreated, "and elected by cosSim:", cos_recreated)
    eng.close()
