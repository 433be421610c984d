"""CPU checks of the descheduling fuzz cases (tests/desched_fuzz_cases.py): from the oracle and the two Python
references alone, every case reaches what tests/test_gpu_desched_fuzz.py runs it for, so that the GPU test cannot
pass vacuously.  Every condition is an assert; nothing is skipped."""
import pytest

import desched_cos_ref as cos
import desched_fuzz_cases as fz
import desched_ref as ref
from test_gpu_desched import oracle_run

WIDE = (2 ** 30, 0)
ODD_GPUS = {3, 5, 6, 7}


@pytest.fixture(scope="module")
def facts():
    """Per (fuzz case, score policy): the frag plan at ratio 1.0 and the cosSim plans at the default and wide bars."""
    out = {}
    for spec in fz.FUZZ:
        c = fz.from_fuzz(*spec)
        for sched in fz.FUZZ_POLICIES:
            res, state = oracle_run(c, ("fuzz",) + spec, sched)
            victims, budget, info = ref.plan(c["onodes"], c["otyp"], c["oev"], res, state, ref.MULTI_POD, 1.0)
            one = ref.plan(c["onodes"], c["otyp"], c["oev"], res, state, ref.ONE_POD, 1.0)[0]
            cv, _, cinfo = cos.plan(c["onodes"], c["oev"], res, state, 1.0)
            wv, _, winfo = cos.plan(c["onodes"], c["oev"], res, state, 1.0, *WIDE)
            out[spec, sched] = dict(case=c, victims=victims, one=one, budget=budget, info=info, cos=cv, cos_info=cinfo,
                                    wide=wv, wide_info=winfo)
            print(spec, sched, "typed", sum(1 for t in c["otyp"] if t[3]), "of", len(c["otyp"]), "frag victims",
                  len(victims), "budget", budget, info, "cos", len(cv), cinfo, "wide", len(wv), winfo)
    return out


def test_every_cluster_has_a_typed_table_and_a_frag_victim(facts):
    for (spec, sched), f in facts.items():
        if spec[1] == 1:
            continue
        assert any(t[3] for t in f["case"]["otyp"]), spec       # frag_F<true> on the device
        assert f["victims"] and f["one"], (spec, sched)
        assert ref.as_tuples(f["one"]) == ref.as_tuples(f["victims"])  # (the same pods as written)


def test_add_skips_pods_under_fgd(facts):
    # NodeResource.Add fails (the non-zero CPU default of a zero-CPU pod passes the capacity): on every cluster
    # of 40 nodes or more, and somewhere under BestFit too
    for (spec, sched), f in facts.items():
        if sched == "FGD" and spec[1] >= 40:
            assert f["info"]["skipped_by_add"] > 0, spec
    assert any(f["info"]["skipped_by_add"] > 0 for (_, sched), f in facts.items() if sched == "BestFit")


def test_some_victim_holds_several_gpus(facts):
    multi = [(k, v["event"]) for k, f in facts.items() for v in f["victims"] if bin(v["gpu_mask"]).count("1") > 1]
    print("multi-GPU victims:", multi)
    assert multi


def test_some_victim_sits_on_a_3_5_6_or_7_gpu_node(facts):
    odd = [(k, v["node"], f["case"]["onodes"][v["node"]]["gpu"]) for k, f in facts.items() for v in f["victims"]
           if f["case"]["onodes"][v["node"]]["gpu"] in ODD_GPUS]
    print("victims on 3/5/6/7-GPU nodes:", len(odd), "in", len({k for k, _, _ in odd}), "(case, policy) pairs")
    assert odd
    cos_odd = [k for k, f in facts.items() for v in f["wide"] if f["case"]["onodes"][v["node"]]["gpu"] in ODD_GPUS]
    assert cos_odd


def test_cossim_victims_under_both_bars(facts):
    assert any(f["cos"] for f in facts.values())
    assert any(f["wide"] and f["wide_info"]["with_victim"] < f["wide_info"]["candidates"] for f in facts.values())


def test_one_node_cluster_has_a_budget_and_no_frag_victim(facts):
    ones = [(k, f) for k, f in facts.items() if k[0][1] == 1]
    assert len(ones) == len(fz.FUZZ_POLICIES)
    for k, f in ones:
        assert f["victims"] == [] and f["budget"] > 0, k


def test_a_cut_stream_is_valid():
    full = fz.from_fuzz(21, 150, 580, 0.2)
    assert 650 <= full["n"] <= 750
    for n in (0, 1, 256, 257):
        c = fz.from_fuzz(21, 150, 580, 0.2, n_events=n)
        assert c["n"] == len(c["oev"]) == n
        assert all(0 <= e["ref"] < i for i, e in enumerate(c["oev"]) if e.get("delete"))


def test_ragged_replicas_have_victims():
    # the replicas of test_gpu_desched_fuzz.py::test_ragged_replicas: the three longer streams give frag and
    # cosSim victims, the empty one nothing, the one-event one a budget of one at most
    from test_gpu_desched_fuzz import RAGGED_N, RAGGED_SCHEDS
    for r, n in enumerate(RAGGED_N):
        c = fz.from_fuzz(20 + r, 150, 580, 0.2, n_events=n)
        res, state = oracle_run(c, ("ragged", r), RAGGED_SCHEDS[r])
        victims, budget, info = ref.plan(c["onodes"], c["otyp"], c["oev"], res, state, ref.ONE_POD, 1.0)
        wide, _, winfo = cos.plan(c["onodes"], c["oev"], res, state, 1.0, *WIDE)
        print(r, c["n"], RAGGED_SCHEDS[r], "frag", len(victims), budget, info, "cos wide", len(wide), winfo)
        if r in (1, 2, 3):
            assert victims and wide and budget > len(victims)
        elif r == 0:
            assert (victims, budget, wide) == ([], 0, [])
        else:
            assert budget == info["bound"] <= 1


def test_second_round_reaches_the_recreated_pods():
    # test_gpu_desched_fuzz.py::test_second_round_on_extended_streams, from the references alone: replicas get
    # different victim counts, the first victims are gone in the second plan and their copies are bound pods
    import desched_cases as cases
    import pyoracle as O
    c = fz.from_fuzz(2, 97, 900, 0.25)
    lengths, recreated, elected = set(), 0, 0
    for sched in cases.OPENB_POLICIES:
        res, state = oracle_run(c, ("fuzz", 2, 97, 900, 0.25), sched)
        first = [v["event"] for v in ref.plan(c["onodes"], c["otyp"], c["oev"], res, state, ref.MULTI_POD, 0.3)[0]]
        assert first
        oev = ref.extend_events(c["oev"], [dict(event=e) for e in first])
        lengths.add(len(oev))
        pol, sel = cases.oracle_policy(sched)
        res2, state2 = O.run_events(c["onodes"], c["otyp"], oev, policy=pol, gpu_sel=sel)[:2]
        bound = ref.bound_pods(oev, res2)
        assert not set(bound) & set(first)
        recreated += sum(1 for e in bound if e >= c["n"] + len(first))
        second = ref.plan(c["onodes"], c["otyp"], oev, res2, state2, ref.ONE_POD, 1.0)[0]
        wide = cos.plan(c["onodes"], oev, res2, state2, 1.0, *WIDE)[0]
        assert second and wide
        elected += sum(1 for v in second + wide if v["event"] >= c["n"] + len(first))
        print(sched, "first", len(first), "second", len(second), "cos", len(wide))
    print("re-created pods bound:", recreated, "elected again:", elected)
    assert len(lengths) > 1 and recreated > 0


def test_scrambled_names_are_unique_and_scrambled():
    for n in sorted(set(fz.COS_STRIDE_N + fz.COS_SWITCH_N + fz.FRAG_STRIDE_N + fz.FRAG_SWITCH_N)):
        names = fz.scrambled_names(n)
        assert len(set(names)) == n and len({len(s) for s in names}) == 1
        if n > 3:
            assert names != sorted(names)


@pytest.mark.parametrize("n", fz.COS_STRIDE_N + fz.COS_SWITCH_N)
def test_flat_cos_every_node_has_a_victim(n):
    c = fz.flat_cos(n)
    res, state = oracle_run(c, ("flat_cos", n), "FGD")
    victims, budget, info = cos.plan(c["onodes"], c["oev"], res, state, 1.0)
    assert info["with_victim"] == info["candidates"] == info["bound"] == budget == len(victims) == n
    keys = {v["gpu_left"] for v in victims}
    print(n, "distinct milli-GPU left:", sorted(keys))
    # both sort keys matter (below eight nodes the seven-value cycle gives every node a key of its own)
    assert len(keys) == min(n, 7)
    if n > 7:
        assert 1 < len(keys) < n
        half = cos.plan(c["onodes"], c["oev"], res, state, 0.5)[0]
        assert half[-1]["gpu_left"] == victims[len(half)]["gpu_left"]  # the budget cuts inside a run of equal keys


@pytest.mark.parametrize("n", fz.FRAG_STRIDE_N + fz.FRAG_SWITCH_N)
def test_flat_frag_every_node_has_a_victim(n):
    c = fz.flat_frag(n)
    res, state = oracle_run(c, ("flat_frag", n), "FGD")
    assert sorted(r[0] for r in res) == list(range(n))  # one pod on each node
    victims, budget, info = ref.plan(c["onodes"], c["otyp"], c["oev"], res, state, ref.ONE_POD, 1.0)
    assert info["bound"] == budget == len(victims) == len({v["node"] for v in victims}) == n
    prios = {v["frag_before"] for v in victims}
    print(n, "distinct F:", sorted(prios))
    assert len(prios) == min(n, 7)
    if n > 7:
        assert 1 < len(prios) < n
        half = ref.plan(c["onodes"], c["otyp"], c["oev"], res, state, ref.ONE_POD, 0.5)[0]
        assert sorted({v["frag_before"] for v in half}) == [300.0, 350.0, 400.0, 450.0]
        assert half[-1]["frag_before"] == victims[len(half)]["frag_before"]  # the name rank decides who is in


def test_shared_table_case_has_victims_of_every_policy_up_to_the_last_nodes():
    n, m = fz.SHARED_TAB_N, fz.SHARED_TAB_PODS
    assert n * 24 > n * 20 > 60 * 1024  # both policies' tables are in HBM, cosSim's the larger
    c = fz.flat_frag(n, m)
    res, state = oracle_run(c, ("shared_tab", n, m), "FGD")
    assert len({r[0] for r in res}) == m  # one pod a node
    for victims in (ref.plan(c["onodes"], c["otyp"], c["oev"], res, state, ref.MULTI_POD, 1.0)[0],
                    cos.plan(c["onodes"], c["oev"], res, state, 1.0, *WIDE)[0],
                    ref.plan(c["onodes"], c["otyp"], c["oev"], res, state, ref.ONE_POD, 1.0)[0]):
        assert len(victims) == m and max(v["node"] for v in victims) > n - 64

