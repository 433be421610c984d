"""Known answers that pin tests/desched_cos_ref.py, the reference of the cosSim descheduling tests (no GPU).

The hand-made cluster (desched_cos_cases.hand), worked out here at the reference's bars (CPU 2000, GPU 500).
A node is a candidate with CPU left < 2000 and a GPU with more than 500 milli left; the similarity of a pod
is the cosine of [CPU left + pod CPU, milli-GPU left + pod milli] and [pod CPU, pod milli].

  node 0 (c0, 3000 CPU): e0 takes 1000: 2000 left, exactly the bar -> not a candidate (the reference skips at >=).
  node 1 (c1, 1 GPU): e1 takes 500 milli: 500 left, exactly the bar -> not a candidate (strictly more is needed).
  node 2 (c3) and node 3 (c2), 2 GPUs, 4000 CPU: two pods of 1500 CPU / 400 milli each: 1000 CPU and 1200
      milli left.  Either pod: [2500, 1600] . [1500, 400] = 4390000 over sqrt(8810000) * sqrt(2410000) = 0.9527...
      Equal similarities: the lower event wins (e2, e4).  Equal milli-GPU left: "c2" (index 3) before "c3".
  node 4 (c4, 1500 CPU): e6 requests no CPU; Add gives back the non-zero default 100: 1600 > 1500 -> skipped.
      A candidate without a victim.
  node 5 (c5, 2 GPUs, 1500 CPU): e7 takes 750 CPU and a whole GPU.  [1500, 2000] . [750, 1000] = 3125000 over
      2500 * 1250: exactly 1, never below the starting best of 1 -> a candidate without a victim.
  node 6 (c6, 1900 CPU): e8 takes 500 / 200 milli; e9 came and was deleted.  [1900, 1000] . [500, 200] =
      1150000 over sqrt(4610000) * sqrt(290000) = 0.9945...
  Bound pods: e0 .. e8 = 9.  Order: node 3 (1200), node 2 (1200), node 5 (1000), node 6 (800), node 4 (700).
"""
import math

import pytest

import desched_cases as cases
import desched_cos_cases as cos_cases
import desched_cos_ref as cos
import desched_ref as ref
import pyoracle as O

SIM_22 = 4390000.0 / (math.sqrt(8810000.0) * math.sqrt(2410000.0))
SIM_6 = 1150000.0 / (math.sqrt(4610000.0) * math.sqrt(290000.0))


def run_oracle(case, sched="FGD"):
    pol, sel = cases.oracle_policy(sched)
    res, state, _ = O.run_events(case["onodes"], case["otyp"], case["oev"], policy=pol, gpu_sel=sel)
    return res, state


def plan(case, ratio, cpu_bar=cos.CPU_BAR, gpu_bar=cos.GPU_BAR, sched="FGD"):
    res, state = run_oracle(case, sched)
    return cos.plan(case["onodes"], case["oev"], res, state, ratio, cpu_bar, gpu_bar)


@pytest.fixture(scope="module")
def hand():
    return cos_cases.hand()


def test_hand_cluster_is_placed_as_the_comments_say(hand):
    res, state = run_oracle(hand)
    assert [r[0] for r in res] == [0, 1, 2, 2, 3, 3, 4, 5, 6, 6, 6]
    assert [r[4] for r in res] == [0] * 10 + [3]
    assert [s[0] for s in state] == [2000, 1000, 1000, 1000, 1500, 750, 1400]
    assert [sum(s[3]) for s in state] == [700, 500, 1200, 1200, 700, 1000, 800]
    assert max(state[1][3]) == 500 and max(state[5][3]) == 1000
    assert ref.name_ranks(hand["onodes"]) == [0, 1, 3, 2, 4, 5, 6]
    assert ref.bound_pods(hand["oev"], res) == list(range(9))


def test_cosine_is_written_as_the_reference_writes_it():
    assert cos.cosine([1500, 2000], [750, 1000]) == 1.0
    assert cos.cosine([2500, 1600], [1500, 400]) == SIM_22
    assert cos.cosine([0, 0], [1, 1]) == -1.0 and cos.cosine([3, 4], [0, 0]) == -1.0
    assert cos.cosine([0, 5], [7, 0]) == 0.0


def test_hand_similarities(hand):
    res, state = run_oracle(hand)
    node = lambda i: ref.node_resource(hand["onodes"][i], state[i])
    assert cos.similarity_of(node(2), 1500, 400, 1, [0]) == (SIM_22, "ok")
    assert cos.similarity_of(node(4), 100, 300, 1, [0]) == (-1.0, "add")   # 1500 + 100 > 1500
    assert cos.similarity_of(node(5), 750, 1000, 1, [0]) == (1.0, "ok")    # parallel: never elected
    assert cos.similarity_of(node(6), 500, 200, 1, [0]) == (SIM_6, "ok")
    assert cos.find_victim(node(5), [7], hand["oev"], res) is None
    assert cos.find_victim(node(4), [6], hand["oev"], res) is None
    assert cos.find_victim(node(3), [4, 5], hand["oev"], res) == (4, SIM_22)  # e4 and e5 are equal: the lower


def test_hand_plan(hand):
    victims, budget, info = plan(hand, 1.0)
    assert budget == 9 and info == dict(bound=9, candidates=5, with_victim=3)
    # node 3 before node 2 (name), then node 6; nodes 5 and 4 are visited and give none: no budget used
    assert cos.as_tuples(victims) == [(4, 3, 1, 1200, SIM_22), (2, 2, 1, 1200, SIM_22), (8, 6, 1, 800, SIM_6)]
    # ceil(0.2 * 9) = 2: the budget is smaller than the nodes with a victim
    victims, budget, _ = plan(hand, 0.2)
    assert budget == 2 and cos.as_tuples(victims) == [(4, 3, 1, 1200, SIM_22), (2, 2, 1, 1200, SIM_22)]
    assert plan(hand, 0.0)[:2] == ([], 0)


def test_hand_bars_are_strict_on_the_right_side(hand):
    # one milli more on the CPU bar lets node 0 in (2000 < 2001); one less on the GPU bar lets node 1 in (500 > 499)
    victims, _, info = plan(hand, 1.0, cpu_bar=2001)
    assert info["candidates"] == 6 and 0 in [v["node"] for v in victims]
    victims, _, info = plan(hand, 1.0, gpu_bar=499)
    assert info["candidates"] == 6 and 1 in [v["node"] for v in victims]


def test_crowded_and_empty():
    # c0 holds 303 pods; the 299 one-CPU pods of 1000 milli tie at the least similarity: the first of them, e3
    victims, budget, info = plan(cases.crowded(), 1.0)
    assert budget == 303 and info["with_victim"] == 1
    assert [(v["event"], v["node"], v["gpu_left"]) for v in victims] == [(3, 0, 1800)]
    assert plan(cases.empty(), 1.0)[:2] == ([], 0)


def test_flat_cluster_places_one_pod_a_node():
    case = cos_cases.flat()
    res, state = run_oracle(case)
    assert sorted(r[0] for r in res) == list(range(cos_cases.FLAT_N)) and all(r[4] == 0 for r in res)
    victims, budget, info = plan(case, 0.5)
    assert budget == len(victims) == 300 and info["with_victim"] == 600
    # both keys decide: the milli-GPU left falls along the plan, the names rise within one value, and they do
    # not rise with the node index
    keys = [(-v["gpu_left"], case["onodes"][v["node"]]["name"]) for v in victims]
    assert keys == sorted(keys) and len({k[0] for k in keys}) >= 3
    nodes = [v["node"] for v in victims if v["gpu_left"] == victims[0]["gpu_left"]]
    assert nodes != sorted(nodes)


@pytest.mark.parametrize("sched", cases.OPENB_POLICIES)
def test_openb_subset_shapes(sched):
    # the GPU test's shapes: no candidate for FGD at the default bars, ties and a binding budget at (2^30, 0)
    openb = cases.openb64()
    res, state = run_oracle(openb, sched)
    _, _, info = plan(openb, 1.0, sched=sched)
    assert info["candidates"] == {"FGD": 0, "BestFit": 2, "GpuPacking": 3}[sched]
    victims, budget, info = plan(openb, 0.05, 2 ** 30, 0, sched)
    assert budget == 20 == len(victims) < info["with_victim"]
    victims, budget, info = plan(openb, 1.0, 2 ** 30, 0, sched)
    assert 48 <= len(victims) == info["with_victim"] <= 53
    assert all(0 <= v["similarity"] < 1 for v in victims)
    gone = {e["ref"] for e, r in zip(openb["oev"], res) if e.get("delete") and r[4] == 3}
    assert all(res[v["event"]][4] == 0 and v["event"] not in gone for v in victims)
