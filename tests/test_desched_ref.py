"""Known answers that pin tests/desched_ref.py, the reference of the descheduling tests (no GPU).

The hand-made cluster (desched_cases.hand) is small enough to work out here.  Typical pods, any model:
A = (2000 milli-CPU, 500 milli-GPU, freq 0.5), B = (2000, 1000, freq 0.5).  For a node with c CPU left
and GPUs gl, F = 0.5 * termA + 0.5 * termB, where a term is the milli left on the GPUs too small for
the typical pod when the node can host it (c >= 2000 and some GPU >= its milli), else all milli left
(frag.go:148-188 without bin Q3).

  node 0 (h0, 1 GPU, 4000 CPU): e0 holds 400 milli and requests no CPU; e8 came and was deleted.
      gl [600], c 4000: A hosted, nothing below 500 -> 0; B not hosted -> 600.  F = 300.
      e0: Add would put 4000 + 100 (the non-zero default) over the capacity 4000 -> skipped.
  node 1 (h1, 1 GPU, 8000 CPU): e1 300 milli, e2 399 milli.  gl [301], c 6000: A, B not hosted -> F = 301.
      e1: gl [601]: A hosted -> 0, B -> 601: F 300.5, score int64(0.5) = 0: not a victim.
      e2: gl [700]: F 350, score int64(-49) < 0: not a victim.
  node 2 (h3, 2 GPUs) and node 3 (h2, 2 GPUs): two 600-milli pods each, gl [400, 400]: F = 800.
      either pod: gl [1000, 400]: A hosted -> 400, B hosted -> 400: F 400, score 400.  Equal scores:
      the lower event wins (e3 on node 2, e5 on node 3).  Equal F: node 3 is named "h2", rank 2, and
      goes before node 2, "h3", rank 3.
  e7 asks for 8 GPUs and fails; e9 deletes e8.  Bound pods: e0 .. e6 = 7.
"""
import math

import pytest

import desched_cases as cases
import desched_ref as ref
import pyoracle as O


def run_oracle(case, policy="FGD"):
    pol, sel = cases.oracle_policy(policy)
    res, state, _ = O.run_events(case["onodes"], case["otyp"], case["oev"], policy=pol, gpu_sel=sel)
    return res, state


def plan(case, policy, ratio, sched="FGD"):
    res, state = run_oracle(case, sched)
    return ref.plan(case["onodes"], case["otyp"], case["oev"], res, state, policy, ratio)


@pytest.fixture(scope="module")
def hand():
    return cases.hand()


def test_hand_cluster_is_placed_as_the_comments_say(hand):
    res, state = run_oracle(hand)
    assert [r[0] for r in res] == [0, 1, 1, 2, 2, 3, 3, -1, 0, 0]
    assert [r[4] for r in res] == [0, 0, 0, 0, 0, 0, 0, 1, 0, 3]
    assert [(s[0], s[3][:2]) for s in state] == [(4000, [600, 0]), (6000, [301, 0]), (6000, [400, 400]),
                                                  (6000, [400, 400])]
    assert ref.name_ranks(hand["onodes"]) == [0, 1, 3, 2]
    assert ref.bound_pods(hand["oev"], res) == [0, 1, 2, 3, 4, 5, 6]


def test_hand_candidates(hand):
    res, state = run_oracle(hand)
    bound, f_after, f_node, skipped = ref.candidates(hand["onodes"], hand["otyp"], hand["oev"], res, state)
    assert f_node == [300.0, 301.0, 800.0, 800.0]
    assert f_after == {0: None, 1: 300.5, 2: 350.0, 3: 400.0, 4: 400.0, 5: 400.0, 6: 400.0}
    assert skipped == 1  # e0: Add exceeds the CPU capacity


def test_hand_frag_one_pod(hand):
    victims, budget, info = plan(hand, ref.ONE_POD, 1.0)
    assert budget == 7 and info["bound"] == 7 and info["skipped_by_add"] == 1
    # node 3 before node 2 (rank), the lower event of each; nodes 1 (score 0.5 -> 0) and 0 (skipped) give none:
    # the nodes run out before the budget does
    assert ref.as_tuples(victims) == [(5, 3, 1, 400, 800.0, 400.0), (3, 2, 1, 400, 800.0, 400.0)]
    assert len(victims) < budget
    # ceil(0.1 * 7) = 1: the budget binds
    victims, budget, _ = plan(hand, ref.ONE_POD, 0.1)
    assert budget == 1 and ref.as_tuples(victims) == [(5, 3, 1, 400, 800.0, 400.0)]
    assert plan(hand, ref.ONE_POD, 0.0)[:2] == ([], 0)


def test_hand_frag_multi_pod_rescores_against_the_original_state(hand):
    # pop node 3 (800): e5, re-keyed 400; pop node 2 (800): e3, re-keyed 400; pop node 3 again: its
    # candidate e6 is still "the original node + e6" = 400 (deschedule.go:124, :156), against the stored
    # priority 400: score 0, no victim, the node is dropped.  The state after e5's eviction would be
    # gl [1000, 1000], F 0, score 400: an updated state would evict e6 as well.
    victims, budget, info = plan(hand, ref.MULTI_POD, 1.0)
    assert budget == 7
    assert ref.as_tuples(victims) == [(5, 3, 1, 400, 800.0, 400.0), (3, 2, 1, 400, 800.0, 400.0)]
    assert info["max_per_node"] == 1
    after_e5 = O.node_res(7000, [1000, 1000], 2, "M3", 8000)
    assert int(400.0 - O.frag_score(after_e5, O.typical(hand["otyp"]))) == 400


def test_second_eviction_from_a_node_needs_an_updated_state():
    # With the node state kept as the reference keeps it, the first victim of a node has the smallest
    # F(node + pod) up to the truncation; the node's next priority is that value, so every later score is
    # int64(min - F(node + pod)) <= 0 and no node is evicted from twice (DESIGN.md "Descheduling").  The
    # crowded node, 303 candidates with positive scores at the first pop, gives one victim under both policies.
    case = cases.crowded()
    one, budget, info = plan(case, ref.ONE_POD, 1.0)
    multi, _, info_m = plan(case, ref.MULTI_POD, 1.0)
    assert budget == info["bound"] == 303
    assert [v["event"] for v in one] == [293] and ref.as_tuples(multi) == ref.as_tuples(one)
    assert info_m["max_per_node"] == 1


def test_crowded_node_scores():
    # c0: 1500 CPU free, below the typical pods' 2000 / 3000 / 2500.  GPUs: two 600-milli pods and one whole GPU
    # on four devices: 400 + 400 + 0 + 1000 = 1800 left.  F = (0.5 + 0.25 + 0.25) * 1800 = 1800.
    # + a 1000-milli-CPU pod: c 2500: A hosted (a GPU >= 500): 0.5 * 800, B, C: 0.5 * 1800 -> 1300, score 500.
    # + the 2000-milli-CPU pod: c 3500: B hosted too (a whole GPU): 0.25 * 800 -> 400 + 200 + 450 = 1050, score 750.
    case = cases.crowded()
    victims, _, _ = plan(case, ref.MULTI_POD, 0.01)
    assert ref.as_tuples(victims) == [(293, 0, 0, 750, 1800.0, 1050.0)]


def test_empty_cluster():
    assert plan(cases.empty(), ref.ONE_POD, 1.0)[:2] == ([], 0)
    assert plan(cases.empty(), ref.MULTI_POD, 1.0)[:2] == ([], 0)


@pytest.fixture(scope="module")
def openb():
    return cases.openb64()


@pytest.mark.parametrize("sched", cases.OPENB_POLICIES)
def test_openb_subset_covers_both_ends(openb, sched):
    # the GPU test's shapes: deleted and failed pods exist, the budget binds at a low ratio and the nodes run
    # out first at ratio 1
    res, _ = run_oracle(openb, sched)
    assert any(r[4] == 3 and r[0] >= 0 for r in res) and any(r[4] == 1 for r in res)
    for policy in (ref.ONE_POD, ref.MULTI_POD):
        victims, budget, info = plan(openb, policy, 0.05, sched)
        assert budget == math.ceil(0.05 * info["bound"]) and len(victims) == budget > 0
        victims, budget, info = plan(openb, policy, 1.0, sched)
        assert budget == info["bound"] and 0 < len(victims) < budget
        assert all(v["score"] > 0 and v["frag_before"] - v["frag_after"] >= 1 for v in victims)
        gone = {e["ref"] for e, r in zip(openb["oev"], res) if e.get("delete") and r[4] == 3}
        assert all(res[v["event"]][4] == 0 and v["event"] not in gone for v in victims)
