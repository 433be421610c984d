"""Plain-Python restatement of the reference's fragmentation-aware descheduling -- TEST INFRASTRUCTURE.

DescheduleCluster (pkg/simulator/deschedule.go:20-47) with the policies fragOnePod (:94-119) and
fragMultiPod (:121-178), and findVictimPodOnNodeFragAware (deschedule_utils.go:73-106), built only
from the oracle's pieces: orc_node_add for NodeResource.Add, frag_score for F, run_events for the
cluster state after a stream.  The order contract where the reference's own order is a Go map's
(DESIGN.md "Descheduling"): pods of a node in ascending creation-event index, nodes of equal priority
by the rank of their name.
"""
import ctypes as C
import math

import pyoracle as O

ONE_POD, MULTI_POD = "fragOnePod", "fragMultiPod"


def name_ranks(nodes):
    """Rank of every node's name in byte-wise order (the engine's name_rank)."""
    order = sorted(range(len(nodes)), key=lambda i: nodes[i]["name"].encode())
    rank = [0] * len(nodes)
    for r, i in enumerate(order):
        rank[i] = r
    return rank


def node_resource(spec, st):
    """The oracle's NodeResource of node `spec` in state st = (cpu_left, mem_left, pods, gpu_left[8])."""
    return O.node_res(st[0], st[3][:spec["gpu"]], spec["gpu"], spec.get("model", ""), spec["cpu"])


def bound_pods(events, results):
    """Creation events still in the API: scheduled (failed pods were deleted again, simulator.go:359-375)
    and not removed by a later delete event."""
    gone = set()
    for ev, res in zip(events, results):
        if ev.get("delete") and res[4] == 3:
            gone.add(ev["ref"])
    return [i for i, (ev, res) in enumerate(zip(events, results))
            if not ev.get("delete") and res[4] == 0 and i not in gone]


def candidates(nodes, typical_list, events, results, state):
    """Per bound pod: F(node + pod) by NodeResource.Add (None where Add fails), and F of every node.
    Returns (bound event indices, {event: f_after or None}, [F(node)], skipped count)."""
    tp = O.typical(typical_list)
    res_of = [node_resource(nodes[i], state[i]) for i in range(len(nodes))]
    f_node = [O.frag_score(n, tp) for n in res_of]
    bound = bound_pods(events, results)
    f_after, skipped = {}, 0
    for e in bound:
        ev, (node, mask) = events[e], results[e][:2]
        pod = O.pod_res(ev.get("cpu_nz", ev["cpu"]), ev["milli"], ev["num"], ev.get("type", ""))
        ids = [g for g in range(8) if mask >> g & 1]
        out = O.NodeResource()
        rc = O.lib().orc_node_add(C.byref(res_of[node]), C.byref(pod), (C.c_int * 8)(*(ids + [0] * (8 - len(ids)))),
                                  len(ids), C.byref(out))
        if rc != 0:
            f_after[e] = None
            skipped += 1
        else:
            f_after[e] = O.frag_score(out, tp)
    return bound, f_after, f_node, skipped


def find_victim(prio, pods, f_after):
    """findVictimPodOnNodeFragAware: the pod of the largest int64(prio - F(node + pod)), strictly
    positive, the first in list order among equals.  (event, score) or None."""
    best, best_score = None, 0
    for e in pods:
        if f_after[e] is None:
            continue
        score = int(prio - f_after[e])  # fp64 subtraction, truncation toward zero
        if score > best_score:
            best, best_score = e, score
    return None if best is None else (best, best_score)


def plan(nodes, typical_list, events, results, state, policy, ratio, ranks=None):
    """The victims in eviction order, the budget and a few facts about the case.
    results / state: what O.run_events returned for `events`."""
    ranks = ranks or name_ranks(nodes)
    bound, f_after, f_node, skipped = candidates(nodes, typical_list, events, results, state)
    budget = min(int(math.ceil(ratio * float(len(bound)))), len(bound))
    pods_on = {}
    for e in bound:  # ascending event index
        pods_on.setdefault(results[e][0], []).append(e)
    victims, per_node = [], {}

    def evict(n, prio, e, score):
        victims.append(dict(event=e, node=n, gpu_mask=results[e][1], score=score, frag_before=prio,
                            frag_after=f_after[e]))
        per_node[n] = per_node.get(n, 0) + 1

    left = budget
    if policy == ONE_POD:
        # nodes by decreasing F, each visited once (deschedule.go:102-114)
        for n in sorted(range(len(nodes)), key=lambda i: (-f_node[i], ranks[i])):
            if left <= 0:
                break
            v = find_victim(f_node[n], pods_on.get(n, []), f_after)
            if v:
                evict(n, f_node[n], *v)
                left -= 1
    elif policy == MULTI_POD:
        # a priority queue of nodes keyed by F; the candidate states stay "the original node + one pod"
        # (nodeResMap is never updated, deschedule.go:124, :156), the priority becomes F(node + victim)
        prio = {n: f_node[n] for n in range(len(nodes))}
        on = {n: list(p) for n, p in pods_on.items()}
        while left > 0 and prio:
            n = min(prio, key=lambda i: (-prio[i], ranks[i]))
            v = find_victim(prio[n], on.get(n, []), f_after)
            if v:
                evict(n, prio[n], *v)
                prio[n] = f_after[v[0]]
                on[n].remove(v[0])
                left -= 1
            else:
                del prio[n]
    else:
        raise ValueError(policy)
    info = dict(bound=len(bound), skipped_by_add=skipped, max_per_node=max(per_node.values(), default=0))
    return victims, budget, info


def extend_events(events, victims):
    """The oracle event stream with the victims' deletions, then their re-creations, in eviction order."""
    idx = [v["event"] for v in victims]
    out = [dict(e) for e in events]
    for e in idx:
        d = dict(events[e])
        d.update(delete=1, ref=e)
        out.append(d)
    for e in idx:
        out.append(dict(events[e]))
    return out


def as_tuples(victims):
    return [(v["event"], v["node"], v["gpu_mask"], v["score"], v["frag_before"], v["frag_after"]) for v in victims]
