"""Plain-Python restatement of the reference's cosSim descheduling policy -- TEST INFRASTRUCTURE.

descheduleClusterOnCosSim (pkg/simulator/deschedule.go:49-92), findVictimPodOnCosSim and
sortNodeStatusByResource (deschedule_utils.go:15-71), GetResourceSimilarity and
CalculateVectorCosineSimilarity (pkg/utils/utils.go:1181-1218), built from the oracle's orc_node_add
for NodeResource.Add and Python floats (math.sqrt, `*` and `/` are correctly rounded, as Go's are).
The order contract where the reference's order is the fake API's list: pods of a node in ascending
creation-event index.  The node order is the reference's own: names are unique.
"""
import ctypes as C
import math

import desched_ref as ref
import pyoracle as O

CPU_BAR, GPU_BAR = 2000, 500  # deschedule.go:52-53


def cosine(vec1, vec2):
    """CalculateVectorCosineSimilarity: three running sums, two roots, inner / (m1 * m2); -1 on a zero magnitude."""
    m1 = m2 = inner = 0.0
    for a, b in zip(vec1, vec2):
        a, b = float(a), float(b)
        m1 += a * a
        m2 += b * b
        inner += a * b
    m1, m2 = math.sqrt(m1), math.sqrt(m2)
    if m1 == 0 or m2 == 0:
        return -1.0
    return inner / (m1 * m2)


def similarity_of(node_res, cpu_nz, milli, num, ids):
    """GetResourceSimilarity(node + pod, pod) after NodeResource.Add; -1 for every case the reference skips.
    Returns (similarity, why) with why in ok / add / zero / range."""
    pod = O.pod_res(cpu_nz, milli, num, "")
    out = O.NodeResource()
    pad = max(8, len(ids))
    rc = O.lib().orc_node_add(C.byref(node_res), C.byref(pod), (C.c_int * pad)(*(list(ids) + [0] * (pad - len(ids)))),
                              len(ids), C.byref(out))
    if rc != 0:
        return -1.0, "add"
    free = [out.milli_cpu_left, sum(out.milli_gpu_left[g] for g in range(out.n_gpu_left))]
    req = [cpu_nz, milli * num]
    s = cosine(free, req)
    if s == -1.0 and (not any(free) or not any(req)):
        return -1.0, "zero"
    if s < 0 - 1e-3 or s > 1 + 1e-3:
        return -1.0, "range"
    return s, "ok"


def find_victim(node_res, pods, events, results):
    """findVictimPodOnCosSim: the pod of the least similarity in [0, 1), the first in list order among equals.
    (event, similarity) or None."""
    best, best_sim = None, 1.0
    for e in pods:
        ev, mask = events[e], results[e][1]
        s, _ = similarity_of(node_res, ev.get("cpu_nz", ev["cpu"]), ev["milli"], ev["num"],
                             [g for g in range(8) if mask >> g & 1])
        if s >= 0 and s < best_sim:
            best, best_sim = e, s
    return None if best is None else (best, best_sim)


def plan(nodes, events, results, state, ratio, cpu_bar=CPU_BAR, gpu_bar=GPU_BAR):
    """The victims in eviction order, the budget and a few facts about the case.
    results / state: what O.run_events returned for `events`."""
    res_of = [ref.node_resource(nodes[i], state[i]) for i in range(len(nodes))]
    bound = ref.bound_pods(events, results)
    budget = min(int(math.ceil(ratio * float(len(bound)))), len(bound))
    pods_on = {}
    for e in bound:  # ascending event index
        pods_on.setdefault(results[e][0], []).append(e)
    gpu_left = [sum(state[i][3][:nodes[i]["gpu"]]) for i in range(len(nodes))]
    # sortNodeStatusByResource: the nodes below the CPU bar first, by total milli-GPU left descending, then name
    # (the others are skipped by the loop, so their place does not matter)
    order = sorted(range(len(nodes)), key=lambda i: (state[i][0] >= cpu_bar, -gpu_left[i], nodes[i]["name"].encode()))
    victims, left, n_cand, n_with = [], budget, 0, 0
    for i in order:
        if state[i][0] >= cpu_bar:
            continue
        if not any(v > gpu_bar for v in state[i][3][:nodes[i]["gpu"]]):
            continue
        n_cand += 1
        v = find_victim(res_of[i], pods_on.get(i, []), events, results)
        if v:
            n_with += 1
            if left > 0:  # (the reference stops walking here; the count goes on for the tests)
                victims.append(dict(event=v[0], node=i, gpu_mask=results[v[0]][1], gpu_left=gpu_left[i],
                                    similarity=v[1]))
                left -= 1
    return victims, budget, dict(bound=len(bound), candidates=n_cand, with_victim=n_with)


def as_tuples(victims):
    return [(v["event"], v["node"], v["gpu_mask"], v["gpu_left"], v["similarity"]) for v in victims]
