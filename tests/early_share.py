"""How often k_memo's owner may publish a step's winner before its critical F: a CPU count from the oracle's results.

A pod step's winner is max(ex, fresh): ex the best of the other nodes, fresh the key of d, the node the previous
decided event changed, and 0 when Filter of the step's own class refuses d.  Then the winner is ex whatever the F
evaluations on d return, and the owner publishes at once (ksim_memo.hpp, `early`).  This module restates Filter
(predicates of the scheduler framework, open_gpu_share.go Filter) on node states rebuilt from the oracle's results,
counts those steps, and cross-checks the restatement against the oracle's n_feasible on a sample of steps.

scripts/memo_infeasible_share.py prints the table for whole traces; tests/test_gpu_memo_early.py uses the count to
assert that each of its streams reaches the path it is meant to.
"""

MILLI = 1000


def node_states(onodes):
    """Mutable node states from the oracle's node dicts: [cpu_left, mem_left, pods_left, [gpu milli left], model]."""
    return [[n["cpu"], n["mem"], n.get("pods", 1001), [MILLI] * n["gpu"], n.get("model", "")] for n in onodes]


def filter_reason(st, e):
    """None when the node state passes Filter for the event's request, else 'pods' | 'cpu' | 'mem' | 'gpu'
    (no GPU, a GPU model the pod does not accept, or no fit)."""
    cpu_left, mem_left, pods_left, gl, model = st
    if pods_left < 1:
        return "pods"
    if not (e["cpu"] == 0 and e["mem"] == 0):
        if cpu_left < e["cpu"]:
            return "cpu"
        if mem_left < e["mem"]:
            return "mem"
    milli, num = e["milli"], e["num"]
    if milli <= 0:
        return None
    if not gl or num <= 0:
        return "gpu"
    spec = e.get("type", "")
    if spec and model not in spec.split("|"):
        return "gpu"
    if num == 1:
        return None if max(gl) >= milli else "gpu"
    return None if sum(g // milli for g in gl) >= num else "gpu"


def _bind(st, e, mask, sign):
    st[0] -= sign * e["cpu"]
    st[1] -= sign * e["mem"]
    st[2] -= sign
    for g in range(len(st[3])):
        if (mask >> g) & 1:
            st[3][g] -= sign * e["milli"]


def class_of(e):
    return (e["cpu"], e.get("cpu_nz", e["cpu"]), e["mem"], e["milli"], e["num"], e.get("type", ""))


def count(onodes, oevents, results, skip=True, check_every=40, limit=None, visit=None):
    """Walk the stream with the oracle's results (node, gpu_mask, score, n_feasible, status per event).

    skip: the lean kernel's dead-class skip -- an event of a class that found no feasible node earlier is not decided
    and d is carried over it; without it (the general kernel) every event is decided and d is the node event s-1
    changed, none after an event that bound nothing.
    -> dict: live (decided creates), early (d exists and fails Filter for the step's class), d_wins, nod (decided
    with no d), dead_pub (decided steps that found no feasible node at all), reasons {reason: n}, checks, mismatches,
    flags (per event: None not decided / delete, else True early / False).
    visit(s, event, d, states, reason): called on every decided step before its Bind (states: as node_states)."""
    st = node_states(onodes)
    dead = set()
    out = dict(live=0, early=0, d_wins=0, nod=0, dead_pub=0, reasons={}, checks=0, mismatches=0, flags=[])
    d = -1
    for s, (e, r) in enumerate(zip(oevents, results)):
        if limit is not None and s >= limit:
            break
        node, mask, _, nfeas, _ = r
        if e.get("delete", 0):
            out["flags"].append(None)
            d = -1
            if node >= 0:
                _bind(st[node], oevents[e["ref"]], mask, -1)
                d = node
            continue
        if check_every and s % check_every == 0:
            out["checks"] += 1
            if sum(1 for x in st if filter_reason(x, e) is None) != nfeas:
                out["mismatches"] += 1
        c = class_of(e)
        if skip and c in dead:
            out["flags"].append(None)
            continue
        out["live"] += 1
        why = filter_reason(st[d], e) if d >= 0 else None
        out["flags"].append(why is not None)
        if visit is not None:
            visit(s, e, d, st, why)
        if d < 0:
            out["nod"] += 1
        elif why is not None:
            out["early"] += 1
            out["reasons"][why] = out["reasons"].get(why, 0) + 1
        elif node == d:
            out["d_wins"] += 1
        if nfeas == 0:
            out["dead_pub"] += 1
            dead.add(c)
        d = -1
        if node >= 0:
            _bind(st[node], e, mask, +1)
            d = node
    return out
