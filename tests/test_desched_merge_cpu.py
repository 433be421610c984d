"""The host merge of the descheduling plans of a node-sharded cluster's shards (ksim_desched_merge, ksim_cos_merge;
csrc/ksim_desched_merge_host.hpp): no GPU.

Every shard plans the pods on its own nodes and the cluster's plan is the merge of the shards' lists by (frag_before
descending, node rank ascending) -- cosSim: (gpu_left_milli descending, rank ascending) -- cut at
ceil(ratio * sum of the shards' bound pods).  Checked twice:
- the stand-alone program tests/native_desched_merge (the header under the address and undefined-behaviour
  sanitizers) merges synthetic lists -- worlds 1, 2 and 16, empty parts, every part empty, equal priorities across
  shards, budgets of 0, inside and beyond the list, +inf -- and compares with a plain sort of the union, cut;
- the library's entry points through ctypes, loaded without a device: the reference plan (tests/desched_ref.py,
  tests/desched_cos_ref.py on the oracle's replay) at ratio 1.0 of two fuzz clusters is split by rank range into
  1 .. 16 parts with the ranges' bound counts, and the merge at ratios 0.01, 0.05 and 1.0 must equal the
  reference's plan at that ratio: `==` on every field, doubles included, in eviction order, and the budget.
  (A part cut out of the full plan holds every entry a shard's own capped list would give the merge.)
"""
import ctypes as C
import os
import subprocess

import pytest

import desched_cos_ref as cos
import desched_fuzz_cases as fz
import desched_ref as ref
import ksim
from test_gpu_desched import oracle_run

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native_desched_merge")
CASES = [(2, 97, 900, 0.25), (3, 250, 1200, 0.1)]
SCHEDS = ["FGD", "BestFit"]
WORLDS = [1, 2, 3, 5, 7, 16]
RATIOS = [0.01, 0.05, 1.0]
WIDE = (2 ** 30, 0)
KINDS = [ref.ONE_POD, ref.MULTI_POD, "cosSim"]


def test_native_program_under_sanitizers():
    subprocess.run(["make", "-s", "-C", HERE], check=True)
    p = subprocess.run([os.path.join(HERE, "desched_merge_check")], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       universal_newlines=True, timeout=120)
    print(p.stdout, p.stderr)
    assert p.returncode == 0, p.stderr
    lines = p.stdout.strip().splitlines()
    assert lines == ["cases=%d" % (3 * 3 * 2 * 4 * 2 * 8), "ok"]


_REF = {}


def reference(spec, sched):
    """The oracle's replay of a cluster, its name ranks and the bound pods of every node rank."""
    if (spec, sched) not in _REF:
        case = fz.from_fuzz(*spec)
        res, state = oracle_run(case, ("fuzz",) + spec, sched)
        ranks = ref.name_ranks(case["onodes"])
        bound_at = [0] * len(ranks)
        for e in ref.bound_pods(case["oev"], res):
            bound_at[ranks[res[e][0]]] += 1
        _REF[spec, sched] = case, res, state, ranks, bound_at
    return _REF[spec, sched]


def want_plan(spec, sched, kind, ratio):
    case, res, state, _, _ = reference(spec, sched)
    if kind == "cosSim":
        victims, budget, _ = cos.plan(case["onodes"], case["oev"], res, state, ratio, *WIDE)
        return cos.as_tuples(victims), budget
    victims, budget, _ = ref.plan(case["onodes"], case["otyp"], case["oev"], res, state, kind, ratio)
    return ref.as_tuples(victims), budget


def to_record(kind, t, node):
    if kind == "cosSim":
        return ksim.CosVictim(t[0], node, t[2], 0, t[3], t[4])
    return ksim.Victim(t[0], node, t[2], 0, t[3], t[4], t[5])


def to_tuple(kind, v, node):
    if kind == "cosSim":
        return (v.event, node, v.gpu_mask, v.gpu_left_milli, v.similarity)
    return (v.event, node, v.gpu_mask, v.score, v.frag_before, v.frag_after)


def split(spec, sched, kind, world):
    """The full plan by rank range, as the shards of partition() own the nodes: ([list of records], [bound counts]),
    node = the global rank."""
    _, _, _, ranks, bound_at = reference(spec, sched)
    full, _ = want_plan(spec, sched, kind, 1.0)
    n = len(ranks)
    parts, bounds = [], []
    for k in range(world):
        lo, hi = k * n // world, (k + 1) * n // world
        parts.append([to_record(kind, t, ranks[t[1]]) for t in full if lo <= ranks[t[1]] < hi])
        bounds.append(sum(bound_at[lo:hi]))
    return parts, bounds


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("sched", SCHEDS)
@pytest.mark.parametrize("spec", CASES, ids=["s%d-n%d-e%d-d%g" % c for c in CASES])
def test_library_merges_the_reference_plan_split_by_rank_range(spec, sched, kind):
    _, _, _, ranks, bound_at = reference(spec, sched)
    index_of_rank = {r: i for i, r in enumerate(ranks)}
    merge = ksim.cos_merge if kind == "cosSim" else ksim.desched_merge
    full, full_budget = want_plan(spec, sched, kind, 1.0)
    assert full and full_budget == sum(bound_at)
    for world in WORLDS:
        parts, bounds = split(spec, sched, kind, world)
        assert sum(bounds) == full_budget and sum(len(p) for p in parts) == len(full)
        if 2 <= world <= 7:  # from the reference alone: every range of these clusters holds a victim
            assert all(parts), (world, [len(p) for p in parts])
        for ratio in RATIOS:
            want, budget = want_plan(spec, sched, kind, ratio)
            got, got_budget = merge(parts, bounds, ratio)
            assert got_budget == budget, (world, ratio)
            assert [to_tuple(kind, v, index_of_rank[v.node]) for v in got] == want, (world, ratio)
        # the bytes of the records (what travels between processes), in another shard order
        order = list(reversed(range(world)))
        raw = [b"".join(bytes(v) for v in parts[k]) for k in order]
        got, _ = merge(raw, [bounds[k] for k in order], 0.05)
        assert [to_tuple(kind, v, index_of_rank[v.node]) for v in got] == want_plan(spec, sched, kind, 0.05)[0]


def test_the_budget_cuts_inside_the_lists():
    # what the ratios above are there for: 0.01 cuts inside FGD's list on 97 nodes, 0.05 inside BestFit's on 250
    for spec, sched, ratio in ((CASES[0], "FGD", 0.01), (CASES[1], "BestFit", 0.05)):
        for kind in (ref.ONE_POD, ref.MULTI_POD):
            full, _ = want_plan(spec, sched, kind, 1.0)
            cut, budget = want_plan(spec, sched, kind, ratio)
            print(spec, sched, kind, ratio, "budget", budget, "of", len(full), "victims")
            assert 0 < budget == len(cut) < len(full), (spec, sched, kind, ratio)


def test_library_argument_errors():
    L = ksim.lib()
    for fn, rec in ((L.ksim_desched_merge, ksim.Victim), (L.ksim_cos_merge, ksim.CosVictim)):
        one = (rec * 1)()
        ptrs = (C.POINTER(rec) * 17)(*[C.cast(one, C.POINTER(rec))] * 17)
        ns, bs = (C.c_int * 17)(*[1] * 17), (C.c_int64 * 17)(*[1] * 17)
        out, n, b = (rec * 17)(), C.c_int(-1), C.c_int(-1)
        assert fn(None, ns, bs, 1, 1.0, out, 17, C.byref(n), C.byref(b)) == ksim.KSIM_EINVAL
        assert fn(ptrs, None, bs, 1, 1.0, out, 17, C.byref(n), C.byref(b)) == ksim.KSIM_EINVAL
        assert fn(ptrs, ns, None, 1, 1.0, out, 17, C.byref(n), C.byref(b)) == ksim.KSIM_EINVAL
        assert fn(ptrs, ns, bs, 1, 1.0, out, 17, None, C.byref(b)) == ksim.KSIM_EINVAL
        assert fn(ptrs, ns, bs, 0, 1.0, out, 17, C.byref(n), C.byref(b)) == ksim.KSIM_EINVAL
        assert fn(ptrs, ns, bs, 17, 1.0, out, 17, C.byref(n), C.byref(b)) == ksim.KSIM_EINVAL
        assert fn(ptrs, ns, bs, 1, -0.5, out, 17, C.byref(n), C.byref(b)) == ksim.KSIM_EINVAL
        assert fn(ptrs, ns, bs, 1, float("nan"), out, 17, C.byref(n), C.byref(b)) == ksim.KSIM_EINVAL
        ns[1] = -1
        assert fn(ptrs, ns, bs, 2, 1.0, out, 17, C.byref(n), C.byref(b)) == ksim.KSIM_EINVAL
        ns[1] = 1
        assert fn(ptrs, ns, bs, 16, 1.0, out, 15, C.byref(n), C.byref(b)) == ksim.KSIM_ERANGE
        assert (n.value, b.value) == (16, 16)
        assert fn(ptrs, ns, bs, 16, float("inf"), out, 17, C.byref(n), C.byref(b)) == ksim.KSIM_OK and n.value == 16
    # empty inputs, and the shape errors of the Python layer
    assert ksim.desched_merge([[], []], [0, 0], 1.0) == ([], 0)
    assert ksim.cos_merge([b""], [3], 0.5) == ([], 2)
    with pytest.raises(ValueError):
        ksim.desched_merge([], [], 1.0)
    with pytest.raises(ValueError):
        ksim.desched_merge([[]], [1, 2], 1.0)
    with pytest.raises(ValueError):
        ksim.cos_merge([b"\0" * 31], [1], 1.0)
    # the null checks of the device-side entry points come before any device work
    n = C.c_int(-1)
    assert L.ksim_engine_get_victim_part(None, None, 0, C.byref(n), None) == ksim.KSIM_EINVAL
    assert L.ksim_engine_get_cos_victim_part(None, None, 0, C.byref(n), None) == ksim.KSIM_EINVAL
    assert L.ksim_shard_group_deschedule(None, 1, 0, 0.1) == ksim.KSIM_EINVAL
    assert L.ksim_shard_group_deschedule_cossim(None, 1, 0.1, 2000, 500) == ksim.KSIM_EINVAL
    assert L.ksim_shard_group_get_victims(None, 1, None, 0, C.byref(n), None) == ksim.KSIM_EINVAL
    assert L.ksim_shard_group_get_cos_victims(None, 1, None, 0, C.byref(n), None) == ksim.KSIM_EINVAL
