"""k_memo's early publish: when Filter of the step's own class refuses d (the node the previous step changed) the
winner is the precomputed best of the other nodes, and the owner stores the granule before the critical F of d
exist (ksim_memo.hpp, `early`); the join, the score group's keys on d and the result row follow the store.

Every case is compared with the C oracle row for row (node, gpu_mask, score, n_feasible, status) and on the final
node state, at 2, 3 and 25 workgroups per replica, on 64 < N <= 130 nodes (a class scan spans more than one wave
round) and at most about 400 events.  The share of early steps of each stream is counted on the CPU from the
oracle's results (tests/early_share.py, the restatement scripts/memo_infeasible_share.py prints), and each case
asserts that its stream reaches the path it is meant to.  One exception to the node bound: the keys move to HBM
only when they do not fit in LDS, which no cluster of 130 nodes brings about, so that form runs the first 400
events of gpuspec33 on its whole cluster at two workgroups.  Every test needs a gfx950 device.
"""
import functools

import pytest

import early_share as ES
import helpers
import ksim
import pyoracle as O
from fuzz_cases import VOCAB, _mask
from test_gpu_fuzz import check_state
from test_gpu_report import assert_reports

pytestmark = pytest.mark.gpu

MEMO = 3
WGS = pytest.mark.parametrize("wgs", [2, 3, 25])


def build_case(nodes, creates):
    """nodes: (cpu, mem, pods, gpu) each, model G2; creates: (cpu, mem, milli, num) each -> a fuzz_cases-style case."""
    nn = len(nodes)
    names = ["%04d-node-%d" % ((i * 37) % nn, i) for i in range(nn)]  # (37 is coprime to every N used here)
    order = sorted(range(nn), key=lambda i: names[i].encode())
    rank = {i: r for r, i in enumerate(order)}
    arr = (ksim.Node * nn)()
    onodes = []
    for i, (cpu, mem, pods, gpu) in enumerate(nodes):
        n = arr[i]
        n.cpu_alloc_milli, n.mem_alloc_mib, n.pods_alloc = cpu, mem, pods
        n.gpu_count, n.gpu_type, n.name_rank = gpu, 0, rank[i]
        onodes.append(dict(name=names[i], cpu=cpu, mem=mem, pods=pods, gpu=gpu, model=VOCAB[0] if gpu else ""))
    evs, oev = [], []
    for cpu, mem, milli, num in creates:
        evs.append(ksim.make_pod(cpu, milli, num, mem, _mask("", VOCAB), cpu_nz=cpu if cpu > 0 else 100))
        oev.append(dict(cpu=cpu, cpu_nz=cpu if cpu > 0 else 100, mem=mem, milli=milli, num=num, type=""))
    otyp = O.get_typical_pods([(c, m, n, "") for c, _, m, n in creates])
    typ = (ksim.Typical * max(1, len(otyp)))()
    for i, (cpu, milli, num, spec, freq) in enumerate(otyp):
        typ[i].cpu_milli, typ[i].gpu_milli, typ[i].gpu_count = cpu, milli, num
        typ[i].type_mask, typ[i].freq = _mask(spec, VOCAB), freq
    return dict(nodes=arr, events=(ksim.Pod * len(evs))(*evs), n_events=len(evs), typical=typ, typical_n=len(otyp),
                onodes=onodes, oevents=oev, otypical=otyp)


def with_oracle(case, skip=True, with_report=False):
    """The oracle's results, final state (and reports) and the CPU count of early steps, once per case."""
    want, want_state, reps = O.run_events(case["onodes"], case["otypical"], case["oevents"], policy=O.POL_FGD,
                                          gpu_sel=O.SEL_FGD, threads=16, with_report=with_report)
    cnt = ES.count(case["onodes"], case["oevents"], want, skip=skip, check_every=10)
    assert cnt["checks"] > 0 and cnt["mismatches"] == 0, "the Filter restatement disagrees with the oracle's n_feasible"
    case.update(want=want, want_state=want_state, want_reports=reps, count=cnt)
    return case


def share(case):
    """Early steps among the decided steps after the first, percent."""
    c = case["count"]
    return 100.0 * c["early"] / max(c["live"] - 1, 1)


@functools.lru_cache(maxsize=None)
def always_early():
    # 8-GPU nodes, pods of 8 whole GPUs in three classes (three owners): every Bind fills d
    creates = [((1 + k % 3) * 1000, 1024, 1000, 8) for k in range(110)]
    return with_oracle(build_case([(64000, 262144, 110, 8)] * 96, creates))


@functools.lru_cache(maxsize=None)
def never_early():
    # small share pods on large nodes: d always keeps room for the next pod
    # (all 300 together ask for less than one node holds, of every resource)
    creates = [((1 + k % 4) * 100, 512, (20, 30, 25)[k % 3], 1) for k in range(300)]
    return with_oracle(build_case([(128000, 786432, 1001, 8)] * 80, creates))


@functools.lru_cache(maxsize=None)
def sibling():
    # one score group (cpu 1000, 300 milli, one GPU), two classes: A asks for most of a node's memory, B for little.
    # After an A on d the next A finds d infeasible and B does not
    creates = [(1000, 60000 if k % 3 else 1000, 300, 1) for k in range(200)]
    return with_oracle(build_case([(32000, 65536, 110, 4)] * 70, creates))


@functools.lru_cache(maxsize=None)
def cpu_bound():
    # two classes whose CPU request no node can take twice, one whole GPU of eight each
    creates = [(6000 if k % 2 else 5000, 1024, 1000, 1) for k in range(150)]
    return with_oracle(build_case([(8000, 262144, 110, 8)] * 100, creates))


@functools.lru_cache(maxsize=None)
def dead_class():
    # one-GPU nodes: the whole-GPU class X fills the cluster, its next event finds no node at all and the class is
    # dead; the CPU-only class Y goes on
    creates = [(1000, 1024, 1000, 1)] * 70 + [(500, 256, 0, 0), (1000, 1024, 1000, 1)] * 40
    return with_oracle(build_case([(32000, 65536, 110, 1)] * 66, creates))


def mixed_inputs(n_create=400):
    t = ksim.Trace.openb("default")
    rp = t.replay(seed=42, tune_ratio=1.3, shuffle=True)
    keep = list(range(0, t.num_nodes, 12))[:96]
    arr, n = t.typical()
    return t, rp, keep, dict(nodes=helpers.subset_nodes(rp, keep), events=rp.events, n_events=n_create, typical=arr,
                             typical_n=n, onodes=helpers.oracle_subset(t, rp, keep), otypical=helpers.oracle_typical(t),
                             oevents=helpers.oracle_events(t, rp, n_create))


@functools.lru_cache(maxsize=None)
def mixed():
    # the first 400 events of openb default (tune 1.3, shuffled) on a 96-node subset, with the report
    return with_oracle(mixed_inputs()[3], with_report=True)


@functools.lru_cache(maxsize=None)
def mixed_deletes():
    t, rp, keep, case = mixed_inputs()
    evs, oev = helpers.delete_stream(t, rp, 300, 0.3, seed=3)
    case.update(events=evs, n_events=len(evs), oevents=oev)
    return with_oracle(case, skip=False)


@functools.lru_cache(maxsize=None)
def hbm_keys():
    t = ksim.Trace.openb("gpuspec33")
    rp = t.replay(seed=43, tune_ratio=1.3, shuffle=True)
    arr, n = t.typical()
    return with_oracle(dict(nodes=rp.nodes, events=rp.events, n_events=400, typical=arr, typical_n=n,
                            onodes=helpers.oracle_nodes(t, rp), otypical=helpers.oracle_typical(t),
                            oevents=helpers.oracle_events(t, rp, 400)))


def run(case, wgs, report=False):
    eng = ksim.Engine(len(case["onodes"]), 1, run_mode=MEMO, wgs_per_replica=wgs)
    try:
        eng.set_nodes(0, case["nodes"])
        eng.set_typical(0, case["typical"], case["typical_n"])
        eng.set_policy(0, "FGD")
        if report:
            eng.set_report(True)
        eng.load_events(0, case["events"], case["n_events"])
        eng.run()
        assert eng.last_run_wgs() == wgs
        return eng.results(0), eng.nodes(0), eng.reports(0) if report else None, eng.last_run_kernels()
    finally:
        eng.close()


def check(case, wgs, kernel="k_memo", report=False):
    got, state, reps, kern = run(case, wgs, report)
    assert kern == [kernel]
    want = case["want"]
    bad = [i for i, (a, b) in enumerate(zip(got, want)) if a != b]
    assert len(got) == len(want) and not bad, \
        "first mismatch at event %d: gpu %s oracle %s" % (bad[0], got[bad[0]], want[bad[0]])
    check_state(state, case["want_state"])
    if report:
        assert_reports(reps, case["want_reports"])


@WGS
def test_always_early(wgs):
    case = always_early()
    print("always early: %.1f %% of the decided steps after the first" % share(case))
    assert share(case) >= 90.0
    check(case, wgs)


@WGS
def test_never_early(wgs):
    case = never_early()
    assert case["count"]["early"] == 0 and case["count"]["live"] == case["n_events"]
    check(case, wgs)


@WGS
def test_sibling_class_feasible_on_d(wgs):
    # the step's class does not fit d, its sibling of the same score group does: the sibling's key on d is still
    # refreshed from the critical F after the early store, and a later event of the sibling that this d wins shows it
    case = sibling()
    pending, seen = {}, [0, 0]  # node -> the sibling's request refreshed there behind an early store

    def visit(s, e, d, st, why):
        win = case["want"][s][0]
        if win in pending and ES.class_of(e) == pending[win]:
            seen[1] += 1
        pending.pop(win, None)  # the winner's keys are refreshed again on the next step
        if why is None:
            return
        for o in case["oevents"]:
            if (o["cpu_nz"], o["milli"], o["num"]) == (e["cpu_nz"], e["milli"], e["num"]) and \
                    ES.class_of(o) != ES.class_of(e) and ES.filter_reason(st[d], o) is None:
                seen[0] += 1
                pending[d] = ES.class_of(o)
                break

    ES.count(case["onodes"], case["oevents"], case["want"], check_every=0, visit=visit)
    print("sibling: %d early steps with a feasible sibling on d, %d later sibling events won by that d" % tuple(seen))
    assert seen[0] >= 1 and seen[1] >= 1
    check(case, wgs)


@WGS
def test_cpu_bound_infeasibility(wgs):
    case = cpu_bound()
    c = case["count"]
    print("cpu bound: %.1f %% early, reasons %s" % (share(case), c["reasons"]))
    assert c["reasons"].get("cpu", 0) >= 50 and set(c["reasons"]) == {"cpu"}  # (a node keeps seven free GPUs)
    check(case, wgs)


@WGS
def test_dead_class_published_early(wgs):
    # an early publish that carries "no feasible node" (the granule's bit 1), after which the class's events are skipped
    case = dead_class()
    flags, want = case["count"]["flags"], case["want"]
    hits = [s for s, f in enumerate(flags) if f and want[s][3] == 0]
    assert hits, "no early step without a feasible node"
    s0 = hits[0]
    later = [s for s in range(s0 + 1, len(flags)) if ES.class_of(case["oevents"][s]) == ES.class_of(case["oevents"][s0])]
    assert later and all(flags[s] is None for s in later)
    check(case, wgs)


@WGS
def test_mixed_lean(wgs):
    case = mixed()
    print("mixed: %.1f %% of the decided steps after the first publish early" % share(case))
    assert 0.0 < share(case) < 100.0
    check(case, wgs)


@WGS
def test_mixed_report_form(wgs):
    check(mixed(), wgs, report=True)


@WGS
def test_mixed_general_form_with_deletes(wgs):
    case = mixed_deletes()
    assert 0.0 < share(case) < 100.0
    assert any(e.get("delete") for e in case["oevents"])
    check(case, wgs)


def test_keys_in_hbm_form():
    case = hbm_keys()
    print("gpuspec33: %.1f %% early" % share(case))
    assert 0.0 < share(case) < 100.0
    check(case, 2, kernel="k_memo_hkeys")


@WGS
def test_mixed_granule_long_before_the_f_values(wgs, monkeypatch):
    # the hdelay test knob's critical-wave point: the owner's waves 1-9 sleep before their F on about half the
    # steps, so an early granule is out (and the other workgroups a step ahead) long before the join
    monkeypatch.setenv("KSIM_TEST", "hdelay=%s" % "0x2")
    check(mixed(), wgs)
