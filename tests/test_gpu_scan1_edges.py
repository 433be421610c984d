"""k_scan1 and k_scan1_mix on adversarial clusters and at their size edges, against the oracle.

One 256-thread workgroup per replica: thread t scans the node slots t, t + 256, ..., in VGPRs up to
1280 nodes (KSIM_VARIANT scan1=2) or in LDS (scan1=1, and always above 1280).  The tests aim at
  - the node counts where a lane or a slot changes meaning (63 / 64 / 65, 255 / 256 / 257, 1279 / 1280 /
    1281) on fuzz clusters (tests/fuzz_cases.py: GPU-less and 3/5/6/7-GPU nodes, tight pod limits,
    unknown models, pipe lists), whose replays bind in every slot and wave (tests/test_scan1_cases.py);
  - the mixed launch with a different cluster per replica, and with the worst / random GPU selectors;
  - the dead-class skip at the edges of the 128-event window and of the mask's words, and at the class
    count that turns it off (tests/scan1_cases.py), with the skip on and off;
  - the report forms (k_scan1<*, true, *>, k_scan1_mix<true, *>, k_report_overlap behind the mixed
    launch's queue) against the oracle's exact per-event report;
  - resuming from a used state under all five policies.
Bar: per event (node, gpu_mask, score, n_feasible, status) and the final state equal the oracle's;
reports as test_gpu_report.assert_reports.  Every run asserts the kernels it ran on.  Every test
needs a gfx950 device.
"""
import pytest

import ksim
import pyoracle as O
import scan1_cases as SC
from test_gpu_fuzz import check_state
from test_gpu_parity import POLICIES
from test_gpu_report import assert_reports

pytestmark = pytest.mark.gpu

SEED = 5
FGD, CHEAP = POLICIES[0], POLICIES[1:]  # (engine name, oracle policy, oracle selector)
SEL = {"best": O.SEL_BEST, "worst": O.SEL_WORST, "random": O.SEL_RANDOM}
PLACES = [2, 1]  # KSIM_VARIANT scan1: the node records in VGPRs, in LDS
PLACE_IDS = ["vgpr", "lds"]
MIX = (["k_scan1_mix"], 1)  # the kernels of a mixed run and their launches
EDGE_N = [1, 63, 64, 65, 255, 256, 257, 1279, 1280, 1281]


def variant(monkeypatch, place, mix, skip=1, overlap=1):
    monkeypatch.setenv("KSIM_VARIANT", "scan1=%d,scan1_mix=%d,skip=%d,report_overlap=%d" % (place, mix, skip, overlap))


def places(n):
    return PLACES if n <= 1280 else PLACES[1:]  # above 1280 nodes only the LDS form exists


def ragged(n_events, count):
    """count stream lengths from n_events down (the mixed launch orders its replicas longest first)"""
    return [max(1, n_events - (n_events // 11) * r) for r in range(count)]


def run_group(reps, report=False, run_mode=0):
    """One engine at one workgroup per replica; reps: [(case, (name, pol, sel), events, gpusel or None)],
    every case of one node count.  -> ([(results, state, reports)], kernels (each name once) and their launches,
    path, overlapped replicas)"""
    n = len(reps[0][0]["onodes"])
    eng = ksim.Engine(n, len(reps), run_mode=run_mode, wgs_per_replica=1)
    try:
        if report:
            eng.set_report(True)
        for r, (case, (name, _, _), n_ev, gpusel) in enumerate(reps):
            assert len(case["onodes"]) == n
            eng.set_nodes(r, case["nodes"])
            eng.set_typical(r, case["typical"], case["typical_n"])
            eng.set_policy(r, name, gpusel=gpusel, seed=SEED)
            eng.load_events(r, case["events"], n_ev)
        eng.run()
        got = [(eng.results(r), eng.nodes(r), eng.reports(r) if report else None) for r in range(len(reps))]
        ran = (eng.last_run_kernels(), eng.last_run_launches()[0])
        return got, ran, eng.last_run_path(), eng.last_run_report_overlap()
    finally:
        eng.close()


def check_group(reps, got, report=False, what=""):
    for (case, (name, pol, sel), n_ev, gpusel), (res, state, rep) in zip(reps, got):
        want, want_state, want_rep = O.run_events(case["onodes"], case["otypical"], case["oevents"][:n_ev], policy=pol,
                                                  gpu_sel=SEL[gpusel] if gpusel else sel, seed=SEED, threads=16,
                                                  with_report=report)
        bad = [i for i, (a, b) in enumerate(zip(res, want)) if a != b]
        assert len(res) == len(want) and not bad, \
            "%s %s: first mismatch at event %d: gpu %s oracle %s" % (what, name, bad[0], res[bad[0]], want[bad[0]])
        check_state(state, want_state)
        if report:
            assert_reports(rep, want_rep)


def both_kernels(monkeypatch, reps, place, skip=1, report=False, what=""):
    """The replicas (one per cheap policy) on five k_scan1 launches, then in one k_scan1_mix launch."""
    for mix, kernels in ((0, (["k_scan1"], len(reps))), (1, MIX)):
        variant(monkeypatch, place, mix, skip)
        got, ran, path, _ = run_group(reps, report=report)
        assert (ran, path) == (kernels, "k_scan1"), what
        check_group(reps, got, report, "%s %s" % (what, kernels[0][0]))


def one_per_policy(case, lens=None):
    lens = lens or ragged(case["n_events"], len(CHEAP))
    return [(case, p, lens[r], None) for r, p in enumerate(CHEAP)]


# ---- a. node-count edges, both record placements ----
@pytest.mark.parametrize("n,place", [(n, p) for n in EDGE_N for p in places(n)],
                         ids=["n%d-%s" % (n, PLACE_IDS[PLACES.index(p)]) for n in EDGE_N for p in places(n)])
def test_node_count_edges(monkeypatch, n, place):
    both_kernels(monkeypatch, one_per_policy(SC.edge_case(n)), place, what="N=%d" % n)


# ---- b. the mixed launch, a different cluster per replica ----
@pytest.mark.parametrize("n,place", [(97, 2), (97, 1), (1281, 1)], ids=["n97-vgpr", "n97-lds", "n1281-lds"])
def test_mixed_launch_cluster_per_replica(monkeypatch, n, place):
    # seven replicas, seven clusters of one node count; BestFit and GpuClustering twice, at different lengths
    ne = SC.EDGE[n][1]
    pols = [CHEAP[0], CHEAP[1], CHEAP[2], CHEAP[3], CHEAP[4], CHEAP[0], CHEAP[3]]
    lens = [ne, ne * 2 // 3, ne - 1, ne // 2, ne * 3 // 4, ne // 3, ne - 129]
    reps = [(SC.edge_case(n, seed=60 + r), pols[r], lens[r], None) for r in range(7)]
    variant(monkeypatch, place, 1)
    got, ran, path, _ = run_group(reps)
    assert (ran, path) == (MIX, "k_scan1")
    check_group(reps, got, what="N=%d" % n)


# ---- c. the worst and random GPU selectors ----
@pytest.mark.parametrize("place", PLACES, ids=PLACE_IDS)
def test_mixed_launch_gpu_selectors(monkeypatch, place):
    case = SC.edge_case(97)
    reps = [(case, CHEAP[0], 400, "worst"), (case, CHEAP[0], 350, "random"), (case, CHEAP[2], 400, "worst"),
            (case, CHEAP[2], 300, "random")]
    variant(monkeypatch, place, 1)
    got, ran, path, _ = run_group(reps)
    assert (ran, path) == (MIX, "k_scan1")
    check_group(reps, got)
    # the selectors decide: a share pod's GPU differs from the best-fit selector's somewhere
    best = O.run_events(case["onodes"], case["otypical"], case["oevents"], policy=O.POL_BESTFIT, gpu_sel=O.SEL_BEST,
                        seed=SEED, threads=16)[0]
    assert got[0][0] != best and got[1][0][:350] != best[:350] and got[0][0][:350] != got[1][0]


# ---- d. the dead-class skip and the event window ----
@pytest.mark.parametrize("skip", [1, 0], ids=["skip", "noskip"])
@pytest.mark.parametrize("place", PLACES, ids=PLACE_IDS)
@pytest.mark.parametrize("cid", SC.CRAFTED)
def test_dead_class_skip_and_window(monkeypatch, cid, place, skip):
    # every replica replays the whole stream: the dead events sit at the same window positions for all
    case = SC.crafted(cid)
    both_kernels(monkeypatch, one_per_policy(case, [case["n_events"]] * len(CHEAP)), place, skip=skip, what=cid)


@pytest.mark.parametrize("place", PLACES, ids=PLACE_IDS)
def test_mixed_launch_beside_a_replica_over_the_class_limit(monkeypatch, place):
    # 1025 classes in one replica turn the skip off for the whole launch: the others' dead repeats are scanned
    over, at = SC.crafted("limit-1025"), SC.crafted("limit-1024")
    assert len(over["onodes"]) == len(at["onodes"])
    reps = [(over, CHEAP[0], over["n_events"], None), (at, CHEAP[2], at["n_events"], None),
            (at, CHEAP[3], at["n_events"] - 3, None), (over, CHEAP[4], over["n_events"] - 9, None),
            (at, CHEAP[1], at["n_events"], None)]
    variant(monkeypatch, place, 1)
    got, ran, path, _ = run_group(reps)
    assert (ran, path) == (MIX, "k_scan1")
    check_group(reps, got)


# ---- e. the report forms against the oracle's exact per-event report ----
def report_case(cid):
    return SC.crafted(cid) if isinstance(cid, str) else SC.edge_case(cid)


REPORT_CASES = [(c, p) for c in (97, 257, "window-400", 1281) for p in (places(c) if isinstance(c, int) else PLACES)]


@pytest.mark.parametrize("cid,place", REPORT_CASES, ids=["%s-%s" % (c, PLACE_IDS[PLACES.index(p)]) for c, p in REPORT_CASES])
def test_report_forms(monkeypatch, cid, place):
    # (the oracle's exact report costs it a pass over the nodes per event: 120 events at 1281 nodes)
    case = report_case(cid)
    both_kernels(monkeypatch, one_per_policy(case, ragged(120 if cid == 1281 else case["n_events"], len(CHEAP))), place,
                 report=True, what=str(cid))


@pytest.mark.parametrize("place", PLACES, ids=PLACE_IDS)
@pytest.mark.parametrize("cid", [97, 257, "window-400"])
def test_report_overlapped_behind_fgd(monkeypatch, cid, place):
    # an FGD replica on k_hmemo and the five cheap ones in one k_scan1_mix launch, concurrently: the mixed group's
    # replicas report through its ticket queue (k_report_overlap) as each ends, or all after the launch
    case = report_case(cid)
    reps = [(case, FGD, case["n_events"], None)] + one_per_policy(case)
    monkeypatch.setenv("KSIM_TEST", "report_overlap=1")
    for overlap in (1, 0):
        variant(monkeypatch, place, 1, overlap=overlap)
        got, ran, path, overlapped = run_group(reps, report=True, run_mode=5)
        assert ran == (["k_hmemo", "k_scan1_mix"], 2), overlap
        assert overlapped == (len(CHEAP) if overlap else 0)
        check_group(reps, got, report=True, what="%s overlap=%d" % (cid, overlap))


# ---- f. resume from a used state, all five policies ----
def node_fields(s):
    return (s.cpu_used_milli, s.mem_used_mib, s.pods_used, list(s.gpu_used_milli), list(s.tag_count))


@pytest.mark.parametrize("place", PLACES, ids=PLACE_IDS)
def test_resume_from_a_used_state(monkeypatch, place):
    case = SC.edge_case(257)
    n, k = case["n_events"], 170
    variant(monkeypatch, place, 1)

    def run(reps):
        got, ran, path, _ = run_group(reps)
        assert (ran, path) == (MIX, "k_scan1")
        return got
    whole = [(case, p, n, None) for p in CHEAP]
    full = run(whole)
    check_group(whole, full)
    head = run([(case, p, k, None) for p in CHEAP])
    # Random's draws hash the event's index: its tail keeps the indices behind k pods no node can take
    tail_ev = (ksim.Pod * (n - k))(*[case["events"][k + i] for i in range(n - k)])
    pad_ev = (ksim.Pod * n)(*([ksim.make_pod(SC.BIG_CPU * 100)] * k + list(tail_ev)))
    tails = []
    for r, p in enumerate(CHEAP):
        mid = head[r][1]
        # the state carries partly used GPUs and tag counts
        assert any(0 < mid[i].gpu_used_milli[g] < 1000 for i in range(257) for g in range(mid[i].gpu_count)), p[0]
        assert any(sum(mid[i].tag_count) > 0 for i in range(257)), p[0]
        pad = p[0] == "Random"
        tails.append((dict(case, nodes=mid, events=pad_ev if pad else tail_ev), p, n if pad else n - k, None))
    tail = run(tails)
    for r, p in enumerate(CHEAP):
        assert head[r][0] == full[r][0][:k], p[0]
        assert tail[r][0][-(n - k):] == full[r][0][k:], p[0]
        assert [node_fields(s) for s in tail[r][1]] == [node_fields(s) for s in full[r][1]], p[0]
