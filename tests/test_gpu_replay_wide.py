"""k_replay's exchange at 65-256 workgroups per replica (kSub = 4: one wave-0 lane polls up to four granule columns,
lane + 64 j) against the oracle, on clusters of a few hundred nodes.

At these widths a slice holds one to ten nodes, so the winner, the only feasible node, the Score error and BestFit's
differing score sit in columns past 63 all the time; a wrong mask or column index in one of the exchange's folds
(`exchange`, `pf_collect`, `pf_miss_round`, the polls) changes a decision.  Widths: 65 and 193 (one lane in the last
column), 128 (two full columns), 129 (the first lane of the third), 256 (all four; N where the cluster has fewer
nodes).  Clusters: tests/fuzz_cases.py's case 3 (deletions: the general instantiation; one node per slice at 250, and
at 193 only 125 slices hold nodes) and case 6 (create-only: the lean one; 5 to 56 empty trailing slices).  Every
policy, the cluster report, PWR and PWR + FGD (the one-round exchange and its miss round), several replicas in one
launch (the granule base of a replica) and the node-sharded group's exchange over world x K columns
(KSIM_TEST=group_k).  Bar: per event (node, GPU mask, score, feasible count, status) and the final state equal the
oracle's, the reports equal its exact sums.  Every run asserts the kernel and the width it ran at: a grid the device
cannot hold is narrowed silently (replay_narrow), and a narrower run would test another exchange.

Every test needs a gfx950 device; a run is skipped only on a device with fewer CUs than workgroups it asks for.
"""
import pytest

import ksim
import ksim.shard as SH
import pyoracle as O
from fuzz_cases import make_case
from test_gpu_fuzz import REPORT_KEYS, check_state
from test_gpu_parity import POLICIES
from test_gpu_report import assert_reports

pytestmark = pytest.mark.gpu

WIDTHS = [65, 128, 129, 193, 256]
# (seed, nodes, creations, delete probability): cases 3 and 6 of tests/test_gpu_fuzz.py
CASE_DEL, CASE_LEAN = (3, 250, 1200, 0.1), (6, 600, 2000, 0.0)
CASES = [CASE_DEL, CASE_LEAN]
CASE_IDS = ["s%d-n%d-e%d-d%g" % c for c in CASES]
CHEAP = POLICIES[1:]

_CASES, _PWR_CASES, _TRACE = {}, {}, []


@pytest.fixture(autouse=True)
def whole_device(monkeypatch):
    # KSIM_CUS caps the co-resident grid (choose_wgs would answer K = 1 or a narrower K); no test knob left over
    monkeypatch.delenv("KSIM_CUS", raising=False)
    monkeypatch.delenv("KSIM_TEST", raising=False)


def get_case(params):
    if params not in _CASES:
        _CASES[params] = make_case(*params)
    return _CASES[params]


def widths(n):
    return sorted({min(w, n) for w in WIDTHS})


def need_cus(workgroups):
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if cus < workgroups:
        pytest.skip("the device has %d CUs, the run asks for %d co-resident workgroups" % (cus, workgroups))


def oracle(case, pol, sel, report=False, **kw):
    # (pyoracle keeps the replays of this process: one oracle run per (case, policy), whichever test asks first)
    return O.run_events(case["onodes"], case["otypical"], case["oevents"], policy=pol, gpu_sel=sel, threads=16,
                        with_report=report, **kw)


def assert_events(got, want, label):
    bad = [i for i, (a, b) in enumerate(zip(got, want)) if a != b]
    assert len(got) == len(want) and not bad, \
        "%s: first mismatch at event %d: gpu %s oracle %s" % (label, bad[0], got[bad[0]], want[bad[0]])


def assert_content(want, errors=False):
    """The oracle's own stream holds what a wrong fold would get wrong (a later change of fuzz_cases.py must not
    empty the test): an event no node can host, one with exactly one feasible node, and for BestFit a Score error."""
    assert any(r[4] == ksim.UNSCHEDULABLE for r in want)
    assert any(r[3] == 1 and r[4] != ksim.DELETED for r in want)
    if errors:
        assert any(r[4] == ksim.ERROR for r in want)


def run_wide(cases, policy, wgs, seed=5, run_mode=2, report=False, power_model=None, want_wgs=None):
    """One engine, one replica per case (the same node count), at `wgs` workgroups per replica on k_replay.
    -> per replica (results, final nodes, reports or None, power reports or None)"""
    n = len(cases[0]["onodes"])
    need_cus(len(cases) * wgs if want_wgs is None else len(cases) * want_wgs)
    eng = ksim.Engine(n, len(cases), run_mode=run_mode, wgs_per_replica=wgs)
    try:
        if report:
            eng.set_report(True)
        for r, c in enumerate(cases):
            eng.set_nodes(r, c["nodes"])
            eng.set_typical(r, c["typical"], c["typical_n"])
            eng.set_policy(r, policy, seed=seed)
            if power_model is not None:
                eng.set_power_model(r, power_model)
            eng.load_events(r, c["events"], c["n_events"])
        eng.run()
        assert eng.last_run_path() == "k_replay"
        assert eng.last_run_wgs() == (wgs if want_wgs is None else want_wgs)
        return [(eng.results(r), eng.nodes(r), eng.reports(r) if report else None,
                 eng.power_reports(r) if report and power_model is not None else None) for r in range(len(cases))]
    finally:
        eng.close()


# ---- a. every policy, both instantiations, every width ----
@pytest.mark.parametrize("params", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("name,pol,sel", POLICIES, ids=[p[0] for p in POLICIES])
def test_wide_all_policies_vs_oracle(params, name, pol, sel):
    case = get_case(params)
    want, want_state, _ = oracle(case, pol, sel, seed=5)
    assert_content(want, errors=name == "BestFit")
    for w in widths(params[1]):
        (got, state, _, _), = run_wide([case], name, w)
        assert_events(got, want, "%s K=%d" % (name, w))
        check_state(state, want_state)


# ---- every column of 129 holds nodes: 258 nodes, two per slice, the third column's one lane holds nodes 256, 257 ----
# (cases 3 and 6 leave column 128 of the 129-wide runs empty: their slices are cut for 125 and 120 workgroups)
CASE_258 = (8, 258, 1000, 0.1)


@pytest.mark.parametrize("name,pol,sel", POLICIES, ids=[p[0] for p in POLICIES])
def test_wide_129_every_column_holds_nodes(name, pol, sel):
    case = get_case(CASE_258)
    want, want_state, _ = oracle(case, pol, sel, seed=5)
    assert_content(want, errors=name == "BestFit")
    assert any(r[4] == ksim.SCHEDULED and r[0] >= 256 for r in want)  # the last column's slice wins an event
    for w in (129, 193):
        (got, state, _, _), = run_wide([case], name, w)
        assert_events(got, want, "%s K=%d" % (name, w))
        check_state(state, want_state)


# ---- BestFit's "scores differ" bit 17 alone: the one slice whose scores differ sits past column 63 ----
def odd_node_case(n, odd):
    """n nodes alike but node `odd` (more CPU and memory: a lower BestFit score), and three pods alike.  For the
    first pod every slice's best raw score is the same, and only the slice of `odd` holds two scores: NormalizeScore's
    hi > lo (the winner's 100 instead of 0, plugin_utils.go:48-74) hangs on that slice's bit 17 alone."""
    nodes, onodes = (ksim.Node * n)(), []
    for i in range(n):
        cpu, mem = (96000, 262144) if i == odd else (32000, 65536)
        nd = nodes[i]
        nd.cpu_alloc_milli, nd.mem_alloc_mib, nd.pods_alloc = cpu, mem, 110
        nd.gpu_count, nd.gpu_type, nd.name_rank = 4, 1, i
        onodes.append(dict(name="%04d-node-%d" % (i, i), cpu=cpu, mem=mem, pods=110, gpu=4, model="T4"))
    pods = [(4000, 2048, 500, 1, "")] * 3
    evs = [ksim.make_pod(c, milli, num, m, ksim.KSIM_TYPE_ANY, cpu_nz=c) for c, m, milli, num, _ in pods]
    oev = [dict(cpu=c, cpu_nz=c, mem=m, milli=milli, num=num, type="") for c, m, milli, num, _ in pods]
    otyp = O.get_typical_pods([(c, milli, num, s) for c, _, milli, num, s in pods])
    typ = (ksim.Typical * len(otyp))()
    for i, (cpu, milli, num, _, freq) in enumerate(otyp):
        typ[i].cpu_milli, typ[i].gpu_milli, typ[i].gpu_count = cpu, milli, num
        typ[i].type_mask, typ[i].freq = ksim.KSIM_TYPE_ANY, freq
    return dict(nodes=nodes, events=(ksim.Pod * len(evs))(*evs), n_events=len(evs), typical=typ, typical_n=len(otyp),
                onodes=onodes, oevents=oev, otypical=otyp)


@pytest.mark.parametrize("odd", [257, 200, 130, -1], ids=["last", "node200", "node130", "none"])
def test_wide_bestfit_differing_score_in_one_high_slice(odd):
    case = odd_node_case(258, odd)
    want, want_state, _ = oracle(case, O.POL_BESTFIT, O.SEL_BEST, seed=5)
    # the oracle's own first event: 258 feasible nodes, normalised to 100 only where the odd node exists
    assert want[0][3:] == (258, ksim.SCHEDULED) and want[0][2] == (100000 if odd >= 0 else 0)
    # node 257's slice is column 64 of 65, 85 of 128 and 128 of the wider runs (a polling lane's second and third
    # column); nodes 200 and 130 sit in the second column from 128 and 129 workgroups on
    for w in widths(258):
        (got, state, _, _), = run_wide([case], "BestFit", w)
        assert_events(got, want, "odd node %d K=%d" % (odd, w))
        check_state(state, want_state)


# ---- b. the cluster report's stores (snap / prev): the general instantiation, with and without deletions ----
@pytest.mark.parametrize("params", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("name,pol,sel", POLICIES[:2] + POLICIES[4:5], ids=["FGD", "BestFit", "GpuClustering"])
def test_wide_cluster_report(params, name, pol, sel):
    case = get_case(params)
    want_res, _, want = oracle(case, pol, sel, report=True, seed=5)
    for w in (129, min(256, params[1])):
        (res, _, got, _), = run_wide([case], name, w, report=True)
        assert_events(res, want_res, "%s K=%d" % (name, w))
        assert len(got) == len(want)
        for i, (g, x) in enumerate(zip(got, want)):
            assert g["frag_bins"] == x["frag_bins_exact"], (w, i)
            assert [g[k] for k in REPORT_KEYS] == [x[k] for k in REPORT_KEYS], (w, i)


# ---- c. PWR and PWR + FGD: pf_collect and pf_miss_round over four columns per lane ----
# On the openb model vocabulary, so that the reference's energy tables (const.go:41-124) apply.  The cluster with
# deletions is seed 33: the oracle's run of its 1796 events (296 deletions) has 193 / 192 / 168 unschedulable events
# and 43 / 40 / 50 with exactly one feasible node under "PWR" / "PWR 500 FGD 500" / "PWR 100 FGD 900"; the
# create-only one (tests/test_gpu_fuzz.py's) 101 / 104 / 76 and 15 / 13 / 20.
PWR_LEAN, PWR_DEL = (32, 300, 1200, 0.0), (33, 280, 1500, 0.2)
PWR_CASES = [PWR_LEAN, PWR_DEL]
PWR_IDS = ["s%d-n%d-e%d-d%g" % c for c in PWR_CASES]
PWR_POLICIES = ["PWR", "PWR 500 FGD 500", "PWR 100 FGD 900"]
PWR_WIDTHS = [65, 129, 256]


def openb():
    if not _TRACE:
        _TRACE.append(ksim.Trace.openb("default"))
    return _TRACE[0]


def pwr_case(params):
    if params not in _PWR_CASES:
        _PWR_CASES[params] = make_case(*params, models=openb().type_names())
    return _PWR_CASES[params]


def pwr_oracle(case, policy, report=False):
    name, w = ksim.parse_policy(policy)
    pol, sel = (O.POL_PWR, O.SEL_PWR) if name == "PWR" and not w else (O.POL_PWR_FGD, O.SEL_FGD)
    w_pwr, w_fgd = w if w else (0, 0)
    return oracle(case, pol, sel, report=report, w_pwr=w_pwr, w_fgd=w_fgd)


@pytest.mark.parametrize("params", PWR_CASES, ids=PWR_IDS)
@pytest.mark.parametrize("policy", PWR_POLICIES)
def test_wide_pwr_vs_oracle(params, policy):
    case = pwr_case(params)
    want, want_state, _ = pwr_oracle(case, policy)
    assert_content(want)
    for w in sorted({min(k, params[1]) for k in PWR_WIDTHS}):
        (got, state, _, _), = run_wide([case], policy, w, seed=0, run_mode=0, power_model=openb().power_model())
        assert_events(got, want, "%s K=%d" % (policy, w))
        check_state(state, want_state)


# 258 nodes: two per slice at 129 workgroups and more, so the third column's one lane holds nodes (the 300- and
# 280-node clusters, three per slice, leave every column past 99 and 93 of the 129-wide run empty)
PWR_258 = (34, 258, 1100, 0.2)


@pytest.mark.parametrize("params", PWR_CASES + [PWR_258], ids=PWR_IDS + ["s%d-n%d-e%d-d%g" % PWR_258])
@pytest.mark.parametrize("knob", ["pf_guess=0", "pf_memo_ver0=%d" % (0x3fff - 3)], ids=["no-guess", "version-wrap"])
def test_wide_pwr_fgd_miss_round_and_version_wrap(monkeypatch, params, knob):
    # pf_guess=0: no class ever has a guessed NormalizeScore range, so every step with two or more feasible nodes
    # goes through pf_miss_round (three columns at 129 workgroups, one lane in the last); pf_memo_ver0: the slots'
    # memo versions start three changes before their 14-bit field wraps
    monkeypatch.setenv("KSIM_TEST", knob)
    case = pwr_case(params)
    want, want_state, _ = pwr_oracle(case, "PWR 500 FGD 500")
    assert_content(want)
    if params == PWR_258:
        assert any(r[4] == ksim.SCHEDULED and r[0] >= 256 for r in want)  # the last column's slice wins an event
    for w in (129, 256):
        (got, state, _, _), = run_wide([case], "PWR 500 FGD 500", w, seed=0, run_mode=0,
                                       power_model=openb().power_model())
        assert_events(got, want, "%s K=%d" % (knob, w))
        check_state(state, want_state)


@pytest.mark.parametrize("policy", PWR_POLICIES)
def test_wide_pwr_report(policy):
    # the cluster report and the [Power] report behind a wide general launch with deletions
    case = pwr_case(PWR_DEL)
    want_res, _, want = pwr_oracle(case, policy, report=True)
    (res, _, got, power), = run_wide([case], policy, 129, seed=0, run_mode=0, report=True,
                                     power_model=openb().power_model())
    assert_events(res, want_res, policy)
    for r, p in zip(got, power):
        r["power"] = p
    assert_reports(got, want)


# ---- d. several replicas in one wide launch: the granule base (blockIdx.x / Kx) * 2 * Kx * kGranW, Kx > 64 ----
@pytest.mark.parametrize("name,count,wgs,pdel", [("BestFit", 2, 128, 0.0), ("GpuPacking", 3, 85, 0.0),
                                                 ("GpuClustering", 3, 85, 0.2), ("FGD", 3, 85, 0.2)],
                         ids=["BestFit-2x128", "GpuPacking-3x85", "GpuClustering-3x85-deletes", "FGD-3x85-deletes"])
def test_wide_multi_replica(name, count, wgs, pdel):
    # each replica its own cluster and a ragged stream length, each against its own oracle run
    pol, sel = next((p, s) for n, p, s in POLICIES if n == name)
    cases = [get_case((20 + r, 300, 400 + 200 * r, pdel)) for r in range(count)]
    runs = run_wide(cases, name, wgs)
    for r, (c, (got, state, _, _)) in enumerate(zip(cases, runs)):
        want, want_state, _ = oracle(c, pol, sel, seed=5)
        assert any(x[4] == ksim.UNSCHEDULABLE for x in want)
        assert pdel == 0.0 or any(x[4] == ksim.DELETED and x[0] >= 0 for x in want)
        assert_events(got, want, "%s replica %d" % (name, r))
        check_state(state, want_state)


# ---- e. widths the engine does not grant ----
def test_wide_request_above_the_limit_runs_at_256():
    case = get_case(CASE_LEAN)
    want, want_state, _ = oracle(case, O.POL_BESTFIT, O.SEL_BEST, seed=5)
    (got, state, _, _), = run_wide([case], "BestFit", 300, want_wgs=256)
    assert_events(got, want, "BestFit K=300")
    check_state(state, want_state)


def test_wide_request_the_device_cannot_hold_runs_at_one():
    # choose_wgs: R * K workgroups must be co-resident; two replicas at 200 are more than the device's CUs, and the
    # run takes one workgroup per replica (streams with deletions: k_replay itself, not k_scan1)
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    cases = [get_case((20 + r, 300, 400 + 200 * r, 0.2)) for r in range(2)]
    runs = run_wide(cases, "BestFit", 200, want_wgs=200 if 400 <= cus else 1)
    for r, (c, (got, state, _, _)) in enumerate(zip(cases, runs)):
        want, want_state, _ = oracle(c, O.POL_BESTFIT, O.SEL_BEST, seed=5)
        assert_events(got, want, "replica %d" % r)
        check_state(state, want_state)


# ---- the node-sharded group (run_replay_group): one exchange over world x K columns, past 64 ----
# KSIM_TEST=group_k sets the slices per shard (replay_group_slices picks one per 384 nodes otherwise).  Case 6 over
# 2 x 33 = 66, 3 x 43 = 129, 5 x 51 = 255 and 2 x 128 = 256 columns.
GROUPS = [(2, 33), (3, 43), (5, 51), (2, 128)]
GROUP_IDS = ["w%d-k%d" % g for g in GROUPS]


def run_group(monkeypatch, case, name, world, group_k, report=False):
    need_cus(world * group_k)
    monkeypatch.setenv("KSIM_TEST", "group_k=%d" % group_k)
    kw = {}
    if report:
        from test_gpu_shard_report import power_model
        kw = dict(report=True, power_model=power_model())
    g = SH.ShardGroup(case["nodes"], (case["typical"], case["typical_n"]), world, policy=name, seed=5, **kw)
    try:
        g.load_events(case["events"], case["n_events"])
        g.run()
        assert g.engines[0].last_run_kernels() == ["k_replay_group"]
        assert g.engines[0].last_run_wgs() == group_k
        return g.results(), (g.reports() if report else None), (g.power_reports() if report else None)
    finally:
        g.close()


@pytest.mark.parametrize("world,group_k", GROUPS, ids=GROUP_IDS)
@pytest.mark.parametrize("name,pol,sel", CHEAP, ids=[p[0] for p in CHEAP])
def test_wide_sharded_group_vs_oracle(monkeypatch, world, group_k, name, pol, sel):
    case = get_case(CASE_LEAN)
    want, _, _ = oracle(case, pol, sel, seed=5)
    got, _, _ = run_group(monkeypatch, case, name, world, group_k)
    assert_events(got, want, "%s %d x %d" % (name, world, group_k))


@pytest.mark.parametrize("world,group_k", [GROUPS[1], GROUPS[3]], ids=[GROUP_IDS[1], GROUP_IDS[3]])
@pytest.mark.parametrize("name,pol,sel", [POLICIES[1], POLICIES[4]], ids=["BestFit", "GpuClustering"])
def test_wide_sharded_group_report(monkeypatch, world, group_k, name, pol, sel):
    # the group's general instantiation (the report stores) at more than 64 columns; the shards' exact records merged
    from test_gpu_shard_report import with_power
    case = get_case(CASE_LEAN)
    want_res, _, want = oracle(case, pol, sel, report=True, seed=5)
    got, reports, power = run_group(monkeypatch, case, name, world, group_k, report=True)
    assert_events(got, want_res, "%s %d x %d" % (name, world, group_k))
    assert_reports(with_power(reports, power), want)
