"""PWR and PWR+FGD on a node-sharded cluster (DESIGN.md "PWR on shards"): every event (node, GPU mask, score,
feasible count, status) and the final node records equal the oracle's on the unsharded cluster, bit for bit.

PWRScorePlugin.NormalizeScore (pwr_score.go:104-141) needs the min / max raw score over the feasible nodes of the
whole cluster.  On the per-pod path a sharded PWR cycle takes two exchange rounds per created pod: the shards' raw
ranges (k_step), then their best keys under the cluster's range (k_step_pwr), and k_shard_commit finishes as for
every policy.  A create-only in-process group runs on the persistent group launch (k_replay_group), whose granule
exchange spans every shard's columns.  The tests cover the in-process group on both paths, the wide exchange, the
RCCL and the host exchange of one engine, two shard processes over gloo, the reports, a descheduling plan behind a
PWR run, and the refusals.

The clusters are tests/fuzz_cases.py's on the openb model vocabulary (so that the reference's energy tables apply,
as tests/test_gpu_fuzz.py::test_fuzz_pwr builds them) and two hand-built ones.  Every test needs a gfx950 device.
"""
import pytest

import desched_ref as ref
import ksim
import ksim.shard as SH
import pyoracle as O
from fuzz_cases import make_case
from test_gpu_fuzz import check_state
from test_gpu_report import assert_reports

pytestmark = pytest.mark.gpu

# (seed, nodes, creations, delete probability)
CASES = [(31, 60, 700, 0.2), (32, 300, 1200, 0.0), (4, 7, 300, 0.4), (5, 1, 60, 0.3)]
CREATE_ONLY = (32, 300, 1200, 0.0)
WORLDS = [1, 2, 3, 5, 7]
POLICIES = ["PWR", "PWR 500 FGD 500", "PWR 100 FGD 900"]
STEP_KERNELS = ["k_step", "k_step_pwr"]
GROUP_KERNELS = ["k_replay_group"]

_TRACE, _CASES, _WANT = [], {}, {}


def trace():
    if not _TRACE:
        _TRACE.append(ksim.Trace.openb("default"))
    return _TRACE[0]


def get_case(params):
    if params not in _CASES:
        _CASES[params] = make_case(*params, models=trace().type_names())
    return _CASES[params]


def oracle_policy(policy):
    name, w = ksim.parse_policy(policy)
    pol, sel = (O.POL_PWR, O.SEL_PWR) if name == "PWR" and not w else (O.POL_PWR_FGD, O.SEL_FGD)
    return dict(policy=pol, gpu_sel=sel, w_pwr=w[0] if w else 0, w_fgd=w[1] if w else 0)


def oracle_case(case, policy, n_events=None, with_report=False):
    oev = case["oevents"] if n_events is None else case["oevents"][:n_events]
    return O.run_events(case["onodes"], case["otypical"], oev, threads=16, with_report=with_report,
                        **oracle_policy(policy))


def oracle(params, policy):
    """(results, final state, reports) of the oracle on the unsharded cluster, once per (case, policy)."""
    if (params, policy) not in _WANT:
        _WANT[params, policy] = oracle_case(get_case(params), policy, with_report=True)
    return _WANT[params, policy]


def make_group(case, policy, world, report=False, power=True, pm=None):
    pm = pm if pm is not None else (trace().power_model() if power else None)
    return SH.ShardGroup(case["nodes"], (case["typical"], case["typical_n"]), world, policy=policy, report=report,
                         power_model=pm)


def group_kernels(params, world, policy):
    """The path of an in-process group: a create-only stream takes the persistent group launch (a world of one has
    a single column and no exchange to span), a stream with deletions the per-pod path (DESIGN.md "PWR on shards")."""
    return GROUP_KERNELS if params[3] == 0 and world >= 2 else STEP_KERNELS


def group_state(g):
    """The final node records by input index, gathered per shard in rank order."""
    state = {}
    for e, (_, _, idx) in zip(g.engines, g.parts):
        local = e.nodes(0)
        for j, i in enumerate(idx):
            state[i] = local[j]
    return state


def assert_events(got, want):
    bad = [i for i, (a, b) in enumerate(zip(got, want)) if a != b]
    assert len(got) == len(want) and not bad, "first mismatch at %d: %s vs %s" % (bad[0], got[bad[0]], want[bad[0]])


# ---- in-process groups on the fuzz clusters ----

@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("params", CASES, ids=["s%d-n%d-e%d-d%g" % c for c in CASES])
def test_group_equals_oracle(params, world, policy):
    if params[1] < world:
        pytest.skip("fewer nodes than shards")
    case = get_case(params)
    want, want_state, _ = oracle(params, policy)
    g = make_group(case, policy, world)
    try:
        g.load_events(case["events"], case["n_events"])
        g.run()
        got, state = g.results(), group_state(g)
        kernels = [e.last_run_kernels() for e in g.engines]
    finally:
        g.close()
    assert kernels == [group_kernels(params, world, policy)] * world, kernels
    assert_events(got, want)
    check_state(state, want_state)
    if params[3] > 0 and params[1] > 1:
        assert any(r[4] == ksim.DELETED and r[0] >= 0 for r in got)


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("world", [2, 5])
def test_create_only_on_the_step_path(monkeypatch, world, policy):
    # KSIM_VARIANT=shard_replay=0 keeps a create-only group on the per-pod path: its two rounds per pod
    monkeypatch.setenv("KSIM_VARIANT", "shard_replay=0")
    case = get_case(CREATE_ONLY)
    want, want_state, _ = oracle(CREATE_ONLY, policy)
    g = make_group(case, policy, world)
    try:
        g.load_events(case["events"], case["n_events"])
        g.run()
        got, state, kernels = g.results(), group_state(g), g.engines[0].last_run_kernels()
    finally:
        g.close()
    assert kernels == STEP_KERNELS
    assert_events(got, want)
    check_state(state, want_state)


# ---- the persistent group launch: the wide exchange ----

@pytest.mark.parametrize("policy,knob", [("PWR", ""), ("PWR 500 FGD 500", ""), ("PWR 500 FGD 500", ",pf_guess=0")],
                         ids=["PWR", "PWR+FGD", "PWR+FGD-miss-round"])
@pytest.mark.parametrize("world,group_k", [(2, 3), (3, 22), (16, 16)], ids=["w2-k3", "w3-k22", "w16-k16"])
def test_wide_group_exchange(monkeypatch, world, group_k, policy, knob):
    # KSIM_TEST=group_k: that many slices per shard -- 6 columns, 66 (past 64: four columns per polling lane) and 256.
    # pf_guess=0 (PWR+FGD): no guessed range is ever right, so every step with two feasible nodes re-keys under the
    # cluster's range and takes the miss round across the shards' columns
    from test_gpu_replay_wide import need_cus
    need_cus(world * group_k)
    monkeypatch.delenv("KSIM_CUS", raising=False)
    monkeypatch.setenv("KSIM_TEST", "group_k=%d%s" % (group_k, knob))
    case = get_case(CREATE_ONLY)
    want, want_state, _ = oracle(CREATE_ONLY, policy)
    assert sum(1 for r in want if r[3] > 1) > 100  # steps that need the cluster's range
    g = make_group(case, policy, world)
    try:
        g.load_events(case["events"], case["n_events"])
        g.run()
        got, state = g.results(), group_state(g)
        kernels, wgs = g.engines[0].last_run_kernels(), g.engines[0].last_run_wgs()
    finally:
        g.close()
    assert kernels == GROUP_KERNELS and wgs == group_k
    assert_events(got, want)
    check_state(state, want_state)


@pytest.mark.parametrize("policy", ["PWR", "PWR 500 FGD 500"])
def test_group_launch_key_field_overflow_is_erange(policy):
    # a raw PWR score outside the 24-bit key field (a 1 GW device) ends a group run as it ends an unsharded one
    case = flat_cluster(["T4", "T4"])
    src = trace().power_model()
    pm = ksim.PowerModel.from_buffer_copy(bytes(src))
    pm.gpu_full_w[trace().type_names().index("T4")] = 1e9
    g = make_group(case, policy, 2, pm=pm)
    try:
        g.load_events(case["events"], case["n_events"])
        with pytest.raises(ksim.KsimError) as ei:
            g.run()
    finally:
        g.close()
    assert ei.value.code == ksim.KSIM_ERANGE


# ---- NormalizeScore's lo == hi branch is decided on the cluster's range ----

def flat_cluster(models, per_shard=4):
    """len(models) shards' worth of identical idle 4-GPU nodes, shard k's of GPU model models[k]; names in input
    order, so that partition() gives shard k the k-th run of nodes."""
    names = trace().type_names()
    n = per_shard * len(models)
    nodes = (ksim.Node * n)()
    onodes = []
    for i in range(n):
        m = models[i // per_shard]
        nd = nodes[i]
        nd.cpu_alloc_milli, nd.mem_alloc_mib, nd.pods_alloc = 64000, 262144, 110
        nd.gpu_count, nd.gpu_type, nd.name_rank = 4, names.index(m), i
        onodes.append(dict(name="%04d-flat-%d" % (i, i), cpu=64000, mem=262144, pods=110, gpu=4, model=m))
    pods = [(4000, 2048, 500, 1, "")] * 6 + [(8000, 4096, 1000, 2, "")] * 4
    evs = [ksim.make_pod(c, milli, num, mem, ksim.KSIM_TYPE_ANY, cpu_nz=c) for c, mem, milli, num, _ in pods]
    oev = [dict(cpu=c, cpu_nz=c, mem=mem, milli=milli, num=num, type="") for c, mem, milli, num, _ in pods]
    otyp = O.get_typical_pods([(c, milli, num, s) for c, _, milli, num, s in pods])
    typ = (ksim.Typical * len(otyp))()
    for i, (cpu, milli, num, _, freq) in enumerate(otyp):
        typ[i].cpu_milli, typ[i].gpu_milli, typ[i].gpu_count = cpu, milli, num
        typ[i].type_mask, typ[i].freq = ksim.KSIM_TYPE_ANY, freq
    return dict(nodes=nodes, events=(ksim.Pod * len(evs))(*evs), n_events=len(evs), typical=typ, typical_n=len(otyp),
                onodes=onodes, oevents=oev, otypical=otyp)


def shard_of(case, world, node):
    return next(k for k, (_, _, idx) in enumerate(SH.partition(case["nodes"], world)) if node in idx)


PATHS = [("", GROUP_KERNELS), ("shard_replay=0", STEP_KERNELS)]
PATH_IDS = ["group-launch", "step-path"]


@pytest.mark.parametrize("variant,kernels", PATHS, ids=PATH_IDS)
@pytest.mark.parametrize("policy", POLICIES)
def test_equal_raw_scores_on_every_shard(monkeypatch, policy, variant, kernels):
    monkeypatch.setenv("KSIM_VARIANT", variant)
    # one GPU model on the whole cluster: every feasible raw score of the first pod is the same on every shard,
    # the cluster's lo == hi, every node normalizes to 100
    case = flat_cluster(["T4", "T4"])
    want, want_state, _ = oracle_case(case, policy)
    g = make_group(case, policy, 2)
    try:
        g.load_events(case["events"], case["n_events"])
        g.run()
        got, state = g.results(), group_state(g)
        assert g.engines[0].last_run_kernels() == kernels
    finally:
        g.close()
    assert_events(got, want)
    check_state(state, want_state)


@pytest.mark.parametrize("variant,kernels", PATHS, ids=PATH_IDS)
@pytest.mark.parametrize("policy", ["PWR", "PWR 500 FGD 500"])
def test_equal_raw_scores_within_each_shard_only(monkeypatch, policy, variant, kernels):
    monkeypatch.setenv("KSIM_VARIANT", variant)
    # One GPU model per shard (G3: 50 / 400 W, T4: 10 / 70 W): within a shard every raw score of the first pod is
    # equal (lo == hi: a shard-local range would send every node of BOTH shards to 100), between the shards they
    # differ (the cluster's lo < hi: one shard's nodes get 100, the other's 0).  Under shard-local ranges the two
    # shards tie in PWR, so the winner of the first pod falls where the rest of the key puts it -- the same POSITION
    # in the cluster whichever shard holds which model; under the cluster's range it follows the model.  The oracle
    # check below (CPU) pins that: each shard alone gives the first pod the same score (the tie), and on the whole
    # cluster the winner changes shard when the models swap shards.  So in at least one of the two arrangements a
    # shard-local range picks another node than the cluster's; both are run.
    arrangements = [flat_cluster(["G3", "T4"]), flat_cluster(["T4", "G3"])]
    first_winner_shard = []
    for case in arrangements:
        want, want_state, _ = oracle_case(case, policy)
        alone = []
        for k in range(2):
            sub = dict(case, onodes=case["onodes"][4 * k:4 * k + 4])
            alone.append(oracle_case(sub, policy, n_events=1)[0][0])
        assert alone[0][4] == alone[1][4] == ksim.SCHEDULED and alone[0][2] == alone[1][2], alone  # equal scores: the tie
        assert want[0][4] == ksim.SCHEDULED
        first_winner_shard.append(shard_of(case, 2, want[0][0]))
        g = make_group(case, policy, 2)
        try:
            g.load_events(case["events"], case["n_events"])
            g.run()
            got, state = g.results(), group_state(g)
            assert g.engines[0].last_run_kernels() == kernels
        finally:
            g.close()
        assert_events(got, want)
        check_state(state, want_state)
    assert first_winner_shard[0] != first_winner_shard[1], first_winner_shard  # the winner follows the model


# ---- reports ----

@pytest.mark.parametrize("world", [2, 5])
@pytest.mark.parametrize("policy", ["PWR", "PWR 500 FGD 500"])
@pytest.mark.parametrize("params", [CASES[0], CREATE_ONLY], ids=["deletes", "create-only"])
def test_group_reports_equal_oracle(params, world, policy):
    # (create-only: the group launch's general instantiation, which has the report stores)
    case = get_case(params)
    want_res, _, want = oracle(params, policy)
    g = make_group(case, policy, world, report=True)
    try:
        g.load_events(case["events"], case["n_events"])
        g.run()
        got, reports, power = g.results(), g.reports(), g.power_reports()
        parts = [bytes(p) for p in g.report_parts()]
        kernels = g.engines[0].last_run_kernels()
    finally:
        g.close()
    assert kernels == group_kernels(params, world, policy)
    assert_events(got, want_res)
    merged = [dict(r) for r in reports]
    for r, p in zip(merged, power):
        r["power"] = p
    assert_reports(merged, want)
    assert SH.merge_reports(parts) == (reports, power)  # the host merge of the shards' parts = the device merge


# ---- descheduling behind a PWR group run ----

def test_deschedule_after_a_pwr_group_run():
    params, policy = CASES[0], "PWR 500 FGD 500"
    case = get_case(params)
    res, state, _ = oracle(params, policy)
    victims, budget, _ = ref.plan(case["onodes"], case["otypical"], case["oevents"], res, state, ref.ONE_POD, 0.1)
    g = make_group(case, policy, 3)
    try:
        g.load_events(case["events"], case["n_events"])
        g.run()
        g.deschedule(ref.ONE_POD, 0.1)
        got, got_budget = g.victims()
    finally:
        g.close()
    assert [(v.event, v.node, v.gpu_mask, v.score, v.frag_before, v.frag_after) for v in got] == ref.as_tuples(victims)
    assert got_budget == budget and len(got) > 0


# ---- one engine: the RCCL and the host exchange at a world of one ----

def shard_engine(case, policy, n_events, comm_id=None, gather=None, power=True):
    n = len(case["onodes"])
    parts = SH.partition(case["nodes"], 1)
    e = ksim.Engine(n, 1)
    e.set_shard(0, 1, 0, n, comm_id)
    if gather is not None:
        e.set_shard_exchange(gather)
    e.set_nodes(0, parts[0][1])
    e.set_typical(0, case["typical"], case["typical_n"])
    e.set_policy(0, policy)
    if power:
        e.set_power_model(0, trace().power_model())
    e.load_events(0, case["events"], n_events)
    return e, parts


@pytest.mark.parametrize("policy", ["PWR", "PWR 500 FGD 500"])
def test_rccl_world1(policy):
    # ncclAllGather twice per pod (hipGraph-captured when the capture accepts it), deletes included
    params = CASES[0]
    case = get_case(params)
    want, _, _ = oracle(params, policy)
    e, parts = shard_engine(case, policy, case["n_events"], comm_id=ksim.shard_comm_id())
    try:
        e.run()
        got = SH.merge_results([e.results(0)], parts)
        kernels = e.last_run_kernels()
    finally:
        e.close()
    assert kernels == STEP_KERNELS
    assert_events(got, want)


@pytest.mark.parametrize("policy", ["PWR", "PWR 500 FGD 500"])
def test_host_exchange_world1(policy):
    # the caller's exchange is called once per round: twice for every creation (all of them are scored)
    params = CREATE_ONLY
    case = get_case(params)
    n_ev = 400
    want = oracle(params, policy)[0][:n_ev]
    calls = []

    def gather(rec):
        calls.append(rec)
        return list(rec)
    e, parts = shard_engine(case, policy, n_ev, gather=gather)
    try:
        e.run()
        got = SH.merge_results([e.results(0)], parts)
    finally:
        e.close()
    assert len(calls) == 2 * n_ev
    # round A carries no key, round B the shard's best one
    assert all(calls[2 * i][0] == 0 for i in range(n_ev))
    assert any(calls[2 * i + 1][0] != 0 for i in range(n_ev))
    assert_events(got, want)


def test_host_exchange_deletes_take_one_round():
    params, policy = CASES[0], "PWR 500 FGD 500"
    case = get_case(params)
    want, _, _ = oracle(params, policy)
    calls = []

    def gather(rec):
        calls.append(rec)
        return list(rec)
    e, parts = shard_engine(case, policy, case["n_events"], gather=gather)
    try:
        e.run()
        got = SH.merge_results([e.results(0)], parts)
    finally:
        e.close()
    deletes = sum(1 for ev in case["oevents"] if ev.get("delete"))
    assert deletes > 0 and len(calls) == 2 * (case["n_events"] - deletes) + deletes
    assert_events(got, want)


@pytest.mark.parametrize("bad", ["raise", "size", "foreign"])
def test_host_exchange_bad_second_round_fails(bad):
    case = get_case(CREATE_ONLY)
    calls = []

    def gather(rec):
        calls.append(rec)
        if len(calls) != 2:  # the first pod's round B
            return list(rec)
        if bad == "raise":
            raise RuntimeError("transport down")
        if bad == "size":
            return list(rec) + [0]
        return list(rec[:3]) + [rec[3] ^ 1]  # not this shard's record at its rank
    e, _ = shard_engine(case, "PWR 500 FGD 500", 50, gather=gather)
    try:
        with pytest.raises(ksim.KsimError) as ei:
            e.run()
    finally:
        e.close()
    assert ei.value.code == ksim.KSIM_ESTATE
    assert len(calls) == 2


# ---- two shard processes, host exchange ----

N_EV_PROC = 300


def _host_rank_main(rank, world, port, q):
    import os
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    case = make_case(*CASES[0], models=ksim.Trace.openb("default").type_names())
    merged, ms = SH.run_distributed(case["nodes"], (case["typical"], case["typical_n"]), case["events"], N_EV_PROC, dist,
                                    policy="PWR 500 FGD 500", exchange="host",
                                    power_model=ksim.Trace.openb("default").power_model())
    q.put((rank, merged, ms))
    dist.destroy_process_group()


@pytest.mark.timeout(240)
def test_host_exchange_two_processes():
    # two fresh shard processes on the one GPU, both rounds of every pod over gloo (deletes among the events)
    import multiprocessing as mp
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_host_rank_main, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        res = sorted((q.get(timeout=200) for _ in procs), key=lambda x: x[0])
    finally:
        for p in procs:
            if p.is_alive():
                p.join(20)
            if p.is_alive():
                p.kill()
    for p in procs:
        p.join(30)
        assert p.exitcode == 0
    want = oracle_case(get_case(CASES[0]), "PWR 500 FGD 500", n_events=N_EV_PROC)[0]
    assert any(r[4] == ksim.DELETED for r in want)
    assert_events(res[0][1], want)
    assert_events(res[1][1], want)


# ---- refusals ----

def test_pwr_shard_without_a_power_model():
    case = get_case(CASES[0])
    e, _ = shard_engine(case, "PWR", 20, gather=lambda rec: list(rec), power=False)
    try:
        with pytest.raises(ksim.KsimError) as ei:
            e.run()
    finally:
        e.close()
    assert ei.value.code == ksim.KSIM_ESTATE
    g = make_group(case, "PWR 500 FGD 500", 2, power=False)
    try:
        g.load_events(case["events"], 20)
        with pytest.raises(ksim.KsimError) as ei:
            g.run()
    finally:
        g.close()
    assert ei.value.code == ksim.KSIM_ESTATE


def test_device_exchange_stays_fgd_only():
    # a shard with mapped peers runs k_hmemo's slices: FGD only, whatever power model is set
    case = get_case(CASES[0])
    n = len(case["onodes"])
    parts = SH.partition(case["nodes"], 1)
    e = ksim.Engine(n, 1)
    try:
        e.set_shard(0, 1, 0, n, None)
        e.set_shard_peers([e.shard_peer_handle()])
        e.set_nodes(0, parts[0][1])
        e.set_typical(0, case["typical"], case["typical_n"])
        e.set_policy(0, "PWR 500 FGD 500")
        e.set_power_model(0, trace().power_model())
        e.load_events(0, case["events"], 20)
        with pytest.raises(ksim.KsimError) as ei:
            e.run()
    finally:
        e.close()
    assert ei.value.code == ksim.KSIM_ENOTSUP
