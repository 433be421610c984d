"""The per-event cluster report of a node-sharded cluster (analysis.go:59-119, 24-56), merged exactly.

Every shard reports the nodes it owns -- an event's node term where it owns the changed node, the arrived milli on
shard 0 -- and the shards' exact records (128-bit fixed point and counters) are added as integers: on the device for an
in-process group (k_report_merge, ShardGroup.reports), on the host between processes (ksim_report_merge,
ksim.shard.merge_reports).  Bar: for every event the merged report equals the oracle's exact-sum report bit for bit
(tests/test_gpu_report.py's assert_reports: the 7 bins, every counter, total GPUs, the power terms), whatever the
number of shards and whichever kernels replayed the events, and the two merges give the same records.

The clusters are tests/fuzz_cases.py's: every shard binds, every shard undoes binds in the cases with deletions, each
case has creates no node can host, and the 7-node case gives shards of one or two nodes.  Every test needs a gfx950
device, and resolves the entry points it uses before it creates an engine.
"""
import pytest

import ksim
import ksim.shard as SH
import pyoracle as O
from fuzz_cases import MODELS, make_case
from test_gpu_report import assert_reports

pytestmark = pytest.mark.gpu

# (seed, nodes, creations, delete probability)
CASES = [(2, 97, 900, 0.25), (3, 250, 1200, 0.1), (4, 7, 300, 0.4), (1, 40, 500, 0.0)]
CREATE_ONLY = (1, 40, 500, 0.0)
POLICIES = [("FGD", O.POL_FGD, O.SEL_FGD), ("BestFit", O.POL_BESTFIT, O.SEL_BEST),
            ("GpuClustering", O.POL_CLUSTERING, O.SEL_BEST)]
WORLDS = [1, 2, 3, 5, 7]


def need_api():
    """The entry points of this feature, resolved before any engine exists."""
    return SH.merge_reports, ksim.Engine.report_parts, SH.ShardGroup.reports, SH.ShardGroup.power_reports


_CASES, _RUNS, _PM = {}, {}, []


def get_case(params):
    if params not in _CASES:
        _CASES[params] = make_case(*params)
    return _CASES[params]


def power_model():
    """The reference's energy tables (const.go:41-124) in the fuzz clusters' model vocabulary."""
    if not _PM:
        t = ksim.Trace.openb("default")
        src, names = t.power_model(), t.type_names()
        pm = ksim.PowerModel()
        for i in range(ksim.MAX_CPU_MODELS):
            pm.cpu_idle_w[i], pm.cpu_full_w[i], pm.cpu_cores[i] = src.cpu_idle_w[i], src.cpu_full_w[i], src.cpu_cores[i]
        pm.cpu_valid = src.cpu_valid
        for i, m in enumerate(MODELS):
            j = names.index(m)
            pm.gpu_idle_w[i], pm.gpu_full_w[i] = src.gpu_idle_w[j], src.gpu_full_w[j]
            pm.gpu_valid |= 1 << i
        _PM.append(pm)
    return _PM[0]


def oracle(params, pol, sel):
    c = get_case(params)
    want_res, _, want = O.run_events(c["onodes"], c["otypical"], c["oevents"], policy=pol, gpu_sel=sel, seed=5,
                                     threads=16, with_report=True)
    return want_res, want


def with_power(reports, power):
    out = [dict(r) for r in reports]
    for r, p in zip(out, power):
        r["power"] = p
    return out


def run_group(params, name, world, variant=""):
    """One group run (kept for the tests that look at it from different sides): results, the device merge, the
    shards' parts, the kernels and the report time."""
    key = (params, name, world, variant)
    if key not in _RUNS:
        need_api()
        c = get_case(params)
        g = SH.ShardGroup(c["nodes"], (c["typical"], c["typical_n"]), world, policy=name, seed=5, report=True,
                          power_model=power_model())
        try:
            g.load_events(c["events"], c["n_events"])
            g.run()
            _RUNS[key] = dict(results=g.results(), reports=g.reports(), power=g.power_reports(),
                              parts=[bytes(p) for p in g.report_parts()], kernels=g.engines[0].last_run_kernels(),
                              report_ms=[e.last_report_ms() for e in g.engines])
        finally:
            g.close()
    return _RUNS[key]


def worlds_of(params):
    return [w for w in WORLDS if w <= params[1]]  # (no shard without a node)


GROUPS = [(p, w) for p in CASES for w in worlds_of(p)]
GROUP_IDS = ["s%d-n%d-e%d-d%g-w%d" % (p + (w,)) for p, w in GROUPS]


@pytest.mark.parametrize("params,world", GROUPS, ids=GROUP_IDS)
@pytest.mark.parametrize("name,pol,sel", POLICIES, ids=[p[0] for p in POLICIES])
def test_group_report_equals_oracle(params, world, name, pol, sel):
    need_api()
    want_res, want = oracle(params, pol, sel)
    run = run_group(params, name, world)
    assert run["results"] == want_res
    assert_reports(with_power(run["reports"], run["power"]), want)


@pytest.mark.parametrize("params,world", GROUPS, ids=GROUP_IDS)
@pytest.mark.parametrize("name,pol,sel", POLICIES, ids=[p[0] for p in POLICIES])
def test_host_merge_equals_device_merge(params, world, name, pol, sel):
    need_api()
    run = run_group(params, name, world)
    assert len(run["parts"]) == world
    reports, power = SH.merge_reports(run["parts"])
    assert reports == run["reports"]
    assert power == run["power"]


@pytest.mark.parametrize("world", [2, 3, 5, 7])
@pytest.mark.parametrize("name,pol,sel", POLICIES, ids=[p[0] for p in POLICIES])
def test_report_runs_on_the_persistent_group_launch(world, name, pol, sel):
    # create-only: the FGD group on k_hmemo's slices, the cheap policies' on k_replay's (its general instantiation,
    # which has the report stores), one launch for the group, the report kernels and the merge behind it
    need_api()
    run = run_group(CREATE_ONLY, name, world)
    assert run["kernels"] == (["k_hmemo_group"] if name == "FGD" else ["k_replay_group"]), run["kernels"]
    assert all(ms > 0 for ms in run["report_ms"]) and len(set(run["report_ms"])) == 1


@pytest.mark.parametrize("name,pol,sel,variant", [POLICIES[0] + ("shard_hmemo=0",), POLICIES[1] + ("shard_replay=0",)],
                         ids=["FGD-step", "BestFit-step"])
@pytest.mark.parametrize("params", [CASES[0], CREATE_ONLY], ids=["deletes", "create-only"])
def test_step_path_report_equals_oracle(monkeypatch, params, name, pol, sel, variant):
    # the per-pod k_step + gather + commit path of a group: each shard's delta takes the node term of its own nodes
    # only (results carry global ranks), and no snapshot is read where another shard bound
    need_api()
    monkeypatch.setenv("KSIM_VARIANT", variant)
    want_res, want = oracle(params, pol, sel)
    run = run_group(params, name, 2, variant)
    assert run["kernels"] == ["k_step"]
    assert run["results"] == want_res
    assert_reports(with_power(run["reports"], run["power"]), want)
    assert SH.merge_reports(run["parts"]) == (run["reports"], run["power"])


def test_empty_event_stream():
    need_api()
    c = make_case(7, 30, 0)
    g = SH.ShardGroup(c["nodes"], (c["typical"], c["typical_n"]), 3, report=True, power_model=power_model())
    try:
        g.load_events(c["events"], 0)
        g.run()
        assert g.results() == []
        assert g.reports() == [] and g.power_reports() == []
        assert SH.merge_reports(g.report_parts()) == ([], [])
    finally:
        g.close()


def test_unsharded_engine_parts_merge_to_its_reports():
    need_api()
    c = get_case(CASES[0])
    e = ksim.Engine(len(c["onodes"]), 1)
    try:
        e.set_nodes(0, c["nodes"])
        e.set_typical(0, c["typical"], c["typical_n"])
        e.set_policy(0, "FGD", seed=5)
        e.set_power_model(0, power_model())
        e.set_report(True)
        e.load_events(0, c["events"], c["n_events"])
        with pytest.raises(ksim.KsimError) as ei:  # no run yet
            e.report_parts(0)
        assert ei.value.code == ksim.KSIM_ESTATE
        e.run()
        assert SH.merge_reports([e.report_parts(0)]) == (e.reports(0), e.power_reports(0))
        _, want = oracle(CASES[0], O.POL_FGD, O.SEL_FGD)
        assert_reports(with_power(e.reports(0), e.power_reports(0)), want)
    finally:
        e.close()


def test_shard_refuses_rounded_partial_reports():
    # a shard's own reports would be a rounded partial sum: the exact parts are the way (KSIM_ENOTSUP); a group
    # that has not run has no merged report (KSIM_ESTATE)
    need_api()
    c = get_case(CASES[2])
    g = SH.ShardGroup(c["nodes"], (c["typical"], c["typical_n"]), 2, report=True, power_model=power_model())
    try:
        g.load_events(c["events"], c["n_events"])
        for call in (g.engines[0].reports, g.engines[1].reports, g.engines[0].power_reports):
            with pytest.raises(ksim.KsimError) as ei:
                call(0)
            assert ei.value.code == ksim.KSIM_ENOTSUP
        with pytest.raises(ksim.KsimError) as ei:
            g.reports()
        assert ei.value.code == ksim.KSIM_ESTATE
    finally:
        g.close()


@pytest.mark.parametrize("exchange", ["rccl", "host"])
def test_process_exchanges_world1_report(exchange):
    # the per-pod k_step path of a shard process (ksim_engine_run: ncclAllGather, or the caller's host exchange) at a
    # world of one: its report through the parts and the host merge, against the oracle
    need_api()
    params = CASES[0]
    c = get_case(params)
    want_res, want = oracle(params, O.POL_FGD, O.SEL_FGD)
    parts = SH.partition(c["nodes"], 1)
    e = ksim.Engine(len(c["onodes"]), 1)
    try:
        e.set_shard(0, 1, 0, len(c["onodes"]), ksim.shard_comm_id() if exchange == "rccl" else None)
        if exchange == "host":
            e.set_shard_exchange(lambda rec: list(rec))
        e.set_nodes(0, parts[0][1])
        e.set_typical(0, c["typical"], c["typical_n"])
        e.set_policy(0, "FGD", seed=5)
        e.set_power_model(0, power_model())
        e.set_report(True)
        e.load_events(0, c["events"], c["n_events"])
        e.run()
        assert e.last_run_kernels() == ["k_step"]
        assert SH.merge_results([e.results(0)], parts) == want_res
        reports, power = SH.merge_reports([bytes(e.report_parts(0))])
    finally:
        e.close()
    assert_reports(with_power(reports, power), want)


def _device_rank_main(rank, world, port, n_create, q):
    import os
    import torch.distributed as dist
    import helpers
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    t = ksim.Trace.openb("default")
    rp = t.replay(seed=7)
    nodes = helpers.subset_nodes(rp, list(range(1, t.num_nodes, 5)))
    events, _ = helpers.delete_stream(t, rp, n_create, p_delete=0.2, seed=4)
    merged, ms, reports = SH.run_distributed(nodes, t.typical(), events, len(events), dist, policy="FGD", seed=3,
                                             exchange="device", report=True, power_model=t.power_model())
    q.put((rank, merged, reports, ms))
    dist.destroy_process_group()


@pytest.mark.timeout(150)
def test_device_exchange_two_processes_report():
    # two shard processes on the one GPU (k_hmemo slices exchanging granules through IPC-mapped buffers), each
    # reporting its own nodes behind its replay; the ranks gather the exact parts and merge them on the host
    need_api()
    import inspect
    assert "report" in inspect.signature(SH.run_distributed).parameters
    import multiprocessing as mp
    import socket
    import helpers
    n_create = 300
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_device_rank_main, args=(r, 2, port, n_create, q)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        res = sorted((q.get(timeout=100) for _ in procs), key=lambda x: x[0])
    finally:
        for p in procs:
            if p.is_alive():
                p.join(20)
            if p.is_alive():
                p.kill()
    for p in procs:
        p.join(30)
        assert p.exitcode == 0
    t = ksim.Trace.openb("default")
    rp = t.replay(seed=7)
    keep = list(range(1, t.num_nodes, 5))
    _, oev = helpers.delete_stream(t, rp, n_create, p_delete=0.2, seed=4)
    want_res, _, want = O.run_events(helpers.oracle_subset(t, rp, keep), helpers.oracle_typical(t), oev,
                                     policy=O.POL_FGD, gpu_sel=O.SEL_FGD, seed=3, threads=16, with_report=True)
    assert any(r[4] == ksim.DELETED and r[0] >= 0 for r in want_res)
    for rank, merged, reports, _ in res:
        assert merged == want_res, rank
        assert_reports(reports, want)
