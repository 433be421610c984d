"""Descheduling on a node-sharded cluster: every shard plans the pods on its own nodes, the parts are merged exactly.

Bar: `==` on every field of every victim, doubles included, in eviction order, and on the budget, against
tests/desched_ref.py / tests/desched_cos_ref.py run on the ORACLE's replay of the whole, unsharded cluster
(test_gpu_desched.want_plan, test_gpu_desched_cos.want_plan) -- for the merge on the device (k_victim_merge,
ShardGroup.victims / cos_victims) and for the host merge of the shards' parts (ksim.desched_merge / ksim.cos_merge),
whatever the number of shards and whichever kernels replayed the events.  The group's results equal the oracle's
first, so a planning mismatch is not a replay mismatch in disguise.

The clusters: tests/fuzz_cases.py's (every shard binds; with deletions every shard undoes binds, and the owner's
record of the delete event must read as deleted on every group path; the 7-node case gives shards of one node; on the
create-only case at world 2 one shard has no frag victim under FGD); tests/desched_fuzz_cases.py's flat clusters,
whose priorities tie over a seventh of the nodes under scrambled names, so that neighbouring places of the merged
list come from different shards; and 6145 flat nodes at world 2, one shard's select tables in LDS (3072 nodes) and
the other's in HBM (3073).  Every test needs a gfx950 device, and resolves the entry points it uses before it
creates an engine.
"""
import bisect

import pytest

import desched_cases as cases
import desched_cos_ref as cos
import desched_fuzz_cases as fz
import desched_ref as ref
import ksim
import ksim.desched
import ksim.shard as SH
import pyoracle as O
import test_gpu_desched as frag
import test_gpu_desched_cos as cosm
from test_gpu_desched import oracle_run

pytestmark = pytest.mark.gpu

# (seed, nodes, creations, delete probability)
CASES = [(2, 97, 900, 0.25), (3, 250, 1200, 0.1), (4, 7, 300, 0.4), (1, 40, 500, 0.0)]
CREATE_ONLY = (1, 40, 500, 0.0)
SCHEDS = ["FGD", "BestFit"]
WORLDS = [1, 2, 3, 5, 7]
FRAG = [ref.ONE_POD, ref.MULTI_POD]
FRAG_RATIOS = [0.0, 0.01, 0.1, 1.0]
COS_BARS = [(2000, 500), (2 ** 30, 0)]
COS_RATIOS = [0.05, 1.0]
WIDE = cosm.WIDE


def need_api():
    """The entry points of this feature, resolved before any engine exists."""
    return (ksim.Engine.victim_part, ksim.Engine.cos_victim_part, ksim.desched_merge, ksim.cos_merge,
            SH.ShardGroup.deschedule, SH.ShardGroup.deschedule_cossim, SH.ShardGroup.victims, SH.ShardGroup.cos_victims,
            SH.ShardGroup.victim_parts, ksim.desched.run_group)


def frag_tuples(victims):
    return [(v.event, v.node, v.gpu_mask, v.score, v.frag_before, v.frag_after) for v in victims]


def cos_tuples(victims):
    return [(v.event, v.node, v.gpu_mask, v.gpu_left_milli, v.similarity) for v in victims]


_CASES, _RUNS, _WANT = {}, {}, {}


def get_case(key):
    """key: a fuzz spec (4-tuple), ("flat_frag", n) or ("flat_cos", n)."""
    if key not in _CASES:
        _CASES[key] = getattr(fz, key[0])(key[1]) if isinstance(key[0], str) else fz.from_fuzz(*key)
    return _CASES[key]


def okey(key):
    """The key of a case in test_gpu_desched's cache of oracle replays (shared with tests/test_gpu_desched_fuzz.py)."""
    return key if isinstance(key[0], str) else ("fuzz",) + key


def want_frag(key, sched, policy, ratio):
    k = (key, sched, policy, ratio)
    if k not in _WANT:
        _WANT[k] = frag.want_plan(get_case(key), okey(key), sched, policy, ratio)
    return _WANT[k]


def want_cos(key, sched, ratio, bars):
    k = (key, sched, "cos", ratio, bars)
    if k not in _WANT:
        _WANT[k] = cosm.want_plan(get_case(key), okey(key), sched, ratio, bars)
    return _WANT[k]


def make_group(key, sched, world):
    c = get_case(key)
    g = SH.ShardGroup(c["nodes"], c["typ"], world, policy=sched)
    g.load_events(c["events"], c["n"])
    return g


def plans_of(g, frag_plans, cos_plans):
    """For every asked plan: the device merge, and the host merge of the shards' parts (node = the input index)."""
    out = {}
    for policy, ratio in frag_plans:
        g.deschedule(policy, ratio)
        victims, budget = g.victims()
        parts, bounds = g.victim_parts()
        hv, hb = SH.merge_victims(parts, bounds, ratio, g.parts)
        out[policy, ratio] = dict(device=(frag_tuples(victims), budget), host=(frag_tuples(hv), hb),
                                  part_n=[len(p) for p in parts], bounds=bounds)
    for bars, ratio in cos_plans:
        g.deschedule_cossim(ratio, *bars)
        victims, budget = g.cos_victims()
        parts, bounds = g.victim_parts(cos=True)
        hv, hb = SH.merge_victims(parts, bounds, ratio, g.parts, cos=True)
        out["cos", bars, ratio] = dict(device=(cos_tuples(victims), budget), host=(cos_tuples(hv), hb),
                                       part_n=[len(p) for p in parts], bounds=bounds)
    return out


def run_group(key, sched, world, variant="", frag_plans=None, cos_plans=None):
    """One group run and its plans (kept for the tests that look at it from different sides)."""
    k = (key, sched, world, variant)
    if k not in _RUNS:
        need_api()
        if frag_plans is None:
            frag_plans = [(p, q) for p in FRAG for q in FRAG_RATIOS]
        if cos_plans is None:
            cos_plans = [(b, q) for b in COS_BARS for q in COS_RATIOS]
        g = make_group(key, sched, world)
        try:
            g.run()
            run = dict(results=g.results(), kernels=g.engines[0].last_run_kernels())
            run["plans"] = plans_of(g, frag_plans, cos_plans)
            run["ms"] = g.engines[0].last_deschedule_ms()
            _RUNS[k] = run
        finally:
            g.close()
    return _RUNS[k]


def check_run(run, key, sched):
    """Every plan of a cached run against the reference: the device merge, and the host merge equal to it."""
    assert run["results"] == oracle_run(get_case(key), okey(key), sched)[0]
    n_victims = 0
    for pk, got in run["plans"].items():
        if pk[0] == "cos":
            want = want_cos(key, sched, pk[2], pk[1])
        else:
            want = want_frag(key, sched, pk[0], pk[1])
        assert got["device"] == want, pk
        assert got["host"] == got["device"], pk
        n_victims += len(want[0])
    return n_victims


def worlds_of(spec):
    return [w for w in WORLDS if w <= spec[1]]  # (no shard without a node)


GROUPS = [(p, w) for p in CASES for w in worlds_of(p)]
GROUP_IDS = ["s%d-n%d-e%d-d%g-w%d" % (p + (w,)) for p, w in GROUPS]


@pytest.mark.parametrize("spec,world", GROUPS, ids=GROUP_IDS)
@pytest.mark.parametrize("sched", SCHEDS)
def test_fuzz_cluster_plans_equal_reference(spec, world, sched):
    need_api()
    run = run_group(spec, sched, world)
    assert check_run(run, spec, sched) > 0
    assert run["ms"] > 0
    # the bound pods of the shards add up to the reference's: the budget at ratio 1 is every bound pod
    for pk, got in run["plans"].items():
        if pk[-1] == 1.0:
            assert sum(got["bounds"]) == got["device"][1], pk


def test_a_shard_without_a_frag_victim():
    need_api()
    run = run_group(CREATE_ONLY, "FGD", 2)
    part_n = run["plans"][ref.MULTI_POD, 1.0]["part_n"]
    assert min(part_n) == 0 and max(part_n) > 0, part_n


@pytest.mark.parametrize("world", [2, 3, 5, 7])
@pytest.mark.parametrize("sched", SCHEDS)
def test_plan_after_the_persistent_group_launch(world, sched):
    # create-only: the FGD group on k_hmemo's slices, BestFit's on k_replay's
    need_api()
    run = run_group(CREATE_ONLY, sched, world)
    assert run["kernels"] == (["k_hmemo_group"] if sched == "FGD" else ["k_replay_group"]), run["kernels"]
    check_run(run, CREATE_ONLY, sched)


def test_plan_after_the_step_path_with_deletions():
    # BestFit with deletions: the per-pod k_step + gather + commit path of a group; the owner of a deleted pod
    # holds the delete event's record as deleted, so its creation is neither counted nor a candidate
    need_api()
    run = run_group(CASES[0], "BestFit", 2)
    assert run["kernels"] == ["k_step"]
    check_run(run, CASES[0], "BestFit")


@pytest.mark.parametrize("spec", [CASES[0], CREATE_ONLY], ids=["deletes", "create-only"])
def test_plan_after_the_fgd_step_path(monkeypatch, spec):
    need_api()
    monkeypatch.setenv("KSIM_VARIANT", "shard_hmemo=0")
    run = run_group(spec, "FGD", 2, "shard_hmemo=0")
    assert run["kernels"] == ["k_step"]
    check_run(run, spec, "FGD")


FLAT_N = [65, 257, 513]
FLAT_WORLDS = [2, 3, 16]


@pytest.mark.parametrize("world", FLAT_WORLDS)
@pytest.mark.parametrize("n", FLAT_N)
def test_flat_frag_merge_edges(n, world):
    # every node has a victim and the priorities tie over a seventh of the nodes: the whole merged order at ratio
    # 1.0, half of it, and a budget of one
    need_api()
    key = ("flat_frag", n)
    one = 0.5 / n
    run = run_group(key, "FGD", world, frag_plans=[(p, q) for p in FRAG for q in (1.0, 0.5, one)], cos_plans=[])
    check_run(run, key, "FGD")
    for p in FRAG:
        assert [len(run["plans"][p, q]["device"][0]) for q in (1.0, 0.5, one)] == [n, (n + 1) // 2, 1]
        assert run["plans"][p, 1.0]["part_n"] == [(k + 1) * n // world - k * n // world for k in range(world)]
    # neighbouring places of the merged list come from different shards
    nodes = get_case(key)["nodes"]
    starts = [k * n // world for k in range(world)]
    merged = run["plans"][ref.ONE_POD, 1.0]["device"][0]
    owner = [bisect.bisect_right(starts, nodes[v[1]].name_rank) - 1 for v in merged]
    assert set(owner) == set(range(world))
    assert sum(1 for a, b in zip(owner, owner[1:]) if a != b) >= 2 * (world - 1)


@pytest.mark.parametrize("world", FLAT_WORLDS)
@pytest.mark.parametrize("n", FLAT_N)
def test_flat_cos_merge_edges(n, world):
    need_api()
    key = ("flat_cos", n)
    one = 0.5 / n
    bars = (cos.CPU_BAR, cos.GPU_BAR)
    run = run_group(key, "FGD", world, frag_plans=[], cos_plans=[(bars, q) for q in (1.0, 0.5, one)])
    check_run(run, key, "FGD")
    assert [len(run["plans"]["cos", bars, q]["device"][0]) for q in (1.0, 0.5, one)] == [n, (n + 1) // 2, 1]


def test_one_shard_in_lds_and_one_in_hbm():
    # 6145 flat nodes at world 2: 3072 nodes (20 B a node: 60 KiB, the largest in-LDS launch of k_desched_select)
    # and 3073 (tables in HBM).  fragOnePod at ratio 1.0 writes both shards' whole order out.  The reference's
    # fragMultiPod scans every node per pop in Python, so that policy runs at ratio 0.01 (62 pops, the re-key in
    # both kinds of table); its full order at the switch sizes is tests/test_gpu_desched_fuzz.py's.
    need_api()
    n = 6145
    assert (3072 * 20 <= 60 * 1024) and (3073 * 20 > 60 * 1024) and [n // 2, n - n // 2] == [3072, 3073]
    key = ("flat_frag", n)
    run = run_group(key, "FGD", 2, frag_plans=[(ref.ONE_POD, 1.0), (ref.MULTI_POD, 0.01)], cos_plans=[])
    check_run(run, key, "FGD")
    assert run["plans"][ref.ONE_POD, 1.0]["part_n"] == [3072, 3073]
    assert len(run["plans"][ref.ONE_POD, 1.0]["device"][0]) == n
    assert len(run["plans"][ref.MULTI_POD, 0.01]["device"][0]) == 62


def code_of(call, *args):
    with pytest.raises(ksim.KsimError) as ei:
        call(*args)
    return ei.value.code


def test_repeat_and_invalidation():
    need_api()
    spec, sched = CASES[0], "FGD"
    c = get_case(spec)
    g = make_group(spec, sched, 3)
    try:
        assert code_of(g.deschedule, ref.ONE_POD, 0.1) == ksim.KSIM_ESTATE   # before a group run
        assert code_of(g.victims) == ksim.KSIM_ESTATE
        g.run()
        assert code_of(g.victims) == ksim.KSIM_ESTATE                          # before a plan
        # the three policies in a row on one group, and the first again
        for _ in range(2):
            g.deschedule(ref.MULTI_POD, 0.1)
            assert (frag_tuples(g.victims()[0]), g.victims()[1]) == want_frag(spec, sched, ref.MULTI_POD, 0.1)
            assert code_of(g.cos_victims) == ksim.KSIM_ESTATE                  # the getter of the other kind
            g.deschedule_cossim(1.0, *WIDE)
            assert (cos_tuples(g.cos_victims()[0]), g.cos_victims()[1]) == want_cos(spec, sched, 1.0, WIDE)
            assert code_of(g.victims) == ksim.KSIM_ESTATE
            g.deschedule(ref.ONE_POD, 1.0)
            assert (frag_tuples(g.victims()[0]), g.victims()[1]) == want_frag(spec, sched, ref.ONE_POD, 1.0)
        assert g.results() == oracle_run(c, okey(spec), sched)[0]     # planning changed no state
        # a shard's own list is not the cluster's plan
        assert code_of(g.engines[1].victims, 0) == ksim.KSIM_ENOTSUP
        assert code_of(g.engines[1].cos_victims, 0) == ksim.KSIM_ENOTSUP
        # engines that are not that group
        assert code_of(ksim.shard_group_victims, g.engines[:2]) == ksim.KSIM_EINVAL
        assert code_of(ksim.shard_group_victims, g.engines[::-1]) == ksim.KSIM_EINVAL
        assert code_of(ksim.shard_group_deschedule, g.engines[1:], ref.ONE_POD, 0.1) == ksim.KSIM_EINVAL
        # a plan of a shard's own replaces the one the merged list was made from
        g.engines[2].deschedule(ref.ONE_POD, 0.5)
        assert code_of(g.victims) == ksim.KSIM_ESTATE
        g.deschedule(ref.ONE_POD, 1.0)
        assert g.victims()[1] == want_frag(spec, sched, ref.ONE_POD, 1.0)[1]
        # new events on one shard drop its plan, and the group must run again before it plans
        g.engines[1].load_events(0, c["events"], c["n"])
        assert code_of(g.victims) == ksim.KSIM_ESTATE
        assert code_of(g.deschedule, ref.ONE_POD, 1.0) == ksim.KSIM_ESTATE
        g.run()
        g.deschedule(ref.ONE_POD, 1.0)
        assert (frag_tuples(g.victims()[0]), g.victims()[1]) == want_frag(spec, sched, ref.ONE_POD, 1.0)
    finally:
        g.close()


def test_unsharded_engine_part_is_its_plan():
    need_api()
    spec = CASES[0]
    c = get_case(spec)
    eng = frag.make_engine(c)
    try:
        eng.run()
        assert code_of(eng.victim_part) == ksim.KSIM_ESTATE
        eng.deschedule(ref.MULTI_POD, 0.1)
        victims, budget = eng.victims(0)
        part, bound = eng.victim_part()
        assert frag_tuples(part) == frag_tuples(victims) and (frag_tuples(part), budget) == \
            want_frag(spec, "FGD", ref.MULTI_POD, 0.1)
        assert bound == want_frag(spec, "FGD", ref.MULTI_POD, 1.0)[1]
        assert code_of(eng.cos_victim_part) == ksim.KSIM_ESTATE
        eng.deschedule_cossim(1.0, *WIDE)
        part, cbound = eng.cos_victim_part()
        assert cos_tuples(part) == cos_tuples(eng.cos_victims(0)[0]) and cbound == bound
    finally:
        eng.close()


def test_reschedule_a_group_and_plan_again():
    need_api()
    spec, sched, world = CASES[0], "FGD", 3
    c = get_case(spec)
    g = make_group(spec, sched, world)
    try:
        g.run()
        out = ksim.desched.run_group(g, ref.ONE_POD, 0.1)
        want, budget = want_frag(spec, sched, ref.ONE_POD, 0.1)
        assert (frag_tuples(out["victims"]), out["budget"]) == (want, budget) and want
        n0, nv = c["n"], len(want)
        assert (out["n"], out["n_original"], out["post_eviction"], out["post_deschedule"]) == \
            (n0 + 2 * nv, n0, n0 + nv - 1, n0 + 2 * nv - 1)
        first = [v[0] for v in want]
        oev = ref.extend_events(c["oev"], [dict(event=e) for e in first])
        pol, sel = cases.oracle_policy(sched)
        res, state = O.run_events(c["onodes"], c["otyp"], oev, policy=pol, gpu_sel=sel)[:2]
        assert g.results() == res
        assert all(res[n0 + k][4] == ksim.DELETED and res[n0 + k][0] == want[k][1] for k in range(nv))
        # a second plan on the extended stream: the first victims are gone, their copies are candidates
        for policy in FRAG:
            g.deschedule(policy, 1.0)
            victims, b2, _ = ref.plan(c["onodes"], c["otyp"], oev, res, state, policy, 1.0)
            assert (frag_tuples(g.victims()[0]), g.victims()[1]) == (ref.as_tuples(victims), b2) and victims
            assert not {v["event"] for v in victims} & set(first)
        bound = ref.bound_pods(oev, res)
        assert not set(bound) & set(first) and any(e >= n0 + nv for e in bound)
        g.deschedule_cossim(1.0, *WIDE)
        victims, b2, _ = cos.plan(c["onodes"], oev, res, state, 1.0, *WIDE)
        assert (cos_tuples(g.cos_victims()[0]), g.cos_victims()[1]) == (cos.as_tuples(victims), b2) and victims
    finally:
        g.close()


def _rank_main(rank, world, port, spec, sched, exchange, desched, q):
    import os
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    c = fz.from_fuzz(*spec)
    merged, ms, (victims, budget) = SH.run_distributed(c["nodes"], c["typ"], c["events"], c["n"], dist, policy=sched,
                                                       exchange=exchange, desched=desched)
    tuples = cos_tuples(victims) if desched[0] == "cosSim" else frag_tuples(victims)
    q.put((rank, merged, tuples, budget, ms))
    dist.destroy_process_group()


@pytest.mark.timeout(240)
@pytest.mark.parametrize("sched,exchange,desched", [("FGD", "device", (ref.MULTI_POD, 0.1)),
                                                    ("BestFit", "host", ("cosSim", 0.05) + WIDE)],
                         ids=["FGD-device-fragMultiPod", "BestFit-host-cosSim"])
def test_two_processes_plan_and_merge_on_the_host(sched, exchange, desched):
    # two shard processes on the one GPU: each plans its part behind its run, the ranks gather the parts' bytes and
    # bound counts, and each merges them on the host
    need_api()
    import inspect
    assert "desched" in inspect.signature(SH.run_distributed).parameters
    import multiprocessing as mp
    import socket
    spec = CASES[0]
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_rank_main, args=(r, 2, port, spec, sched, exchange, desched, q)) for r in range(2)]
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
    want_res = oracle_run(get_case(spec), okey(spec), sched)[0]
    if desched[0] == "cosSim":
        want = want_cos(spec, sched, desched[1], desched[2:])
    else:
        want = want_frag(spec, sched, *desched)
    assert want[0]
    for rank, merged, victims, budget, _ in res:
        assert merged == want_res, rank
        assert (victims, budget) == want, rank
