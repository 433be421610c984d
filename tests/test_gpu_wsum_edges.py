"""k_wsum at its edges: crafted clusters and streams of a few dozen events, against the Python reference cycle of
tests/weighted_ref.py (proved against the oracle by tests/test_weighted_ref_cpu.py), plus the error codes of
ksim_engine_set_plugin_weights / ksim_engine_run that need an engine.  Every test needs a gfx950 device.

Slot ownership: thread t of the 1024-thread workgroup owns the node slots t, t + 1024, ...; a wave is 64 threads.  So
the node counts are 1, 2, 63 / 64 / 65 (a wave's last lane, the next wave's first) and 1023 / 1024 / 1025 (the last
thread's slot, and the first thread's second slot).
"""
import ctypes as C

import pytest

import ksim
import pyoracle as O
import weighted_ref
import wsum_cases as W

pytestmark = pytest.mark.gpu

BLOCK = 1024  # ksim_plan.hpp wsum::kBlock
SHAPES = [0, 1, 2, 4, 8, 8, 2]
PODS = [(2000, 500, 1), (4000, 1000, 1), (1000, 0, 0), (8000, 1000, 2), (1500, 250, 1), (3000, 700, 1), (16000, 1000, 8),
        (500, 100, 1)]
WORKLOAD = [(4000, 1000, 8, ""), (4000, 1000, 1, ""), (2000, 500, 1, ""), (1000, 250, 1, ""), (8000, 1000, 2, ""),
            (1000, 0, 0, "")]


def models():
    t, _ = W.trace()
    return t.type_names()


def generic_nodes(n):
    """(cpu, mem, pods, gpu, model index): every GPU count, two GPU models, CPU sizes 16 .. 64 cores"""
    return [(16000 + 8000 * (i % 7), 262144, 1000, SHAPES[i % 7], i % 2) for i in range(n)]


def typical(workload):
    """-> (engine table, n, oracle list); a type string "A|B" names models by name"""
    names = models()
    otyp = O.get_typical_pods(workload, threshold=100)
    typ = (ksim.Typical * len(otyp))()
    for i, (cpu, milli, num, spec, freq) in enumerate(otyp):
        typ[i].cpu_milli, typ[i].gpu_milli, typ[i].gpu_count, typ[i].freq = cpu, milli, num, freq
        typ[i].type_mask = sum(1 << names.index(s) for s in spec.split("|")) if spec else ksim.KSIM_TYPE_ANY
    return typ, len(otyp), otyp


def case(nodes, pods, workload=WORKLOAD, ranks=None):
    """nodes: [(cpu, mem, pods, gpu, model)]; pods: [(cpu, milli, num[, cpu_nz[, type names]])] or ("del", ref).
    Name ranks run against the node index unless given."""
    names, n = models(), len(nodes)
    ranks = ranks if ranks is not None else [n - 1 - i for i in range(n)]
    arr = (ksim.Node * n)()
    onodes = []
    for i, (cpu, mem, pa, gpu, model) in enumerate(nodes):
        a = arr[i]
        a.cpu_alloc_milli, a.mem_alloc_mib, a.pods_alloc = cpu, mem, pa
        a.gpu_count, a.gpu_type, a.name_rank = gpu, model if gpu else 0, ranks[i]
        onodes.append(dict(name="%06d-n%d" % (ranks[i], i), cpu=cpu, mem=mem, pods=pa, gpu=gpu,
                           model=names[model] if gpu else ""))
    evs, oev = [], []
    for q in pods:
        if q[0] == "del":
            d = ksim.Pod()
            C.memmove(C.byref(d), C.byref(evs[q[1]]), C.sizeof(ksim.Pod))
            d.is_delete, d.ref = 1, q[1]
            evs.append(d)
            od = dict(oev[q[1]])
            od.update(delete=1, ref=q[1])
            oev.append(od)
            continue
        cpu, milli, num = q[:3]
        cpu_nz = q[3] if len(q) > 3 else cpu
        spec = q[4] if len(q) > 4 else ""
        mask = sum(1 << names.index(s) for s in spec.split("|")) if spec else ksim.KSIM_TYPE_ANY
        evs.append(ksim.make_pod(cpu, milli, num, 0, mask, cpu_nz=cpu_nz))
        oev.append(dict(cpu=cpu, cpu_nz=cpu_nz, mem=0, milli=milli, num=num, type=spec))
    typ, nt, otyp = typical(workload)
    return dict(nodes=arr, n=n, events=(ksim.Pod * max(1, len(evs)))(*evs), n_events=len(evs), typical=typ, nt=nt,
                onodes=onodes, oevents=oev, otypical=otyp)


def engine(c, weights, gpusel, dim_ext=None, norm=None, power=True, **kw):
    t, _ = W.trace()
    eng = ksim.Engine(c["n"], 1, **kw)
    eng.set_nodes(0, c["nodes"])
    eng.set_typical(0, c["typical"], c["nt"])
    if power:
        eng.set_power_model(0, t.power_model())
    eng.set_policy(0, "Weighted", gpusel=gpusel, dim_ext=dim_ext, norm=norm, weights=weights)
    eng.load_events(0, c["events"], c["n_events"])
    return eng


def run_both(c, weights, gpusel="best", dim_ext=None, norm=None, report=False):
    eng = engine(c, weights, gpusel, dim_ext, norm)
    try:
        if report:
            eng.set_report(True)
        eng.run()
        assert eng.last_run_path() == "k_wsum"
        res, state = eng.results(0), eng.nodes(0)
    finally:
        eng.close()
    want, want_state = weighted_ref.run(c["onodes"], c["otypical"], c["oevents"], weights, gpusel,
                                        getattr(O, "DIM_" + (dim_ext or "merge").upper()),
                                        getattr(O, "NORM_" + (norm or "max").upper()))
    W.assert_same(res, want, state, want_state)
    return [tuple(r) for r in res]


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1])
def test_node_counts_at_the_block_edges(n):
    # the last slot is the only node with 128 cores: the first pod fits nowhere else, the second there and on node 0
    nodes = generic_nodes(n)
    nodes[-1] = (128000, 262144, 1000, 8, 1)
    c = case(nodes, [(100000, 0, 0), (20000, 500, 1)] + [PODS[k % len(PODS)] for k in range(38)])
    res = run_both(c, {"FGD": 600, "BestFit": 400}, "FGD")
    assert res[0][0] == n - 1 and res[0][3] == 1 and res[1][4] == ksim.SCHEDULED
    assert sum(r[4] == ksim.SCHEDULED for r in res) >= min(40, 3 * n)


def test_one_feasible_node_wins_whatever_its_plugins_say():
    # node 1 has no GPU; the pod's non-zero CPU request (Score) exceeds node 0's CPU, so BestFit's Score is -1 there:
    # with one feasible node the cycle never scores (generic_scheduler.go:158-164)
    c = case([(8000, 65536, 100, 2, 0), (64000, 65536, 100, 0, 0)], [(100, 500, 1, 32000)])
    res = run_both(c, {"FGD": 1000, "BestFit": 1}, "best")
    assert res[0] == (0, 1, 0, 1, ksim.SCHEDULED)


@pytest.mark.parametrize("kind", ["bestfit", "clustering", "dotprod"])
def test_score_error_on_one_of_two_feasible_nodes_aborts(kind):
    if kind == "bestfit":      # cpu_nz above node 0's CPU: getBestFitScore returns -1 there
        c = case([(8000, 65536, 100, 2, 0), (64000, 65536, 100, 2, 0)], [(100, 500, 1, 32000), (100, 500, 1)])
        w = {"FGD": 1000, "BestFit": 1}
    elif kind == "clustering":  # two shared GPUs: the pod's affinity tag is the reference's panic (-2)
        c = case([(8000, 65536, 100, 2, 0), (64000, 65536, 100, 2, 0)], [(100, 500, 2), (100, 500, 1)])
        w = {"FGD": 1000, "GpuClustering": 1}
    else:                       # node 0 has 3 x MaxSpecCpu left: its DotProduct score is -50, outside 0..100 (the
        # scores are 100 (1 - x) with x >= 0: a score leaves the range downwards, never above 100)
        c = case([(384000, 65536, 100, 2, 0), (64000, 65536, 100, 2, 0)], [(100, 500, 1, 128000), (100, 500, 1)])
        w = {"FGD": 1000, "DotProd": 1}
    res = run_both(c, w, "best")
    assert res[0] == (-1, 0, 0, 2, ksim.ERROR)  # nothing bound: the next pod sees the empty cluster
    assert res[1][4] == ksim.SCHEDULED and res[1][3] == 2


def test_all_raw_scores_equal():
    # identical empty nodes: BestFit normalises to 0 on every node and PWR to 100 (plugin_utils.go:48-74,
    # pwr_score.go:104-141); the tie goes to the smallest name, rank 0 = the last node
    c = case([(32000, 65536, 100, 4, 0)] * 5, [(2000, 500, 1)] * 12)
    res = run_both(c, {"BestFit": 700, "PWR": 300}, "best")
    assert res[0][:3] == (4, 1, 100 * 300) and res[0][3] == 5


def test_name_tie_break_by_rank():
    # GpuPacking scores every identical empty node alike: the total ties, the name rank decides; ranks in reverse
    # input order, then a permutation
    c = case([(32000, 65536, 100, 4, 0)] * 6, [(2000, 1000, 1)] * 3)
    assert [r[0] for r in run_both(c, {"GpuPacking": 500, "DotProd": 500})][0] == 5
    c = case([(32000, 65536, 100, 4, 0)] * 6, [(2000, 1000, 1)] * 3, ranks=[3, 5, 0, 4, 1, 2])
    assert run_both(c, {"GpuPacking": 500, "DotProd": 500})[0][0] == 2


def test_typed_pods_on_two_gpu_models():
    # a typical table that names GPU models (the typed frag_F) and pods that accept one model or both
    a, b = models()[0], models()[1]
    wl = [(4000, 1000, 1, a), (2000, 500, 1, b), (2000, 500, 1, a + "|" + b), (1000, 250, 1, ""), (1000, 0, 0, "")]
    pods = [(2000, 500, 1, 2000, a), (2000, 500, 1, 2000, b), (4000, 1000, 1, 4000, a), (1000, 250, 1), (2000, 500, 1, 2000, a + "|" + b)] * 8
    c = case(generic_nodes(20), pods, workload=wl)
    res = run_both(c, {"FGD": 600, "BestFit": 400}, "FGD")
    assert sum(r[4] == ksim.SCHEDULED for r in res) >= 30


@pytest.mark.parametrize("entries", [1, 70])
def test_typical_table_sizes(entries):
    wl = [(1000 + 100 * k, 100 + 10 * (k % 60), 1, "") for k in range(entries)]
    c = case(generic_nodes(20), [PODS[k % len(PODS)] for k in range(32)], workload=wl)
    assert c["nt"] == entries and (entries == 1 or entries > 64)
    run_both(c, {"FGD": 900, "GpuPacking": 100}, "FGD")


def test_reserve_failure_on_the_winner():
    # two shared GPUs: feasible and scored, but allocateGpuId panics on the request (open_gpu_share.go:266-268)
    c = case(generic_nodes(10), [(1000, 400, 2), (1000, 400, 1)])
    res = run_both(c, {"FGD": 600, "BestFit": 400}, "best")
    assert res[0][0] == -1 and res[0][2] == 0 and res[0][3] >= 2 and res[0][4] == ksim.ERROR
    assert res[1][4] == ksim.SCHEDULED


def test_delete_of_a_failed_creation_and_of_a_bound_one():
    pods = [(2000, 500, 1), (10 ** 6, 0, 0), ("del", 1), (2000, 500, 1), ("del", 0), (2000, 500, 1)]
    c = case(generic_nodes(9), pods)
    res = run_both(c, {"FGD": 600, "GpuClustering": 400}, "FGD", report=True)
    assert res[1][4] == ksim.UNSCHEDULABLE and res[2] == (-1, 0, 0, 0, ksim.DELETED)
    assert res[4][4] == ksim.DELETED and res[4][:2] == res[0][:2]


def test_largest_legal_weights():
    # 100 * sum(w) must stay below 2^24, the packed key's score field.  The largest legal sum is 167772: a total of
    # 16777200 = 2^24 - 16 (2^24 - 100 is not a multiple of 100)
    c = case(generic_nodes(12), [PODS[k % len(PODS)] for k in range(24)])
    res = run_both(c, {"FGD": 167771, "BestFit": 1}, "FGD")
    assert max(r[2] for r in res) > (1 << 23) and max(r[2] for r in res) <= 16777200
    eng = engine(c, {"FGD": 1}, "FGD")
    try:
        with pytest.raises(ksim.KsimError) as ei:
            eng.set_plugin_weights(0, {"FGD": 167772, "BestFit": 1})
        assert ei.value.code == ksim.KSIM_ERANGE
    finally:
        eng.close()


def code(fn, *a, **kw):
    with pytest.raises(ksim.KsimError) as ei:
        fn(*a, **kw)
    return ei.value.code


def test_error_codes():
    t, rp = W.trace()
    c = case(generic_nodes(8), [PODS[k % len(PODS)] for k in range(8)])
    L = ksim.lib()
    eng = ksim.Engine(8, 1)
    try:
        eng.set_nodes(0, c["nodes"])
        eng.set_typical(0, c["typical"], c["nt"])
        eng.load_events(0, c["events"], c["n_events"])
        eng.set_policy(0, "FGD")
        assert code(eng.set_plugin_weights, 0, {"FGD": 1}) == ksim.KSIM_ESTATE   # not a WEIGHTED replica
        ksim.check(L.ksim_engine_set_policy(eng.h, 0, ksim.POLICY["Weighted"], ksim.GPUSEL["FGD"], 0), "set_policy")
        assert code(eng.run) == ksim.KSIM_ESTATE                                 # no weights yet
        assert L.ksim_engine_set_plugin_weights(eng.h, 0, None) == ksim.KSIM_EINVAL
        assert code(eng.set_plugin_weights, 1, {"FGD": 1}) == ksim.KSIM_EINVAL
        assert code(eng.set_plugin_weights, 0, {"FGD": -1, "BestFit": 5}) == ksim.KSIM_ERANGE
        assert code(eng.set_plugin_weights, 0, {"FGD": 0}) == ksim.KSIM_ERANGE
        assert code(eng.set_plugin_weights, 0, {"FGD": 1, "Random": 1}) == ksim.KSIM_ENOTSUP
        assert code(eng.set_plugin_weights, 0, {"BestFit": 1}) == ksim.KSIM_ENOTSUP  # selector FGD, FGD's weight 0
        for sel, w in (("PWR", {"FGD": 1}), ("DotProd", {"PWR": 1})):
            eng.set_policy(0, "Weighted", gpusel="best", weights={"FGD": 1})
            ksim.check(L.ksim_engine_set_policy(eng.h, 0, 8, ksim.GPUSEL[sel], 0), "set_policy")  # any selector
            assert code(eng.set_plugin_weights, 0, w) == ksim.KSIM_ENOTSUP
            assert code(eng.run) == ksim.KSIM_ENOTSUP  # the selector is checked again at run
        eng.set_policy(0, "Weighted", gpusel="best", weights={"PWR": 1, "BestFit": 1})
        assert code(eng.run) == ksim.KSIM_ESTATE                                 # PWR without a power model
        eng.set_power_model(0, t.power_model())
        eng.run()
        assert eng.last_run_path() == "k_wsum"
        pod = c["events"][0]
        assert code(eng.filter_score, 0, pod) == ksim.KSIM_ENOTSUP
        assert code(eng.schedule, 0, pod) == ksim.KSIM_ENOTSUP
        assert code(eng.reserve, 0, pod, 0) == ksim.KSIM_ENOTSUP
    finally:
        eng.close()
    eng = engine(c, {"FGD": 1}, "FGD", run_mode=1)  # the per-pod path has no weighted combination
    try:
        assert code(eng.run) == ksim.KSIM_ENOTSUP
    finally:
        eng.close()


def test_cluster_past_one_workgroups_lds_is_refused():
    # 1722 nodes fit with every plugin on and the report's record (92 B per node), 1723 do not
    for n, ok in ((1722, True), (1723, False)):
        c = case(generic_nodes(n), PODS[:4])
        eng = engine(c, {"FGD": 1, "BestFit": 1, "DotProd": 1, "GpuPacking": 1, "GpuClustering": 1, "PWR": 1}, "FGD")
        try:
            eng.set_report(True)
            if ok:
                eng.run()
                assert eng.last_run_path() == "k_wsum"
            else:
                assert code(eng.run) == ksim.KSIM_ENOTSUP
        finally:
            eng.close()


def test_shard_is_refused():
    c = case(generic_nodes(8), PODS[:4])
    eng = engine(c, {"FGD": 1}, "FGD")
    try:
        eng.set_shard(0, 1, 0, 8)
        assert code(eng.run) == ksim.KSIM_ENOTSUP
    finally:
        eng.close()
