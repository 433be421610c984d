"""Inputs and reference replays shared by the weighted-combination tests (not collected): tests/test_weighted_ref_cpu.py,
tests/test_gpu_wsum.py.

Leg A (the oracle reaches): the first 400 events of openb default, seed 42, on the 173-node subset range(3, 1213, 7), as
tests/test_gpu_pwr.py -- it fills and then fails -- and a create / delete stream over the same subset.
Leg B (true mixtures): 400 events of the same trace on the 135 nodes range(1, 1213, 9) -- the first 200 creations, a
deletion of two of every three of them, then 67 more creations (mix_stream) -- and the reference of
tests/weighted_ref.py, made once per mixture and shared.  A create-only stream does not exercise every combination: a
mixture that GpuPacking dominates keeps the cluster packed, with one partly used node at a time, and then chooses what
GpuPacking alone would; the deletions leave many partly used nodes, whose GpuPacking scores tie.
"""
import ctypes as C

import helpers
import ksim
import pyoracle as O
import weighted_ref

N_EV = 400
DELETE_AFTER = 150

# leg A: weights -> (oracle policy, oracle selector, engine selector, dim_ext, norm)
SINGLES = {
    "FGD": (O.POL_FGD, O.SEL_FGD, "FGD", "merge", "max"),
    "BestFit": (O.POL_BESTFIT, O.SEL_BEST, "best", "merge", "max"),
    "DotProd": (O.POL_DOTPROD, O.SEL_BEST, "best", "merge", "max"),
    "DotProd-share-node": (O.POL_DOTPROD, O.SEL_DOTPROD, "DotProd", "share", "node"),
    "GpuPacking": (O.POL_PACKING, O.SEL_BEST, "best", "merge", "max"),
    "GpuClustering": (O.POL_CLUSTERING, O.SEL_BEST, "best", "merge", "max"),
    "PWR": (O.POL_PWR, O.SEL_PWR, "PWR", "merge", "max"),
}
PAIRS = [(500, 500), (100, 900), (50, 950), (1, 1)]

# leg B: name -> (weights, selector); every stream must exercise the combination (divergence >= 10 %)
MIXTURES = {
    "FGD 700 BestFit 300": ({"FGD": 700, "BestFit": 300}, "FGD"),
    "BestFit 500 PWR 500": ({"BestFit": 500, "PWR": 500}, "best"),
    "DotProd 500 GpuPacking 500": ({"DotProd": 500, "GpuPacking": 500}, "best"),
    "FGD 400 GpuClustering 300 PWR 300": ({"FGD": 400, "GpuClustering": 300, "PWR": 300}, "FGD"),
    "all six": ({"FGD": 310, "BestFit": 270, "DotProd": 90, "GpuPacking": 130, "GpuClustering": 110, "PWR": 190}, "FGD"),
    "1 and 50000": ({"BestFit": 1, "FGD": 50000}, "FGD"),
}
MIX_CREATE, MIX_EV = 200, 400  # creations before the deletions; events in all

_CACHE = {}


def trace():
    if "trace" not in _CACHE:
        _CACHE["trace"] = ksim.Trace.openb("default")
        _CACHE["replay"] = _CACHE["trace"].replay(seed=42)
    return _CACHE["trace"], _CACHE["replay"]


def keep_a():
    t, _ = trace()
    return list(range(3, t.num_nodes, 7))  # 173 nodes, every GPU model


def keep_b():
    t, _ = trace()
    return list(range(1, t.num_nodes, 9))  # 135 nodes


def _stream(oev, n_create, deleted, n_total):
    """creations 0 .. n_create-1, a deletion of each creation in `deleted`, then creations up to n_total events
    -> (engine events, oracle events)"""
    _, rp = trace()
    evs, oevs = [], []

    def create(i):
        e = ksim.Pod()
        C.memmove(C.byref(e), C.byref(rp.events[i]), C.sizeof(ksim.Pod))
        evs.append(e)
        oevs.append(dict(oev[i]))

    for i in range(n_create):
        create(i)
    for ref in deleted:
        d = ksim.Pod()
        C.memmove(C.byref(d), C.byref(rp.events[ref]), C.sizeof(ksim.Pod))
        d.is_delete, d.ref = 1, ref
        evs.append(d)
        od = dict(oev[ref])
        od.update(delete=1, ref=ref)
        oevs.append(od)
    for i in range(n_create, n_create + n_total - len(evs)):
        create(i)
    return (ksim.Pod * len(evs))(*evs), oevs


def mix_stream():
    """Leg B's stream: MIX_CREATE creations, a deletion of two of every three of them (a delete of a creation that
    failed changes nothing), then creations up to MIX_EV events.  -> (engine events, oracle events)"""
    if "mix" not in _CACHE:
        _, _, oev = oracle_inputs(keep_b(), MIX_EV)
        _CACHE["mix"] = _stream(oev, MIX_CREATE, [r for r in range(MIX_CREATE) if r % 3 != 0], MIX_EV)
    return _CACHE["mix"]


def oracle_inputs(keep, n_ev):
    """(onodes, otypical, oevents) of the subset, made once."""
    k = ("oin", tuple(keep), n_ev)
    if k not in _CACHE:
        t, rp = trace()
        _CACHE[k] = (helpers.oracle_subset(t, rp, keep), helpers.oracle_typical(t), helpers.oracle_events(t, rp, n_ev))
    return _CACHE[k]


def delete_stream(keep):
    """Leg A's create / delete stream: the first 150 creations, then a deletion of every third pod the FGD replay of
    those creations bound, then the rest of the 400 creations (the way tests/test_gpu_parity.py builds them).
    -> (engine events, oracle events)"""
    k = ("del", tuple(keep))
    if k in _CACHE:
        return _CACHE[k]
    t, rp = trace()
    onodes, otyp, oev = oracle_inputs(keep, N_EV)
    first, _, _ = O.run_events(onodes, otyp, oev[:DELETE_AFTER], policy=O.POL_FGD, gpu_sel=O.SEL_FGD, threads=16)
    bound = [i for i, r in enumerate(first) if r[0] >= 0][::3]
    _CACHE[k] = _stream(oev, DELETE_AFTER, bound, N_EV + len(bound))
    return _CACHE[k]


def reference(name):
    """The Python reference's replay of mixture `name` on leg B's inputs: (multi-feasible steps, steps whose choice
    differs from every participating plugin's own, results, final state); made once."""
    k = ("ref", name)
    if k not in _CACHE:
        weights, sel = MIXTURES[name]
        onodes, otyp, _ = oracle_inputs(keep_b(), MIX_EV)
        _CACHE[k] = weighted_ref.divergence(onodes, otyp, mix_stream()[1], weights, sel)
    return _CACHE[k]


def engine_run(keep, events, n_ev, weights, gpusel, dim_ext=None, norm=None, report=False, policy="Weighted"):
    """One replica on k_wsum (or, with another `policy`, on whatever the engine picks) -> (results, state, path, engine
    left open when report, else None)."""
    t, rp = trace()
    arr, n = t.typical()
    eng = ksim.Engine(len(keep), 1)
    try:
        eng.set_nodes(0, helpers.subset_nodes(rp, keep))
        eng.set_typical(0, arr, n)
        eng.set_power_model(0, t.power_model())
        if policy == "Weighted":
            eng.set_policy(0, "Weighted", gpusel=gpusel, dim_ext=dim_ext, norm=norm, weights=weights)
        else:
            eng.set_policy(0, policy, gpusel=gpusel, dim_ext=dim_ext, norm=norm)
        if report:
            eng.set_report(True)
        eng.load_events(0, events, n_ev)
        eng.run()
        out = eng.results(0), eng.nodes(0), eng.last_run_path()
        if report:
            return out + (eng,)
    except Exception:
        eng.close()
        raise
    eng.close()
    return out + (None,)


def assert_same(res, want, state, want_state):
    bad = [i for i, (a, b) in enumerate(zip(res, want)) if tuple(a) != tuple(b)]
    assert len(res) == len(want) and not bad, "first mismatch at event %d: gpu %s reference %s" % (
        bad[0], res[bad[0]], want[bad[0]])
    for i, (cpu_left, mem_left, pods, gl) in enumerate(want_state):
        s = state[i]
        assert s.cpu_alloc_milli - s.cpu_used_milli == cpu_left and s.pods_used == pods, i
        assert s.mem_alloc_mib - s.mem_used_mib == mem_left, i
        assert [1000 - s.gpu_used_milli[g] if g < s.gpu_count else 0 for g in range(8)] == list(gl), i
