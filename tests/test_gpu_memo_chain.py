"""k_memo's per-step chain at the smallest shapes where it can go wrong.

wave_F keeps every fold buffer all +0.0 between evaluations: a lane stores its one cell and zeroes it again
after the fold, the kernel zeroes the buffers once before the step loop, and the decider's F waves share
them.  The owner's nine critical waves hand their F to wave 0 inside the step, off any barrier.  The
cases: stream lengths around the 128-event window, a class that dies right at the window edge, typical
tables of 1 / 63 / 64 / 65 / 130 entries (lanes past the table store nothing; a second and a third
chunk), a step whose changed node offers eight GPU candidates (all nine critical waves live), whole-GPU
pods, the first step and the step after an unschedulable pod (no changed node), a state whose F is
exactly 0.0, and consecutive events of one owner.  Every case is
compared event for event and in final state with the oracle, on the lean kernel and once on each other
instantiation (general: a delete directly after its create; report; decider; stress / general under
KSIM_TEST=hdelay=7).  All on at most 64 nodes and 400 events -- but for the keys-in-HBM form, which the
engine only chooses when a replica's keys do not fit in LDS beside the cluster: that one runs gpuspec33 on
its whole cluster with 2 500 events (enough classes that it is reached).
"""
import ctypes as C

import pytest

import helpers
import ksim
import pyoracle as O
from test_gpu_parity import assert_same, engine_run, oracle_run

pytestmark = pytest.mark.gpu

MEMO, DECIDER = 3, 4
UNSCHED = (-1, 0, 0, 0)  # node, mask, score, n_feasible of a pod no node can take


class Stream:
    """The events `idx` of a replay, in that order: stands in for the replay in engine_run / oracle_run."""

    def __init__(self, rp, idx):
        self.nodes, self.node_names = rp.nodes, rp.node_names
        self.pod_index = [rp.pod_index[k] for k in idx]
        self.n = len(idx)
        self.events = (ksim.Pod * max(1, self.n))()
        for j, k in enumerate(idx):
            C.memmove(C.byref(self.events[j]), C.byref(rp.events[k]), C.sizeof(ksim.Pod))


class Ctx:
    def __init__(self):
        self.t = t = ksim.Trace.openb("default")
        self.rp = rp = t.replay(seed=42, tune_ratio=1.3, shuffle=True)
        self.pods = t.pods()
        tn = t.nodes()
        self.by = {g: [i for i, n in enumerate(tn) if n["gpu"] == g] for g in (1, 2, 4, 8)}
        self.keep = sorted(self.by[8][:24] + self.by[4][:8] + self.by[2][:24] + self.by[1][:8])  # 64 nodes
        self.small = sorted(self.by[4][:12] + self.by[2][:20] + self.by[1][:8])  # 40 nodes, none with 8 GPUs
        self.onodes = helpers.oracle_nodes(t, rp)
        self.otyp = helpers.oracle_typical(t)
        self.built = {}

    def case(self, name):  # built once, shared by the forms that run it
        if name not in self.built:
            self.built[name] = CASES[name](self)
        return self.built[name]

    def pod(self, k):
        return self.pods[self.rp.pod_index[k]]

    def req(self, k):
        p = self.pod(k)
        return (p["cpu"], p["mem"], p["milli"], p["num"], p["spec"] if p["num"] > 0 else "")

    def oev(self, st):  # helpers.oracle_events without reading the trace's pods again on every call
        return [dict(cpu=p["cpu"], cpu_nz=p["cpu"], mem=p["mem"], milli=p["milli"], num=p["num"],
                     type=p["spec"] if p["num"] > 0 else "") for p in (self.pods[i] for i in st.pod_index)]

    def oracle(self, keep, st, otyp=None):
        return O.run_events([self.onodes[i] for i in keep], self.otyp if otyp is None else otyp, self.oev(st),
                            policy=O.POL_FGD, gpu_sel=O.SEL_FGD, threads=16 if len(keep) > 16 else 1)[:2]


@pytest.fixture(scope="module")
def ctx():
    return Ctx()


# ---- the cases: (nodes kept, stream, typical-table indices or None); each builder asserts, with the oracle on
# the CPU, that the stream has the property it is there for

def case_length(c, n):
    return c.keep, Stream(c.rp, range(n)), None


def case_dead_edge(c, pos):
    """Event `pos` belongs to a class that became dead at event pos - 1 (its first occurrence: no node of the
    shrunk cluster can ever take it), and so does event pos + 1."""
    big = [k for k in range(c.rp.n) if c.pod(k)["num"] == 8]
    assert big, "the trace has 8-GPU pods"
    breq = c.req(big[0])
    rest = [k for k in range(c.rp.n) if c.req(k) != breq]
    st = Stream(c.rp, rest[:pos - 1] + [big[0]] * 3 + rest[pos - 1:pos + 60])
    want, _ = c.oracle(c.small, st)
    assert want[pos - 1][:4] == UNSCHED and want[pos][:4] == UNSCHED and want[pos + 1][:4] == UNSCHED
    assert any(w[0] >= 0 for w in want[pos + 2:])  # the step after an unschedulable pod decides without a changed node
    return c.small, st, None


def case_typical(c, m):
    nt = len(c.otyp)
    return c.keep, Stream(c.rp, range(200)), ([i % nt for i in range(m)] if m >= nt else list(range(m)))


def case_eight_candidates(c):
    """Share pods packed on one 8-GPU node until its GPUs hold eight distinct milli-left values, every one enough
    for the share pods that follow: their steps evaluate d's current state and eight candidates."""
    keep = c.by[8][:2]
    share = {}
    for k in range(c.rp.n):
        p = c.pod(k)
        if p["num"] == 1 and 0 < p["milli"] < 1000:
            share.setdefault(p["milli"], k)
    small = min(share)
    idx, target, nd = [], None, 0
    while nd < 8 and len(idx) < 40:  # greedy: the pod that leaves the most distinct values, then the most room
        best = None
        for m in sorted(share):
            want, state = c.oracle(keep, Stream(c.rp, idx + [share[m]]))
            node = want[-1][0]
            if node < 0 or (target is not None and node != target):
                continue
            gl = state[node][3]
            key = (len(set(gl)), min(gl))
            if min(gl) >= small and (best is None or key > best[0]):
                best = (key, m, node)
        if best is None:
            break
        idx.append(share[best[1]])
        target, nd = best[2], best[0][0]
    assert nd == 8, "eight distinct milli-left values on one node (got %d)" % nd
    st = Stream(c.rp, idx + [share[small]] * 4)
    want, state = c.oracle(keep, Stream(c.rp, idx))
    assert want[-1][0] == target and len(set(state[target][3])) == 8 and min(state[target][3]) >= small
    return keep, st, None


def case_zero_f(c):
    """Whole-GPU pods on one-GPU nodes: the node the first one fills has no GPU milli left, so its F -- the
    next step's Fc[0] -- is exactly 0.0."""
    keep = c.by[1][:6]
    whole = [k for k in range(c.rp.n) if c.pod(k)["num"] == 1 and c.pod(k)["milli"] == 1000]
    whole = [k for k in whole[:40] if c.oracle(keep, Stream(c.rp, [k]))[0][0][0] >= 0][:4]  # those these nodes can take
    assert whole
    share = [k for k in range(c.rp.n) if c.pod(k)["num"] == 1 and 0 < c.pod(k)["milli"] < 1000][:6]
    st = Stream(c.rp, whole + share)
    want, state = c.oracle(keep, Stream(c.rp, whole[:1]))
    node = want[0][0]
    assert node >= 0 and state[node][3][0] == 0
    nres = O.node_res(state[node][0], [0], gpu_type=c.onodes[keep[node]]["model"])
    assert O.frag_score(nres, O.typical(c.otyp)) == 0.0
    return keep, st, None


def case_same_owner(c):
    """Every event twice in a row: consecutive events of one class, so of one owner."""
    st = Stream(c.rp, [k // 2 for k in range(300)])
    want, _ = c.oracle(c.keep, st)
    assert any(c.pod(k)["num"] >= 1 and c.pod(k)["milli"] == 1000 and want[2 * k][0] >= 0 for k in range(150)), \
        "a whole-GPU (Sub) class is placed"
    return c.keep, st, None


CASES = {
    "len127": lambda c: case_length(c, 127), "len128": lambda c: case_length(c, 128),
    "len129": lambda c: case_length(c, 129), "len257": lambda c: case_length(c, 257),
    "dead127": lambda c: case_dead_edge(c, 127), "dead128": lambda c: case_dead_edge(c, 128),
    "typ1": lambda c: case_typical(c, 1), "typ63": lambda c: case_typical(c, 63), "typ64": lambda c: case_typical(c, 64),
    "typ65": lambda c: case_typical(c, 65), "typ130": lambda c: case_typical(c, 130),
    "eight": case_eight_candidates, "zeroF": case_zero_f, "same_owner": case_same_owner,
}
# once through each other instantiation: the window edge, a dead class at it, a second and a third typical
# chunk, nine live critical waves, F == 0.0, one owner twice
OTHER = ["len129", "len257", "dead128", "typ65", "typ130", "eight", "zeroF", "same_owner"]


def run_case(c, name, form="lean", wgs=4):
    keep, st, tidx = c.case(name)
    arr, n = c.t.typical()
    otyp = c.otyp
    if tidx is not None:
        sub = (ksim.Typical * len(tidx))()
        for j, i in enumerate(tidx):
            C.memmove(C.byref(sub[j]), C.byref(arr[i]), C.sizeof(ksim.Typical))
        arr, n, otyp = sub, len(tidx), [c.otyp[i] for i in tidx]
    evs, oev = st.events, c.oev(st)
    if form == "general":  # a delete directly after its create (the first event's)
        d = ksim.Pod()
        C.memmove(C.byref(d), C.byref(evs[0]), C.sizeof(ksim.Pod))
        d.is_delete, d.ref = 1, 0
        evs = (ksim.Pod * (st.n + 1))(evs[0], d, *[evs[k] for k in range(1, st.n)])
        od = dict(oev[0])
        od.update(delete=1, ref=0)
        oev = [oev[0], od] + oev[1:]
    want, want_state, _ = O.run_events([c.onodes[i] for i in keep], otyp, oev, policy=O.POL_FGD, gpu_sel=O.SEL_FGD,
                                       threads=16)
    eng = ksim.Engine(len(keep), 1, run_mode=DECIDER if form == "decider" else MEMO, wgs_per_replica=wgs)
    try:
        if form == "report":
            eng.set_report(True)
        eng.set_nodes(0, helpers.subset_nodes(c.rp, keep))
        eng.set_typical(0, arr, n)
        eng.set_policy(0, "FGD")
        eng.load_events(0, evs, len(oev))
        eng.run()
        assert eng.last_run_kernels()[0] == "k_memo" and eng.last_run_wgs() == wgs
        res, state = eng.results(0), eng.nodes(0)
    finally:
        eng.close()
    assert_same(res, want, state, want_state, keep)


@pytest.mark.parametrize("n", [127, 128, 129, 257])
def test_stream_lengths(ctx, n):
    res, state = engine_run(ctx.t, ctx.rp, ctx.keep, n, "FGD", run_mode=MEMO, wgs=4)
    want, want_state, _ = oracle_run(ctx.t, ctx.rp, ctx.keep, n, O.POL_FGD, O.SEL_FGD)
    assert_same(res, want, state, want_state, ctx.keep)


@pytest.mark.parametrize("name", [k for k in CASES if not k.startswith("len") and k != "same_owner"])
def test_lean(ctx, name):
    run_case(ctx, name)


def test_same_owner_twice(ctx):
    run_case(ctx, "same_owner", wgs=2)


@pytest.mark.parametrize("name", OTHER)
@pytest.mark.parametrize("form", ["general", "report", "decider"])
def test_other_instantiations(ctx, form, name):
    run_case(ctx, name, form, wgs=3 if form == "decider" else 4)


@pytest.mark.parametrize("form", ["lean", "report", "general"])
def test_keys_in_hbm(form):
    t = ksim.Trace.openb("gpuspec33")
    rp = t.replay(seed=43)
    arr, n = t.typical()
    n_ev = 2500  # the stream must bring enough classes that their keys do not fit in LDS
    evs, oev = rp.events, helpers.oracle_events(t, rp, n_ev)
    if form == "general":  # a delete directly after its create
        d = ksim.Pod()
        C.memmove(C.byref(d), C.byref(evs[0]), C.sizeof(ksim.Pod))
        d.is_delete, d.ref = 1, 0
        evs = (ksim.Pod * (n_ev + 1))(evs[0], d, *[evs[k] for k in range(1, n_ev)])
        od = dict(oev[0])
        od.update(delete=1, ref=0)
        oev = [oev[0], od] + oev[1:]
    want, want_state, _ = O.run_events(helpers.oracle_nodes(t, rp), helpers.oracle_typical(t), oev, policy=O.POL_FGD,
                                       gpu_sel=O.SEL_FGD, threads=16)
    eng = ksim.Engine(t.num_nodes, 1, run_mode=MEMO, wgs_per_replica=25)
    try:
        if form == "report":
            eng.set_report(True)
        eng.set_nodes(0, rp.nodes)
        eng.set_typical(0, arr, n)
        eng.set_policy(0, "FGD")
        eng.load_events(0, evs, len(oev))
        eng.run()
        assert eng.last_run_kernels() == ["k_memo_hkeys"]
        res, state = eng.results(0), eng.nodes(0)
    finally:
        eng.close()
    assert_same(res, want, state, want_state, None)


@pytest.mark.parametrize("form", ["lean", "general"], ids=["stress", "general"])
def test_hand_over_stress(ctx, monkeypatch, form):
    # every delay point on: the lean kernel with the delays compiled in, and the general one
    monkeypatch.setenv("KSIM_TEST", "hdelay=7")
    run_case(ctx, "len257", form)
