"""k_memo's look-ahead top-2: the next create event's class scanned in phase A, the changed node merged after C.

At step s the workgroup that owns the class of event s + 1 needs that class's two best keys before step s + 1.
Its waves 10-14 scan the class's keys over every node but d (the node event s - 1 changed) while the step's
refresh runs, and the list wave merges d's fresh key in once it is stored: top2(S) = merge2(top2(S \\ {d}), key_d).
What can go wrong is an index (the lane stride of the scan, the excluded column, the window's look-ahead slot),
the merged key's source (wave 0's store for the step's own score group, the list wave's for every other), or a
step on which the old full scan still runs (the first create event, the first live step after a run of dead ones).

Every case is compared with the oracle event for event and in final state.  Each builder first asserts on the CPU
that its stream has the property it is there for, with a model of the step written here from the oracle's own
pieces (Filter by the rules below, O.fgd_score, ties to the smallest name) that is itself checked against the
oracle's decision and feasible count on every event of the stream, and a model of the host's class placement
(memo_assign: score groups whole, largest first, to the workgroup with the fewest groups).
"""
import pytest

import helpers
import ksim
import pyoracle as O
from test_gpu_memo_chain import Ctx, Stream, MEMO, UNSCHED
from test_gpu_parity import assert_same
from test_gpu_report import assert_reports

pytestmark = pytest.mark.gpu

SCAN_LANES = 5 * 64  # L: waves 10-14 scan (ksim_memo.hpp kScanMask)
L = SCAN_LANES


@pytest.fixture(scope="module")
def ctx():
    return Ctx()


# ---- the CPU model of a stream: per event its class, the cluster before it, and every class's ranking on demand

class Walk:
    """The oracle's run of stream `st` on nodes `keep`, replayed node by node: pre[i] is the cluster before event
    i as [(cpu_left, mem_left, [gpu milli left])], node[i] the node event i changed (-1 none)."""

    def __init__(self, c, keep, st, oev=None):
        self.c, self.keep = c, keep
        self.oev = oev = c.oev(st) if oev is None else oev
        self.want, self.final, _ = O.run_events([c.onodes[i] for i in keep], c.otyp, oev, policy=O.POL_FGD,
                                                gpu_sel=O.SEL_FGD, threads=16 if len(keep) > 16 else 1)
        self.n = len(oev)
        self.model = [c.onodes[i]["model"] for i in keep]
        self.ngpu = [c.onodes[i]["gpu"] for i in keep]
        order = sorted(range(len(keep)), key=lambda j: c.rp.nodes[keep[j]].name_rank)
        self.rank = {j: r for r, j in enumerate(order)}
        self.typ = O.typical(c.otyp)
        self.req = [(e["cpu"], e["mem"], e["milli"], e["num"], e["type"]) for e in oev]
        self.is_del = [bool(e.get("delete", 0)) for e in oev]
        ids = {}
        self.cls = [-1 if self.is_del[i] else ids.setdefault(q, len(ids)) for i, q in enumerate(self.req)]
        self.cls_req = {v: k for k, v in ids.items()}
        state = [[n["cpu"], n["mem"], [1000] * n["gpu"]] for n in (c.onodes[i] for i in keep)]
        self.pre, self.node = [], []
        for i, w in enumerate(self.want):
            self.pre.append([(a, b, list(g)) for a, b, g in state])
            nd, mask = w[0], w[1]
            self.node.append(nd)
            if nd < 0:
                continue
            e = oev[oev[i]["ref"]] if self.is_del[i] else oev[i]
            sign = -1 if self.is_del[i] else 1
            state[nd][0] -= sign * e["cpu"]
            state[nd][1] -= sign * e["mem"]
            for g in range(8):
                if (mask >> g) & 1:
                    state[nd][2][g] -= sign * e["milli"]
        for j, (cpu_left, mem_left, _, gl) in enumerate(self.final):  # the replay above is the oracle's
            assert (state[j][0], state[j][1], state[j][2]) == (cpu_left, mem_left, gl[:self.ngpu[j]]), j
        # the model's decision and feasible count are the oracle's on every create event
        for i in range(self.n):
            if not self.is_del[i]:
                r = self.ranking(i, self.cls[i])
                assert len(r) == self.want[i][3], (i, len(r), self.want[i])
                assert (r[0][2] if r else -1) == self.want[i][0], (i, r[:2], self.want[i])

    def feasible(self, s, j, q):
        cpu, mem, milli, num, spec = q
        return (s[0] >= cpu and s[1] >= mem and (num == 0 or spec == "" or spec == self.model[j])
                and sum(1 for g in s[2] if g >= milli) >= num)

    def ranking(self, i, cls):
        """Feasible nodes of class `cls` on the cluster before event i, best first: (score, -rank, node)."""
        q = self.cls_req[cls]
        pod = O.pod_res(q[0], q[2], q[3], q[4])
        out = []
        for j, s in enumerate(self.pre[i]):
            if self.feasible(s, j, q):
                sc = O.fgd_score(O.node_res(s[0], s[2], gpu_type=self.model[j]), pod, self.typ)[0]
                out.append((sc, -self.rank[j], j))
        return sorted(out, reverse=True)

    def owners(self, K):
        """memo_assign for K workgroups: class -> (workgroup, score group)."""
        groups = {}
        for cid in sorted(self.cls_req):
            q = self.cls_req[cid]
            groups.setdefault((q[0], q[2], q[3]), []).append(cid)
        gl = sorted(groups.items(), key=lambda kv: -len(kv[1]))  # stable: first appearance among equals
        ncls = len(self.cls_req)
        for cw in range(max(1, (ncls + K - 1) // K), 65):
            used, ng, own, ok = [0] * K, [0] * K, {}, True
            for gk, members in gl:
                best = -1
                for w in range(K):
                    if used[w] + len(members) <= cw and (best < 0 or ng[w] < ng[best] or
                                                         (ng[w] == ng[best] and used[w] < used[best])):
                        best = w
                if best < 0:
                    ok = False
                    break
                ng[best] += 1
                used[best] += len(members)
                for cid in members:
                    own[cid] = (best, gk)
            if ok:
                return own
        raise AssertionError("the classes do not pack")

    def scans(self):
        """The steps s of a lean launch at which the owner of event s + 1's class looks ahead: s is decided (its
        class was not dead before it; the events of dead classes are skipped as runs, and the old full scan serves
        the event after a run) and event s + 1 is a create."""
        dead, out = set(), []
        for s in range(self.n - 1):
            if self.cls[s] in dead:
                continue
            if not self.is_del[s] and self.want[s][:4] == UNSCHED:
                dead.add(self.cls[s])
            if not self.is_del[s + 1]:
                out.append(s)
        return out


def run(c, keep, st, form="lean", wgs=4, evs=None, oev=None):
    """One engine run of the stream against the oracle; `form`: lean | report | general (the caller's delete
    stream in evs / oev)."""
    arr, n = c.t.typical()
    evs = st.events if evs is None else evs
    oev = c.oev(st) if oev is None else oev
    want, want_state, want_rep = O.run_events([c.onodes[i] for i in keep], c.otyp, oev, policy=O.POL_FGD,
                                              gpu_sel=O.SEL_FGD, threads=16 if len(keep) > 16 else 1,
                                              with_report=form == "report")
    eng = ksim.Engine(len(keep), 1, run_mode=MEMO, wgs_per_replica=wgs)
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
        rep = eng.reports(0) if form == "report" else None
    finally:
        eng.close()
    assert_same(res, want, state, want_state, keep)
    if form == "report":
        assert_reports(rep, want_rep)


def spread(c, n):
    """n nodes of every GPU count, evenly through the cluster."""
    tn = c.t.num_nodes
    return sorted({(k * tn) // n for k in range(n)})


def built(c, name, fn):
    key = "top2:" + name
    if key not in c.built:
        c.built[key] = fn()
    return c.built[key]


# ---- workgroups per replica

def case_wgs(c):
    st = Stream(c.rp, range(300))
    w = Walk(c, c.keep, st)
    sc = w.scans()
    for K in (1, 2, 3):
        own = w.owners(K)
        same = [s for s in sc if own[w.cls[s]][0] == own[w.cls[s + 1]][0]]
        assert len(same) == len(sc) if K == 1 else 0 < len(same) < len(sc), (K, len(same), len(sc))
    # one workgroup: the merged key comes from wave 0's own-group store and from the list wave's
    own = w.owners(1)
    d_steps = [s for s in sc if s > 0 and w.node[s - 1] >= 0]
    assert any(own[w.cls[s]][1] == own[w.cls[s + 1]][1] for s in d_steps)
    assert any(own[w.cls[s]][1] != own[w.cls[s + 1]][1] for s in d_steps)
    return c.keep, st


@pytest.mark.parametrize("wgs", [1, 2, 3])
def test_workgroups_per_replica(ctx, wgs):
    keep, st = built(ctx, "wgs", lambda: case_wgs(ctx))
    run(ctx, keep, st, wgs=wgs)


# ---- node counts

def case_tiny(c, n):
    """N of 2 and 5: share pods of one class packed until nothing takes them, then the rest of the trace.  The
    look-ahead class has two, one and no feasible node; d is its only feasible node (nothing left once it is
    excluded); its second key is 0."""
    keep = c.by[1][:n] if n == 2 else sorted(c.by[1][:3] + c.by[2][:2])
    share = [k for k in range(c.rp.n) if c.pod(k)["num"] == 1 and 200 <= c.pod(k)["milli"] <= 333
             and c.pod(k)["cpu"] <= 1000 and c.pod(k)["mem"] <= 4096]  # three or four to a GPU, and nothing else binds
    other = [k for k in range(c.rp.n) if c.pod(k)["num"] == 1 and 0 < c.pod(k)["milli"] < 200
             and c.req(k) != c.req(share[0])]
    st = Stream(c.rp, [share[0]] * (4 * n) + other[:6] + [share[0]] * 2 + other[6:40])
    w = Walk(c, keep, st)
    sc = [s for s in w.scans() if s > 0]
    nf = {len(w.ranking(s, w.cls[s + 1])) for s in sc}
    assert {0, 1, 2} <= nf, nf
    only_d = [s for s in sc if w.node[s - 1] >= 0 and [r[2] for r in w.ranking(s, w.cls[s + 1])] == [w.node[s - 1]]]
    assert only_d, "a step whose look-ahead class has d as its only feasible node"
    return keep, st


def case_nodes(c, n):
    keep = spread(c, n)
    assert len(keep) == n
    st = Stream(c.rp, range(400))
    w = Walk(c, keep, st)
    sc = w.scans()
    assert len(sc) > 300
    # the excluded column is spread over the scan's lanes and strides
    d = {w.rank[w.node[s - 1]] for s in sc if s > 0 and w.node[s - 1] >= 0}
    assert len(d) > 20 and len({x % 64 for x in d}) > 10
    if n > 2 * L:
        assert any(x >= 2 * L for x in d), "a changed node in a lane's third key"
    return keep, st


@pytest.mark.parametrize("n", [2, 5])
def test_tiny_clusters(ctx, n):
    keep, st = built(ctx, "tiny%d" % n, lambda: case_tiny(ctx, n))
    run(ctx, keep, st, wgs=2)


@pytest.mark.parametrize("n", [63, 64, 65, L - 1, L, L + 1, 2 * L + 61])
def test_node_counts(ctx, n):
    keep, st = built(ctx, "n%d" % n, lambda: case_nodes(ctx, n))
    run(ctx, keep, st, wgs=3)


# ---- the changed node and the look-ahead class's top-2

def case_d_in_top2(c):
    """The first 400 events on the 64-node cluster hold steps whose d, for the look-ahead class: was the best
    node and still is; was the best node and is no longer feasible; was the second-best node."""
    st = Stream(c.rp, range(400))
    w = Walk(c, c.keep, st)
    best_stays = best_gone = second = 0
    for s in w.scans():
        if s == 0 or w.node[s - 1] < 0:
            continue
        d, cn = w.node[s - 1], w.cls[s + 1]
        before = [r[2] for r in w.ranking(s - 1, cn)[:2]]  # before event s - 1 changed d
        after = [r[2] for r in w.ranking(s, cn)]
        if len(before) == 2 and before[0] == d:
            best_stays += after[:1] == [d]
            best_gone += d not in after
        second += len(before) == 2 and before[1] == d
    assert best_stays and best_gone and second, (best_stays, best_gone, second)
    return c.keep, st


def test_changed_node_in_top2(ctx):
    keep, st = built(ctx, "dtop2", lambda: case_d_in_top2(ctx))
    run(ctx, keep, st, wgs=2)


def test_changed_node_stays_best(ctx):
    # share pods packed on one node (test_gpu_memo_chain's case): d is the class's best before and after
    keep, st, _ = ctx.case("eight")
    w = Walk(ctx, keep, st)
    assert any(s > 0 and w.node[s - 1] >= 0 and w.node[s - 1] == w.node[s] == w.node[s + 1]
               and w.cls[s] == w.cls[s + 1] and w.want[s + 1][3] >= 2 for s in w.scans())
    run(ctx, keep, st, wgs=2)


# ---- where the look-ahead class lives

def test_next_class_placement(ctx):
    keep, st = built(ctx, "wgs", lambda: case_wgs(ctx))
    w = Walk(ctx, keep, st)
    own = w.owners(2)
    sc = [s for s in w.scans() if s > 0 and w.node[s - 1] >= 0]
    pairs = [(own[w.cls[s]], own[w.cls[s + 1]]) for s in sc]
    assert any(a == b for a, b in pairs), "in the step's own score group"
    assert any(a[0] == b[0] and a[1] != b[1] for a, b in pairs), "another group on the step's workgroup"
    assert any(a[0] != b[0] for a, b in pairs), "on another workgroup"
    run(ctx, keep, st, wgs=2)


# ---- special steps

@pytest.mark.parametrize("pos", [127, 128])
def test_dead_run_at_the_window_edge(ctx, pos):
    """test_gpu_memo_chain's dead-class stream: event pos - 1 is the first of a class no node can take (the
    look-ahead class dies at that step), pos and pos + 1 are skipped as one run (the old scan, for pos + 2),
    pos + 2 is decided without a changed node and looks ahead on the new path; with pos = 127 / 128 the steps
    126..129 look ahead across the window refill."""
    keep, st, _ = ctx.case("dead%d" % pos)
    w = Walk(ctx, keep, st)
    assert w.cls[pos - 1] == w.cls[pos] == w.cls[pos + 1] and w.cls[pos - 1] not in w.cls[:pos - 1]
    assert w.want[pos - 1][:4] == UNSCHED and any(w.want[j][0] >= 0 for j in range(pos + 2, w.n))
    sc = w.scans()
    assert pos - 1 in sc and pos + 2 in sc and pos not in sc and pos + 1 not in sc
    assert all(s in sc for s in (125, 126)) and st.n > 130
    run(ctx, keep, st, wgs=3)


def test_window_edge_lookahead(ctx):
    # no dead class near the edge: every step 126..129 looks ahead, with and without the owner changing
    keep, st = built(ctx, "wgs", lambda: case_wgs(ctx))
    w = Walk(ctx, keep, st)
    assert all(s in w.scans() and w.node[s - 1] >= 0 for s in (126, 127, 128, 129))
    own = w.owners(3)
    assert len({own[w.cls[s]][0] for s in (126, 127, 128, 129, 130)}) > 1
    run(ctx, keep, st, wgs=3)


# ---- deletes (the general instantiation): the next event is a delete, then a create follows

def case_deletes(c):
    sub = Stream(c.rp, range(250))
    evs, oev = helpers.delete_stream(c.t, sub, 250, 0.3, seed=7)
    w = Walk(c, c.keep, None, oev)
    pat = [i for i in range(1, w.n - 1) if w.is_del[i] and not w.is_del[i - 1] and not w.is_del[i + 1]]
    assert len(pat) > 20 and any(w.node[i] >= 0 and w.node[i - 1] >= 0 for i in pat)
    return c.keep, evs, oev


def test_deletes(ctx):
    keep, evs, oev = built(ctx, "del", lambda: case_deletes(ctx))
    run(ctx, keep, None, form="general", wgs=3, evs=evs, oev=oev)


# ---- once on each other instantiation

def test_report_rows(ctx):
    keep, st = built(ctx, "wgs", lambda: case_wgs(ctx))
    run(ctx, keep, st, form="report", wgs=3)


@pytest.mark.parametrize("form", ["stress", "general"])
def test_hand_over_delays(ctx, monkeypatch, form):
    monkeypatch.setenv("KSIM_TEST", "hdelay=7")  # every delay point on
    if form == "general":
        keep, evs, oev = built(ctx, "del", lambda: case_deletes(ctx))
        run(ctx, keep, None, form="general", wgs=3, evs=evs, oev=oev)
    else:
        keep, st = built(ctx, "wgs", lambda: case_wgs(ctx))
        run(ctx, keep, st, wgs=3)


def test_keys_in_hbm():
    t = ksim.Trace.openb("gpuspec33")
    rp = t.replay(seed=43)
    arr, n = t.typical()
    n_ev = 2500  # the stream must bring enough classes that their keys do not fit in LDS
    want, want_state, _ = O.run_events(helpers.oracle_nodes(t, rp), helpers.oracle_typical(t),
                                       helpers.oracle_events(t, rp, n_ev), policy=O.POL_FGD, gpu_sel=O.SEL_FGD,
                                       threads=16)
    eng = ksim.Engine(t.num_nodes, 1, run_mode=MEMO, wgs_per_replica=25)
    try:
        eng.set_nodes(0, rp.nodes)
        eng.set_typical(0, arr, n)
        eng.set_policy(0, "FGD")
        eng.load_events(0, rp.events, n_ev)
        eng.run()
        assert eng.last_run_kernels() == ["k_memo_hkeys"]
        res, state = eng.results(0), eng.nodes(0)
    finally:
        eng.close()
    assert_same(res, want, state, want_state, None)


def test_replicas_at_their_own_widths(ctx):
    # one launch, three replicas of the same stream at 1, 2 and 5 workgroups
    keep, st = built(ctx, "wgs", lambda: case_wgs(ctx))
    arr, n = ctx.t.typical()
    want, want_state = ctx.oracle(keep, st)
    widths = (1, 2, 5)
    eng = ksim.Engine(len(keep), len(widths), run_mode=MEMO)
    try:
        for r, k in enumerate(widths):
            eng.set_nodes(r, helpers.subset_nodes(ctx.rp, keep))
            eng.set_typical(r, arr, n)
            eng.set_policy(r, "FGD")
            eng.set_replica_wgs(r, k)
            eng.load_events(r, st.events, st.n)
        eng.run()
        assert eng.last_run_kernels()[0] == "k_memo"
        outs = [(eng.results(r), eng.nodes(r)) for r in range(len(widths))]
    finally:
        eng.close()
    for res, state in outs:
        assert_same(res, want, state, want_state, keep)
