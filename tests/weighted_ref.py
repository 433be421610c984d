"""A Python reference cycle for weighted combinations of score plugins (not collected; tests/test_weighted_ref_cpu.py
proves it against the C oracle where the oracle reaches, the GPU tests compare k_wsum with it).

The C oracle's replay (orc_run_events) knows single plugins and the PWR + FGD pair only.  This module holds the
per-node state itself and restates what surrounds the plugins' Score functions:
  Filter           tests/early_share.py's restatement (fit.go:230-290, open_gpu_share.go:81-118)
  NormalizeScore   BestFit's (plugin_utils.go:48-74: 0 for every node when max == min) and PWR's
                   (pwr_score.go:104-141: 100 then)
  the range check, the weights, the sum   framework.go:686-704, generic_scheduler.go:511-519
  selectHost       max total, ties to the smallest node name (generic_scheduler.go:187-212)
  Reserve          best / worst restated (open_gpu_share.go:285-323); the FGD / PWR / DotProduct selectors take the
                   mask the oracle's leaf call returns on the winner
  Bind, delete     simulator.go:416-422
Every raw score comes from the oracle's leaf functions through pyoracle: orc_fgd_score, orc_best_fit_score,
orc_dot_product_score_cfg, orc_packing_score, orc_clustering_score, orc_pwr_score.  Score errors: BestFit's -1,
GpuPacking's allocation failure, GpuClustering's tag -2, PWR's missing energy model.  (The plugins' "node not
accessible" error cannot occur on a feasible node of these streams: a pod that names GPU models asks for GPUs, and
Filter then checks the model.)
"""
import ctypes as C

import early_share
import pyoracle as O

PLUGINS = ["FGD", "BestFit", "DotProd", "GpuPacking", "GpuClustering", "PWR"]
MILLI = 1000


def pod_tag(e):
    """GetGpuAffinityFromPodAnnotation (open-gpu-share/utils/pod.go:111-123); -2 where the reference panics."""
    if e["num"] == 0:
        return -1
    if e["num"] == 1 and e["milli"] < MILLI:
        return 0
    if e["milli"] == MILLI and 1 <= e["num"] <= 8:
        return e["num"]
    return -2


def normalize_bestfit(scores):
    lo, hi = min(scores), max(scores)
    return [0 if hi == lo else (s - lo) * 100 // (hi - lo) for s in scores]


def normalize_pwr(scores):
    lo, hi = min(scores), max(scores)
    return [100 if hi == lo else (s - lo) * 100 // (hi - lo) for s in scores]


class Cluster:
    def __init__(self, onodes, otypical, dim_ext=O.DIM_MERGE, norm=O.NORM_MAX):
        self.nodes = onodes
        self.st = early_share.node_states(onodes)
        self.tags = [[0] * 9 for _ in onodes]
        self.tp = O.typical(otypical)
        self.dim_ext, self.norm = dim_ext, norm
        # a node's raw scores change only when the node does: memoised by (plugin, node, its version, pod class)
        self.ver = [0] * len(onodes)
        self.memo = {}

    def node_res(self, i):
        d, st = self.nodes[i], self.st[i]
        return O.node_res(st[0], st[3], d["gpu"], d.get("model", ""), d["cpu"], d.get("cpu_model", ""))

    def raw(self, name, i, e):
        """(raw score, GPU mask of the plugin's own selector, Score error) of plugin `name` on node i."""
        key = (name, i, self.ver[i], early_share.class_of(e))
        if key not in self.memo:
            self.memo[key] = self._raw(name, i, e)
        return self.memo[key]

    def _raw(self, name, i, e):
        nr, pr = self.node_res(i), O.pod_res(e.get("cpu_nz", e["cpu"]), e["milli"], e["num"], e.get("type", ""))
        if name == "FGD":
            s, m = O.fgd_score(nr, pr, self.tp)
            return s, m, 0
        if name == "BestFit":
            s = O.lib().orc_best_fit_score(C.byref(nr), C.byref(pr))
            return s, 0, int(s == -1)
        if name == "DotProd":
            s, m = O.dot_product_score(nr, pr, self.dim_ext, self.norm)
            return s, m, 0
        if name == "GpuPacking":
            if e["milli"] <= 0:
                return 0, 0, 0
            er = C.c_int(0)
            s = O.lib().orc_packing_score(C.byref(nr), C.byref(pr), C.byref(er))
            return (0 if er.value else s), 0, er.value
        if name == "GpuClustering":
            tag = pod_tag(e)
            if tag == -2:
                return 0, 0, 1
            return O.lib().orc_clustering_score(C.byref(nr), C.byref(pr), tag, (C.c_int32 * 9)(*self.tags[i])), 0, 0
        if name == "PWR":
            s, m, er = O.pwr_score(nr, pr)
            return (0 if er else s), m, er
        raise KeyError(name)

    def reserve(self, i, e, gpusel):
        """allocateGpuId (open_gpu_share.go:252-283) on node i: the mask, or <= 0 when Reserve fails."""
        if e["milli"] <= 0:
            return 0
        gl, milli, num = self.st[i][3], e["milli"], e["num"]
        if milli < MILLI and num > 1:
            return -1  # open_gpu_share.go:266-268: the reference panics on several shared GPUs
        if gpusel in ("FGD", "PWR", "DotProd"):
            return self.raw(gpusel, i, e)[1]
        if milli < MILLI:
            fit = [g for g in range(len(gl)) if gl[g] >= milli]
            if not fit:
                return -1
            pick = min(fit, key=lambda g: gl[g]) if gpusel == "best" else max(fit, key=lambda g: gl[g])
            return 1 << pick
        free = [g for g in range(len(gl)) if gl[g] == MILLI][:num]  # AllocateExclusiveGpuId (resource.go:383-403)
        return sum(1 << g for g in free) if len(free) == num else -1

    def bind(self, i, e, mask, sign):
        self.ver[i] += 1
        early_share._bind(self.st[i], e, mask, sign)
        if pod_tag(e) >= 0:
            self.tags[i][pod_tag(e)] += sign

    def totals(self, feas, e, weights):
        """(per feasible node total, any error) under `weights` ({plugin: weight})."""
        tot, anyerr = [0] * len(feas), False
        for name in PLUGINS:
            w = weights.get(name, 0)
            if w <= 0:
                continue
            rs = [self.raw(name, i, e) for i in feas]
            anyerr = anyerr or any(r[2] for r in rs)
            sc = [r[0] for r in rs]
            if name == "BestFit":
                sc = normalize_bestfit(sc)
            if name == "PWR":
                sc = normalize_pwr(sc)
            anyerr = anyerr or any(s < 0 or s > 100 for s in sc)
            tot = [t + w * s for t, s in zip(tot, sc)]
        return tot, anyerr

    def select_host(self, feas, tot):
        best = 0
        for k in range(1, len(feas)):
            if tot[k] > tot[best] or (tot[k] == tot[best] and self.nodes[feas[k]]["name"] < self.nodes[feas[best]]["name"]):
                best = k
        return best


def run(onodes, otypical, oevents, weights, gpusel="best", dim_ext=O.DIM_MERGE, norm=O.NORM_MAX, visit=None):
    """-> (results [(node, gpu_mask, score, n_feasible, status)], final state [(cpu_left, mem_left, pods, gl[8])]).
    visit(cluster, step, event, feasible, winner index into feasible): called at every step with two or more
    feasible nodes that was decided without an error, before the Bind."""
    cl = Cluster(onodes, otypical, dim_ext, norm)
    res = []
    for step, e in enumerate(oevents):
        if e.get("delete"):
            c = res[e["ref"]]
            if c[0] >= 0 and c[4] == 0:
                cl.bind(c[0], oevents[e["ref"]], c[1], -1)
                res.append((c[0], c[1], 0, 0, 3))
            else:
                res.append((-1, 0, 0, 0, 3))
            continue
        feas = [i for i in range(len(onodes)) if early_share.filter_reason(cl.st[i], e) is None]
        nf = len(feas)
        if nf == 0:
            res.append((-1, 0, 0, 0, 1))
            continue
        if nf == 1:
            win, score = feas[0], 0  # generic_scheduler.go:158-164
        else:
            tot, anyerr = cl.totals(feas, e, weights)
            if anyerr:
                res.append((-1, 0, 0, nf, 2))
                continue
            k = cl.select_host(feas, tot)
            if visit:
                visit(cl, step, e, feas, k)
            win, score = feas[k], tot[k]
        mask = cl.reserve(win, e, gpusel)
        if e["milli"] > 0 and mask <= 0:
            res.append((-1, 0, 0, nf, 2))
            continue
        cl.bind(win, e, mask, +1)
        res.append((win, mask, score, nf, 0))
    state = [(st[0], st[1], onodes[i].get("pods", 1001) - st[2], st[3] + [0] * (8 - len(st[3]))) for i, st in enumerate(cl.st)]
    return res, state


def divergence(onodes, otypical, oevents, weights, gpusel="best", dim_ext=O.DIM_MERGE, norm=O.NORM_MAX):
    """Of the steps with two or more feasible nodes (decided without error): how many, and how many choose a node
    that differs from the choice EACH participating plugin would make alone on the same state."""
    cnt = [0, 0]
    names = [n for n in PLUGINS if weights.get(n, 0) > 0]

    def visit(cl, step, e, feas, k):
        cnt[0] += 1
        differs = True
        for n in names:
            tot, _ = cl.totals(feas, e, {n: 1000})
            differs = differs and cl.select_host(feas, tot) != k
        cnt[1] += int(differs)

    res, state = run(onodes, otypical, oevents, weights, gpusel, dim_ext, norm, visit=visit)
    return cnt[0], cnt[1], res, state
