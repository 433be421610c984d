"""What a descheduling plan costs at C5 size, unsharded and on in-process shard groups: the 100k-node cluster after the
first N events of its stream (FGD), then fragOnePod, fragMultiPod and cosSim planned at one ratio
- on the unsharded engine (Engine.last_deschedule_ms), and
- on in-process groups of `world` shards (ShardGroup.deschedule: every shard's part, then the merge on the device;
  engine 0's last_deschedule_ms spans both, the merge's share comes from KSIM_GROUP_TIMES=1, the engine's stderr line).
One warm-up plan, then the median of `repeats`.  The victim lists (node = the input index) must have the same sha256
in every setting: the script exits 1 otherwise.

Prints one JSON object.
Usage (GPU box): python3 scripts/shard_desched_cost.py [--events 5000] [--worlds 2 8] [--ratio 0.1] [--repeats 3]"""
import argparse
import hashlib
import json
import os
import re
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kubernetes-scheduler-simulator_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ksim  # noqa: E402
import ksim.shard as SH  # noqa: E402
from c5_shard_report_cost import cluster, stderr_to  # noqa: E402

PLANS = ["fragOnePod", "fragMultiPod", "cosSim"]


def digest(victims):
    return hashlib.sha256(b"".join(bytes(v) for v in victims)).hexdigest()


def plan_unsharded(e, plan, ratio):
    if plan == "cosSim":
        ms = e.deschedule_cossim(ratio)
        victims, budget = e.cos_victims(0)
    else:
        ms = e.deschedule(plan, ratio)
        victims, budget = e.victims(0)
    return ms, victims, budget


def plan_group(g, plan, ratio):
    """-> (engine 0's plan ms, the merge's ms, victims, budget, the shards' list lengths and bound counts)"""
    with tempfile.NamedTemporaryFile("r", suffix=".err") as f:
        os.environ["KSIM_GROUP_TIMES"] = "1"
        with stderr_to(f.name):
            ms = g.deschedule_cossim(ratio) if plan == "cosSim" else g.deschedule(plan, ratio)
        os.environ.pop("KSIM_GROUP_TIMES")
        m = re.search(r"merge ([0-9.]+)", f.read())
    victims, budget = g.cos_victims() if plan == "cosSim" else g.victims()
    parts, bounds = g.victim_parts(cos=plan == "cosSim")
    return ms, float(m.group(1)) if m else None, victims, budget, [len(p) for p in parts], bounds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=5000)
    ap.add_argument("--worlds", type=int, nargs="+", default=[2, 8])
    ap.add_argument("--ratio", type=float, default=0.1)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    t, rp, typ, n_ev = cluster(a.events)
    out = {"events": n_ev, "nodes": t.num_nodes, "ratio": a.ratio, "repeats": a.repeats, "unsharded": {}, "groups": []}
    want = {}
    e = ksim.Engine(t.num_nodes, 1)
    try:
        e.set_nodes(0, rp.nodes)
        e.set_typical(0, *typ)
        e.set_policy(0, "FGD")
        e.load_events(0, rp.events, n_ev)
        out["run_ms"] = e.run()
        for plan in PLANS:
            plan_unsharded(e, plan, a.ratio)
            ms = []
            for _ in range(a.repeats):
                m, victims, budget = plan_unsharded(e, plan, a.ratio)
                ms.append(m)
            want[plan] = digest(victims)
            out["unsharded"][plan] = {"ms": ms, "median_ms": statistics.median(ms), "victims": len(victims),
                                      "budget": budget, "sha256": want[plan]}
            print("unsharded %s: %s" % (plan, ms), file=sys.stderr, flush=True)
    finally:
        e.close()
    equal = True
    for world in a.worlds:
        g = SH.ShardGroup(rp.nodes, typ, world, policy="FGD")
        try:
            g.load_events(rp.events, n_ev)
            run_ms = g.run()
            for plan in PLANS:
                plan_group(g, plan, a.ratio)
                ms, merge = [], []
                for _ in range(a.repeats):
                    m, mm, victims, budget, part_n, bounds = plan_group(g, plan, a.ratio)
                    ms.append(m)
                    merge.append(mm)
                sha = digest(victims)
                equal = equal and sha == want[plan]
                out["groups"].append({"world": world, "plan": plan, "run_ms": run_ms, "ms": ms, "merge_ms": merge,
                                      "median_ms": statistics.median(ms),
                                      "median_merge_ms": statistics.median(merge) if None not in merge else None,
                                      "victims": len(victims), "budget": budget, "part_n": part_n, "bound": bounds,
                                      "shards_with_bound_pods": sum(1 for b in bounds if b > 0), "sha256": sha,
                                      "equals_unsharded": sha == want[plan]})
                print("world %d %s: %s merge %s" % (world, plan, ms, merge), file=sys.stderr, flush=True)
        finally:
            g.close()
    out["all_equal"] = equal
    print(json.dumps(out))
    return 0 if equal else 1


if __name__ == "__main__":
    sys.exit(main())
