"""What PWR and PWR+FGD cost on a node-sharded cluster at C5 size: the 100k-node cluster, the first N events of its
stream, each policy
- on the unsharded engine (Engine.run), and
- on in-process groups of `world` shards (ShardGroup.run), once on the persistent group launch (k_replay_group) and
  once on the per-pod path with its two exchange rounds per pod (KSIM_VARIANT=shard_replay=0: the path a group with
  delete events takes); DESIGN.md "PWR on shards".
One warm-up run, then the median of `repeats` (device ms of the whole run, and microseconds per pod).  The merged
results must have the same sha256 in every setting of a policy: the script exits 1 otherwise.

Prints one JSON object and writes it to --out (default profiles/r16/shard_pwr/cost.json).
Usage (GPU box): python3 scripts/shard_pwr_cost.py [--events 5000] [--worlds 2 8] [--repeats 3]"""
import argparse
import hashlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kubernetes-scheduler-simulator_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ksim  # noqa: E402
import ksim.shard as SH  # noqa: E402
from c5_shard_report_cost import cluster  # noqa: E402

POLICIES = ["PWR", "PWR 500 FGD 500"]


def digest(results):
    return hashlib.sha256(repr([tuple(r) for r in results]).encode()).hexdigest()


def timed(run, repeats):
    run()
    return [run() for _ in range(repeats)]


def record(ms, n_ev, results, kernels, **kw):
    med = statistics.median(ms)
    out = {"ms": ms, "median_ms": med, "us_per_pod": med * 1e3 / n_ev, "kernels": kernels, "sha256": digest(results)}
    out.update(kw)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=5000)
    ap.add_argument("--worlds", type=int, nargs="+", default=[2, 8])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16", "shard_pwr", "cost.json"))
    a = ap.parse_args()
    t, rp, typ, n_ev = cluster(a.events)
    pm = t.power_model()
    out = {"events": n_ev, "nodes": t.num_nodes, "repeats": a.repeats, "policies": {}}
    equal = True
    for policy in POLICIES:
        rec = {"groups": []}
        e = ksim.Engine(t.num_nodes, 1)
        try:
            e.set_nodes(0, rp.nodes)
            e.set_typical(0, *typ)
            e.set_policy(0, policy)
            e.set_power_model(0, pm)
            e.load_events(0, rp.events, n_ev)
            ms = timed(e.run, a.repeats)
            rec["unsharded"] = record(ms, n_ev, e.results(0), e.last_run_kernels(), wgs=e.last_run_wgs())
        finally:
            e.close()
        want = rec["unsharded"]["sha256"]
        print("%s unsharded: %s" % (policy, ms), file=sys.stderr, flush=True)
        for world, variant in [(w, v) for w in a.worlds for v in ("", "shard_replay=0")]:
            os.environ["KSIM_VARIANT"] = variant
            g = SH.ShardGroup(rp.nodes, typ, world, policy=policy, power_model=pm)
            try:
                g.load_events(rp.events, n_ev)
                ms = timed(g.run, a.repeats)
                r = record(ms, n_ev, g.results(), g.engines[0].last_run_kernels(), world=world, variant=variant,
                           wgs=g.engines[0].last_run_wgs())
            finally:
                g.close()
                os.environ.pop("KSIM_VARIANT")
            r["equals_unsharded"] = r["sha256"] == want
            equal = equal and r["equals_unsharded"]
            rec["groups"].append(r)
            print("%s world %d %s: %s" % (policy, world, variant or "group launch", ms), file=sys.stderr, flush=True)
        out["policies"][policy] = rec
    out["all_equal"] = equal
    text = json.dumps(out, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(json.dumps(out))
    return 0 if equal else 1


if __name__ == "__main__":
    sys.exit(main())
