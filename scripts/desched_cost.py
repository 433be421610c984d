"""What a descheduling plan costs on the C2 job, and whether two builds of the library plan alike and as fast: the
openb default trace, all nodes, seeds 42..51 as ten replicas, FGD (tune 1.3, shuffled), run once; then each of
fragOnePod, fragMultiPod and cosSim (the reference's bars) is planned at ratio 0.3: a warm-up plan, then `repeats`
timed plans whose device time is ksim_engine_last_deschedule_ms.

Every measurement is a fresh child process (the library is KSIM_LIB_PATH's).  Without --lib-b the in-tree build is
measured `--alternations` times.  --lib-b PATH: a second build (e.g. the parent commit's); the children alternate
B A B A ..., so both builds run under the same conditions in one visit to the device.  Per policy:
- figure of a process: the median of its timed plans; median and spread (max - min) of a build: over its processes;
- pass: the median of this build is not above the other's by more than the other's own spread;
- same output: the sha256 of every replica's victim array and budget, equal in every process of both builds.

Prints one JSON object (raw lists, medians, spreads, verdicts); exit status 1 when a verdict fails.
Usage (GPU box): python3 scripts/desched_cost.py [--lib-b PATH] [--alternations 5] [--repeats 3] [--ratio 0.3]"""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kubernetes-scheduler-simulator_amd"))

import ksim  # noqa: E402

POLICIES = ["fragOnePod", "fragMultiPod", "cosSim"]
SEEDS = list(range(42, 52))


def c2_engine():
    t = ksim.Trace.openb("default")
    arr, n = t.typical()
    eng = ksim.Engine(t.num_nodes, len(SEEDS))
    for r, s in enumerate(SEEDS):
        rp = t.replay(seed=s, tune_ratio=1.3, shuffle=True)
        eng.set_nodes(r, rp.nodes)
        eng.set_typical(r, arr, n)
        eng.set_policy(r, "FGD")
        eng.load_events(r, rp.events, rp.n)
    return eng


def plan(eng, policy, ratio):
    return eng.deschedule_cossim(ratio) if policy == "cosSim" else eng.deschedule(policy, ratio)


def digest(eng, policy):
    h = hashlib.sha256()
    n_victims = 0
    for r in range(len(SEEDS)):
        victims, budget = eng.cos_victims(r) if policy == "cosSim" else eng.victims(r)
        h.update(b"".join(bytes(v) for v in victims))
        h.update(b"%d;%d;" % (len(victims), budget))
        n_victims += len(victims)
    return h.hexdigest(), n_victims


def child_main(a):
    eng = c2_engine()
    run_ms = eng.run()
    out = {"lib": ksim.LIB_PATH, "build_id": ksim.build_id(), "run_ms": run_ms, "ms": {}, "sha256": {}, "victims": {}}
    for policy in POLICIES:
        plan(eng, policy, a.ratio)  # warm-up
        out["ms"][policy] = [plan(eng, policy, a.ratio) for _ in range(a.repeats)]
        out["sha256"][policy], out["victims"][policy] = digest(eng, policy)
    eng.close()
    print(json.dumps(out))


def run_child(lib, a):
    env = dict(os.environ, KSIM_LIB_PATH=lib)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--repeats", str(a.repeats), "--ratio",
                        repr(a.ratio)], env=env, stdout=subprocess.PIPE, universal_newlines=True, timeout=300, check=True)
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib-b", default=None)
    ap.add_argument("--alternations", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--ratio", type=float, default=0.3)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child_main(a)
    libs = ([("b", os.path.abspath(a.lib_b))] if a.lib_b else []) + [("a", ksim.LIB_PATH)]
    runs = []
    for i in range(a.alternations):
        for name, lib in libs:
            runs.append(dict(name=name, **run_child(lib, a)))
            print("%s %d: %s" % (name, i, {p: ["%.4f" % x for x in runs[-1]["ms"][p]] for p in POLICIES}),
                  file=sys.stderr, flush=True)
    out = {"job": "C2: openb default, all nodes, seeds 42..51, FGD, tune 1.3, shuffled; ratio %g" % a.ratio,
           "alternations": a.alternations, "repeats": a.repeats, "runs": runs, "policies": {}, "ok": True}
    for p in POLICIES:
        c = {"same_output": len({r["sha256"][p] for r in runs}) == 1, "victims": runs[0]["victims"][p]}
        for name, _ in libs:
            figs = [statistics.median(r["ms"][p]) for r in runs if r["name"] == name]
            c[name] = {"process_ms": figs, "median_ms": statistics.median(figs), "spread_ms": max(figs) - min(figs)}
        if a.lib_b:
            c["pass"] = c["a"]["median_ms"] <= c["b"]["median_ms"] + c["b"]["spread_ms"]
        out["policies"][p] = c
        out["ok"] = out["ok"] and c["same_output"] and c.get("pass", True)
    print(json.dumps(out))
    return 0 if out["ok"] else 1


if __name__ == "__main__":
    sys.exit(main())
