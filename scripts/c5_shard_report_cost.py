"""What the per-event cluster report costs a node-sharded run at C5 size: the 100k-node cluster, the first N events,
an in-process shard group of `world` shards on one device, a warm-up run and then a timed run with the report off and
one with it on, per world and policy.  Beside it the unsharded engine's report time for the same events.

--lib-b PATH: a second build of the library (e.g. the parent commit's).  Each (world, policy) is then also run,
report off, by child processes alternating between that build and this one (B A B A, a fresh process each, so both
builds run under the same conditions), and the two builds' report-off times and each build's own process-to-process
spread come from one visit to the device.

Prints one JSON object; the merge's share of the report comes from KSIM_GROUP_TIMES=1 (the engine's stderr line).
Usage (GPU box): python3 scripts/c5_shard_report_cost.py [--events 5000] [--worlds 2 8] [--policies FGD BestFit]
                 [--repeats 3] [--lib-b PATH]"""
import argparse
import contextlib
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kubernetes-scheduler-simulator_amd"))

import ksim  # noqa: E402
import ksim.shard as SH  # noqa: E402


@contextlib.contextmanager
def stderr_to(path):
    """The process's stderr (the engine's C stdio included) into a file."""
    sys.stderr.flush()
    saved = os.dup(2)
    with open(path, "w") as f:
        os.dup2(f.fileno(), 2)
        try:
            yield
        finally:
            os.dup2(saved, 2)
            os.close(saved)


def cluster(events):
    t = ksim.Trace.openb("default").synthetic(100_000, 1_000_000, seed=0)
    rp = t.replay(seed=1, tune_ratio=0.0, shuffle=False)
    return t, rp, t.typical(), events


def group_off(rp, typ, n_ev, world, policy, repeats):
    """Report off: a warm-up run, then `repeats` timed runs (device ms each) and the kernels."""
    g = SH.ShardGroup(rp.nodes, typ, world, policy=policy)
    try:
        g.load_events(rp.events, n_ev)
        g.run()
        ms = [g.run() for _ in range(repeats)]
        return ms, g.engines[0].last_run_kernels()
    finally:
        g.close()


def group_on(t, rp, typ, n_ev, world, policy, repeats):
    g = SH.ShardGroup(rp.nodes, typ, world, policy=policy, report=True, power_model=t.power_model())
    try:
        g.load_events(rp.events, n_ev)
        g.run()
        ms, rms, merge = [], [], []
        for _ in range(repeats):
            with tempfile.NamedTemporaryFile("r", suffix=".err") as f:
                os.environ["KSIM_GROUP_TIMES"] = "1"
                with stderr_to(f.name):
                    ms.append(g.run())
                os.environ.pop("KSIM_GROUP_TIMES")
                m = re.search(r"merge ([0-9.]+)", f.read())
            rms.append(g.engines[0].last_report_ms())
            merge.append(float(m.group(1)) if m else None)
        last = g.reports()[-1]
        return ms, rms, merge, g.engines[0].last_run_kernels(), last
    finally:
        g.close()


def unsharded_report(t, rp, typ, n_ev, policy):
    e = ksim.Engine(t.num_nodes, 1)
    try:
        e.set_nodes(0, rp.nodes)
        e.set_typical(0, *typ)
        e.set_policy(0, policy)
        e.set_power_model(0, t.power_model())
        e.set_report(True)
        e.load_events(0, rp.events, n_ev)
        e.run()
        ms = e.run()
        return ms, e.last_report_ms(), e.last_run_kernels(), e.reports(0)[-1]
    finally:
        e.close()


def child_main(a):
    """--child: one (world, policy), report off, on the library KSIM_LIB_PATH names; prints the device ms list."""
    t, rp, typ, n_ev = cluster(a.events)
    ms, kernels = group_off(rp, typ, n_ev, a.worlds[0], a.policies[0], a.repeats)
    print(json.dumps({"ms": ms, "kernels": kernels}))


def run_child(lib, a, world, policy):
    env = dict(os.environ, KSIM_LIB_PATH=lib)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--events", str(a.events), "--worlds",
                        str(world), "--policies", policy, "--repeats", str(a.repeats)], env=env,
                       stdout=subprocess.PIPE, universal_newlines=True, timeout=600, check=True)
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=5000)
    ap.add_argument("--worlds", type=int, nargs="+", default=[2, 8])
    ap.add_argument("--policies", nargs="+", default=["FGD", "BestFit"])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--lib-b", default=None)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child_main(a)
    t, rp, typ, n_ev = cluster(a.events)
    out = {"events": n_ev, "nodes": t.num_nodes, "repeats": a.repeats, "configs": [], "unsharded": []}
    for policy in a.policies:
        ms, rms, kernels, last = unsharded_report(t, rp, typ, n_ev, policy)
        out["unsharded"].append({"policy": policy, "kernels": kernels, "device_ms": ms, "report_ms": rms})
        for world in a.worlds:
            c = {"world": world, "policy": policy}
            if a.lib_b:  # B A B A: the other build and this one, report off, a fresh child process each
                c["ab_off"] = [{"lib": name, **run_child(lib, a, world, policy)}
                               for name, lib in (("b", a.lib_b), ("a", ksim.LIB_PATH)) * 2]
            c["off_ms"], c["off_kernels"] = group_off(rp, typ, n_ev, world, policy, a.repeats)
            c["on_ms"], c["report_ms"], c["merge_ms"], c["on_kernels"], glast = group_on(t, rp, typ, n_ev, world,
                                                                                         policy, a.repeats)
            c["last_report_equals_unsharded"] = glast == last
            out["configs"].append(c)
            print("world %d %s: off %s on %s report %s merge %s" % (world, policy, c["off_ms"], c["on_ms"],
                                                                    c["report_ms"], c["merge_ms"]),
                  file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
