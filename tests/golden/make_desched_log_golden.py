"""Writes tests/golden/desched_log_golden.json: what the REFERENCE's own log parser makes of our
descheduling logs.

Pipeline, run where the reference tree exists (it never travels with the repository):
  1. tests/desched_log_case.py oracle_log -> the `simon apply` log of tests/log_case.py's cluster (243
     nodes, 3000 events, FGD) followed by a descheduling stage, for cosSim at the reference's bars and for
     fragOnePod, both at ratio 0.1, written by ksim.analysis.write_desched_log from the oracle's reports,
     power reports and the cluster at the three stage ends;
  2. the reference's scripts/analysis.py log_to_csv on a directory holding that log -> analysis.csv, the
     per-experiment summary row with its *_init_schedule / *_post_eviction / *_post_deschedule columns.
The JSON holds only data: per policy the log's sha256, its line count, the victims and the summary row the
reference's script produced.
Run:  python tests/golden/make_desched_log_golden.py <path of the reference tree>
"""
import hashlib
import importlib.util
import json
import sys
import tempfile
from pathlib import Path

HERE = Path(__file__).resolve().parent
REPO = HERE.parents[1]
sys.path[:0] = [str(REPO / "kubernetes-scheduler-simulator_amd"), str(REPO / "oracle"), str(REPO / "tests")]



def main():
    import pandas as pd
    import desched_log_case as case
    import log_case
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    spec = importlib.util.spec_from_file_location("ref_analysis", Path(sys.argv[1]) / "scripts" / "analysis.py")
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    out = {"case": dict(trace=log_case.TRACE, seed=log_case.SEED, tune=log_case.TUNE, stride=log_case.STRIDE,
                        n_events=log_case.N_EVENTS, sched=case.SCHED, ratio=case.RATIO), "policies": {}}
    for policy in case.POLICIES:
        with tempfile.TemporaryDirectory() as td:
            logdir = Path(td) / "logs"
            logdir.mkdir()
            log = logdir / ("log-cc_tn1.3_ts42_dr0.1_dp%s.yaml-sc_fgd.yaml.log" % policy)
            victims, budget = case.oracle_log(log, policy)
            sha = hashlib.sha256(log.read_bytes()).hexdigest()
            ref.log_to_csv(logdir, Path(td) / "analysis.csv")
            row = pd.read_csv(Path(td) / "analysis.csv").iloc[0].to_dict()
            out["policies"][policy] = {"log_sha256": sha, "log_lines": sum(1 for _ in open(log)),
                                       "victims": [v["event"] for v in victims], "budget": budget,
                                       "row": {k: (float(v) if not isinstance(v, str) else v) for k, v in row.items()}}
            print(policy, sha[:16], len(victims), budget, len(row))
    with open(HERE / "desched_log_golden.json", "w") as f:
        json.dump(out, f, sort_keys=True)
    print("wrote", HERE / "desched_log_golden.json")


if __name__ == "__main__":
    main()
