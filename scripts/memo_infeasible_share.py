#!/usr/bin/env python3
"""On how many pod steps can k_memo's owner publish before its critical F?  A CPU count, no GPU needed.

The step's winner is max(ex, fresh); fresh is 0 when Filter of the step's class refuses d, the node the previous
decided step changed, and then the owner publishes ex at once (ksim_memo.hpp, `early`).  For a trace and seeds this
replays FGD on the C oracle (tune 1.3, shuffled, as bench.py's C2 and C4 do), rebuilds the node states from its
results and prints, per seed: events, live steps (class not yet dead), steps on which d is infeasible for the step's
class with the share, the share of steps d wins, the reasons, and the cross-check of the Filter restatement
(tests/early_share.py) against the oracle's n_feasible on every 40th step.

  python scripts/memo_infeasible_share.py                     # openb default, seeds 42-51 (C2)
  python scripts/memo_infeasible_share.py --trace gpushare100 --seeds 42 43
  python scripts/memo_infeasible_share.py --general --limit 4000 --seeds 42   # the KSIM_PROFILE=2 trace's steps
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("kubernetes-scheduler-simulator_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))

import early_share  # noqa: E402
import helpers  # noqa: E402
import ksim  # noqa: E402
import pyoracle as O  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--trace", default="default", help="openb pod list (default, gpushare100, gpuspec33, ...)")
    ap.add_argument("--seeds", type=int, nargs="*", default=list(range(42, 52)))
    ap.add_argument("--tune", type=float, default=1.3)
    ap.add_argument("--general", action="store_true",
                    help="count as the general kernel steps (no dead-class skip: every event decided, no d after an "
                         "event that bound nothing)")
    ap.add_argument("--limit", type=int, default=None, help="only the first LIMIT events")
    ap.add_argument("--threads", type=int, default=min(16, os.cpu_count() or 1))
    args = ap.parse_args()
    t = ksim.Trace.openb(args.trace)
    otyp = helpers.oracle_typical(t)
    print("| seed | events | live steps | d infeasible for the step's class | d wins | no d | cpu / mem / gpu / pods | "
          "n_feasible checks (mismatches) |")
    print("|---|---|---|---|---|---|---|---|")
    bad = 0
    for seed in args.seeds:
        rp = t.replay(seed=seed, tune_ratio=args.tune, shuffle=True)
        onodes, oev = helpers.oracle_nodes(t, rp), helpers.oracle_events(t, rp)
        res, _, _ = O.run_events(onodes, otyp, oev, policy=O.POL_FGD, gpu_sel=O.SEL_FGD, threads=args.threads)
        c = early_share.count(onodes, oev, res, skip=not args.general, limit=args.limit)
        live = max(c["live"], 1)
        rs = c["reasons"]
        print("| %d | %d | %d | %d = %.1f %% | %.1f %% | %d | %d / %d / %d / %d | %d (%d) |"
              % (seed, len(c["flags"]), c["live"], c["early"], 100.0 * c["early"] / live, 100.0 * c["d_wins"] / live,
                 c["nod"], rs.get("cpu", 0), rs.get("mem", 0), rs.get("gpu", 0), rs.get("pods", 0), c["checks"],
                 c["mismatches"]))
        bad += c["mismatches"]
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
