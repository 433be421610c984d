"""The Python reference cycle of tests/weighted_ref.py, proved against the C oracle where the oracle reaches, and the
mixtures' streams shown to exercise their combinations (no GPU needed).

Leg A's inputs (tests/wsum_cases.py: the first 400 events of openb default, seed 42, on the 173-node subset, and the
create / delete stream): with a single plugin at weight 1000, and with the four PWR + FGD pairs, the reference equals
O.run_events row for row and in the final state.

Per mixture of leg B: among the steps with two or more feasible nodes, at least 10 % choose a node that differs from
the choice each participating plugin would make alone on the same state.  Leg B's stream (tests/wsum_cases.py
mix_stream: 400 openb events on 135 nodes -- 200 creations, a deletion of two of every three of them, 67 more
creations) has 267 such steps, and the reference counts FGD 700 BestFit 300 10.9 %, BestFit 500 PWR 500 29.2 %,
DotProd 500 GpuPacking 500 14.2 %, FGD 400 GpuClustering 300 PWR 300 15.7 %, all six 14.6 %, BestFit 1 FGD 50000 59.2 %.
The deletions are what makes DotProd 500 GpuPacking 500 reach the bar: on create-only openb streams (five traces, two
seeds, subsets of 96 - 173 nodes by stride and by GPU count, 300 and 400 events, every dimExtMethod / normMethod) that
pair stayed at 0 - 2 %, because GpuPacking's term dominates, keeps the cluster packed with one partly used node at a
time, and the pair then chooses what GpuPacking alone would.
"""
import pytest

import pyoracle as O
import weighted_ref
import wsum_cases as W

DIM = {"merge": O.DIM_MERGE, "share": O.DIM_SHARE}
NORM = {"max": O.NORM_MAX, "node": O.NORM_NODE}


def same(res, want, state, want_state):
    bad = [i for i, (a, b) in enumerate(zip(res, want)) if tuple(a) != tuple(b)]
    assert len(res) == len(want) and not bad, "first mismatch at event %d: reference %s oracle %s" % (
        bad[0], res[bad[0]], want[bad[0]])
    assert [(c, m, p, list(g)) for c, m, p, g in state] == [(c, m, p, list(g)) for c, m, p, g in want_state]


@pytest.mark.parametrize("stream", ["create", "delete"])
@pytest.mark.parametrize("name", sorted(W.SINGLES))
def test_single_plugin_equals_oracle(name, stream):
    pol, osel, sel, dim_ext, norm = W.SINGLES[name]
    onodes, otyp, oev = W.oracle_inputs(W.keep_a(), W.N_EV)
    if stream == "delete":
        oev = W.delete_stream(W.keep_a())[1]
    want, want_state, _ = O.run_events(onodes, otyp, oev, policy=pol, gpu_sel=osel, threads=16, dim_ext=DIM[dim_ext],
                                       norm=NORM[norm])
    res, state = weighted_ref.run(onodes, otyp, oev, {name.split("-")[0]: 1000}, sel, DIM[dim_ext], NORM[norm])
    same(res, want, state, want_state)
    assert sum(1 for r in res if r[4] == 0) > 300
    if stream == "delete":
        assert sum(1 for r in res if r[4] == 3) == 50


@pytest.mark.parametrize("pair", W.PAIRS, ids=lambda p: "PWR%d-FGD%d" % p)
def test_pwr_fgd_pairs_equal_oracle(pair):
    onodes, otyp, oev = W.oracle_inputs(W.keep_a(), W.N_EV)
    want, want_state, _ = O.run_events(onodes, otyp, oev, policy=O.POL_PWR_FGD, gpu_sel=O.SEL_FGD, threads=16,
                                       w_pwr=pair[0], w_fgd=pair[1])
    res, state = weighted_ref.run(onodes, otyp, oev, {"PWR": pair[0], "FGD": pair[1]}, "FGD")
    same(res, want, state, want_state)


@pytest.mark.parametrize("name", sorted(W.MIXTURES))
def test_mixture_stream_exercises_the_combination(name):
    multi, differs, res, _ = W.reference(name)
    print("%s: %d of %d multi-feasible steps (%.1f %%) differ from every single plugin's choice" % (
        name, differs, multi, 100.0 * differs / max(1, multi)))
    assert multi >= 250 and all(r[4] in (0, 3) for r in res) and sum(r[4] == 3 for r in res) == 133
    assert differs >= 0.10 * multi
