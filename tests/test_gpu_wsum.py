"""GPU parity of the weighted combinations of score plugins (KSIM_POLICY_WEIGHTED, kernel k_wsum).

Leg A -- the new path against the C oracle, where the oracle reaches: every single plugin as {plugin: 1000} and the
PWR + FGD pairs forced onto k_wsum, row for row (node, mask, score, n_feasible, status) and in the final state, on the
first 400 events of openb default, seed 42, on the 173-node subset (tests/wsum_cases.py); one create / delete stream;
one run with the cluster report on, compared with the oracle's exact report rows as tests/test_gpu_report.py does.
Leg B -- true mixtures against the Python reference cycle of tests/weighted_ref.py (tests/test_weighted_ref_cpu.py
proves that reference against the oracle and counts how far each stream exercises its combination).
Every test needs a gfx950 device.
"""
import pytest

import ksim
import pyoracle as O
import wsum_cases as W
from test_gpu_report import assert_reports

pytestmark = pytest.mark.gpu

DIM = {"merge": O.DIM_MERGE, "share": O.DIM_SHARE}
NORM = {"max": O.NORM_MAX, "node": O.NORM_NODE}


def oracle_single(name, oev, with_report=False):
    pol, osel, _, dim_ext, norm = W.SINGLES[name]
    onodes, otyp, _ = W.oracle_inputs(W.keep_a(), W.N_EV)
    return O.run_events(onodes, otyp, oev, policy=pol, gpu_sel=osel, threads=16, dim_ext=DIM[dim_ext], norm=NORM[norm],
                        with_report=with_report)


@pytest.mark.parametrize("name", sorted(W.SINGLES))
def test_single_plugin_equals_oracle(name):
    _, _, sel, dim_ext, norm = W.SINGLES[name]
    _, rp = W.trace()
    res, state, path, _ = W.engine_run(W.keep_a(), rp.events, W.N_EV, {name.split("-")[0]: 1000}, sel, dim_ext, norm)
    assert path == "k_wsum"
    want, want_state, _ = oracle_single(name, W.oracle_inputs(W.keep_a(), W.N_EV)[2])
    W.assert_same(res, want, state, want_state)


@pytest.mark.parametrize("pair", W.PAIRS, ids=lambda p: "PWR%d-FGD%d" % p)
def test_pwr_fgd_pair_on_k_wsum_equals_oracle(pair):
    _, rp = W.trace()
    res, state, path, _ = W.engine_run(W.keep_a(), rp.events, W.N_EV, {"PWR": pair[0], "FGD": pair[1]}, "FGD")
    assert path == "k_wsum"
    onodes, otyp, oev = W.oracle_inputs(W.keep_a(), W.N_EV)
    want, want_state, _ = O.run_events(onodes, otyp, oev, policy=O.POL_PWR_FGD, gpu_sel=O.SEL_FGD, threads=16,
                                       w_pwr=pair[0], w_fgd=pair[1])
    W.assert_same(res, want, state, want_state)


def test_literal_pwr_fgd_string_keeps_k_replay():
    # out of scope: routing the literal "PWR a FGD b" away from k_replay<PWR+FGD>
    _, rp = W.trace()
    res, _, path, _ = W.engine_run(W.keep_a(), rp.events, 100, None, None, policy="PWR 500 FGD 500")
    assert path == "k_replay"
    res2, _, path2, _ = W.engine_run(W.keep_a(), rp.events, 100, {"PWR": 500, "FGD": 500}, "FGD")
    assert path2 == "k_wsum" and res == res2


@pytest.mark.parametrize("name", ["FGD", "GpuClustering", "PWR"])
def test_create_delete_stream_equals_oracle(name):
    _, _, sel, dim_ext, norm = W.SINGLES[name]
    evs, oev = W.delete_stream(W.keep_a())
    res, state, path, _ = W.engine_run(W.keep_a(), evs, len(evs), {name: 1000}, sel, dim_ext, norm)
    assert path == "k_wsum"
    want, want_state, _ = oracle_single(name, oev)
    W.assert_same(res, want, state, want_state)
    assert sum(1 for r in res if r[4] == ksim.DELETED and r[0] >= 0) == 50


@pytest.mark.parametrize("stream", ["create", "delete"])
def test_report_equals_oracle(stream):
    # the report's records (snap / prev) come from k_wsum's general instantiation; k_report_delta / k_report_scan and
    # the [Power] report run unchanged on them
    _, rp = W.trace()
    evs, oev = (rp.events, W.oracle_inputs(W.keep_a(), W.N_EV)[2]) if stream == "create" else W.delete_stream(W.keep_a())
    res, _, path, eng = W.engine_run(W.keep_a(), evs, len(oev), {"FGD": 1000}, "FGD", report=True)
    try:
        got, pw = eng.reports(0), eng.power_reports(0)
    finally:
        eng.close()
    for r, p in zip(got, pw):
        r["power"] = p
    assert path == "k_wsum"
    want_res, _, want = oracle_single("FGD", oev, with_report=True)
    assert [tuple(r) for r in res] == [tuple(r) for r in want_res]
    assert_reports(got, want)


@pytest.mark.parametrize("name", sorted(W.MIXTURES))
def test_mixture_equals_reference(name):
    weights, sel = W.MIXTURES[name]
    _, rp = W.trace()
    res, state, path, _ = W.engine_run(W.keep_b(), W.mix_stream()[0], W.MIX_EV, weights, sel)
    assert path == "k_wsum"
    _, _, want, want_state = W.reference(name)
    W.assert_same(res, want, state, want_state)


def test_mixture_from_policy_string_and_kernel_name():
    # Engine.set_policy("FGD 700 BestFit 300"): policy, weights and the harness's default selector in one call
    t, rp = W.trace()
    arr, n = t.typical()
    import helpers
    eng = ksim.Engine(len(W.keep_b()), 1)
    try:
        eng.set_nodes(0, helpers.subset_nodes(rp, W.keep_b()))
        eng.set_typical(0, arr, n)
        eng.set_policy(0, "FGD 700 BestFit 300")
        eng.load_events(0, W.mix_stream()[0], W.MIX_EV)
        eng.run()
        assert eng.last_run_path() == "k_wsum" and eng.last_run_kernels() == ["k_wsum"] and eng.last_run_wgs() == 1
        res, state = eng.results(0), eng.nodes(0)
    finally:
        eng.close()
    _, _, want, want_state = W.reference("FGD 700 BestFit 300")
    W.assert_same(res, want, state, want_state)


def test_weighted_beside_other_policies():
    # one run, three replicas on leg B's create / delete stream: FGD, BestFit and a weighted combination (k_wsum) as
    # one more K = 1 group; every replica decides what it decides alone
    t, rp = W.trace()
    arr, n = t.typical()
    import helpers
    keep = W.keep_b()
    eng = ksim.Engine(len(keep), 3)
    try:
        for r, pol in enumerate(["FGD", "BestFit", "BestFit 500 PWR 500"]):
            eng.set_nodes(r, helpers.subset_nodes(rp, keep))
            eng.set_typical(r, arr, n)
            eng.set_power_model(r, t.power_model())
            eng.set_policy(r, pol)
            eng.load_events(r, W.mix_stream()[0], W.MIX_EV)
        eng.run()
        kernels, path = eng.last_run_kernels(), eng.last_run_path()
        res = [eng.results(r) for r in range(3)]
        state = eng.nodes(2)
    finally:
        eng.close()
    assert "k_wsum" in kernels and len(kernels) >= 2 and path != "k_wsum"
    _, _, want, want_state = W.reference("BestFit 500 PWR 500")
    W.assert_same(res[2], want, state, want_state)
    onodes, otyp, _ = W.oracle_inputs(keep, W.MIX_EV)
    oev = W.mix_stream()[1]
    for r, (pol, sel) in enumerate([(O.POL_FGD, O.SEL_FGD), (O.POL_BESTFIT, O.SEL_BEST)]):
        w, _, _ = O.run_events(onodes, otyp, oev, policy=pol, gpu_sel=sel, threads=16)
        assert [tuple(x) for x in res[r]] == [tuple(x) for x in w]
