"""wsum_total (ksim_device.hpp) -- the NormalizeScore / range check / weighted sum k_wsum runs per feasible node --
compiled for the host (tests/native_wsum) against the oracle: orc_normalize_score for BestFit, orc_normalize_score_pwr
for PWR, and the oracle's weight loop (fgd_oracle.c, "framework.go:686-704": every score outside 0..100 is an error,
then score x weight, summed over the plugins).  Exhaustive small ranges and seeded random vectors, including
lo == hi and BestFit's raw scores far below zero.  No GPU needed.
"""
import ctypes as C
import itertools
import os
import random
import subprocess

import pytest

import pyoracle as O

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native_wsum")
FGD, BESTFIT, DOTPROD, PACKING, CLUSTERING, RANDOM, PWR = range(7)


@pytest.fixture(scope="module")
def wm():
    subprocess.run(["make", "-s", "-C", HERE, "libwsummath.so"], check=True)
    L = C.CDLL(os.path.join(HERE, "libwsummath.so"))
    L.wm_totals.argtypes = [C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    assert L.wm_num_plugins() == 7
    return L


def device(wm, raws, w):
    n = len(raws)
    flat = (C.c_int * (7 * n))(*[v for r in raws for v in r])
    out = (C.c_int * n)()
    err = wm.wm_totals(flat, n, (C.c_int * 7)(*w), out)
    return list(out), bool(err)


def oracle(raws, w):
    n = len(raws)
    tot, err = [0] * n, False
    for p in range(7):
        if w[p] <= 0:
            continue
        arr = (C.c_int64 * n)(*[r[p] for r in raws])
        if p == BESTFIT:
            O.lib().orc_normalize_score(arr, n)
        if p == PWR:
            O.lib().orc_normalize_score_pwr(arr, n)
        for i in range(n):
            err = err or arr[i] > 100 or arr[i] < 0
            tot[i] += arr[i] * w[p]
    return tot, err


def check(wm, raws, w):
    got, gerr = device(wm, raws, w)
    want, werr = oracle(raws, w)
    assert gerr == werr, (raws, w)
    if not werr:  # (an error aborts the cycle: the totals are not read)
        assert got == want, (raws, w)


def test_exhaustive_small_ranges(wm):
    # one plugin at a time beside a fixed second one: every raw value in -3..103 on 2 nodes, a coarser grid on 3 and 4
    vals = list(range(-3, 104))
    for p in (FGD, BESTFIT, DOTPROD, PACKING, CLUSTERING, PWR):
        w = [0] * 7
        w[p] = 3
        w[FGD if p != FGD else PACKING] = 2
        for a, b in itertools.product(vals, vals):
            raws = [[50] * 7, [50] * 7]
            raws[0][p], raws[1][p] = a, b
            check(wm, raws, w)
    grid = [-3, -1, 0, 1, 49, 50, 99, 100, 101, 103]
    for p in (BESTFIT, PWR, DOTPROD):
        w = [0] * 7
        w[p] = 7
        for n in (3, 4):
            for vs in itertools.product(grid, repeat=n):
                check(wm, [[0, 0, 0, 0, 0, 0, 0][:p] + [v] + [0] * (6 - p) for v in vs], w)


def test_random_vectors(wm):
    rnd = random.Random(20240807)
    hits = dict(eq_bf=0, eq_pw=0, neg_bf=0, err=0, ok=0)
    for _ in range(4000):
        n = rnd.randint(2, 12)
        w = [rnd.choice([0, 0, 1, 50, 300, 700, 1000, 50000]) for _ in range(7)]
        w[RANDOM] = 0
        if not any(w):
            w[rnd.choice([FGD, BESTFIT, PWR])] = 1
        raws = []
        kind = rnd.random()
        bf0, pw0 = rnd.randint(-(1 << 22), 100), rnd.randint(-4000, 0)
        for _i in range(n):
            r = [rnd.randint(0, 100) for _ in range(7)]
            # BestFit's raw score runs far below 0 on a node with more CPU left than MaxSpecCpu; PWR's are energy
            # deltas <= 0; DotProduct may leave 0..100
            r[BESTFIT] = bf0 if kind < 0.2 else rnd.randint(-(1 << 22), 100) if kind < 0.5 else rnd.randint(0, 100)
            r[PWR] = pw0 if 0.1 < kind < 0.3 else rnd.randint(-4000, 0)
            if rnd.random() < 0.03:
                r[DOTPROD] = rnd.choice([-1, 101, 250])
            raws.append(r)
        check(wm, raws, w)
        _, e = oracle(raws, w)
        hits["err" if e else "ok"] += 1
        hits["eq_bf"] += len(set(r[BESTFIT] for r in raws)) == 1 and w[BESTFIT] > 0
        hits["eq_pw"] += len(set(r[PWR] for r in raws)) == 1 and w[PWR] > 0
        hits["neg_bf"] += min(r[BESTFIT] for r in raws) < -1000 and w[BESTFIT] > 0
    assert all(v > 50 for v in hits.values()), hits


def test_lo_equals_hi(wm):
    # BestFit contributes 0 to every node and PWR 100 when all raw scores are equal (plugin_utils.go:48-74,
    # pwr_score.go:104-141)
    raws = [[10, 77, 0, 0, 0, 0, -300], [20, 77, 0, 0, 0, 0, -300], [30, 77, 0, 0, 0, 0, -300]]
    got, err = device(wm, raws, [1, 1000, 0, 0, 0, 0, 10])
    assert not err and got == [10 + 1000, 20 + 1000, 30 + 1000]
    check(wm, raws, [1, 1000, 0, 0, 0, 0, 10])
