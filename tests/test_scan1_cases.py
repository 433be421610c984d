"""CPU checks of the inputs of tests/test_gpu_scan1_edges.py: the oracle alone replays every crafted
stream (tests/scan1_cases.py) and every fuzz cluster of the node-count edges under the five cheap
policies, and the replays hold what the GPU tests rely on -- dead events at the window edges and the
mask's word edges, binds after them, binds in every register slot and wave, single-feasible events,
BestFit's Score errors -- so a later edit of the builders cannot empty those tests."""
import pytest

import ksim
import pyoracle as O
import scan1_cases as SC

CHEAP = [("BestFit", O.POL_BESTFIT, O.SEL_BEST), ("DotProd", O.POL_DOTPROD, O.SEL_BEST),
         ("GpuPacking", O.POL_PACKING, O.SEL_BEST), ("GpuClustering", O.POL_CLUSTERING, O.SEL_BEST),
         ("Random", O.POL_RANDOM, O.SEL_RANDOM)]
SEED = 5
OK, UNSCHED, ERROR = ksim.SCHEDULED, ksim.UNSCHEDULABLE, ksim.ERROR
DEAD = (-1, 0, 0, 0, UNSCHED)  # node, mask, score, n_feasible, status of an event no node can take


def replay(case, pol, sel):
    return O.run_events(case["onodes"], case["otypical"], case["oevents"], policy=pol, gpu_sel=sel, seed=SEED, threads=16)[0]


def dying(e):
    return e["cpu"] >= SC.BIG_CPU or e["num"] == 8


def check_dead_events(case, res, dead_at):
    """Exactly the events dead_at are repeats of a class that found no node before (the kernel skips
    those); every other event of a dying class binds or is that class's first failure."""
    ev, ids = case["oevents"], SC.class_ids(case["oevents"])
    failed, repeats = set(), []
    for i, (e, r) in enumerate(zip(ev, res)):
        if ids[i] in failed:
            assert r == DEAD, (i, r)
            repeats.append(i)
        elif dying(e) and r[4] != OK:
            assert r == DEAD, (i, r)  # the first failure: unschedulable, 0 feasible nodes
            failed.add(ids[i])
        else:
            assert r[4] == OK and r[0] >= 0, (i, e, r)  # fillers and the first whole-8 pods bind
    assert repeats == sorted(dead_at)
    return failed


@pytest.mark.parametrize("name,pol,sel", CHEAP, ids=[p[0] for p in CHEAP])
@pytest.mark.parametrize("length", SC.WINDOW_LENGTHS)
def test_window_streams(length, name, pol, sel):
    case = SC.crafted("window-%d" % length)
    assert case["n_events"] == length
    res = replay(case, pol, sel)
    ids = SC.class_ids(case["oevents"])
    want_dead = [i for i in list(SC.WINDOW_DEAD) + list(SC.WINDOW_RUN) if i < length]
    failed = check_dead_events(case, res, want_dead)
    # both dying classes, first seen before event 100: the whole-8 class is id 2 (two binds, then dead at 9), the
    # born-dead class new at event 40
    assert [ids[i] for i in (2, 5, 9)] == [2, 2, 2] and ids[40] not in ids[:40] and failed == {2, ids[40]}
    assert [res[i][4] for i in (2, 5, 9, 40)] == [OK, OK, UNSCHED, UNSCHED]
    assert res[2][0] != res[5][0] and bin(res[2][1]).count("1") == 8
    assert set(SC.WINDOW_DEAD) == {126, 127, 128, 129, 255, 256, 257}
    assert len(SC.WINDOW_RUN) >= 10 and SC.WINDOW_RUN[0] < 383 and SC.WINDOW_RUN[-1] > 384
    # live events on both sides of every boundary the stream goes past; a bind follows every boundary
    for before, after in ((125, 130), (254, 258), (SC.WINDOW_RUN[0] - 1, SC.WINDOW_RUN[-1] + 1)):
        assert after >= length or (res[before][4] == OK and res[after][4] == OK)
    assert length < 400 or res[SC.WINDOW_RUN[-1] + 1][4] == OK
    # the truncated streams end with a dead event: one before a window's last, its last, the next window's first
    assert (res[-1] == DEAD) == (length != 400)


@pytest.mark.parametrize("name,pol,sel", CHEAP, ids=[p[0] for p in CHEAP])
def test_word_stream(name, pol, sel):
    case = SC.crafted("word")
    res = replay(case, pol, sel)
    ids = SC.class_ids(case["oevents"])
    first = [ids.index(k) for k in SC.WORD_IDS]
    assert first == [31, 32, 33] and all(case["oevents"][i]["cpu"] >= SC.BIG_CPU for i in first)
    repeats = [i for i, k in enumerate(ids) if k in SC.WORD_IDS and i not in first]
    assert len(repeats) == 9
    assert check_dead_events(case, res, repeats) == set(SC.WORD_IDS)
    # after every repeat: the neighbours 30 and 34, the same bits one word down and one word up -- all bind
    for i in repeats:
        near = ids[i + 1:i + 10]
        assert near == [30, 34, 0, 1, 2, 63, 64, 65, 66]
        assert all(res[j][4] == OK for j in range(i + 1, i + 10))


@pytest.mark.parametrize("name,pol,sel", CHEAP, ids=[p[0] for p in CHEAP])
@pytest.mark.parametrize("n_classes", SC.LIMIT_CLASSES)
def test_limit_streams(n_classes, name, pol, sel):
    case = SC.crafted("limit-%d" % n_classes)
    res = replay(case, pol, sel)
    ids = SC.class_ids(case["oevents"])
    assert max(ids) + 1 == n_classes and len(case["onodes"]) <= 6
    dead_id = n_classes - 1  # 1023: the last bit of the last word; 1024: past the mask, and the skip is off
    first = ids.index(dead_id)
    assert first == n_classes - 1 and case["oevents"][first]["cpu"] >= SC.BIG_CPU
    repeats = [i for i, k in enumerate(ids) if k == dead_id and i != first]
    assert len(repeats) == 8
    assert check_dead_events(case, res, repeats) == {dead_id}
    after = {ids[i + 1] for i in repeats}
    assert after == {n_classes - 3, 32}  # a neighbour id binds right after
    # and the classes a wrong word or bit would kill come back: 0, the last word's first bit, the dead id's neighbours
    assert {0, 31, 992, n_classes - 2} <= set(ids[first:])


@pytest.mark.parametrize("n", sorted(SC.EDGE))
def test_edge_clusters_reach_the_slots_and_lanes(n):
    case = SC.edge_case(n)
    assert len(case["onodes"]) == n and not any(e.get("delete") for e in case["oevents"])
    for name, pol, sel in CHEAP:
        res = replay(case, pol, sel)
        binds = [r[0] for r in res if r[4] == OK]
        # a bind in every register slot node // 256 that holds nodes, and in every wave (node % 256) // 64
        assert {b // 256 for b in binds} == set(range((n + 255) // 256)), name
        if n >= 256:
            assert {(b % 256) // 64 for b in binds} == {0, 1, 2, 3}, name
        elif n > 64:
            assert {(b % 256) // 64 for b in binds} == set(range((n + 63) // 64)), name
        assert any(r[4] == UNSCHED for r in res), name
        if SC.SINGLE[n] == "all" or name in SC.SINGLE[n]:
            assert any(r[3] == 1 for r in res), name
        # BestFit's Score error aborts a cycle with more than one feasible node: none on a one-node cluster, where
        # the single-feasible shortcut never reaches Score
        if name == "BestFit" and n > 1:
            assert any(r[4] == ERROR and r[3] > 1 for r in res)
