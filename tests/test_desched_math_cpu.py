"""victim_eval (ksim_desched.hpp), compiled for the host, against the oracle's NodeResource.Add + F.

A few thousand fuzzed (node, pod, GPU mask, typical table) cases: typed and untyped tables, share,
whole-GPU, 8-GPU and CPU-only pods, and the ways Add fails (CPU over the capacity, a device over 1000
milli, a device the node does not have).  The verdict and both F values must agree bit for bit.
"""
import ctypes as C
import os
import random
import subprocess

import pytest

import helpers
import ksim
import pyoracle as O
from test_device_math_cpu import TYPES, table

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native_desched")


@pytest.fixture(scope="module")
def dd():
    subprocess.run(["make", "-s", "-C", HERE], check=True)
    L = C.CDLL(os.path.join(HERE, "libdeschedmath.so"))
    L.dd_victim_eval.argtypes = [C.c_int, C.c_int * 8, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint,
                                 C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                 C.POINTER(C.c_double)]
    L.dd_victim_score.argtypes = [C.c_double, C.c_double]
    L.dd_victim_score.restype = C.c_longlong
    return L


@pytest.fixture(scope="module")
def tables():
    # untyped (default) and typed (gpuspec33: typical pods that name GPU models)
    return [helpers.oracle_typical(ksim.Trace.openb("default")), helpers.oracle_typical(ksim.Trace.openb("gpuspec33"))]


def rand_case(rnd):
    """(cpu_left, gl[8], cnt, cap, cpu_nz, milli, num, mask): a node after some pods were bound and one of
    them, or a pod that cannot be given back."""
    cnt = rnd.choice([0, 1, 2, 4, 8, 8])
    cap = rnd.choice([4000, 32000, 64000, 96000, 128000])
    gl = [rnd.choice([0, 0, 1000, rnd.randint(0, 1000), rnd.randint(0, 1000)]) for _ in range(cnt)] + [0] * (8 - cnt)
    kind = rnd.random()
    if kind < 0.2 or cnt == 0:        # CPU-only pod
        milli, num, mask = 0, 0, 0
    elif kind < 0.55:                 # share pod on one device
        milli, num = rnd.choice([100, 250, 300, 460, 500, 810, 999]), 1
        mask = 1 << rnd.randrange(cnt)
    elif kind < 0.8:                  # whole GPUs
        milli, num = 1000, rnd.choice([1, 1, 2, 4, 8])
        num = min(num, cnt)
        mask = sum(1 << g for g in rnd.sample(range(cnt), num))
    elif kind < 0.9:                  # every device of an 8-GPU node
        milli, num, mask = 1000, cnt, (1 << cnt) - 1
    else:                             # a device the node does not have
        milli, num, mask = rnd.choice([100, 500, 1000]), 1, 1 << rnd.randrange(cnt, 9) if cnt < 8 else 1 << 8
    fits = rnd.random() < 0.7
    if fits:                          # make room: the pod's milli are in use on its devices
        for g in range(min(cnt, 8)):
            if mask >> g & 1:
                gl[g] = min(gl[g], 1000 - milli)
    cpu_nz = rnd.choice([100, 1000, 4000, 11908, 32000])
    cpu_left = rnd.randint(0, cap - cpu_nz) if (cap >= cpu_nz and rnd.random() < 0.85) else rnd.randint(max(0, cap - cpu_nz + 1), cap)
    return cpu_left, gl, cnt, cap, cpu_nz, milli, num, mask


def test_victim_eval_fuzz(dd, tables):
    rnd = random.Random(7)
    seen = dict(ok=0, cpu=0, gpu=0, nodev=0, cpu_only=0, eight=0)
    for tlist in tables:
        tpi, tpf = table(tlist)
        otp = O.typical(tlist)
        for _ in range(2500):
            cpu_left, gl, cnt, cap, cpu_nz, milli, num, mask = rand_case(rnd)
            ty = rnd.randrange(len(TYPES))
            node = O.node_res(cpu_left, gl[:cnt], cnt, TYPES[ty], cap)
            pod = O.pod_res(cpu_nz, milli, num, "")
            ids = [g for g in range(9) if mask >> g & 1]
            out = O.NodeResource()
            rc = O.lib().orc_node_add(C.byref(node), C.byref(pod), (C.c_int * 9)(*(ids + [0] * (9 - len(ids)))), len(ids),
                                      C.byref(out))
            f_node, f_after = C.c_double(-1), C.c_double(-1)
            ok = dd.dd_victim_eval(cpu_left, (C.c_int * 8)(*gl), cnt, ty, cap, cpu_nz, milli, num, mask, len(tlist), tpi,
                                   tpf, C.byref(f_node), C.byref(f_after))
            assert f_node.value == O.frag_score(node, otp)
            assert ok == (1 if rc == 0 else 0), (cpu_left, gl, cnt, cap, cpu_nz, milli, num, mask)
            if ok:
                want = O.frag_score(out, otp)
                assert f_after.value == want
                assert dd.dd_victim_score(f_node.value, want) == int(f_node.value - want)
                seen["ok"] += 1
                seen["cpu_only"] += num == 0
                seen["eight"] += num == 8
            elif cpu_left + cpu_nz > cap:
                seen["cpu"] += 1
            elif any(g >= cnt for g in ids):
                seen["nodev"] += 1
            else:
                seen["gpu"] += 1
    assert all(v >= 20 for v in seen.values()), seen


def test_victim_score_truncates_toward_zero(dd):
    assert dd.dd_victim_score(301.0, 300.5) == 0
    assert dd.dd_victim_score(301.0, 350.0) == -49
    assert dd.dd_victim_score(300.0, 350.5) == -50
    assert dd.dd_victim_score(800.0, 400.0) == 400
    assert dd.dd_victim_score(800.75, 400.0) == 400
