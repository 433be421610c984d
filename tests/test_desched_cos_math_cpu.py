"""cos_similarity (ksim_desched.hpp), compiled for the host, against tests/desched_cos_ref.py.

A few thousand fuzzed (node, pod, GPU mask) cases: share, whole-GPU, 8-GPU and CPU-only pods, the three
ways Add fails (CPU over the capacity, a device over 1000 milli, a device the node does not have), a zero
magnitude and parallel vectors.  The comparison is `==` on the doubles: the sums are exact, and sqrt, `*`
and `/` round correctly on both sides.
"""
import ctypes as C
import os
import random
import subprocess

import pytest

import desched_cos_ref as cos
import pyoracle as O
from test_desched_math_cpu import rand_case

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native_desched_cos")


@pytest.fixture(scope="module")
def dc():
    subprocess.run(["make", "-s", "-C", HERE], check=True)
    L = C.CDLL(os.path.join(HERE, "libdeschedcos.so"))
    L.dc_cos_similarity.argtypes = [C.c_int, C.c_int * 8, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint]
    L.dc_cos_similarity.restype = C.c_double
    L.dc_cos_elects.argtypes = [C.c_double]
    L.dc_cos_bits.argtypes = [C.c_double]
    L.dc_cos_bits.restype = C.c_ulonglong
    return L


def special_case(rnd):
    """A zero magnitude (a pod that asks for nothing, or a node with nothing left after it) or a pod
    parallel to what the node has left after Add."""
    kind = rnd.randrange(3)
    if kind == 0:    # the pod's vector is zero
        cnt = rnd.choice([0, 1, 4])
        gl = [rnd.randint(0, 1000) for _ in range(cnt)] + [0] * (8 - cnt)
        return rnd.randint(0, 4000), gl, cnt, 4000, 0, 0, 0, 0
    if kind == 1:    # the node's vector is zero
        return 0, [0] * 8, rnd.choice([0, 2]), 4000, 0, 0, 0, 0
    k = rnd.randint(2, 6)  # node + pod = k x pod
    c, m = rnd.choice([100, 750, 1000, 11908]), rnd.randint(1, 1000 // k)
    g = rnd.randrange(4)
    gl = [0] * 8
    gl[g] = (k - 1) * m
    return (k - 1) * c, gl, 4, k * c + rnd.choice([0, 500]), c, m, 1, 1 << g


def test_cos_similarity_fuzz(dc):
    rnd = random.Random(11)
    seen = dict(ok=0, cpu=0, gpu=0, nodev=0, zero=0, parallel=0, share=0, whole=0, eight=0, cpu_only=0, elected=0)
    for i in range(6000):
        special = i % 6 == 5
        cpu_left, gl, cnt, cap, cpu_nz, milli, num, mask = special_case(rnd) if special else rand_case(rnd)
        node = O.node_res(cpu_left, gl[:cnt], cnt, "", cap)
        ids = [g for g in range(9) if mask >> g & 1]
        want, why = cos.similarity_of(node, cpu_nz, milli, num, ids)
        got = dc.dc_cos_similarity(cpu_left, (C.c_int * 8)(*gl), cnt, cap, cpu_nz, milli, num, mask)
        assert got == want, (cpu_left, gl, cnt, cap, cpu_nz, milli, num, mask, why)
        assert dc.dc_cos_elects(got) == (1 if 0 <= want < 1 else 0)
        if why == "add":
            if cpu_left + cpu_nz > cap:
                seen["cpu"] += 1
            elif any(g >= cnt for g in ids):
                seen["nodev"] += 1
            else:
                seen["gpu"] += 1
            continue
        assert why in ("ok", "zero")   # a cosine of non-negative vectors never leaves [-1e-3, 1 + 1e-3]
        seen[why] += 1
        if why == "zero":
            continue
        seen["elected"] += 0 <= want < 1
        seen["parallel"] += special
        seen["cpu_only"] += num == 0
        seen["share"] += num == 1 and milli < 1000
        seen["whole"] += num >= 1 and milli == 1000
        seen["eight"] += num == 8
        if special:
            assert abs(want - 1.0) <= 2.0 ** -51
    assert all(v >= 20 for v in seen.values()), seen


def test_bits_order_as_the_similarities(dc):
    rnd = random.Random(5)
    vals = sorted([0.0, 5e-324, 2.0 ** -1022, 0.5, 1.0 - 2.0 ** -53] + [rnd.random() for _ in range(200)])
    bits = [dc.dc_cos_bits(v) for v in vals]
    assert bits == sorted(bits) and len(set(bits)) == len(set(vals))
    assert dc.dc_cos_bits(-0.0) == dc.dc_cos_bits(0.0) == 0
    assert [dc.dc_cos_elects(v) for v in (0.0, -0.0, 0.999, 1.0, 1.0005, -1.0, -1e-4)] == [1, 1, 1, 0, 0, 0, 0]
