"""Descheduling cases from the adversarial generator and flat clusters of any size -- TEST INFRASTRUCTURE.

Same shape as desched_cases._case: onodes / otyp / oev for the oracle, nodes / typ / events / n for the engine.
tests/test_desched_fuzz_cases.py asserts on the CPU that every case reaches what it is there for;
tests/test_gpu_desched_fuzz.py runs them on the device.
"""
import math

import desched_cos_cases as cos_cases
from fuzz_cases import make_case

# (seed, nodes, creations, delete probability): the clusters of tests/test_gpu_fuzz.py that fit a few seconds of
# reference time, and three at the 64 / 256-thread edges of the node count.  Their typical tables are typed
# (GPU specs in the created pods), their nodes have 0 to 8 GPUs, tight pod limits and tiny memory, their pods
# zero-CPU requests, up to 8 GPUs and specs naming a model no node has.
FUZZ = [(1, 40, 500, 0.0), (2, 97, 900, 0.25), (3, 250, 1200, 0.1), (4, 7, 300, 0.4), (5, 1, 60, 0.3),
        (41, 63, 400, 0.2), (42, 65, 400, 0.2), (43, 257, 700, 0.2)]
FUZZ_POLICIES = ["FGD", "BestFit"]

# flat clusters: the stride edges of the two 256-thread select kernels, and both sides of their LDS / HBM switch
# (60 KiB of tables: 2560 nodes of 24 B for k_cos_select, 3072 of 20 B for k_desched_select)
COS_STRIDE_N = [1, 2, 3, 64, 65, 255, 256, 257, 512, 513]
COS_SWITCH_N = [2560, 2561]
FRAG_STRIDE_N = [1, 63, 64, 65, 255, 256, 257]
FRAG_SWITCH_N = [3072, 3073]
# one engine planning every policy in turn over one buffer of tables in HBM: past both switches, the usual stream
SHARED_TAB_N, SHARED_TAB_PODS = 3073, 700

FRAG_MILLI = [600, 700, 800, 900, 550, 650, 750]


def from_fuzz(seed, n_nodes, n_create, p_delete, n_events=None):
    """fuzz_cases.make_case in the descheduling tests' shape.  n_events cuts the stream: a cut stream stays
    valid, because every delete refers to an earlier creation.  The typical table stays the whole stream's."""
    c = make_case(seed, n_nodes, n_create, p_delete)
    n = c["n_events"] if n_events is None else n_events
    assert 0 <= n <= c["n_events"]
    return dict(onodes=c["onodes"], otyp=c["otypical"], oev=c["oevents"][:n], nodes=c["nodes"],
                typ=(c["typical"], c["typical_n"]), events=c["events"], n=n)


def scrambled_names(n):
    """n unique names whose byte order is a permutation far from the index order: i -> i * m mod n with m the
    first multiplier from 125 up that is coprime to n, in a width that holds n."""
    m = 125
    while math.gcd(m, n) != 1:
        m += 1
    width = len(str(n))
    names = ["f%0*d" % (width, i * m % n) for i in range(n)]
    assert len(set(names)) == n
    return names


def flat_cos(n):
    """desched_cos_cases.flat() at n nodes: one-GPU nodes of 1500 milli-CPU with scrambled names and n pods of
    1000 milli-CPU, so the CPU forces one pod a node; the GPU milli cycle through seven values.  Under the default
    bars every node is a cosSim candidate with a victim, and the node order needs both sort keys."""
    nodes = [(name, 0, 1, 1500, 1000) for name in scrambled_names(n)]
    pods = [dict(cpu=1000, milli=cos_cases.FLAT_MILLI[i % 7], num=1, model=None) for i in range(n)]
    return cos_cases._case(nodes, cos_cases.TYP, pods)


def flat_frag(n, n_pods=None):
    """n one-GPU nodes of 4000 milli-CPU with scrambled names and n pods of 2500 milli-CPU: one pod a node, and
    the 1500 milli-CPU left host neither typical pod, so F(node) is the GPU milli left (seven values) and giving
    the pod back makes it 0.  Every node has a frag victim; the priorities tie over a seventh of the nodes.
    n_pods < n: only that many nodes get a pod (and a frag victim, and under wide bars a cosSim one)."""
    nodes = [(name, 0, 1, 4000, 1000) for name in scrambled_names(n)]
    pods = [dict(cpu=2500, milli=FRAG_MILLI[i % 7], num=1, model=None) for i in range(n if n_pods is None else n_pods)]
    return cos_cases._case(nodes, cos_cases.TYP, pods)
