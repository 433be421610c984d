"""Hand-made cases of the cosSim descheduling tests, as matching oracle and engine inputs -- TEST INFRASTRUCTURE.

Same shape as desched_cases: onodes / otyp / oev for the oracle, nodes / typ / events / n for the engine.
"""
import ksim

MODELS = ["M%d" % i for i in range(8)]
TYP = [(2000, 500, 1, 0.5), (2000, 1000, 1, 0.5)]


def _case(node_specs, typ, pods):
    """node_specs: (name, model id, gpus, cpu, mem); typ: (cpu, milli, num, freq), any model;
    pods: dicts cpu, cpu_nz, mem, milli, num, model (id or None), delete / ref."""
    order = sorted(range(len(node_specs)), key=lambda i: node_specs[i][0].encode())
    rank = {i: r for r, i in enumerate(order)}
    nodes = (ksim.Node * len(node_specs))()
    onodes = []
    for i, (name, model, gpus, cpu, mem) in enumerate(node_specs):
        nodes[i].cpu_alloc_milli, nodes[i].mem_alloc_mib, nodes[i].pods_alloc = cpu, mem, 1001
        nodes[i].gpu_count, nodes[i].gpu_type, nodes[i].name_rank = gpus, model, rank[i]
        onodes.append(dict(name=name, cpu=cpu, mem=mem, pods=1001, gpu=gpus, model=MODELS[model] if gpus else ""))
    tarr = (ksim.Typical * len(typ))()
    for i, (cpu, milli, num, freq) in enumerate(typ):
        tarr[i] = ksim.Typical(cpu, milli, num, ksim.KSIM_TYPE_ANY, 0, freq)
    otyp = [(cpu, milli, num, "", freq) for cpu, milli, num, freq in typ]
    events = (ksim.Pod * len(pods))()
    oev = []
    for i, p in enumerate(pods):
        model = p.get("model")
        e = ksim.make_pod(p["cpu"], p["milli"], p["num"], p.get("mem", 0),
                          ksim.KSIM_TYPE_ANY if model is None else 1 << model, p.get("cpu_nz", p["cpu"]))
        e.is_delete, e.ref = p.get("delete", 0), p.get("ref", -1)
        events[i] = e
        oev.append(dict(cpu=p["cpu"], cpu_nz=p.get("cpu_nz", p["cpu"]), mem=p.get("mem", 0), milli=p["milli"],
                        num=p["num"], type="" if model is None else MODELS[model], delete=p.get("delete", 0),
                        ref=p.get("ref", -1)))
    return dict(onodes=onodes, otyp=otyp, oev=oev, nodes=nodes, typ=(tarr, len(typ)), events=events, n=len(pods))


def gpu_pod(model, cpu, milli, num=1, cpu_nz=None):
    return dict(cpu=cpu, cpu_nz=cpu if cpu_nz is None else cpu_nz, milli=milli, num=num, model=model)


def hand():
    """Seven one-model nodes; every pod names its node's model, so the placement is forced.
    tests/test_desched_cos_ref.py works the answers out by hand (default bars: CPU 2000, GPU 500)."""
    nodes = [
        ("c0", 0, 1, 3000, 1000),   # 2000 milli-CPU left: exactly at the CPU bar
        ("c1", 1, 1, 3000, 1000),   # its one GPU has 500 milli left: exactly at the GPU bar
        ("c3", 2, 2, 4000, 1000),   # index 2 is named after index 3 ...
        ("c2", 3, 2, 4000, 1000),   # ... and has the same milli-GPU left: index 3 goes first
        ("c4", 4, 1, 1500, 1000),   # its pod cannot be given back (the non-zero CPU default)
        ("c5", 5, 2, 1500, 1000),   # its pod is parallel to the node it would leave: similarity 1
        ("c6", 6, 1, 1900, 1000),
    ]
    pods = [
        gpu_pod(0, 1000, 300),            # e0 -> node 0
        gpu_pod(1, 2000, 500),            # e1 -> node 1
        gpu_pod(2, 1500, 400),            # e2 -> node 2
        gpu_pod(2, 1500, 400),            # e3 -> node 2: identical to e2
        gpu_pod(3, 1500, 400),            # e4 -> node 3
        gpu_pod(3, 1500, 400),            # e5 -> node 3: identical to e4
        gpu_pod(4, 0, 300, cpu_nz=100),   # e6 -> node 4: no CPU request, the default 100 does not fit back
        gpu_pod(5, 750, 1000),            # e7 -> node 5
        gpu_pod(6, 500, 200),             # e8 -> node 6
        gpu_pod(6, 100, 100),             # e9 -> node 6 ...
        dict(cpu=100, milli=100, num=1, model=6, delete=1, ref=9),  # e10: ... and deleted again
    ]
    return _case(nodes, TYP, pods)


FLAT_N = 600
FLAT_MILLI = [100, 200, 300, 400, 450, 250, 350]


def flat():
    """600 one-GPU nodes of 1500 milli-CPU whose names are scrambled against the index order, and 600 pods of
    1000 milli-CPU: the CPU forces one pod a node.  The GPU milli cycle through seven values, so the node order
    is decided by both keys, over more nodes than a workgroup has threads."""
    nodes = [("f%03d" % (i * 119 % FLAT_N), 0, 1, 1500, 1000) for i in range(FLAT_N)]
    pods = [dict(cpu=1000, milli=FLAT_MILLI[i % 7], num=1, model=None) for i in range(FLAT_N)]
    return _case(nodes, TYP, pods)
