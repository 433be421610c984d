"""Descheduling test cases, each as matching oracle and engine inputs -- TEST INFRASTRUCTURE.

A case is a dict: onodes / otyp / oev (the oracle's node dicts, typical tuples, event dicts), and
nodes / typ / events (ksim.Node array, (ksim.Typical array, n), ksim.Pod array) for the engine.
"""
import ksim

MODELS = ["M0", "M1", "M2", "M3"]


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
    """Four one-model nodes; every GPU pod names its node's model, so the placement is forced.
    Node index 2 is named after index 3: at equal F, index 3 (rank 2) goes before index 2 (rank 3).
    tests/test_desched_ref.py works the answers out by hand."""
    nodes = [("h0", 0, 1, 4000, 1000), ("h1", 1, 1, 8000, 1000), ("h3", 2, 2, 8000, 1000), ("h2", 3, 2, 8000, 1000)]
    typ = [(2000, 500, 1, 0.5), (2000, 1000, 1, 0.5)]
    pods = [
        gpu_pod(0, 0, 400, cpu_nz=100),   # e0 -> node 0: no CPU request, the non-zero default does not fit back
        gpu_pod(1, 1000, 300),            # e1 -> node 1
        gpu_pod(1, 1000, 399),            # e2 -> node 1: 301 milli left
        gpu_pod(2, 1000, 600),            # e3 -> node 2
        gpu_pod(2, 1000, 600),            # e4 -> node 2: 400 + 400 left
        gpu_pod(3, 1000, 600),            # e5 -> node 3
        gpu_pod(3, 1000, 600),            # e6 -> node 3: 400 + 400 left
        gpu_pod(0, 1000, 1000, num=8),    # e7: fails (no node has 8 GPUs of model M0)
        gpu_pod(0, 500, 100),             # e8 -> node 0
        dict(cpu=500, milli=100, num=1, model=0, delete=1, ref=8),  # e9: e8 deleted again
    ]
    return _case(nodes, typ, pods)


def crowded():
    """One node holding 300 one-CPU pods and three GPU pods (more pods than a wave, and than a 256-thread
    workgroup), an idle second node.  1500 milli-CPU stay free, below both typical pods' CPU; evicting a
    1000-milli pod lifts it over the first typical pod's 2000, evicting the one 2000-milli pod (event 293)
    over both: the victim sits behind 290 equal candidates."""
    nodes = [("c0", 0, 4, 306500, 100000), ("c1", 1, 1, 500, 10)]  # 305000 requested on c0; nothing fits c1
    typ = [(2000, 500, 1, 0.5), (3000, 1000, 1, 0.25), (2500, 0, 0, 0.25)]
    pods = [gpu_pod(0, 500, 600), gpu_pod(0, 500, 600), gpu_pod(0, 3000, 1000)]
    for i in range(300):
        pods.append(dict(cpu=2000 if i == 290 else 1000, milli=0, num=0, mem=10, model=None))
    return _case(nodes, typ, pods)


def empty():
    """No pod gets bound: one pod that fits nowhere."""
    nodes = [("e0", 0, 1, 4000, 1000), ("e1", 1, 1, 4000, 1000)]
    return _case(nodes, [(2000, 500, 1, 1.0)], [gpu_pod(0, 1000, 1000, num=4)])


OPENB_POLICIES = ["FGD", "BestFit", "GpuPacking"]


def openb64():
    """64 openb nodes, the first 600 pods of seed 42 with deletions mixed in (helpers.delete_stream),
    the trace's own typical table."""
    import helpers
    t = ksim.Trace.openb("default")
    rp = t.replay(seed=42, tune_ratio=1.3, shuffle=True)
    keep = list(range(0, t.num_nodes, 19))[:64]
    events, oev = helpers.delete_stream(t, rp, 600)
    return dict(onodes=helpers.oracle_subset(t, rp, keep), otyp=helpers.oracle_typical(t), oev=oev,
                nodes=helpers.subset_nodes(rp, keep), typ=t.typical(), events=events, n=len(events))


def oracle_policy(name):
    import pyoracle as O
    return {"FGD": (O.POL_FGD, O.SEL_FGD), "BestFit": (O.POL_BESTFIT, O.SEL_BEST),
            "GpuPacking": (O.POL_PACKING, O.SEL_BEST)}[name]
