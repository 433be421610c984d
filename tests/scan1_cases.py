"""Crafted create-only streams for k_scan1's dead-class skip and its 128-event window
(tests/test_scan1_cases.py, tests/test_gpu_scan1_edges.py).

Random fuzz clusters (tests/fuzz_cases.py) hardly reach the skip, and never at a window edge, so these
streams put dead events where the kernel's bookkeeping changes: at the last and the first position of a
128-event window, at the first and the last bit of a word of the dead-class mask, and at the class
count where the host turns the skip off.  Three kinds of pod class, class ids in order of first
appearance (ksim_plan.hpp classify_events):
  filler       tiny CPU-only pods, always feasible; one class per distinct cpu value
  born dead    more CPU than any node has: the first event already finds no node
  dies mid-run whole-8-GPU pods on a cluster with two 8-GPU nodes: two bind, the third finds nothing
The cases have make_case's dict shape, so test_gpu_fuzz's run_engine / check_state take them.
"""
import ksim

MODELS = ["G2", "T4"]
BIG_CPU = 500000          # born dead: above every node's CPU (at most 128000)
WHOLE8 = (4000, 1000, 8)  # dies mid-run: (cpu, milli, num)
# the target workload (the report's fragmentation bins): fixed and small, whatever the stream's classes
WORKLOAD = [(4000, 1000, 8, ""), (4000, 1000, 1, ""), (2000, 500, 1, ""), (1000, 250, 1, ""), (8000, 1000, 2, "")]

WINDOW_DEAD = (126, 127, 128, 129, 255, 256, 257)  # repeats of the dying classes at the window edges
WINDOW_RUN = range(378, 390)                       # consecutive dead events over 383 / 384
WINDOW_LENGTHS = (127, 128, 129, 257, 400)
WORD_IDS = (31, 32, 33)                            # born-dead classes at a word's last and first bits
LIMIT_CLASSES = (1024, 1025)                       # the skip on with its last bit used; the skip off


def cluster(n_plain, cpu_nodes=4, whole8=2):
    """-> [(cpu, mem, pods, gpu, model)]: `whole8` 8-GPU nodes, `cpu_nodes` GPU-less ones with the most
    CPU, n_plain nodes of 1 to 4 GPUs; the kinds interleaved so that every wave of the scan holds some."""
    plain = [(32000 + 16000 * (i % 5), 262144, 1000, 1 + i % 4, i % 2) for i in range(n_plain)]
    w8, big = (96000, 786432, 1000, 8, 1), (128000, 786432, 1000, 0, 0)
    special = [w8] * (whole8 - whole8 // 2) + [big] * cpu_nodes + [w8] * (whole8 // 2)  # an 8-GPU node in wave 1
    out, step = [], max(1, (n_plain + len(special)) // max(1, len(special)))
    while plain or special:
        if special and (len(out) % step == step - 1 or not plain):
            out.append(special.pop(0))
        else:
            out.append(plain.pop(0))
    return out


def filler(i):
    return (1 + i, 0, 0)  # class i of the fillers: cpu 1 + i milli


def dead_cpu(k=0):
    return (BIG_CPU + k, 0, 0)


def build(nodes, pods):
    """nodes: cluster(); pods: [(cpu, milli, num)] -> make_case's dict"""
    import pyoracle as O

    n = len(nodes)
    # names: ranks run against the node index, so the smallest-name tie-break is not the index order
    names = ["%04d-n%d" % (n - 1 - i, i) for i in range(n)]
    arr = (ksim.Node * n)()
    onodes = []
    for i, (cpu, mem, pods_alloc, gpu, model) in enumerate(nodes):
        a = arr[i]
        a.cpu_alloc_milli, a.mem_alloc_mib, a.pods_alloc = cpu, mem, pods_alloc
        a.gpu_count, a.gpu_type, a.name_rank = gpu, model if gpu else 0, n - 1 - i
        onodes.append(dict(name=names[i], cpu=cpu, mem=mem, pods=pods_alloc, gpu=gpu, model=MODELS[model] if gpu else ""))
    evs = [ksim.make_pod(cpu, milli, num, 0, ksim.KSIM_TYPE_ANY, cpu_nz=cpu) for cpu, milli, num in pods]
    oev = [dict(cpu=cpu, cpu_nz=cpu, mem=0, milli=milli, num=num, type="") for cpu, milli, num in pods]
    otyp = O.get_typical_pods(WORKLOAD)
    typ = (ksim.Typical * len(otyp))()
    for i, (cpu, milli, num, _, freq) in enumerate(otyp):
        typ[i].cpu_milli, typ[i].gpu_milli, typ[i].gpu_count = cpu, milli, num
        typ[i].type_mask, typ[i].freq = ksim.KSIM_TYPE_ANY, freq
    return dict(nodes=arr, events=(ksim.Pod * max(1, len(evs)))(*evs), n_events=len(evs), typical=typ,
                typical_n=len(otyp), onodes=onodes, oevents=oev, otypical=otyp)


def window_pods(length=400):
    """Both dying classes first appear before event 100 (the whole-8 class dies at event 9), then come
    back at WINDOW_DEAD and as the run WINDOW_RUN; fillers of 37 classes everywhere else."""
    pods = [filler(i % 37) for i in range(400)]
    for i in (2, 5, 9):
        pods[i] = WHOLE8
    pods[40] = dead_cpu()
    for k, i in enumerate(list(WINDOW_DEAD) + list(WINDOW_RUN)):
        pods[i] = dead_cpu() if k % 2 == 0 else WHOLE8
    return pods[:length]


def window_case(length=400):
    return build(cluster(64), window_pods(length))


def word_pods():
    """Fillers take the class ids 0..30, three born-dead classes 31, 32, 33, fillers 34..66; then every
    dead class comes back between repeats of the fillers whose bits a wrong word or bit would set:
    30 and 34 (the neighbours), 0, 1 and 2 (the same bits one word down), 63, 64, 65 and 66 (one word up)."""
    pods = [filler(i) for i in range(31)] + [dead_cpu(k) for k in range(3)] + [filler(i) for i in range(31, 64)]
    near = [filler(i) for i in (30, 31, 0, 1, 2, 60, 61, 62, 63)]  # filler(31 + j) has the class id 34 + j
    for rnd in range(3):
        for k in range(3):
            pods += [dead_cpu(k)] + near
    return pods


def word_case():
    return build(cluster(64), word_pods())


def limit_pods(n_classes):
    """n_classes - 1 filler classes, then the born-dead class as the last id, its repeats between fillers
    of the first and the last ids and of id 992, the last word's first bit (1024 classes: the last bit of
    the last word; 1025: the skip is off, and a kernel that kept it on would set bit 0 of the next wave's
    mask -- class 0)."""
    nf = n_classes - 1
    pods = [filler(i) for i in range(nf)] + [dead_cpu()]
    for _ in range(4):
        pods += [filler(0), filler(nf - 1), dead_cpu(), filler(nf - 2), filler(992), filler(31), dead_cpu(), filler(32)]
    return pods


def limit_case(n_classes):
    # six nodes: the 1024 fillers ask for 525 cores in all, five 128-core nodes hold them
    return build(cluster(1, cpu_nodes=5, whole8=0), limit_pods(n_classes))


# The create-only fuzz clusters (fuzz_cases.make_case) of the node-count edges: N -> (seed, creations).  63 / 64 / 65:
# a wave's last lane; 255 / 256 / 257: a thread's second slot (at 257 slot 1 holds one lane of wave 0); 1279 / 1280: the
# last register slot, full; 1281: the first N with the records in LDS only.  The seeds are the first from 41 on whose
# oracle replays bind in every slot and every wave (at 65: on node 64) under every policy (tests/test_scan1_cases.py asserts it).
EDGE = {1: (41, 300), 63: (41, 300), 64: (41, 300), 65: (42, 300), 97: (41, 400), 255: (41, 400), 256: (41, 400),
        257: (42, 400), 1279: (41, 1500), 1280: (41, 1500), 1281: (43, 1500)}
# the policies whose replay of that case has an event with exactly one feasible node (the shortcut past Score)
SINGLE = {1: "all", 63: "all", 64: "all", 65: "all", 97: "all", 255: ("DotProd", "Random"),
          256: ("DotProd", "GpuPacking", "Random"), 257: ("DotProd", "GpuPacking", "GpuClustering", "Random"),
          1279: (), 1280: (), 1281: ()}
_EDGE_CACHE = {}


def edge_case(n, seed=None):
    """The fuzz cluster of N nodes (EDGE's seed, or another seed with the same number of creations); made once."""
    from fuzz_cases import make_case
    key = (n, EDGE[n][0] if seed is None else seed)
    if key not in _EDGE_CACHE:
        _EDGE_CACHE[key] = make_case(key[1], n, EDGE[n][1], 0.0)
    return _EDGE_CACHE[key]


def class_ids(oevents):
    """classify_events restated: ids by first appearance over (cpu, cpu_nz, mem, milli, num, mask)"""
    seen, out = {}, []
    for e in oevents:
        k = (e["cpu"], e["cpu_nz"], e["mem"], e["milli"], e["num"], e["type"])
        out.append(seen.setdefault(k, len(seen)))
    return out


CRAFTED = ["window-%d" % n for n in WINDOW_LENGTHS] + ["word"] + ["limit-%d" % n for n in LIMIT_CLASSES]
_CRAFTED_CACHE = {}


def crafted(cid):
    """The crafted case of that id (CRAFTED: every stream of the three variants); made once."""
    if cid not in _CRAFTED_CACHE:
        kind, _, n = cid.partition("-")
        _CRAFTED_CACHE[cid] = {"window": window_case, "limit": limit_case}[kind](int(n)) if n else word_case()
    return _CRAFTED_CACHE[cid]
