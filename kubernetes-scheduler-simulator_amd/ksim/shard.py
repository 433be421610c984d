"""Node-sharded single cluster (C5 across GPUs) -- host side.

The cluster's nodes are split into `world` contiguous ranges of name rank (the selectHost key,
generic_scheduler.go:187-212), one engine per range.  Every shard sees every event; per pod the
shards exchange a 32-byte record and only the owner of the winning node binds
(ksim_engine_set_shard).  This module builds the shards from a global node list and merges the
per-shard results back into global results (node = the input index, as an unsharded engine reports).
"""
import ctypes as C

import ksim


def partition(nodes, world):
    """Split a global ksim.Node array into `world` shards by name rank.
    Returns [(offset, local ksim.Node array ordered by rank, [global input index of each local node])]."""
    n = len(nodes)
    by_rank = sorted(range(n), key=lambda i: nodes[i].name_rank)
    assert [nodes[i].name_rank for i in by_rank] == list(range(n)), "name ranks must be 0..N-1"
    out = []
    for k in range(world):
        lo, hi = k * n // world, (k + 1) * n // world
        arr = (ksim.Node * max(1, hi - lo))()
        for j, i in enumerate(by_rank[lo:hi]):
            C.memmove(C.byref(arr[j]), C.byref(nodes[i]), C.sizeof(ksim.Node))
        out.append((lo, arr, by_rank[lo:hi]))
    return out


def merge_results(per_shard, parts):
    """Global results from the shards' results: per step, the record of the shard that owns the
    reported node (global rank) is authoritative; node ranks become input indices."""
    index_of_rank = {}
    owner_of_rank = {}
    for k, (off, _, idx) in enumerate(parts):
        for j, i in enumerate(idx):
            index_of_rank[off + j] = i
            owner_of_rank[off + j] = k
    out = []
    for s in range(len(per_shard[0])):
        r = per_shard[0][s]
        if r[0] >= 0:
            r = per_shard[owner_of_rank[r[0]]][s]
        node = index_of_rank[r[0]] if r[0] >= 0 else -1
        out.append((node,) + tuple(r[1:]))
    return out


def victims_by_index(victims, parts):
    """Copies of merged victim records with `node` mapped from the global rank to the input index, as
    merge_results maps a result's node."""
    index_of_rank = {off + j: i for off, _, idx in parts for j, i in enumerate(idx)}
    out = []
    for v in victims:
        w = type(v).from_buffer_copy(bytes(v))
        w.node = index_of_rank[v.node]
        out.append(w)
    return out


def merge_victims(parts_per_shard, bounds, ratio, parts, cos=False):
    """(victims, budget) of the cluster from one Engine.victim_part() list (cos: cos_victim_part(); or the bytes of
    its records) and one bound-pod count per shard: ksim.desched_merge / ksim.cos_merge on the host, then node =
    the input index.  parts: partition()'s."""
    victims, budget = (ksim.cos_merge if cos else ksim.desched_merge)(parts_per_shard, bounds, ratio)
    return victims_by_index(victims, parts), budget


def merge_reports(parts_per_shard):
    """(reports, power_reports) of the cluster from one Engine.report_parts() array (or its bytes) per shard:
    ksim.report_merge, the exact integer sum rounded once."""
    return ksim.report_merge(parts_per_shard)


class ShardGroup:
    """`world` shards of one cluster on one device, run in lockstep (ksim_shard_group_run).
    report=True: every shard reports its own nodes after the replay and the records are merged on the device
    (reports() / power_reports(); report_parts() gives each shard's exact records).  power_model: the energy
    model of the [Power] report, set on every shard; a PWR policy ("PWR", "PWR 500 FGD 500": Engine.set_policy's
    strings) needs it and schedules by it -- NormalizeScore's raw range is the whole cluster's, through the group
    launch's exchange on a create-only stream, through a second exchange round per pod otherwise."""

    def __init__(self, nodes, typical, world, policy="FGD", seed=0, device=0, report=False, power_model=None):
        arr, n = typical
        self.parts = partition(nodes, world)
        self.engines = []
        for k, (off, local, idx) in enumerate(self.parts):
            e = ksim.Engine(len(idx), 1, device=device)
            e.set_shard(k, world, off, len(nodes))
            e.set_nodes(0, local)
            e.set_typical(0, arr, n)
            e.set_policy(0, policy, seed=seed)
            if power_model is not None:
                e.set_power_model(0, power_model)
            if report:
                e.set_report(True)
            self.engines.append(e)

    def load_events(self, events, n):
        for e in self.engines:
            e.load_events(0, events, n)

    def run(self):
        return ksim.shard_group_run(self.engines)

    def results(self):
        return merge_results([e.results(0) for e in self.engines], self.parts)

    def reports(self):
        """The cluster's report after every event, merged on the device (dicts as Engine.reports)."""
        return ksim.shard_group_reports(self.engines)

    def power_reports(self):
        """The cluster's [Power] report after every event (needs power_model)."""
        return ksim.shard_group_reports(self.engines, power=True)

    def report_parts(self):
        """Each shard's exact per-event records (Engine.report_parts), in shard order."""
        return [e.report_parts(0) for e in self.engines]

    # descheduling (ksim_engine.h "Descheduling on a node-sharded cluster"); ksim.desched.run_group reschedules
    def deschedule(self, policy, ratio):
        """Plan "fragOnePod" / "fragMultiPod" on the last run(): every shard's part, merged on the device
        (ksim_shard_group_deschedule).  Returns engine 0's plan time in ms, the merge included."""
        return ksim.shard_group_deschedule(self.engines, policy, ratio)

    def deschedule_cossim(self, ratio, cpu_bar=ksim.COS_CPU_BAR_MILLI, gpu_bar=ksim.COS_GPU_BAR_MILLI):
        """Plan by the cosSim policy (ksim_shard_group_deschedule_cossim)."""
        return ksim.shard_group_deschedule_cossim(self.engines, ratio, cpu_bar, gpu_bar)

    def victims(self):
        """(the cluster's victims in eviction order, budget) of the last frag plan: the device merge, node = the
        input index as in results()."""
        victims, budget = ksim.shard_group_victims(self.engines)
        return victims_by_index(victims, self.parts), budget

    def cos_victims(self):
        """(the cluster's victims, budget) of the last cosSim plan, node = the input index."""
        victims, budget = ksim.shard_group_cos_victims(self.engines)
        return victims_by_index(victims, self.parts), budget

    def victim_parts(self, cos=False):
        """Each shard's own list and bound-pod count (Engine.victim_part; cos: cos_victim_part), in shard order:
        ([lists], [bounds]), node = the global rank, as ksim.desched_merge / ksim.cos_merge take them."""
        got = [e.cos_victim_part() if cos else e.victim_part() for e in self.engines]
        return [g[0] for g in got], [g[1] for g in got]

    def close(self):
        for e in self.engines:
            e.close()


def host_gather(dist, group=None):
    """A ksim_shard_exchange_fn body over torch.distributed (any backend with CPU tensors, e.g.
    gloo): all-gather of the 4-word shard record, returned flat in rank order."""
    import torch
    world = dist.get_world_size(group)

    def signed(v):
        return v - (1 << 64) if v >= 1 << 63 else v

    def gather(record):
        t = torch.tensor([signed(v) for v in record], dtype=torch.int64)
        out = [torch.empty(4, dtype=torch.int64) for _ in range(world)]
        dist.all_gather(out, t, group=group)
        return [int(v) & 0xFFFFFFFFFFFFFFFF for o in out for v in o.tolist()]
    return gather


def run_distributed(nodes, typical, events, n, dist, policy="FGD", seed=0, device=0, engine_cls=None,
                    exchange="rccl", report=False, power_model=None, desched=None):
    """One shard per process (torchrun; backend nccl = RCCL for the launcher's own collectives):
    rank 0 makes the RCCL id of the shards' exchange, every rank builds its shard engine on
    `device`, replays the events, and the per-shard results are gathered and merged on every rank.
    exchange="host": no RCCL communicator; every pod step's record goes through `dist` (host_gather),
    e.g. shards sharing one GPU, or hosts without a common RCCL fabric.
    exchange="device" (FGD): each shard's persistent k_hmemo stores its per-step slice maxima straight into
    every peer's IPC-mapped exchange buffer (ksim_engine_set_shard_peers); `dist` only carries the handles.
    report=True: every shard also reports its own nodes; the ranks gather the exact records (all_gather_object of
    their bytes) and each merges them on the host (merge_reports).  power_model: the [Power] report's energy model.
    A PWR policy ("PWR", "PWR <w> FGD <w>") needs the power_model and runs over exchange="rccl" and "host" (two
    exchange rounds per created pod: the shards' raw score ranges, then their keys under the cluster's range; the
    host gather is called once per round) -- not over "device", which stays FGD only (KSIM_ENOTSUP).
    Returns (merged results, device ms of this rank's run), with report=True (merged results, ms, reports): the
    cluster's report per event, each with its power report under "power" when a power_model was given.
    desched=(policy, ratio) or ("cosSim", ratio, cpu_bar, gpu_bar): after its run each rank plans its part; the ranks
    gather the parts' bytes and bound counts and each merges them on the host (merge_victims).  The return value gains
    (victims, budget) as its last element.  Rescheduling is a second run_distributed on the extended stream
    (ksim.desched.extend_events), left to the caller."""
    engine_cls = engine_cls or ksim.Engine
    rank, world = dist.get_rank(), dist.get_world_size()
    parts = partition(nodes, world)
    off, local, idx = parts[rank]
    if exchange == "rccl":
        box = [shard_comm_id_for(engine_cls) if rank == 0 else None]
        dist.broadcast_object_list(box, src=0)
    elif exchange in ("host", "device"):
        box = [None]
    else:
        raise ValueError("exchange must be 'rccl', 'host' or 'device'")
    e = engine_cls(len(idx), 1, device=device)
    e.set_shard(rank, world, off, len(nodes), box[0])
    if exchange == "host":
        e.set_shard_exchange(host_gather(dist))
    if exchange == "device":  # FGD: the shards' k_hmemo slices exchange granules through IPC-mapped buffers
        handles = [None] * world
        dist.all_gather_object(handles, e.shard_peer_handle())
        e.set_shard_peers(handles)
    e.set_nodes(0, local)
    arr, nt = typical
    e.set_typical(0, arr, nt)
    e.set_policy(0, policy, seed=seed)
    if power_model is not None:
        e.set_power_model(0, power_model)
    if report:
        e.set_report(True)
    e.load_events(0, events, n)
    ms = e.run()
    mine = e.results(0)
    my_parts = bytes(e.report_parts(0)) if report else None
    my_plan = None
    if desched is not None:
        cos = desched[0] == "cosSim"
        if cos:
            e.deschedule_cossim(*desched[1:])
            mine_v, bound = e.cos_victim_part()
        else:
            e.deschedule(*desched)
            mine_v, bound = e.victim_part()
        my_plan = (b"".join(bytes(v) for v in mine_v), bound)
    e.close()
    gathered = [None] * world
    dist.all_gather_object(gathered, mine)
    merged = merge_results(gathered, parts)
    plan = ()
    if desched is not None:
        plans = [None] * world
        dist.all_gather_object(plans, my_plan)
        plan = (merge_victims([p[0] for p in plans], [p[1] for p in plans], desched[1], parts, cos=cos),)
    if not report:
        return (merged, ms) + plan
    all_parts = [None] * world
    dist.all_gather_object(all_parts, my_parts)
    reports, power = merge_reports(all_parts)
    if power_model is not None:
        for r, p in zip(reports, power):
            r["power"] = p
    return (merged, ms, reports) + plan


def shard_comm_id_for(engine_cls):
    f = getattr(engine_cls, "comm_id", None)
    return f() if f is not None else ksim.shard_comm_id()
