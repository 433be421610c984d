"""Descheduling: evict pods and schedule them again (pkg/simulator/deschedule.go:20-47 DescheduleCluster,
policies cosSim / fragOnePod / fragMultiPod).

The plan is made on the device (Engine.deschedule, Engine.deschedule_cossim; csrc/ksim_desched.hpp).  The
rescheduling is the ordinary replay: every replica's stream is extended with one delete event per victim and
then one creation event per victim, both in eviction order, and run again from the set_nodes state
(deschedule.go:87-91, :115-118, :174-177: the victims go through SchedulePods like any other pod).  There is
no second scheduling path.
"""
import ctypes as C

from . import COS_CPU_BAR_MILLI, COS_GPU_BAR_MILLI, Pod

COS_SIM = "cosSim"  # deschedule.go:15


def extend_events(events, n, victims):
    """A new ksim.Pod array: events[:n], then one delete event per victim (is_delete = 1, ref = its
    creation index), then a copy of each victim's creation event, both in eviction order.
    victims: Victim structures or creation-event indices."""
    idx = [v if isinstance(v, int) else v.event for v in victims]
    for e in idx:
        if not 0 <= e < n or events[e].is_delete:
            raise ValueError("victim %d is not a creation event of the stream" % e)
    out = (Pod * max(1, n + 2 * len(idx)))()
    if n:
        C.memmove(out, events, n * C.sizeof(Pod))
    for k, e in enumerate(idx):
        for at, delete in ((n + k, 1), (n + len(idx) + k, 0)):
            C.memmove(C.byref(out[at]), C.byref(events[e]), C.sizeof(Pod))
            out[at].is_delete, out[at].ref = delete, (e if delete else -1)
    return out


def run(engine, policy, ratio, cpu_bar=COS_CPU_BAR_MILLI, gpu_bar=COS_GPU_BAR_MILLI, stages=False):
    """Plan on the last run() of `engine`, extend every replica's stream with its victims, load it and run
    again.  policy: "fragOnePod" / "fragMultiPod" (or their ksim_desched_policy number), or "cosSim" with its
    two thresholds cpu_bar / gpu_bar in milli (the defaults are the values the reference hard-codes; the frag
    policies ignore them).  Returns, per replica, a dict: victims (list of Victim, or of CosVictim), budget,
    events (the extended ksim.Pod array), n (its length), n_original (the length of the stream the plan was
    made on), post_eviction (index of the last eviction: the report row the reference logs as PostEviction)
    and post_deschedule (index of the last event: PostDeschedule).  Without a victim both indices are the last
    event of the original stream (-1 for an empty one).

    stages=True adds stage_nodes: the node records (Engine.nodes) at the ends of the three stages the
    reference logs a ClusterAnalysis block for -- InitSchedule (fetched before the stream is replaced),
    PostEviction (from one extra run of the extended stream cut after the last delete event) and
    PostDeschedule (the final state).  The extra run costs one more replay of the stream per replica; the
    engine is left as after the full extended run either way."""
    if policy == COS_SIM:
        engine.deschedule_cossim(ratio, cpu_bar, gpu_bar)
        plans = [engine.cos_victims(r) for r in range(engine.R)]
    else:
        engine.deschedule(policy, ratio)
        plans = [engine.victims(r) for r in range(engine.R)]
    init_nodes = [engine.nodes(r) for r in range(engine.R)] if stages else None
    out = []
    for r, (victims, budget) in enumerate(plans):
        n = engine.n_events[r]
        src = (Pod * max(1, n)).from_buffer_copy(engine.events[r].tobytes()) if n else (Pod * 1)()
        ext = extend_events(src, n, victims)
        n_ext = n + 2 * len(victims)
        out.append(dict(victims=victims, budget=budget, events=ext, n=n_ext, n_original=n,
                        post_eviction=n + len(victims) - 1, post_deschedule=n_ext - 1))
    if stages:
        # the state after the evictions: the extended stream without the re-creations
        for r, o in enumerate(out):
            engine.load_events(r, o["events"], o["post_eviction"] + 1)
        engine.run()
        evicted_nodes = [engine.nodes(r) for r in range(engine.R)]
    for r, o in enumerate(out):
        engine.load_events(r, o["events"], o["n"])
    engine.run()
    if stages:
        for r, o in enumerate(out):
            o["stage_nodes"] = dict(InitSchedule=init_nodes[r], PostEviction=evicted_nodes[r],
                                    PostDeschedule=engine.nodes(r))
    return out


def run_group(group, policy, ratio, cpu_bar=COS_CPU_BAR_MILLI, gpu_bar=COS_GPU_BAR_MILLI):
    """run() without stages for a ksim.shard.ShardGroup: plan on the group's last run() (every shard's part, merged
    on the device), extend the stream with the cluster's victims, load it on every shard and run the group again.
    Returns the same dict as run() gives per replica (victims: node = the input index)."""
    if policy == COS_SIM:
        group.deschedule_cossim(ratio, cpu_bar, gpu_bar)
        victims, budget = group.cos_victims()
    else:
        group.deschedule(policy, ratio)
        victims, budget = group.victims()
    e0 = group.engines[0]
    n = e0.n_events[0]
    src = (Pod * max(1, n)).from_buffer_copy(e0.events[0].tobytes()) if n else (Pod * 1)()
    ext = extend_events(src, n, victims)
    n_ext = n + 2 * len(victims)
    group.load_events(ext, n_ext)
    group.run()
    return dict(victims=victims, budget=budget, events=ext, n=n_ext, n_original=n,
                post_eviction=n + len(victims) - 1, post_deschedule=n_ext - 1)
