"""Descheduling: evict the pods that cause the most GPU fragmentation and schedule them again
(pkg/simulator/deschedule.go:20-47 DescheduleCluster, policies fragOnePod / fragMultiPod).

The plan is made on the device (Engine.deschedule, csrc/ksim_desched.hpp).  The rescheduling is the
ordinary replay: every replica's stream is extended with one delete event per victim and then one
creation event per victim, both in eviction order, and run again from the set_nodes state
(deschedule.go:115-118, :174-177: the victims go through SchedulePods like any other pod).  There is no
second scheduling path.
"""
import ctypes as C

from . import Pod


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


def run(engine, policy, ratio):
    """Plan on the last run() of `engine`, extend every replica's stream with its victims, load it and run
    again.  Returns, per replica, a dict: victims (list of Victim), budget, events (the extended ksim.Pod
    array), n (its length), post_eviction (index of the last eviction: the report row the reference logs
    as PostEviction) and post_deschedule (index of the last event: PostDeschedule).  Without a victim both
    indices are the last event of the original stream (-1 for an empty one)."""
    engine.deschedule(policy, ratio)
    plans = [engine.victims(r) for r in range(engine.R)]
    out = []
    for r, (victims, budget) in enumerate(plans):
        n = engine.n_events[r]
        src = (Pod * max(1, n)).from_buffer_copy(engine.events[r].tobytes()) if n else (Pod * 1)()
        ext = extend_events(src, n, victims)
        n_ext = n + 2 * len(victims)
        engine.load_events(r, ext, n_ext)
        out.append(dict(victims=victims, budget=budget, events=ext, n=n_ext, post_eviction=n + len(victims) - 1,
                        post_deschedule=n_ext - 1))
    engine.run()
    return out
