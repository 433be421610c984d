"""The owning handles of ksim_host.hpp (DevBuf, DevEvent, DevStream, MappedFlags, GraphExec), compiled for the host
over malloc-backed stand-ins for the HIP calls (tests/native_host).

The program checks grow / alloc / upload / fill, moves (a vector of buffers resized past its capacity), create-once
and release of events, streams, the host-mapped flags and the graph handle, and the all-or-nothing construction of
an engine-shaped struct: every one of the calls a successful build makes is failed in turn, and each time the build
returns the error, hands out nothing and leaves no live block, event, stream or host block.  PeerMap, over stand-ins
for the two IPC calls and a world of 4: the k-th open fails for every k and every rank (exactly the opened ones are
closed, never the own slot, the map is empty), a good map closes world - 1 when its owner dies, a moved-from one
closes nothing.  The communicator's owner, over a counting destroyer: one destroy per communicator, none for null.
It aborts on the first broken expectation; here its exit status and printed tallies are checked.
"""
import os
import re
import subprocess

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native_host")


def test_host_handles():
    subprocess.run(["make", "-s", "-C", HERE], check=True)
    p = subprocess.run([os.path.join(HERE, "host_handles_check")], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       universal_newlines=True, timeout=60)
    print(p.stdout, p.stderr)
    assert p.returncode == 0, p.stderr
    lines = p.stdout.strip().splitlines()
    assert lines[-1] == "ok"
    out = dict(l.split(": ", 1) for l in lines[:-1])
    assert set(out) == {"devbuf", "move", "handles", "all-or-nothing", "peermap", "comm"}
    m = re.match(r"mallocs=(\d+) frees=(\d+) live=0$", out["devbuf"])
    assert m and m.group(1) == m.group(2) and int(m.group(1)) > 0
    assert out["move"] == "live=0"
    assert out["handles"].endswith("live=0")
    m = re.match(r"calls=(\d+) failures_injected=(\d+) blocks=17 events=3 streams=1 host=1 live_after=0$",
                 out["all-or-nothing"])
    assert m and m.group(1) == m.group(2) == "29"
    # PeerMap, a world of 4, every rank: each of the 3 opens failed in turn (0 + 1 + 2 opened and closed again), then
    # one good map (3 opened, 3 closed by the one owner left after two moves)
    assert out["peermap"] == "world=4 failures_injected=12 opens=%d closes=%d live=0" % (4 * 6, 4 * 6)
    assert out["comm"] == "held=3 destroys=3 null_destroys=0 live=0"
