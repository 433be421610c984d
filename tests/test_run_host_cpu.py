"""The per-run diagnostics and the shard transport predicates (csrc/ksim_run_host.hpp): no GPU.

The stand-alone program tests/native_run_host (the header under the address and undefined-behaviour sanitizers) checks
that RunStats{} is every field's documented zero, that note_kernel keeps each name once, in launch order, '+'-joined,
that run_path equals a literal copy of the if-chain ksim_engine_last_run_path had over the loose members (R in 1..3,
every memo / hmemo / rgo / scan1 count with sum <= R, run_mode 0..3, step path, sharded; every path value reached), and that the transport predicates give the entry point x transport table of DESIGN.md, held there as data.
It aborts on the first broken expectation; here its exit status and printed tallies are checked.
"""
import os
import subprocess

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native_run_host")


def count_run_path_cases():
    n = 0
    for R in (1, 2, 3):
        for memo in range(R + 1):
            for hmemo in range(R + 1 - memo):
                for rgo in range(R + 1 - memo - hmemo):
                    n += R + 1 - memo - hmemo - rgo  # scan1
    return n * 4 * 2 * 2


def test_native_program_under_sanitizers():
    subprocess.run(["make", "-s", "-C", HERE], check=True)
    p = subprocess.run([os.path.join(HERE, "run_host_check")], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       universal_newlines=True, timeout=120)
    print(p.stdout, p.stderr)
    assert p.returncode == 0, p.stderr
    lines = p.stdout.strip().splitlines()
    assert lines[-1] == "ok"
    out = dict(l.split(": ", 1) for l in lines[:-1])
    assert set(out) == {"zero", "note_kernel", "run_path", "transport"}
    assert out["zero"] == "fields=14"
    assert out["run_path"] == "cases=%d paths=8" % count_run_path_cases()
    assert out["transport"] == "rows=12 entry_points=6"
