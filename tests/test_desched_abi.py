"""The descheduling entry points' ABI and the stream extension (no GPU needed)."""
import ctypes as C
import os
import subprocess

import pytest

import ksim
import ksim.desched

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_victim_layout_matches_c(tmp_path):
    src = os.path.join(ROOT, "tests", "golden", "abi_victim_size.c")
    exe = str(tmp_path / "ksim_abi_victim")
    subprocess.run(["gcc", "-I" + os.path.join(ROOT, "include"), src, "-o", exe], check=True)
    got = list(map(int, subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()))
    V = ksim.Victim
    assert got == [40, 0, 4, 8, 16, 24, 32]
    assert got == [C.sizeof(V), V.event.offset, V.node.offset, V.gpu_mask.offset, V.score.offset,
                   V.frag_before.offset, V.frag_after.offset]


def test_entry_points_are_bound():
    L = ksim.lib()
    for name in ("ksim_engine_deschedule", "ksim_engine_get_victims", "ksim_engine_last_deschedule_ms"):
        assert name in ksim.SIGNATURES and hasattr(L, name)
    assert L.ksim_abi_version() == 2
    assert ksim.DESCHED_POLICY == {"fragOnePod": 0, "fragMultiPod": 1}


def test_deschedule_has_no_cpu_fallback():
    # without a device no engine exists (tests/test_abi.py) and the planning call itself says so too
    eng = ksim.Engine.__new__(ksim.Engine)
    eng.h, eng.R, eng.N = None, 1, 1
    with pytest.raises(ksim.KsimError) as ei:
        eng.deschedule("fragOnePod", 0.1)
    if ksim.device_count() > 0:
        assert ei.value.code == ksim.KSIM_EINVAL  # a null engine
    else:
        assert ei.value.code == ksim.KSIM_ENODEV
        with pytest.raises(ksim.KsimError) as ei:
            ksim.Engine(16, 1)
        assert ei.value.code == ksim.KSIM_ENODEV
    # the other two reject a null engine before anything else
    n = C.c_int(0)
    assert ksim.lib().ksim_engine_get_victims(None, 0, None, 0, C.byref(n), None) == ksim.KSIM_EINVAL
    assert ksim.lib().ksim_engine_last_deschedule_ms(None, None) == ksim.KSIM_EINVAL


def fields(p):
    return (p.cpu_milli, p.cpu_nz_milli, p.mem_mib, p.gpu_milli, p.gpu_count, p.type_mask, p.is_delete, p.ref)


def test_extend_events_appends_deletes_then_recreations():
    ev = (ksim.Pod * 5)()
    ev[0] = ksim.make_pod(1000, 500, 1, mem=10, type_mask=4)
    ev[1] = ksim.make_pod(0, 0, 0, cpu_nz=100)
    ev[2] = ksim.make_pod(8000, 1000, 2)
    ev[3] = ksim.make_pod(0, 0, 0, cpu_nz=100)
    ev[3].is_delete, ev[3].ref = 1, 1
    ev[4] = ksim.make_pod(2000, 250, 1)  # beyond n: not part of the stream
    victims = [ksim.Victim(event=2), ksim.Victim(event=0)]
    out = ksim.desched.extend_events(ev, 4, victims)
    assert len(out) == 8
    assert [fields(out[i]) for i in range(4)] == [fields(ev[i]) for i in range(4)]
    assert fields(out[4]) == (8000, 8000, 0, 1000, 2, ksim.KSIM_TYPE_ANY, 1, 2)   # delete e2 first
    assert fields(out[5]) == (1000, 1000, 10, 500, 1, 4, 1, 0)                    # then e0
    assert fields(out[6]) == (8000, 8000, 0, 1000, 2, ksim.KSIM_TYPE_ANY, 0, -1)  # re-created in the same order
    assert fields(out[7]) == (1000, 1000, 10, 500, 1, 4, 0, -1)
    # the original array is untouched, no victim gives the stream back, and only creation events can be victims
    assert fields(ev[2]) == (8000, 8000, 0, 1000, 2, ksim.KSIM_TYPE_ANY, 0, -1)
    same = ksim.desched.extend_events(ev, 4, [])
    assert [fields(same[i]) for i in range(4)] == [fields(ev[i]) for i in range(4)]
    with pytest.raises(ValueError):
        ksim.desched.extend_events(ev, 4, [3])
    with pytest.raises(ValueError):
        ksim.desched.extend_events(ev, 4, [4])
