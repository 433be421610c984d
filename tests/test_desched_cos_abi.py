"""The cosSim descheduling entry points' ABI (no GPU needed)."""
import ctypes as C
import inspect
import os
import subprocess

import pytest

import ksim
import ksim.desched

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cos_victim_layout_matches_c(tmp_path):
    src = os.path.join(ROOT, "tests", "golden", "abi_cos_victim_size.c")
    exe = str(tmp_path / "ksim_abi_cos_victim")
    subprocess.run(["gcc", "-I" + os.path.join(ROOT, "include"), src, "-o", exe], check=True)
    got = list(map(int, subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()))
    V = ksim.CosVictim
    assert got == [32, 0, 4, 8, 12, 16, 24]
    assert got == [C.sizeof(V), V.event.offset, V.node.offset, V.gpu_mask.offset, V.reserved.offset,
                   V.gpu_left_milli.offset, V.similarity.offset]


def test_entry_points_are_bound():
    L = ksim.lib()
    for name in ("ksim_engine_deschedule_cossim", "ksim_engine_get_cos_victims"):
        assert name in ksim.SIGNATURES and hasattr(L, name)
    assert ksim.SIGNATURES["ksim_engine_deschedule_cossim"][1][1:] == [C.c_double, C.c_int64, C.c_int64]
    # what the frag entry points pin stays: the ABI version, the policy numbers, and policy 2 is no policy there
    assert L.ksim_abi_version() == 2
    assert ksim.DESCHED_POLICY == {"fragOnePod": 0, "fragMultiPod": 1}
    # the documented defaults are the reference's hard-coded bars (deschedule.go:52-53)
    sig = inspect.signature(ksim.Engine.deschedule_cossim)
    assert (sig.parameters["cpu_bar"].default, sig.parameters["gpu_bar"].default) == (2000, 500)
    assert "cpu_bar" in inspect.signature(ksim.desched.run).parameters


def test_cossim_has_no_cpu_fallback():
    eng = ksim.Engine.__new__(ksim.Engine)
    eng.h, eng.R, eng.N = None, 1, 1
    with pytest.raises(ksim.KsimError) as ei:
        eng.deschedule_cossim(0.1)
    # a null engine where a device exists, else the missing device: never a plan made on the host
    assert ei.value.code == (ksim.KSIM_EINVAL if ksim.device_count() > 0 else ksim.KSIM_ENODEV)
    n = C.c_int(0)
    assert ksim.lib().ksim_engine_get_cos_victims(None, 0, None, 0, C.byref(n), None) == ksim.KSIM_EINVAL


def test_integration_doc_names_the_entry_points():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "ksim_engine_deschedule_cossim" in text and "ksim_engine_get_cos_victims" in text
