"""The weighted combinations' ABI (KSIM_POLICY_WEIGHTED, ksim_engine_set_plugin_weights, KSIM_PATH_WSUM) and the
Python binding's policy strings (no GPU needed).

Without a device no engine exists (ksim_engine_create returns KSIM_ENODEV, tests/test_abi.py), so the argument
checks reachable here are those of a null engine, as in tests/test_desched_abi.py; the error codes that need an
engine are in tests/test_gpu_wsum_edges.py.
"""
import ctypes as C
import os
import re

import pytest

import ksim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_and_signature():
    L = ksim.lib()
    assert hasattr(L, "ksim_engine_set_plugin_weights")
    restype, args = ksim.SIGNATURES["ksim_engine_set_plugin_weights"]
    assert restype is C.c_int and args == [C.c_void_p, C.c_int, C.POINTER(C.c_int32)]
    assert L.ksim_abi_version() == 2  # functions and constants are only added


def test_header_constants():
    src = open(os.path.join(ROOT, "include", "ksim_engine.h")).read()
    assert re.search(r"KSIM_POLICY_WEIGHTED\s*=\s*8\b", src)
    assert re.search(r"#define\s+KSIM_NUM_PLUGINS\s+7\b", src)
    assert re.search(r"#define\s+KSIM_PATH_WSUM\s+9\b", src)
    assert re.search(r"#define\s+KSIM_ABI_VERSION\s+2\b", src)
    assert re.search(r"int\s+ksim_engine_set_plugin_weights\(ksim_engine\*\s*e,\s*int\s+replica,\s*const\s+int32_t\*\s*w", src)
    assert ksim.POLICY["Weighted"] == 8 and ksim.NUM_PLUGINS == 7
    # plugin ids are the policy numbers FGD .. PWR
    assert [ksim.POLICY[n] for n in ("FGD", "BestFit", "DotProd", "GpuPacking", "GpuClustering", "Random", "PWR")] == list(range(7))


def test_null_engine_is_einval():
    L = ksim.lib()
    w = (C.c_int32 * 7)(700, 300, 0, 0, 0, 0, 0)
    assert L.ksim_engine_set_plugin_weights(None, 0, w) == ksim.KSIM_EINVAL
    assert L.ksim_engine_set_policy(None, 0, 8, 0, 0) == ksim.KSIM_EINVAL


def test_no_cpu_fallback():
    # no engine without a device: creating one says so, and the binding's calls on a null engine raise
    if ksim.device_count() == 0:
        with pytest.raises(ksim.KsimError) as ei:
            ksim.Engine(4, 1)
        assert ei.value.code == ksim.KSIM_ENODEV
    eng = ksim.Engine.__new__(ksim.Engine)
    eng.h, eng.R, eng.N = None, 1, 1
    with pytest.raises(ksim.KsimError) as ei:
        eng.set_policy(0, "FGD 700 BestFit 300")
    assert ei.value.code == ksim.KSIM_EINVAL
    with pytest.raises(ksim.KsimError) as ei:
        eng.set_plugin_weights(0, {"FGD": 1})
    assert ei.value.code == ksim.KSIM_EINVAL
    with pytest.raises(KeyError):
        eng.set_plugin_weights(0, {"NoSuchPlugin": 1})


def test_parse_policy():
    P = ksim.parse_policy
    assert P("PWR 500 FGD 500") == ("PWR+FGD", (500, 500))  # the literal keeps its policy (k_replay)
    assert P("PWR_100_FGD_900") == ("PWR+FGD", (100, 900))
    assert P("FGD") == ("FGD", None) and P("Weighted") == ("Weighted", None)
    assert P("FGD 700 BestFit 300") == ("Weighted", {"FGD": 700, "BestFit": 300})
    assert P("FGD_700_BestFit_300") == ("Weighted", {"FGD": 700, "BestFit": 300})
    assert P("DotProd 500 GpuPacking 500") == ("Weighted", {"DotProd": 500, "GpuPacking": 500})
    assert P("FGD 400 GpuClustering 300 PWR 300") == ("Weighted", {"FGD": 400, "GpuClustering": 300, "PWR": 300})
    assert P("FGD 500 PWR 500") == ("Weighted", {"FGD": 500, "PWR": 500})  # not the literal's order
    assert P("BestFit 1000") == ("Weighted", {"BestFit": 1000})


def test_default_selector():
    # generate_config_and_run.py:264-277: the max-weight plugin's selector if it is FGD, DotProd or PWR and dimExt is
    # not merge, else best; the first in the harness's order wins a tie
    G = ksim.weighted_gpusel
    assert G({"FGD": 700, "BestFit": 300}) == "FGD"
    assert G({"FGD": 300, "BestFit": 700}) == "best"
    assert G({"BestFit": 500, "PWR": 500}) == "best"      # BestFit comes first
    assert G({"PWR": 500, "FGD": 500}) == "FGD"           # FGD comes first
    assert G({"PWR": 501, "FGD": 500}) == "PWR"
    assert G({"FGD": 700, "BestFit": 300}, "merge") == "best"
    assert G({"DotProd": 500, "GpuPacking": 500}, "share") == "DotProd"
    assert G({"DotProd": 500, "GpuPacking": 500}) == "best"  # this binding's DotProduct default is merge
    assert G({"GpuClustering": 300, "FGD": 400, "PWR": 300}) == "FGD"
